"""bench.py's plain run (headline figure only) and its --dump-outputs files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(out):
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_dump_outputs_writes_a_fixed_bounded_sample(tmp_path):
    import torch
    import bench
    big = torch.arange(bench.DUMP_MAX_ELEMS + 1000, dtype=torch.float64).reshape(-1, 8)
    small = torch.arange(24, dtype=torch.uint8).reshape(2, 3, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("big", big), ("small", small)])
    a_big, b_big = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a_big.dtype == np.float32 and a_big.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.array_equal(a_big, b_big)
    # the sample is the array's own elements at distinct sorted positions
    assert np.all(np.diff(a_big) > 0) and a_big.max() < big.numel()
    a_small = np.load(tmp_path / "a" / "small.npy")
    assert a_small.dtype == np.float32 and np.array_equal(a_small, small.numpy().astype(np.float32))


def test_plain_self_launch_line_has_no_full_legs():
    """Without --full the N > 1 launcher path prints the headline figure only (no single-rank / all-reduce legs)."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["SD_BENCH_BACKEND"] = "gloo"
    d = _line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
                              "--warmup", "1", "--grad-allreduce", "2"], env=env, capture_output=True,
                             text=True, timeout=300))
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["ms_per_step"] > 0
    assert "grad_allreduce" not in d and "n1_ms_per_step_same_invocation" not in d


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path, ops):
    """A plain run: the headline fields, none of the --full ones, and --dump-outputs files that hold what the
    path computes on the same seeded inputs (forward bit for bit, gradients within the backward's 1e-4)."""
    import torch
    import bench
    from simpledet_amd import synth
    out_dir = tmp_path / "dump"
    d = _line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                              "--warmup", "1", "--dump-outputs", str(out_dir)], capture_output=True, text=True,
                             timeout=600))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["full"] is False
    assert "roofline" not in d and "cpu_baseline" not in d and "ops" not in d
    names = ["out"] + ["d_feat_p%d" % l for l in (2, 3, 4, 5)]
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in names)
    assert sum(os.path.getsize(out_dir / (n + ".npy")) for n in names) <= 64 << 20
    got = {n: np.load(out_dir / (n + ".npy")) for n in names}
    assert all(g.dtype == np.float32 for g in got.values())

    strides = list(synth.FPN_STRIDES)
    feats = [torch.from_numpy(f).cuda() for f in synth.feature_maps(0, 2, 256, synth.FPN_SHAPES)]
    rois = torch.from_numpy(synth.random_rois(0, 2, 512)).cuda()
    out, am = ops.fpn_roi_align_forward_packed(feats, rois, strides, (7, 7), plan=True)
    dy = torch.randn(out.shape, device="cuda", generator=bench.dy_generator(0))
    dfeats = ops.fpn_roi_align_backward_packed(dy, rois, am, [f.shape for f in feats], strides)
    ref = dict(zip(names, [out] + list(dfeats)))
    for n in names:
        want = ref[n].reshape(-1)
        if want.numel() > bench.DUMP_MAX_ELEMS:
            pos = np.sort(np.random.default_rng(0).choice(want.numel(), bench.DUMP_MAX_ELEMS, replace=False))
            want = want[torch.from_numpy(pos).cuda()]
        else:
            assert got[n].shape == tuple(ref[n].shape), n
        want = want.cpu().numpy().reshape(got[n].shape)
        if n == "out":
            assert np.array_equal(got[n], want)
        else:
            assert float(np.abs(got[n] - want).max()) <= 1e-4, n
