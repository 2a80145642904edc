"""Multi-process (gloo, world_size 2, CPU) tests of the N>1 path: sharding of images and
(image, class) problems with no data-path collective, and the flat-bucket gradient all-reduce."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    # sdd.init binds LOCAL_RANK to a GPU wherever one is visible: on a box with fewer GPUs than ranks the
    # ranks share them (every tensor of this test lives on the CPU)
    ndev = torch.cuda.device_count()
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank % ndev if ndev else rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from simpledet_amd import dist as sdd
    r, _, w = sdd.init("gloo")
    assert (r, w) == (rank, world)
    # 1. images shard contiguously, every image exactly once
    lo, hi = sdd.shard_range(5, rank, world)
    mine = list(range(lo, hi))
    allr = sdd.gather_ragged(mine)
    # 2. gradient buckets: rank-dependent grads, averaged
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.zeros(s)) for s in [(300,), (17, 5), (1000, 3), (2,)]]
    for i, p in enumerate(params):
        p.grad = torch.full_like(p, float((rank + 1) * (i + 1)))
    red = sdd.GradBucketReducer(params, bucket_mb=0.004)  # forces several buckets
    ptrs = [p.grad.data_ptr() for p in params]
    red.reduce()
    ok = all(torch.allclose(p.grad, torch.full_like(p, (i + 1) * (world + 1) / 2.0))
             for i, p in enumerate(params))
    ok = ok and ptrs == [p.grad.data_ptr() for p in params]  # persistent views, nothing re-allocated
    # 2b. autograd path: hooks launch a bucket as soon as its last gradient exists
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))
    red2 = sdd.GradBucketReducer(net.parameters(), bucket_mb=0.0002)
    for step in range(2):
        red2.zero_grad()
        x = torch.full((3, 8), float(rank + 1 + step))
        net(x).sum().backward()
        red2.finish()
        # reference: the mean over ranks of the single-process gradients
        ref = [torch.zeros_like(p) for p in net.parameters()]
        for rr in range(world):
            net2 = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))
            net2.load_state_dict(net.state_dict())
            net2(torch.full((3, 8), float(rr + 1 + step))).sum().backward()
            for a, p2 in zip(ref, net2.parameters()):
                a += p2.grad / world
        ok = ok and all(torch.allclose(p.grad, a, atol=1e-5) for p, a in zip(net.parameters(), ref))
    ok = ok and len(red2.buckets) >= 2
    # 2c. a frozen parameter shares a bucket with trained ones (frozen BN / stem in detection nets):
    # the bucket still launches from its last hook; a parameter that gets no gradient in a step
    # (set_to_none) contributes zeros, not the averaged value of the step before
    torch.manual_seed(2)
    a_, b_, c_ = (torch.nn.Parameter(torch.randn(6)) for _ in range(3))
    b_.requires_grad_(False)
    red3 = sdd.GradBucketReducer([a_, b_, c_], bucket_mb=1.0)
    ok = ok and len(red3.buckets) == 1 and red3.buckets[0]["pending"] == 2
    (a_ * float(rank + 1)).sum().backward()
    (c_ * 2.0).sum().backward()
    ok = ok and red3.buckets[0]["handle"] is not None      # launched by the hooks, not by finish()
    red3.finish()
    ok = ok and bool(torch.allclose(a_.grad, torch.full((6,), (world + 1) / 2.0)))
    ok = ok and bool(torch.allclose(c_.grad, torch.full((6,), 2.0)))
    a_.grad = None                                           # optimizer.zero_grad(set_to_none=True)
    c_.grad = None
    (a_ * float(rank + 1)).sum().backward()                  # c_ gets no gradient in this step
    red3.finish()
    ok = ok and bool(torch.allclose(a_.grad, torch.full((6,), (world + 1) / 2.0)))
    ok = ok and c_.grad is not None and bool(torch.all(c_.grad == 0))
    ar = sdd.OverlappedAllReduce(4 * 100)
    ar.buf.fill_(float(rank + 1))
    ar.start()
    ar.finish()
    ok = ok and bool(torch.allclose(ar.buf, torch.full_like(ar.buf, (world + 1) / 2.0)))
    # 3. (image, class) soft-NMS problems round robin; results gathered ragged
    probs = sdd.shard_round_robin(7, rank, world)
    res = sdd.gather_ragged([(p, p * p) for p in probs])
    if rank == 0:
        q.put((allr, len(red.buckets), ok, res))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharding_and_gradient_allreduce():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        allr, nb, ok, res = q.get(timeout=120)
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:  # a rank left waiting for a failed peer must not outlive the test
            if p.is_alive():
                p.terminate()
                p.join(10)
    assert sorted(sum(allr, [])) == list(range(5))
    assert nb >= 3 and ok
    flat = sorted(sum(res, []))
    assert flat == [(p, p * p) for p in range(7)]


def test_shard_helpers_cover_everything_once():
    from simpledet_amd import dist as sdd
    for n in (0, 1, 7, 16):
        for w in (1, 2, 3, 8):
            got = []
            for r in range(w):
                lo, hi = sdd.shard_range(n, r, w)
                got += list(range(lo, hi))
            assert got == list(range(n))
            rr = sorted(sum([sdd.shard_round_robin(n, r, w) for r in range(w)], []))
            assert rr == list(range(n))


def test_bench_self_launch_two_ranks_gloo():
    """`python bench.py --gpus 2` with no torchrun environment re-launches itself through
    torch.distributed.run (127.0.0.1 rendezvous), all-reduces the gradient buffer every step and
    prints ONE JSON line from rank 0.  SD_BENCH_BACKEND=gloo runs that launcher path without GPUs."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["SD_BENCH_BACKEND"] = "gloo"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
                          "--warmup", "1", "--grad-allreduce", "2", "--full"], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["allreduce_correct"] is True
    # `value`'s timed loop is the path alone (it has no collective); the line carries the N = 1 figure of
    # the same invocation, and the reference's gradient all-reduce as separate legs under their own key
    assert d["ms_per_step"] > 0 and d["n1_ms_per_step_same_invocation"] > 0
    assert 0 < d["weak_scaling_eff_same_invocation"] < 1e4   # (sub-millisecond CPU timings under gloo)
    ga = d["grad_allreduce"]
    for k in ("alone_ms", "busbw_GBs", "ops_plus_allreduce_ms_per_step", "exposed_ms",
              "weak_scaling_eff_with_allreduce"):
        assert k in ga and ga[k] is not None and ga[k] >= 0, k
    assert ga["mb_per_step"] == 2 and "NOT in `value`" in ga["what"]
    # the composite leg contains the path's steps plus the collective: it cannot be faster than ~the path
    assert ga["ops_plus_allreduce_ms_per_step"] >= 0.2 * d["ms_per_step"]
    assert len(d["per_rank_ms_per_step"]) == 2


@pytest.mark.gpu
def test_bench_rccl_code_path_with_one_rank():
    """Round 6 ("missing" 1: no RCCL rank had ever executed bench.py's N > 1 code): the whole N > 1 path --
    process group on backend nccl (= RCCL) with `device_id`, the all-reduce of ones, barriers, the all-gather of the
    per-rank times, the broadcast of rank 0's solo leg, `OverlappedAllReduce` on its side stream started behind the
    forward and joined at the end of the step -- under torchrun with ONE rank, which is what a single-GPU box can run
    (SD_BENCH_FORCE_DIST=1; RCCL refuses two ranks on one device).  A communicator of size one still goes through
    RCCL's enqueue / stream-ordering code; what it cannot show is bandwidth."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["SD_BENCH_FORCE_DIST"] = "1"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                          "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                          os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                          "--full", "--no-cpu-baseline", "--no-ops", "--no-extra"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["rccl_ranks"] == 1 and d["value"] > 0
    assert d["n1_ms_per_step_same_invocation"] > 0 and len(d["per_rank_ms_per_step"]) == 1
    ga = d["grad_allreduce"]
    assert ga["mb_per_step"] == 165.0 and ga["alone_ms"] >= 0 and ga["ops_plus_allreduce_ms_per_step"] > 0
