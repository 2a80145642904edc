"""se_block (simpledet_amd/csrc/se_block.hip) against the restatements of tests/se_block_ref.py.

CPU: bad arguments, a hand-made known answer, the clip's three regions in every GPU case.  GPU: per case the small
outputs at k_gpu <= 2 * k_ref + 2, y and dx bit for bit from the device's own a and g; once: workspace reuse, graph
replay, autograd.  The prints of the GPU test are the figures of DESIGN.md 4.31."""
import ctypes
import functools

import numpy as np
import pytest

from simpledet_amd import _lib

from . import se_block_ref as sr

F = np.float32
P = ctypes.c_void_p(256)   # never dereferenced: every CPU case returns before any launch

ROWS = (     # (N, C, H, W), Cr, input seed, dtypes, (path, split)s, biases, pointers one element off 16 bytes
    ((3, 24, 7, 9), 6, 0, ("f32", "f16"), ((1, 0),), (False, True), False),
    ((2, 8, 40, 50), 2, 1, ("f32", "f16"), ((1, 3),), (False,), False),
    ((1, 1100, 3, 3), 37, 0, ("f32",), ((1, 0),), (False,), False),
    ((2, 16, 1, 1), 4, 0, ("f32", "f16"), ((1, 0), (2, 0)), (False,), False),
    ((2, 32, 14, 14), 8, 0, ("f32", "f16"), ((2, 0),), (False,), False),
    ((2, 24, 13, 21), 6, 0, ("f32", "f16"), ((1, 0), (2, 0)), (False,), True),
)
CASES = [(shape, Cr, seed, dt, path, split, bias, off) for shape, Cr, seed, dts, paths, biases, off in ROWS
         for dt in dts for path, split in paths for bias in biases]
IDS = ["%s-cr%d-%s-path%d-split%d%s%s" % ("x".join(map(str, c[0])), c[1], c[3], c[4], c[5], "-bias" if c[6] else "",
                                          "-off" if c[7] else "") for c in CASES]


@functools.lru_cache(maxsize=None)
def _case(shape, Cr, seed, half, bias):
    return sr.make_case(seed, shape, Cr, half, bias)


# ------------------------------------------------------------------------------------------ CPU --
def _wsb(N, C, Cr, HxW, path=0, split=0):
    return int(_lib.lib().cdll.sd_se_block_workspace_bytes(N, C, Cr, ctypes.c_long(HxW), path, split))


def _entry(name, skip=(), ptr=P, N=2, C=8, Cr=2, HxW=16, path=0, split=0, ws=P, wsb=None):
    """one call of an entry point on pointers that are never followed; skip: the pointer slots passed as NULL"""
    nptr = 9 if "fwd" in name else 13
    a = [None if i in skip else ptr for i in range(nptr)]
    wsb = _wsb(N, C, Cr, HxW, path, split) if wsb is None else wsb
    return _lib.lib().call(name, *a, N, C, Cr, ctypes.c_long(HxW), path, split, ws, ctypes.c_size_t(wsb), None)


@pytest.mark.parametrize("name", ["sd_se_block_fwd", "sd_se_block_fwd_f16", "sd_se_block_bwd", "sd_se_block_bwd_f16"])
def test_entry_points_reject_bad_arguments_without_a_gpu(name):
    E = _lib.SimpleDetOpsError
    call = functools.partial(_entry, name)
    optional = (2, 4) if "fwd" in name else (10, 12)        # b1, b2 / db1, db2
    for i in range(9 if "fwd" in name else 13):
        if i in optional:
            continue
        with pytest.raises(E, match="null pointer") as e:
            call(skip=(i,))
        assert e.value.code == -1
    with pytest.raises(E, match="not aligned"):
        call(ptr=ctypes.c_void_p(257))
    for kw in (dict(N=0), dict(C=0), dict(Cr=-1), dict(HxW=0), dict(path=3), dict(path=-1), dict(split=-1),
               dict(split=1025)):
        with pytest.raises(E) as e:
            call(wsb=1 << 20, **kw)
        assert e.value.code == -1, kw
    for kw in (dict(C=4097), dict(Cr=513), dict(N=2, C=1024, HxW=1 << 20)):
        with pytest.raises(E, match="exceed") as e:
            call(wsb=1 << 30, **kw)
        assert e.value.code == _lib.SD_ERR_UNSUPPORTED, kw
    # path 2 on an image that does not fit in LDS: 64 x 1024 halves are 128 KB, as many floats 256 KB
    big = dict(C=64, HxW=1024 if "f16" not in name else 2048, path=2)
    with pytest.raises(E, match="resident") as e:
        call(**big)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(E, match="workspace too small") as e:
        call(wsb=_wsb(2, 8, 2, 16) - 1)
    assert e.value.code == -4
    with pytest.raises(E, match="workspace too small"):
        call(ws=None)


def test_restatement_known_answer_pins_the_clip_and_the_saturated_gate():
    """One image, planes [1, 3] and [0.5, 1.5]: gap = [2, 1].  w1 rows [-1, 0], [1, 1], [2, 4], [3, 0] give
    z1 = [-2, 3, 8, 6]: below 0, inside, above 6, exactly 6; h = [0, 3, 6, 6].  w2 rows [7, 2, 2, 2] and
    [0, -2, -2, -2] give z2 = [30, -30].  With dy = 1: s = [4, 2]; dz1 = dh under the INCLUSIVE mask [0, 1, 0, 1]."""
    x = F([[[1, 3]], [[0.5, 1.5]]]).reshape(1, 2, 1, 2)
    w1 = F([[-1, 0], [1, 1], [2, 4], [3, 0]])
    w2 = F([[7, 2, 2, 2], [0, -2, -2, -2]])
    dy = np.ones_like(x)
    for fwd, bwd in ((lambda *a: sr.fwd_truth(*a)[0], lambda *a: sr.bwd_truth(*a)[0]), (sr.fwd_ref32, sr.bwd_ref32)):
        f = fwd(x, w1, None, w2, None)
        assert f["gap"].tolist() == [[2.0, 1.0]] and f["z1"].tolist() == [[-2.0, 3.0, 8.0, 6.0]]
        a = f["a"].astype(F)
        assert a[0, 0] == F(1.0) and 0 < a[0, 1] < 1e-12                 # sigmoid(+-30) in float32
        assert f["y"].reshape(-1)[:2].astype(F).tolist() == [1.0, 3.0]    # x * 1
        b = bwd(dy, x, f["gap"].astype(F), f["z1"].astype(F), a, w1, w2)
        d = 2.0 * float(a[0, 1]) * (1.0 - float(a[0, 1]))                # dz2[1]; dz2[0] = 4 * (1 * 0) = 0
        assert all(np.isfinite(v).all() for v in b.values())
        assert b["db2"][0] == 0.0 and b["db2"][1] == pytest.approx(d, rel=1e-6)
        db1 = np.asarray(b["db1"], np.float64)
        assert db1[0] == 0.0 and db1[2] == 0.0 and db1[1] == db1[3] == pytest.approx(-2.0 * d, rel=1e-6)
        assert b["g"][0].tolist() == pytest.approx([(1 + 3) * -2.0 * d / 2, 1 * -2.0 * d / 2], rel=1e-6)


def test_every_gpu_case_reaches_the_three_regions_of_the_clip():
    for shape, Cr, seed, dt, path, split, bias, off in CASES:
        c = _case(shape, Cr, seed, dt == "f16", bias)
        z1 = sr.fwd_truth(c["x"], c["w1"], c["b1"], c["w2"], c["b2"])[0]["z1"]
        assert (z1 < 0).any() and ((z1 > 0) & (z1 < 6)).any() and (z1 > 6).any(), (shape, dt, bias)


# ------------------------------------------------------------------------------------------ GPU --
def _cuda(a, half=False, offset=False):
    """a device copy; offset: the data pointer sits one element off a 16-byte boundary"""
    import torch
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float16 if half else torch.float32)
    if not offset:
        return t.cuda()
    buf = torch.empty(t.numel() + 17, dtype=t.dtype, device="cuda")
    start = 1 + (16 - buf.data_ptr() % 16) % 16 // t.element_size()
    o = buf[start:start + t.numel()].view(t.shape)
    o.copy_(t)
    assert o.data_ptr() % 16 == t.element_size()
    return o


def _np(t):
    return t.detach().float().cpu().numpy()


def _device(c, half, offset=False):
    return {k: _cuda(v, half, offset) for k, v in c.items()}


def _both(se, d, path=0, split=0, ws=None):
    f = se.se_block_forward(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], path, split, workspace=ws)
    b = se.se_block_backward(d["dy"], d["x"], f[1], f[2], f[3], d["w1"], d["w2"], path, split, workspace=ws,
                             bias_grads=(d["b1"] is not None, d["b2"] is not None))
    return f + b        # y, gap, z1, a, dx, g, dw1, db1, dw2, db2


def _same(p, q):
    import torch
    return all((s is None and t is None) or torch.equal(s, t) for s, t in zip(p, q))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hip_paths_against_the_truth(ops, case):
    import torch
    from simpledet_amd import se_block as se
    shape, Cr, seed, dt, path, split, bias, off = case
    half = dt == "f16"
    c = _case(shape, Cr, seed, half, bias)
    d = _device(c, half, off)
    y, gap, z1, a, dx, g, dw1, db1, dw2, db2 = out = _both(se, d, path, split)
    torch.cuda.synchronize()
    want = "resident" if path == 2 else "block" if split else "wave"
    assert want in (_lib.lib().cdll.sd_last_dispatch() or b"").decode()
    ft, fT = sr.fwd_truth(c["x"], c["w1"], c["b1"], c["w2"], c["b2"])
    fr = sr.fwd_ref32(c["x"], c["w1"], c["b1"], c["w2"], c["b2"])
    bt, bT = sr.bwd_truth(c["dy"], c["x"], _np(gap), _np(z1), _np(a), c["w1"], c["w2"])
    br = sr.bwd_ref32(c["dy"], c["x"], _np(gap), _np(z1), _np(a), c["w1"], c["w2"])
    got = dict(gap=gap, z1=z1, a=a, g=g, dw1=dw1, dw2=dw2, db1=db1, db2=db2)
    bad = []
    for o in sr.FWD_OUTPUTS + sr.BWD_OUTPUTS:
        if got[o] is None:
            continue
        truth, T, ref = (ft, fT, fr) if o in sr.FWD_OUTPUTS else (bt, bT, br)
        k, kr = sr.k_of(_np(got[o]), truth[o], T[o]), sr.k_of(ref[o], truth[o], T[o])
        print("se_block %s %-3s k_gpu %.3f k_ref %.3f" % (IDS[CASES.index(case)], o, k, kr))
        if not sr.passes(k, kr):
            bad.append("%s: k_gpu %.3f > 2 * %.3f + 2" % (o, k, kr))
    assert not bad, bad
    np_t = np.float16 if half else F
    an, gn = _np(a).reshape(shape[:2] + (1, 1)), _np(g).reshape(shape[:2] + (1, 1))
    assert np.array_equal(y.cpu().numpy(), (c["x"] * an).astype(F).astype(np_t))
    assert np.array_equal(dx.cpu().numpy(), ((c["dy"] * an).astype(F) + gn).astype(F).astype(np_t))
    if path == 2:       # the resident path against the two-pass path: equal a gives equal y, equal g equal dx
        other = _both(se, d, 1, 0)
        assert torch.equal(a, other[3]) and torch.equal(y, other[0])
        assert torch.equal(dx, other[4]) or not torch.equal(g, other[5])


@pytest.mark.gpu
def test_hip_workspace_reuse_graph_replay_and_autograd(ops):
    import torch
    from simpledet_amd import se_block as se
    shape, Cr = ROWS[0][0], ROWS[0][1]
    d1 = _device(_case(shape, Cr, 0, False, True), False)
    d2 = _device(sr.make_case(5, shape, Cr, False, True), False)
    fresh1, fresh2 = _both(se, d1, 1), _both(se, d2, 1)
    ws = torch.full((se.workspace_bytes(shape[0], shape[1], Cr, shape[2] * shape[3], 1, 0),), 0xA5, dtype=torch.uint8,
                    device="cuda")
    assert _same(_both(se, d1, 1, ws=ws), fresh1) and _same(_both(se, d2, 1, ws=ws), fresh2)
    g_in = {k: v.clone() for k, v in d1.items()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap = _both(se, g_in, 1, ws=ws)
    for src, want in ((d2, fresh2), (d1, fresh1), (d2, fresh2)):
        for k in g_in:
            g_in[k].copy_(src[k])
        for t in cap:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(cap, want)
    leaves = {k: v.clone().requires_grad_() for k, v in d1.items() if k != "dy"}
    y = se.se_block(leaves["x"], leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"])
    grads = torch.autograd.grad(y, [leaves[k] for k in ("x", "w1", "b1", "w2", "b2")], d1["dy"])
    auto = _both(se, d1)
    assert torch.equal(y.detach(), auto[0]) and _same(grads, (auto[4], auto[6], auto[7], auto[8], auto[9]))
