"""_contrib_SigmoidCrossEntropy and the fused mask loss (simpledet_amd/csrc/sigmoid_ce.hip) against the restatements
of tests/sigmoid_ce_ref.py.

  CPU: argument validation of the six C entry points (all fail before any launch), the workspace sizes, the ABI
       version, and the float32 restatement over the sweep (finite, its k_ref printed).
  GPU: exact -- count, count_sum, the +0.0 of ignored elements whatever their logit (NaN, inf), where a NaN at a
       counted element goes, sentinels around every output, equal bits with and without the full-size outputs,
       between two calls, between eager and a replayed graph, between aligned and offset pointers, and between the
       fused op and the drop-in operator on the gathered row;
       within a margin -- loss, loss_sum, out and the gradient:
           k = |got - truth| / (eps32 * T + tiny)                      (tests/sigmoid_ce_ref.py)
       and, per case and per output, k on the GPU must not exceed 2 * k_ref + 2, k_ref = the float32 host
       restatement's k on the same case in the same run: the factor 2 for the free order of the row sum, the 2
       units for the final roundings (expf / logf of the device are allowed a few ulp where glibc's are almost
       always correctly rounded); the same rule and justification as tests/test_focal_loss.py.
       Measured on an MI355X: profiles/mask_loss_time.json, key 'margin'.
"""
import ctypes
import functools

import numpy as np
import pytest

from simpledet_amd import _lib

from . import sigmoid_ce_ref as sr

F = np.float32
P256 = ctypes.c_void_p(256)     # never dereferenced: every case that gets one fails validation first


# ------------------------------------------------------------------------------------------ CPU --
def _ce_fwd(n=2, k=8, ptrs=None, ws=P256, wsb=1 << 20):
    p = [P256] * 7 if ptrs is None else ptrs
    return _lib.lib().call("sd_sigmoid_ce_fwd", *p, ctypes.c_long(n), ctypes.c_long(k), ws, ctypes.c_size_t(wsb), None)


def _ce_bwd(n=2, k=8, ptrs=None, ws=P256, wsb=1 << 20):
    p = [P256] * 5 if ptrs is None else ptrs
    return _lib.lib().call("sd_sigmoid_ce_bwd", *p, ctypes.c_long(n), ctypes.c_long(k), 1.0, ws,
                           ctypes.c_size_t(wsb), None)


def _ml_fwd(R=2, K=3, P=8, ptrs=None, ws=P256, wsb=1 << 20):
    p = [P256] * 5 if ptrs is None else ptrs
    return _lib.lib().call("sd_mask_loss_fwd", *p, R, K, ctypes.c_long(P), ws, ctypes.c_size_t(wsb), None)


def _ml_bwd(R=2, K=3, P=8, ptrs=None, ws=P256, wsb=1 << 20):
    p = [P256] * 4 if ptrs is None else ptrs
    return _lib.lib().call("sd_mask_loss_bwd", *p, R, K, ctypes.c_long(P), 1.0, ws, ctypes.c_size_t(wsb), None)


def _null_at(n, i):
    return [None if j == i else P256 for j in range(n)]


def test_abi_version_is_12():
    assert _lib.lib().cdll.sd_abi_version() == 12 == _lib.header_abi_version()


def test_dropin_entry_points_reject_bad_arguments():
    for fn in (_ce_fwd, _ce_bwd):
        for kw in (dict(n=-1), dict(k=-1)):
            with pytest.raises(_lib.SimpleDetOpsError, match="negative dimension"):
                fn(**kw)
        with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small") as e:
            fn(wsb=8)
        assert e.value.code == -4
        with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small"):
            fn(ws=None)
        # 2^31 - 1 elements is the limit: 65536 x 32768 = 2^31
        with pytest.raises(_lib.SimpleDetOpsError, match="exceed the limit") as e:
            fn(n=65536, k=32768)
        assert e.value.code == _lib.SD_ERR_UNSUPPORTED
        with pytest.raises(_lib.SimpleDetOpsError, match="exceed the limit"):
            fn(n=1, k=1 << 31)
    # null pointers, per position.  forward: data label out loss loss_sum count count_sum -- loss / count may be null
    for i in (0, 1, 2, 4, 6):
        with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
            _ce_fwd(ptrs=_null_at(7, i))
    # backward: data label d_data count count_sum -- count may be null
    for i in (0, 1, 2, 4):
        with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
            _ce_bwd(ptrs=_null_at(5, i))
    # empty problems succeed without touching the device (no pointer, no workspace), the sizes still checked
    for fn, np_ in ((_ce_fwd, 7), (_ce_bwd, 5)):
        assert fn(n=0, ptrs=[None] * np_, ws=None, wsb=0) == 0
        assert fn(k=0, ptrs=[None] * np_, ws=None, wsb=0) == 0
        with pytest.raises(_lib.SimpleDetOpsError, match="negative dimension"):
            fn(n=0, k=-1, ptrs=[None] * np_, ws=None, wsb=0)


def test_fused_entry_points_reject_bad_arguments():
    for fn, np_ in ((_ml_fwd, 5), (_ml_bwd, 4)):
        for kw in (dict(R=-1), dict(K=-1), dict(P=-1)):
            with pytest.raises(_lib.SimpleDetOpsError, match="negative dimension"):
                fn(**kw)
        for i in range(np_):
            with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
                fn(ptrs=_null_at(np_, i))
        with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small") as e:
            fn(wsb=8)
        assert e.value.code == -4
        with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small"):
            fn(ws=None)
        with pytest.raises(_lib.SimpleDetOpsError, match="exceed the limit") as e:     # 1024 x 2048 x 1024 = 2^31
            fn(R=1024, K=2048, P=1024)
        assert e.value.code == _lib.SD_ERR_UNSUPPORTED
        for kw in (dict(R=0), dict(K=0), dict(P=0)):
            assert fn(ptrs=[None] * np_, ws=None, wsb=0, **kw) == 0
        with pytest.raises(_lib.SimpleDetOpsError, match="negative dimension"):
            fn(R=0, P=-1, ptrs=[None] * np_, ws=None, wsb=0)


def test_workspace_sizes_are_monotone():
    l = _lib.lib().cdll
    ce = lambda n, k: int(l.sd_sigmoid_ce_workspace_bytes(ctypes.c_long(n), ctypes.c_long(k)))
    ml = lambda R, K, P: int(l.sd_mask_loss_workspace_bytes(R, K, ctypes.c_long(P)))
    ns, ks = (0, 1, 2, 5, 300, 4096), (0, 1, 7, 255, 256, 257, 1023, 4096, 70001, 200704)
    for k in ks:
        sizes = [ce(n, k) for n in ns]
        assert sizes == sorted(sizes) and sizes[0] >= 4
    for n in ns:
        sizes = [ce(n, k) for k in ks]
        assert sizes == sorted(sizes)
    # a unit of 256 elements holds a float and an int
    assert ce(1, 200704) >= 8 * 784 and ce(300, 7) >= 8 * 300
    Rs, Ps = (0, 1, 8, 256, 1024), (0, 1, 15, 196, 784)
    for P in Ps:
        for K in (1, 81):
            sizes = [ml(R, K, P) for R in Rs]
            assert sizes == sorted(sizes)
    for R in Rs:
        sizes = [ml(R, 81, P) for P in Ps]
        assert sizes == sorted(sizes)
        assert ml(R, 1, 784) <= ml(R, 81, 784)
    # the fused op reduces the gathered row: the drop-in operator's size at n = 1, k = R * P
    assert ml(256, 81, 784) == ce(1, 256 * 784)


@functools.lru_cache(maxsize=None)
def _dropin():
    return sr.dropin_cases()


@functools.lru_cache(maxsize=None)
def _fused():
    return sr.fused_cases()


@functools.lru_cache(maxsize=None)
def _k_ref(name):
    """the float32 host restatement's own k per output on one case (fused cases: on the gathered row)"""
    for nm, c in _dropin():
        if nm == name:
            return sr.k_ref(c["x"], c["t"], c["scale"])
    for nm, c in _fused():
        if nm == name:
            x, t, _ = sr.gather(c["logits"], c["cls"], c["target"])
            return sr.k_ref(x, t, c["scale"])
    raise KeyError(name)


def test_restatement_is_finite_over_the_sweep():
    """The float32 restatement: an element is expf, 1 +, logf, a double product and sum rounded once (under 4
    units of eps32 * T); the gradient expf, a double quotient rounded once, / and * (under 4 units)."""
    for name, c in list(_dropin()) + list(_fused()):
        k = _k_ref(name)
        print("%-16s k_ref " % name + "  ".join("%s %.3f" % (o, k[o]) for o in sr.OUTPUTS))
        assert all(np.isfinite(k[o]) for o in sr.OUTPUTS), (name, k)
        if name in dict(_dropin()):
            r = sr.f32(c["x"], c["t"], c["scale"])
            assert all(np.all(np.isfinite(r[o])) for o in r), name
    # a known answer: x = 0, t = 1 -> loss ln 2, gradient -0.5 / count_sum; a row of -1 -> exactly 0 over 1e-5
    r = sr.f32(F([[0.0, 5.0], [1.0, 2.0]]), F([[1.0, -1.0], [-1.0, -1.0]]), 2.0)
    assert r["loss"][0, 0] == F(np.log(2.0)) and r["loss"][0, 1] == 0 and r["count_sum"][0] == F(1) + F(1e-5)
    assert r["d"][0, 0] == F(F(-0.5) / r["count_sum"][0]) * F(2) and r["d"][0, 1] == 0
    assert r["out"][1] == 0 and r["count_sum"][1] == F(1e-5) and not r["d"][1].any()


# ------------------------------------------------------------------------------------------ GPU --
SENT = -777.25


class Guarded:
    """a device tensor of `shape` with four sentinel floats on either side; offset: its data pointer sits 4 bytes
    off its 16-byte boundary (scalar path)"""

    def __init__(self, shape, offset=False, src=None):
        import torch
        n = int(np.prod(shape))
        self.lead = 5 if offset else 4
        self.buf = torch.full((n + 12,), SENT, dtype=torch.float32, device="cuda")
        self.t = self.buf[self.lead:self.lead + n].view(tuple(shape))
        if src is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(src, F)).view(tuple(shape)))
        else:
            self.t.fill_(float("nan"))
        assert self.t.data_ptr() % 16 == (4 if offset else 0)

    def check(self, what):
        n = self.t.numel()
        g = self.buf.cpu().numpy()
        assert np.all(g[:self.lead] == F(SENT)) and np.all(g[self.lead + n:] == F(SENT)), what + ": sentinel overwritten"
        return g[self.lead:self.lead + n].reshape(tuple(self.t.shape))


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def _run_dropin(ops, c, offset=False, full=True):
    """forward (with the full-size outputs or without) and backward -> dict of numpy arrays, sentinels checked"""
    x, t = c["x"], c["t"]
    n = x.shape[0]
    gx, gt = Guarded(x.shape, offset, x), Guarded(t.shape, offset, t)
    o = {k: Guarded((n,)) for k in ("out", "loss_sum", "count_sum", "bwd_count_sum")}
    o.update({k: Guarded(x.shape, offset) for k in ("d",) + (("loss", "count", "bwd_count") if full else ())})
    ops.sigmoid_cross_entropy_forward(gx.t, gt.t, out=o["out"].t, loss_sum=o["loss_sum"].t, count_sum=o["count_sum"].t,
                                      loss=o["loss"].t if full else None, count=o["count"].t if full else None)
    ops.sigmoid_cross_entropy_backward(gx.t, gt.t, c["scale"], d_data=o["d"].t, count_sum=o["bwd_count_sum"].t,
                                       count=o["bwd_count"].t if full else None)
    res = {k: g.check(k) for k, g in o.items()}
    assert np.array_equal(_bits(gx.check("data")), _bits(x)) and np.array_equal(gt.check("label"), t)
    return res


def _exact_checks(name, c, got):
    t = c["t"]
    on = t != F(-1)
    np.testing.assert_array_equal(got["count"], on.astype(F), err_msg=name)
    np.testing.assert_array_equal(got["bwd_count"], on.astype(F), err_msg=name)
    cs = sr.count_sum_f32(t)
    np.testing.assert_array_equal(got["count_sum"], cs, err_msg=name)
    np.testing.assert_array_equal(got["bwd_count_sum"], cs, err_msg=name)
    assert not _bits(got["loss"])[~on].any() and not _bits(got["d"])[~on].any(), name + ": ignored element not +0.0"
    empty = ~on.any(axis=1)
    assert not _bits(got["out"])[empty].any() and not _bits(got["loss_sum"])[empty].any(), name
    assert np.all(got["count_sum"][empty] == F(1e-5))


def _margin(name, got, truth, T, kr, outputs=sr.OUTPUTS):
    worst = {}
    for o in outputs:
        k = sr.k_of(got[o], truth[o], T[o])
        worst[o] = k
        print("%-16s %-8s k_ref %.3f  k_gpu %.3f  bound %.3f" % (name, o, kr[o], k, 2 * kr[o] + 2))
    for o in outputs:
        assert worst[o] <= 2 * kr[o] + 2, "%s %s: k_gpu %.3f > 2 * %.3f + 2" % (name, o, worst[o], kr[o])
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", [d[0] for d in sr.DROPIN])
def test_hip_dropin_exact_and_margin(ops, name):
    c = dict(_dropin())[name]
    got = _run_dropin(ops, c)
    _exact_checks(name, c, got)
    truth, T = sr.truth(c["x"], c["t"], c["scale"])
    _margin(name, got, truth, T, _k_ref(name))
    if name.endswith("-row"):
        r = c["t"].shape[0] // 2
        assert not _bits(got["out"])[r] and got["count_sum"][r] == F(1e-5) and not _bits(got["d"])[r].any()
    # two calls, and a call without the full-size outputs: equal bits
    again = _run_dropin(ops, c)
    lean = _run_dropin(ops, c, full=False)
    for o in got:
        assert np.array_equal(_bits(got[o]), _bits(again[o])), (name, o)
    for o in lean:
        assert np.array_equal(_bits(got[o]), _bits(lean[o])), (name, o)
    # pointers 4 bytes off their 16-byte boundary (the scalar path): equal bits
    off = _run_dropin(ops, c, offset=True)
    for o in got:
        assert np.array_equal(_bits(got[o]), _bits(off[o])), (name, o)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [False, True])
def test_hip_ignored_logits_are_not_looked_at_and_nan_stays_in_its_row(ops, offset):
    c = dict(dict(_dropin())["rows4096"])
    x, t = c["x"].copy(), c["t"]
    clean = _run_dropin(ops, c, offset)
    ign = np.argwhere(t == F(-1))
    assert len(ign) > 30
    for j, (r, col) in enumerate(ign):
        x[r, col] = (np.nan, np.inf, -np.inf)[j % 3]
    c["x"] = x
    got = _run_dropin(ops, c, offset)
    for o in got:        # nothing changes at all: the ignored logits are never looked at
        assert np.array_equal(_bits(got[o]), _bits(clean[o])), o
    assert np.all(np.isfinite(got["out"]))
    assert not _bits(got["loss"])[t == F(-1)].any() and not _bits(got["d"])[t == F(-1)].any()
    # a NaN at a COUNTED element: that element and its row's sums, nothing else
    r, col = np.argwhere(t != F(-1))[4099 % 4096 + 2 * 4096]
    assert r == 2
    x[r, col] = np.nan
    got = _run_dropin(ops, c, offset)
    for o in ("loss", "d"):
        nan = np.isnan(got[o])
        assert nan[r, col] and nan.sum() == 1, o
        keep = ~nan
        assert np.array_equal(_bits(got[o])[keep], _bits(clean[o])[keep]), o
    for o in ("out", "loss_sum"):
        assert np.isnan(got[o][r]) and np.isnan(got[o]).sum() == 1
        assert np.array_equal(_bits(np.delete(got[o], r)), _bits(np.delete(clean[o], r)))
    assert np.array_equal(got["count_sum"], clean["count_sum"])


def _run_fused(ops, c, off_in=False, off_out=False):
    gl, gt = Guarded(c["logits"].shape, off_in, c["logits"]), Guarded(c["target"].shape, off_in, c["target"])
    gc = Guarded(c["cls"].shape, False, c["cls"])
    o = dict(out=Guarded((1,)), count_sum=Guarded((1,)), d=Guarded(c["logits"].shape, off_out))
    ops.mask_loss_forward(gl.t, gc.t, gt.t, out=o["out"].t, count_sum=o["count_sum"].t)
    ops.mask_loss_backward(gl.t, gc.t, gt.t, c["scale"], d_logits=o["d"].t)
    res = {k: g.check(k) for k, g in o.items()}
    assert np.array_equal(_bits(gl.check("logits")), _bits(c["logits"]))
    return res, (gl.t, gc.t, gt.t)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [f[0] for f in sr.FUSED])
def test_hip_fused_equals_the_dropin_on_the_gathered_row(ops, name):
    import torch
    c = dict(_fused())[name]
    R, K, P = c["logits"].shape
    got, (tl, tc, tt) = _run_fused(ops, c)
    x, t, plane = sr.gather(c["logits"], c["cls"], c["target"])
    # every plane that is not selected, and every rejected row, is exactly +0.0
    sel = np.zeros((R, K), bool)
    sel[np.arange(R)[plane >= 0], plane[plane >= 0]] = True
    assert (plane < 0).any() and sel.any()
    assert not _bits(got["d"])[~sel].any(), name
    # bit-equal to the drop-in operator on the torch-gathered, flattened row, rejected rows' targets set to -1
    ok = torch.from_numpy(plane >= 0).cuda()
    idx = torch.from_numpy(np.maximum(plane, 0)).cuda()
    row = tl[torch.arange(R, device="cuda"), idx].reshape(1, -1).contiguous()
    assert np.array_equal(_bits(row.cpu().numpy())[:, np.repeat(plane >= 0, P)], _bits(x)[:, np.repeat(plane >= 0, P)])
    trow = torch.where(ok[:, None], tt, torch.full_like(tt, -1.0)).reshape(1, -1).contiguous()
    out, _, cs = ops.sigmoid_cross_entropy_forward(row, trow)
    d, cs2 = ops.sigmoid_cross_entropy_backward(row, trow, c["scale"])
    assert np.array_equal(_bits(got["out"]), _bits(out.cpu().numpy())), name
    assert np.array_equal(_bits(got["count_sum"]), _bits(cs.cpu().numpy())) and torch.equal(cs, cs2)
    assert got["count_sum"][0] == sr.count_sum_f32(t)[0]
    picked = got["d"][np.arange(R)[plane >= 0], plane[plane >= 0]]
    assert np.array_equal(_bits(picked), _bits(d.cpu().numpy().reshape(R, P)[plane >= 0])), name
    # ... and within the margin of the truth
    truth, T = sr.truth(x, t, c["scale"])
    dense = np.where(sel[:, :, None], got["d"], 0).sum(axis=1).reshape(1, -1)
    _margin(name, dict(out=got["out"], d=dense), truth, T, _k_ref(name), outputs=("out", "d"))
    # two calls; pointers 4 bytes off (inputs and outputs together, then one side at a time): equal bits
    for off_in, off_out in ((False, False), (True, True), (True, False), (False, True)):
        other, _ = _run_fused(ops, c, off_in, off_out)
        for o in got:
            assert np.array_equal(_bits(got[o]), _bits(other[o])), (name, o, off_in, off_out)


@pytest.mark.gpu
def test_hip_capture_and_replay_give_equal_bits(ops):
    import torch
    c = dict(_dropin())["workload"]
    f = dict(_fused())["head"]
    x, t = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["t"]).cuda()
    lg, cl, tg = (torch.from_numpy(f[k]).cuda() for k in ("logits", "cls", "target"))

    def run(ws=(None,) * 4):
        a = ops.sigmoid_cross_entropy_forward(x, t, full=True, workspace=ws[0])
        b = ops.sigmoid_cross_entropy_backward(x, t, c["scale"], workspace=ws[1])
        m = ops.mask_loss_forward(lg, cl, tg, workspace=ws[2])
        d = ops.mask_loss_backward(lg, cl, tg, f["scale"], workspace=ws[3])
        return tuple(a) + tuple(b) + tuple(m) + (d,)
    eager = tuple(e.clone() for e in run())
    wss = [torch.empty(n, dtype=torch.uint8, device="cuda")
           for n in (ops.sigmoid_cross_entropy_workspace_bytes(*c["x"].shape),) * 2
           + (ops.mask_loss_workspace_bytes(*f["logits"].shape),) * 2]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap = run(wss)
    for _ in range(2):
        for o in cap:
            o.fill_(float("nan"))
        for w in wss:
            w.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        for e, g in zip(eager, cap):
            assert torch.equal(e.view(torch.int32), g.view(torch.int32))


@pytest.mark.gpu
def test_autograd_functions_ignore_the_incoming_gradient(ops):
    import torch
    from simpledet_amd import contrib
    f = dict(_fused())["head"]
    lg = torch.from_numpy(f["logits"]).cuda().view(8, 81, 28, 28).requires_grad_()
    cl, tg = torch.from_numpy(f["cls"]).cuda(), torch.from_numpy(f["target"]).cuda().view(8, 28, 28)
    out = contrib.mask_loss(lg, cl, tg, grad_scale=f["scale"])
    assert out.shape == (1,)
    (out * 3.0).sum().backward()              # a loss operator: the head gradient is NOT used
    x, t, plane = sr.gather(f["logits"], f["cls"], f["target"])
    truth, T = sr.truth(x, t, f["scale"])
    g = lg.grad.cpu().numpy().reshape(8, 81, 784)
    sel = np.zeros((8, 81), bool)
    sel[np.arange(8)[plane >= 0], plane[plane >= 0]] = True
    assert not _bits(g)[~sel].any()
    dense = np.where(sel[:, :, None], g, 0).sum(axis=1).reshape(1, -1)
    _margin("autograd", dict(out=out.detach().cpu().numpy(), d=dense), truth, T, _k_ref("head"), outputs=("out", "d"))
    assert torch.equal(lg.grad.view(8, 81, 784), ops.mask_loss_backward(lg.detach(), cl, tg, f["scale"]).view(8, 81, 784))
    # the drop-in operator with autograd
    c = dict(_dropin())["rows1023"]
    xd = torch.from_numpy(c["x"]).cuda().requires_grad_()
    td = torch.from_numpy(c["t"]).cuda()
    o = contrib.sigmoid_cross_entropy(xd, td, grad_scale=c["scale"])
    o.backward(torch.randn_like(o))
    raw = ops.sigmoid_cross_entropy_forward(xd.detach(), td)
    assert torch.equal(o.detach(), raw[0])
    assert torch.equal(xd.grad, ops.sigmoid_cross_entropy_backward(xd.detach(), td, c["scale"])[0])


@pytest.mark.gpu
def test_empty_rows_give_the_empty_sums(ops):
    import torch
    x = torch.empty((3, 0), device="cuda")
    out, loss_sum, count_sum = ops.sigmoid_cross_entropy_forward(x, x)
    assert not out.any() and not loss_sum.any() and torch.all(count_sum == 1e-5) and out.shape == (3,)
    d, cs = ops.sigmoid_cross_entropy_backward(x, x, 128.0)
    assert d.shape == (3, 0) and torch.all(cs == 1e-5)
    out, cs = ops.mask_loss_forward(torch.empty((0, 81, 784), device="cuda"), torch.empty(0, device="cuda"),
                                    torch.empty((0, 784), device="cuda"))
    assert float(out) == 0.0 and float(cs) == float(np.float32(1e-5))
