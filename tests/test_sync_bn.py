"""_contrib_SyncBatchNorm (simpledet_amd/csrc/sync_bn.hip) against the restatements of tests/sync_bn_ref.py.

  CPU: known answers of the restatements; the contract's float32 arithmetic against the float64 truths; the
       workspace size is monotone in N and C; every entry point rejects bad arguments before any launch; the
       wrappers refuse what the kernels do not take.
  GPU: 1. the statistics (mean, var, bpart), per case and output:  k = |got - truth| / (eps32 * T + tiny),
              k_gpu <= 2 * k_ref(case) + 2      and      k_gpu <= 2 * (max k_ref over the zero-offset cases of the
          shape) + 2 on EVERY case, so that a displaced mean costs nothing; the constant channel exactly;
       2. everything behind the statistics bit for bit against *_contract32 fed with the device's own partials, and
          y / dx against the truth under the bound of 1; the inference forward bit for bit;
       3. W = 2, 3 ranks simulated on one GPU by slicing the N = 6 cases;
       4. the split path is taken where it should be and only there;
       5. equal bits over repeated calls, at pointers off their 16-byte boundary, and under graph replay on changed
          inputs;
       6. the _f16 entry points equal cast -> fp32 -> cast bit for bit;
       7. the autograd wrapper against torch.nn.functional.batch_norm differentiated in float64.
  Measured on an MI355X (the prints of the tests): see DESIGN.md 4.24 and profiles/sync_bn_time.json 'margin'.
"""
import ctypes
import functools

import numpy as np
import pytest

from simpledet_amd import _lib

from . import sync_bn_ref as sr

F = np.float32
P = ctypes.c_void_p(256)   # never dereferenced: every CPU case returns before any launch
EXTRA_SHAPES = ((2, 3, 40, 40),)   # 400 items of 8: a workgroup per channel, between the wave and the split path


# ------------------------------------------------------------------------------------------ CPU --
def _wsb(N, C, HxW):
    return int(_lib.lib().cdll.sd_sync_bn_workspace_bytes(N, C, ctypes.c_long(HxW)))


def _dims(kw):
    N, C, HxW = kw.pop("N", 2), kw.pop("C", 8), kw.pop("HxW", 16)
    ws, ptr = kw.pop("ws", P), kw.pop("ptr", P)
    wsb = kw.pop("wsb", None)
    wsb = _wsb(N, C, HxW) if wsb is None else wsb
    return N, C, HxW, ptr, ws, wsb


def _ptrs(n, ptr, skip):
    return [None if i in skip else ptr for i in range(n)]


def _stats(f16=False, skip=(), **kw):
    N, C, HxW, ptr, ws, wsb = _dims(kw)
    a = _ptrs(2, ptr, skip)
    return _lib.lib().call("sd_sync_bn_stats" + ("_f16" if f16 else ""), *a, N, C, ctypes.c_long(HxW), ws,
                           ctypes.c_size_t(wsb), None)


def _apply(f16=False, skip=(), W=1, **kw):
    N, C, HxW, ptr, ws, wsb = _dims(kw)
    a = _ptrs(7, ptr, skip)     # x, parts, gamma, beta, y, mean, var
    return _lib.lib().call("sd_sync_bn_apply" + ("_f16" if f16 else ""), a[0], a[1], W, *a[2:], N, C,
                           ctypes.c_long(HxW), ctypes.c_float(1e-3), 1, ws, ctypes.c_size_t(wsb), None)


def _infer(f16=False, skip=(), **kw):
    N, C, HxW, ptr, ws, wsb = _dims(kw)
    a = _ptrs(6, ptr, skip)
    return _lib.lib().call("sd_sync_bn_infer_fwd" + ("_f16" if f16 else ""), *a, N, C, ctypes.c_long(HxW),
                           ctypes.c_float(1e-3), 1, None)


def _bstats(f16=False, skip=(), **kw):
    N, C, HxW, ptr, ws, wsb = _dims(kw)
    a = _ptrs(4, ptr, skip)
    return _lib.lib().call("sd_sync_bn_bwd_stats" + ("_f16" if f16 else ""), *a, N, C, ctypes.c_long(HxW), ws,
                           ctypes.c_size_t(wsb), None)


def _bapply(f16=False, skip=(), W=1, rank=0, dgamma=P, dbeta=P, mm=P, mv=P, **kw):
    N, C, HxW, ptr, ws, wsb = _dims(kw)
    a = _ptrs(7, ptr, skip)     # dy, x, mean, var, gamma, bparts, dx
    return _lib.lib().call("sd_sync_bn_bwd_apply" + ("_f16" if f16 else ""), *a[:6], W, rank, a[6], dgamma, dbeta,
                           mm, mv, ctypes.c_float(0.9), N, C, ctypes.c_long(HxW), ctypes.c_float(1e-3), 1, ws,
                           ctypes.c_size_t(wsb), None)


ENTRY = {"stats": (_stats, 2, True), "apply": (_apply, 7, True), "infer_fwd": (_infer, 6, False),
         "bwd_stats": (_bstats, 4, True), "bwd_apply": (_bapply, 7, True)}


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_entry_points_reject_bad_arguments_without_a_gpu(entry, f16):
    E = _lib.SimpleDetOpsError
    call, nptr, has_ws = ENTRY[entry]
    call = functools.partial(call, f16)
    for kw in (dict(N=-1), dict(C=-8), dict(HxW=-1)):
        with pytest.raises(E, match="negative dimension") as e:
            call(**kw)
        assert e.value.code == -1
    for i in range(nptr):
        with pytest.raises(E, match="null pointer") as e:
            call(skip=(i,))
        assert e.value.code == -1
    if has_ws:
        with pytest.raises(E, match="workspace too small") as e:
            call(wsb=_wsb(2, 8, 16) - 1)
        assert e.value.code == -4
        with pytest.raises(E, match="workspace too small"):
            call(ws=None)
    # 2^31 - 1 elements is the stated limit: 2 x 1024 x 1048576 = 2^31
    with pytest.raises(E, match="exceed the limit") as e:
        call(N=2, C=1024, HxW=1 << 20, wsb=1 << 30)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(E, match="exceed the limit"):
        call(N=1 << 20, C=1 << 20, HxW=1 << 40, wsb=1 << 30)
    # a pointer off its element alignment
    with pytest.raises(E, match="not aligned"):
        call(ptr=ctypes.c_void_p(257))
    # empty problems succeed without touching the device (no pointer, no workspace)
    for kw in (dict(N=0), dict(C=0), dict(HxW=0)):
        extra = dict(dgamma=None, dbeta=None, mm=None, mv=None) if entry == "bwd_apply" else {}
        assert call(ptr=None, ws=None, wsb=0, **kw, **extra) == 0
    if entry in ("apply", "bwd_apply"):
        for W in (0, -2):
            with pytest.raises(E, match="at least one") as e:
                call(W=W)
            assert e.value.code == -1
        with pytest.raises(E, match="at least one"):       # ... checked on an empty problem too
            call(W=0, N=0)
    if entry == "bwd_apply":
        for W, rank in ((1, 1), (1, -1), (3, 3)):
            with pytest.raises(E, match="rank=") as e:
                call(W=W, rank=rank)
            assert e.value.code == -1
        assert call(W=3, rank=2, N=0) == 0
        for kw in (dict(dgamma=None), dict(dbeta=None), dict(mm=None), dict(mv=None)):
            with pytest.raises(E, match="together") as e:
                call(**kw)
            assert e.value.code == -1


def test_workspace_bytes_is_monotone_in_n_and_c():
    for HxW in (1, 45, 64, 196, 16800, 67200):
        prev = 0
        for N in (1, 2, 3, 6, 8, 64, 1024):
            if N * 256 * HxW >= 1 << 31:
                continue
            b = _wsb(N, 256, HxW)
            assert b >= prev
            prev = b
        prev = 0
        for C in (1, 2, 8, 64, 256, 2048):
            if 2 * C * HxW >= 1 << 31:
                continue
            b = _wsb(2, C, HxW)
            assert b >= prev
            prev = b
    assert _wsb(2, 256, 67200) >= 256 * 16                  # the per-channel coefficients
    assert 0 < _wsb(0, 256, 49) <= 4096 and 0 < _wsb(2, -1, 49) <= 4096


def test_restatement_known_answers():
    """x = [1, 3] in one channel, gamma = 2, beta = 1, eps = 0: mean 2, var 1, y = [-1, 3]; dy = [1, 0]:
    sum dy = 1, sum dy * (x - mean) = -1, dx = 2 * dy - 2 * (-1 / 2) * (x - 2) - 2 * (1 / 2) = [0, 0] (the gradient
    of a two-point normalisation vanishes), dgamma = -1, dbeta = 1.  Over two ranks of one element each the rank
    means are 1 and 3 and the rank variances 0: the combine gives mean 2, var 1 again."""
    x = F([1.0, 3.0]).reshape(2, 1)
    g, b, dy = F([2.0]), F([1.0]), F([1.0, 0.0]).reshape(2, 1)
    for W in (1, 2):
        for f in (sr.fwd_ref32, lambda *a: sr.fwd_truth(*a)[0]):
            r = f(x, g, b, 0.0, False, W)
            assert r["mean"].item() == 2.0 and r["var"].item() == 1.0 and r["y"].reshape(-1).tolist() == [-1.0, 3.0]
            assert f(x, g, b, 0.0, True, W)["y"].reshape(-1).tolist() == [0.0, 2.0]          # fix_gamma: g = 1
        for f in (sr.bwd_ref32, lambda *a: sr.bwd_truth(*a)[0]):
            r = f(dy, x, F([2.0]), F([1.0]), g, 0.0, False, W)
            assert r["dx"].reshape(-1).tolist() == [0.0, 0.0]
            assert r["dgamma"].item() == -1.0 and r["dbeta"].item() == 1.0
            assert r["bpart"].sum(axis=0).reshape(-1).tolist() == [1.0, -1.0]
            assert f(dy, x, F([2.0]), F([1.0]), g, 0.0, True, W)["dgamma"].item() == 0.0
    T = sr.bwd_truth(dy, x, F([2.0]), F([1.0]), g, 0.0, False)[1]
    # TSG = 1, TSP = 1 * (1 + 2) = 3: first element 2 * 1 + 2 * (3 / 2) * (1 + 2) + 2 * (1 / 2) = 12
    assert T["dx"].reshape(-1)[0] == 12.0 and T["dgamma"].item() == 3.0 and T["dbeta"].item() == 1.0
    # the contract: the combine of two ranks, and the element rules from per-channel statistics
    parts = F([[[1.0], [0.0]], [[3.0], [0.0]]])
    m, v = sr.combine_contract(parts)
    assert m.item() == 2.0 and v.item() == 1.0
    m1, v1 = sr.combine_contract(F([[[2.0], [1.0]]]))
    assert m1.item() == 2.0 and v1.item() == 1.0                                              # W = 1: a copy
    assert sr.fwd_contract32(x, m, v, g, b, 0.0, False).reshape(-1).tolist() == [-1.0, 3.0]
    r = sr.bwd_contract32(dy, x, m, v, g, F([[[1.0], [-1.0]]]), 0, 2, 0.0, False, F([0.0]), F([1.0]), 0.5)
    assert r["dx"].reshape(-1).tolist() == [0.0, 0.0] and r["dgamma"].item() == -1.0 and r["dbeta"].item() == 1.0
    assert r["moving_mean"].item() == 1.0 and r["moving_var"].item() == 1.0
    # inference: a = 2 / sqrt(4) = 1, b = 1 - (2 * 2) / 2 = -1
    assert sr.infer_contract32(x, g, b, F([2.0]), F([4.0]), 0.0, False).reshape(-1).tolist() == [0.0, 2.0]


@functools.lru_cache(maxsize=None)
def _cases():
    return sr.cases()


@functools.lru_cache(maxsize=None)
def _evaluated(W=1):
    """[(name, case, truth, T, k_ref, mean32, var32)]; W > 1: the N = 6 cases only"""
    return [(name, c) + sr.evaluate(c, W) for name, c in _cases() if W == 1 or c["x"].shape[0] == 6]


def _zero_ref(ev, outputs):
    """per shape and output: max k_ref over the zero-offset cases"""
    z = {}
    for _, c, _, _, k_ref, _, _ in ev:
        if c["offset"] == 0.0:
            for o in outputs:
                key = (c["x"].shape, o)
                z[key] = max(z.get(key, 0.0), k_ref[o])
    return z


def test_contract32_against_the_truths():
    """The contract's float32 arithmetic, fed with the float32 roundings of the TRUE statistics (so that only the
    element rules are looked at), against the float64 truths: k <= 2 * k_ref + 2 and the zero-offset cap, on every
    case for W = 1 and on the small N = 6 shapes for W = 2, 3 (the rules are per element: the split shape adds
    nothing here but time; the GPU tests run it at every W).  The reference restatement stays finite over the
    sweep; its k is printed."""
    for W in (1, 2, 3):
        ev = _evaluated(1) if W == 1 else [(name, c) + sr.evaluate(c, W) for name, c in _cases()
                                            if c["x"].shape[0] == 6 and c["x"].size < 20000]
        zero = _zero_ref(ev, ("y", "dx", "dgamma"))
        worst = {o: (0.0, 0.0, None) for o in ("y", "dx", "dgamma")}
        kr = {o: 0.0 for o in sr.OUTPUTS}
        for name, c, truth, T, k_ref, mean32, var32 in ev:
            for o in sr.OUTPUTS:
                assert np.isfinite(k_ref[o]), (name, o)
                kr[o] = max(kr[o], k_ref[o])
            n_rank = sr.count(c["x"]) // W
            bparts = truth["bpart"].astype(F)
            got = dict(y=sr.fwd_contract32(c["x"], mean32, var32, c["gamma"], c["beta"], c["eps"], c["fix_gamma"]))
            dxs, dg = [], 0.0
            for r, (dr, xr) in enumerate(zip(sr.slices(c["dy"], W), sr.slices(c["x"], W))):
                b = sr.bwd_contract32(dr, xr, mean32, var32, c["gamma"], bparts, r, n_rank, c["eps"], c["fix_gamma"])
                dxs.append(b["dx"])
                dg = dg + b["dgamma"].astype(np.float64)
            got.update(dx=np.concatenate(dxs), dgamma=dg)
            for o in worst:
                k = sr.k_of(got[o], truth[o], T[o])
                if k > worst[o][0]:
                    worst[o] = (k, k_ref[o], name)
                assert k <= 2 * k_ref[o] + 2, (W, name, o, k, k_ref[o])
                assert k <= 2 * zero[(c["x"].shape, o)] + 2, (W, name, o, k, zero[(c["x"].shape, o)])
        print("W=%d contract worst k: %s" % (W, "  ".join("%s %.3f (k_ref %.3f, %s)" % ((o,) + w) for o, w in worst.items())))
        print("W=%d k_ref max: %s" % (W, "  ".join("%s %.3g" % (o, kr[o]) for o in sr.OUTPUTS)))
    # the constant channel: variance exactly 0 in the truth and the restatement
    name, c, truth, T, k_ref, mean32, var32 = _evaluated(1)[-1]
    assert name == "constant" and mean32[1] == 1.5 and var32[1] == 0.0
    r = sr.fwd_ref32(c["x"], c["gamma"], c["beta"], c["eps"], False)
    assert r["mean"][1] == 1.5 and r["var"][1] == 0.0


def test_wrappers_refuse_what_the_kernels_do_not_take():
    import torch
    from simpledet_amd import ops
    x = torch.zeros(2, 4, 3, 3)
    v = torch.zeros(4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sync_batch_norm_forward(x, v, v)
    with pytest.raises(TypeError, match="float32 or float16"):
        ops.sync_bn_stats(x.double())
    with pytest.raises(ValueError, match="batch, channel"):
        ops.sync_bn_stats(torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sync_batch_norm_backward(x, x, v, v, v)
    with pytest.raises(TypeError):
        ops.sync_batch_norm_forward(x, v, v, 1e-3)          # eps, fix_gamma, gather are keyword-only


# ------------------------------------------------------------------------------------------ GPU --
def _cuda(a, offset=False, dtype=None):
    """a device copy; offset: the data pointer sits one element off a 16-byte boundary (4 bytes, 2 for halves)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    if not offset:
        return t.cuda()
    buf = torch.empty(t.numel() + 9, dtype=t.dtype, device="cuda")
    start = 1 + (16 - buf.data_ptr() % 16) % 16 // t.element_size()
    o = buf[start:start + t.numel()].view(t.shape)
    o.copy_(t)
    assert o.data_ptr() % 16 == t.element_size()
    return o


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    import torch
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _np_bits_equal(got, want):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def _dispatch():
    return (_lib.lib().cdll.sd_last_dispatch() or b"").decode()


def _ranks(ops, c, W, offset=False):
    """the phased calls over W rank slices of the batch -> dict of numpy arrays; parts / bparts are the device's own.
    The backward runs on the device's own mean / var."""
    import torch
    g, b = _cuda(c["gamma"]), _cuda(c["beta"])
    xs = [_cuda(a, offset) for a in sr.slices(c["x"], W)]
    dys = [_cuda(a, offset) for a in sr.slices(c["dy"], W)]
    kw = dict(eps=c["eps"], fix_gamma=c["fix_gamma"])
    parts = torch.stack([ops.sync_bn_stats(x) for x in xs])
    fwd = [ops.sync_bn_apply(x, parts, g, b, **kw) for x in xs]
    mean, var = fwd[0][1], fwd[0][2]
    bparts = torch.stack([ops.sync_bn_bwd_stats(dy, x, mean) for dy, x in zip(dys, xs)])
    mm0, mv0 = np.linspace(-1, 1, g.numel()).astype(F), np.linspace(0.5, 2, g.numel()).astype(F)
    bwd, moving = [], []
    for r, (dy, x) in enumerate(zip(dys, xs)):
        mm, mv = _cuda(mm0), _cuda(mv0)
        bwd.append(ops.sync_bn_bwd_apply(dy, x, mean, var, g, bparts, r, moving_mean=mm, moving_var=mv, momentum=0.9,
                                         **kw))
        moving.append((mm, mv))
    torch.cuda.synchronize()
    return dict(parts=_np(parts), bparts=_np(bparts), mean=_np(mean), var=_np(var),
                means=[_np(f[1]) for f in fwd], vars=[_np(f[2]) for f in fwd],
                y=np.concatenate([_np(f[0]) for f in fwd]), ys=[_np(f[0]) for f in fwd],
                dxs=[_np(o[0]) for o in bwd], dx=np.concatenate([_np(o[0]) for o in bwd]),
                dgammas=[_np(o[1]) for o in bwd], dbetas=[_np(o[2]) for o in bwd],
                moving=[(_np(a), _np(b_)) for a, b_ in moving], mm0=mm0, mv0=mv0)


def _check_margins(ops, W):
    """tests 1 to 3 for one W: the statistics' margins, everything behind them bit for bit, y / dx / dgamma / dbeta
    against the whole-batch truth"""
    ev = _evaluated(W)
    outs = ("mean", "var", "bpart", "y", "dx", "dgamma", "dbeta")
    zero = _zero_ref(ev, outs)
    worst = {o: (0.0, 0.0, None) for o in outs}
    failures = []
    for i, (name, c, truth, T, k_ref, mean32, var32) in enumerate(ev):
        d = _ranks(ops, c, W, offset=i % 5 == 3)            # every fifth case off the 16-byte boundary
        n_rank = sr.count(c["x"]) // W
        # -- bit for bit behind the statistics, from the device's own partials
        m, v = sr.combine_contract(d["parts"])
        for r in range(W):
            assert _np_bits_equal(d["means"][r], m) and _np_bits_equal(d["vars"][r], v), (name, r, "mean / var")
        if W == 1:
            assert _np_bits_equal(d["mean"], d["parts"][0, 0]) and _np_bits_equal(d["var"], d["parts"][0, 1]), name
        for r, (xr, dr) in enumerate(zip(sr.slices(c["x"], W), sr.slices(c["dy"], W))):
            want_y = sr.fwd_contract32(xr, d["mean"], d["var"], c["gamma"], c["beta"], c["eps"], c["fix_gamma"])
            assert _np_bits_equal(d["ys"][r], want_y), (name, r, "y")
            want = sr.bwd_contract32(dr, xr, d["mean"], d["var"], c["gamma"], d["bparts"], r, n_rank, c["eps"],
                                     c["fix_gamma"], d["mm0"], d["mv0"], 0.9)
            assert _np_bits_equal(d["dxs"][r], want["dx"]), (name, r, "dx")
            assert _np_bits_equal(d["dgammas"][r], want["dgamma"]), (name, r, "dgamma")
            assert _np_bits_equal(d["dbetas"][r], want["dbeta"]), (name, r, "dbeta")
            assert _np_bits_equal(d["moving"][r][0], want["moving_mean"]), (name, r, "moving_mean")
            assert _np_bits_equal(d["moving"][r][1], want["moving_var"]), (name, r, "moving_var")
        # -- margins: the backward's truth and k_ref are formed from the float32 mean / var the device's backward
        #    was given (its own), the forward's from x alone
        bt, bT = sr.bwd_truth(c["dy"], c["x"], d["mean"], d["var"], c["gamma"], c["eps"], c["fix_gamma"], W)
        bref = sr.bwd_ref32(c["dy"], c["x"], d["mean"], d["var"], c["gamma"], c["eps"], c["fix_gamma"], W)
        got = dict(mean=d["mean"], var=d["var"], bpart=d["bparts"], y=d["y"], dx=d["dx"],
                   dgamma=np.sum([g.astype(np.float64) for g in d["dgammas"]], axis=0),
                   dbeta=np.sum([g.astype(np.float64) for g in d["dbetas"]], axis=0))
        for o in outs:
            if o in ("mean", "var", "y"):
                k, kr = sr.k_of(got[o], truth[o], T[o]), k_ref[o]
            else:
                k, kr = sr.k_of(got[o], bt[o], bT[o]), sr.k_of(bref[o], bt[o], bT[o])
            if k > worst[o][0]:
                worst[o] = (k, kr, name)
            if not k <= 2 * kr + 2:
                failures.append("%s %s: k_gpu %.3f > 2 * %.3f + 2" % (name, o, k, kr))
            z = zero[(c["x"].shape, o)]
            if not k <= 2 * z + 2:
                failures.append("%s %s (zero-offset cap): k_gpu %.3f > 2 * %.3f + 2" % (name, o, k, z))
    for o in outs:
        print("sync_bn W=%d %-6s: worst k_gpu %.3f (k_ref %.3f there, %s)" % ((W, o) + worst[o]))
    assert not failures, "\n".join(failures[:20])


@pytest.mark.gpu
def test_hip_statistics_margin_and_the_rest_bit_for_bit(ops):
    _check_margins(ops, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [2, 3])
def test_hip_simulated_ranks(ops, W):
    _check_margins(ops, W)


@pytest.mark.gpu
def test_hip_constant_channel_is_exact(ops):
    name, c, truth, T, k_ref, mean32, var32 = _evaluated(1)[-1]
    assert name == "constant"
    for W in (1, 2):
        d = _ranks(ops, c, W)
        assert d["mean"][1] == 1.5 and d["var"][1] == 0.0, (W, d["mean"][1], d["var"][1])
        assert np.all(d["parts"][:, 0, 1] == 1.5) and np.all(d["parts"][:, 1, 1] == 0.0)
        # inv = 1 / sqrt(eps): (g * 0) * inv + beta = beta exactly, and dx = dy * (g * inv) + b * 0 + c
        assert np.all(d["y"][:, 1] == c["beta"][1])
        inv = F(1.0) / np.sqrt(F(0.0) + F(c["eps"]))
        want = sr.bwd_contract32(c["dy"][:, 1:2], c["x"][:, 1:2], F([1.5]), F([0.0]), c["gamma"][1:2],
                                 d["bparts"][:, :, 1:2].sum(axis=0, keepdims=True), 0, sr.count(c["x"]), c["eps"], False)
        if W == 1:
            assert _np_bits_equal(d["dx"][:, 1:2], want["dx"])
            assert d["dgammas"][0][1] == F(d["bparts"][0, 1, 1] * inv)
        assert np.isfinite(d["dx"]).all()


@pytest.mark.gpu
def test_hip_inference_forward_bit_for_bit(ops):
    import torch
    rs = np.random.RandomState(5)
    for shape in sr.SHAPES + EXTRA_SHAPES:
        for fix in (True, False):
            c = sr.make_case(rs, shape, "zeros", fix, 3.0, 1e-3)
            C = shape[1]
            mm, mv = rs.standard_normal(C).astype(F), (rs.random_sample(C) + 0.1).astype(F)
            for offset in (False, True):
                y = ops.sync_bn_infer_forward(_cuda(c["x"], offset), _cuda(c["gamma"]), _cuda(c["beta"]), _cuda(mm),
                                              _cuda(mv), 1e-3, fix, y=_cuda(np.full(shape, np.nan, F), offset))
                torch.cuda.synchronize()
                want = sr.infer_contract32(c["x"], c["gamma"], c["beta"], mm, mv, 1e-3, fix)
                assert _np_bits_equal(_np(y), want), (shape, fix, offset)


@pytest.mark.gpu
def test_hip_phased_calls_equal_the_one_rank_wrappers(ops):
    import torch
    rs = np.random.RandomState(6)
    for shape in ((3, 7, 5, 9), (6, 16, 8, 8), sr.SPLIT_SHAPE):
        c = sr.make_case(rs, shape, "random", False, 3.0, 1e-3)
        x, dy, g, b = _cuda(c["x"]), _cuda(c["dy"]), _cuda(c["gamma"]), _cuda(c["beta"])
        part = ops.sync_bn_stats(x)
        y, mean, var = ops.sync_bn_apply(x, part[None], g, b, 1e-3, False)
        bpart = ops.sync_bn_bwd_stats(dy, x, mean)
        dx, dgamma, dbeta = ops.sync_bn_bwd_apply(dy, x, mean, var, g, bpart[None], 0, 1e-3, False)
        y2, mean2, var2 = ops.sync_batch_norm_forward(x, g, b, eps=1e-3, fix_gamma=False, gather=None)
        dx2, dg2, db2 = ops.sync_batch_norm_backward(dy, x, mean2, var2, g, eps=1e-3, fix_gamma=False, gather=None)
        for p, q in ((y, y2), (mean, mean2), (var, var2), (dx, dx2), (dgamma, dg2), (dbeta, db2)):
            assert _same_bits(p, q), shape
        # a gather callable sees the rank's part and decides parts and the rank
        seen = []

        def gather(p):
            seen.append(tuple(p.shape))
            return torch.stack([p, p]), 1
        y3, mean3, var3 = ops.sync_batch_norm_forward(x, g, b, eps=1e-3, fix_gamma=False, gather=gather)
        assert seen == [(2, shape[1])] and _same_bits(mean3, mean) and _same_bits(y3, y)    # two equal ranks


@pytest.mark.gpu
def test_hip_split_path_is_taken_where_it_should_be(ops):
    import torch
    seen = {}
    for shape in sr.SHAPES + EXTRA_SHAPES:
        x = torch.randn(shape, device="cuda")
        part = ops.sync_bn_stats(x)
        f = _dispatch()
        ops.sync_bn_bwd_stats(x, x, part[0].contiguous())
        seen[shape] = (f, _dispatch())
    torch.cuda.synchronize()
    for shape, ds in seen.items():
        for d in ds:
            assert ("(split)" in d) == (shape == sr.SPLIT_SHAPE), (shape, d)
    for d in seen[sr.SPLIT_SHAPE]:
        assert "L8,vec,block> x 13 chunks" in d and "merge_kernel" in d, d     # 6 * 16800 / 8 = 12600 items of 1024
    assert all("wave" in d for d in seen[(6, 16, 8, 8)]) and all("L1,narrow,wave" in d for d in seen[(3, 7, 5, 9)])
    assert all("L8,vec,block>" in d for d in seen[(2, 3, 40, 40)])
    assert "sbn_stats_kernel" in seen[(6, 5)][0] and "sbn_bwd_stats_kernel" in seen[(6, 5)][1]


SENTINEL = -777.5       # (a half holds it exactly)


def _all_outputs(ops, x, dy, g, b, kw, ws=None, y=None, dx=None):
    part = ops.sync_bn_stats(x, workspace=ws)
    y, mean, var = ops.sync_bn_apply(x, part[None], g, b, y=y, workspace=ws, **kw)
    bpart = ops.sync_bn_bwd_stats(dy, x, mean, workspace=ws)
    dx, dgamma, dbeta = ops.sync_bn_bwd_apply(dy, x, mean, var, g, bpart[None], 0, dx=dx, workspace=ws, **kw)
    return part, y, mean, var, bpart, dx, dgamma, dbeta


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_hip_bit_stability_calls_offsets_and_graph_replay(ops, half):
    """equal bits over two calls, with every data pointer one element off a 16-byte boundary inside sentinel-filled
    buffers that stay untouched, and under replay of a captured graph on changed inputs"""
    import torch
    rs = np.random.RandomState(12)
    dt = torch.float16 if half else torch.float32
    for shape in ((3, 7, 5, 9), (6, 16, 8, 8), (6, 8, 12), (2, 3, 40, 40), sr.SPLIT_SHAPE):
        c = sr.make_case(rs, shape, "random", False, 3.0, 1e-3)
        kw = dict(eps=1e-3, fix_gamma=False)
        g, b = _cuda(c["gamma"]), _cuda(c["beta"])
        x, dy = _cuda(c["x"], dtype=dt), _cuda(c["dy"], dtype=dt)
        first = [t.clone() for t in _all_outputs(ops, x, dy, g, b, kw)]
        again = _all_outputs(ops, x, dy, g, b, kw)
        for p, q in zip(first, again):
            assert _same_bits(p, q), shape
        # -- offset pointers, outputs carved out of sentinel-filled buffers
        n = x.numel()
        xo, dyo = _cuda(c["x"], True, dt), _cuda(c["dy"], True, dt)
        pad = 64 + 1
        bufs = [torch.full((n + 2 * pad,), SENTINEL, dtype=dt, device="cuda") for _ in range(2)]
        views = []
        for bf in bufs:
            start = pad + (16 - (bf.data_ptr() + pad * bf.element_size()) % 16) % 16 // bf.element_size() + 1
            views.append((bf, start, bf[start:start + n].view(shape)))
            assert views[-1][2].data_ptr() % 16 == bf.element_size()
        off = _all_outputs(ops, xo, dyo, g, b, kw, y=views[0][2], dx=views[1][2])
        torch.cuda.synchronize()
        for p, q in zip(first, off):
            assert _same_bits(p, q), (shape, "offset")
        for bf, start, _ in views:
            assert torch.all(bf[:start] == SENTINEL) and torch.all(bf[start + n:] == SENTINEL), shape
        # -- a captured graph replayed on changed inputs
        N, C = shape[:2]
        wsb = ops.sync_bn_workspace_bytes(N, C, n // (N * C))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        ws2 = torch.empty_like(ws)
        xg, dyg = x.clone(), dy.clone()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                part = ops.sync_bn_stats(xg, workspace=ws)
                yy, mean, var = ops.sync_bn_apply(xg, part[None], g, b, workspace=ws, **kw)
                bpart = ops.sync_bn_bwd_stats(dyg, xg, mean, workspace=ws2)
                dxx, dgamma, dbeta = ops.sync_bn_bwd_apply(dyg, xg, mean, var, g, bpart[None], 0, workspace=ws2, **kw)
        cap = (part, yy, mean, var, bpart, dxx, dgamma, dbeta)
        c2 = sr.make_case(rs, shape, "random", False, 0.0, 1e-3)
        x2, dy2 = _cuda(c2["x"], dtype=dt), _cuda(c2["dy"], dtype=dt)
        want2 = [t.clone() for t in _all_outputs(ops, x2, dy2, g, b, kw)]
        for xin, dyin, want in ((x2, dy2, want2), (x, dy, first)):
            xg.copy_(xin)
            dyg.copy_(dyin)
            for t in cap:
                t.fill_(float("nan"))
            ws.fill_(0xFF)
            ws2.fill_(0xFF)
            graph.replay()
            torch.cuda.synchronize()
            for p, q in zip(want, cap):
                assert _same_bits(p, q), (shape, "graph")


@pytest.mark.gpu
def test_hip_f16_equals_cast_fp32_cast(ops):
    import torch
    rs = np.random.RandomState(13)
    for shape in ((3, 7, 5, 9), (6, 16, 8, 8), (2, 6, 6, 6), sr.SPLIT_SHAPE):   # 36: items of 4, halves by element
        for fix in (False, True):
            c = sr.make_case(rs, shape, "random", fix, 3.0, 1e-3)
            kw = dict(eps=1e-3, fix_gamma=fix)
            g, b = _cuda(c["gamma"]), _cuda(c["beta"])
            C = shape[1]
            mm, mv = _cuda(rs.standard_normal(C).astype(F)), _cuda((rs.random_sample(C) + 0.1).astype(F))
            for offset in (False, True):
                xh, dyh = _cuda(c["x"], offset, torch.float16), _cuda(c["dy"], offset, torch.float16)
                xf, dyf = xh.float(), dyh.float()
                h = _all_outputs(ops, xh, dyh, g, b, kw)
                f = _all_outputs(ops, xf, dyf, g, b, kw)
                for i, (p, q) in enumerate(zip(h, f)):
                    if p.dtype == torch.float16:
                        assert q.dtype == torch.float32 and _same_bits(p, q.half()), (shape, fix, offset, i)
                    else:
                        assert _same_bits(p, q), (shape, fix, offset, i)
                yh = ops.sync_bn_infer_forward(xh, g, b, mm, mv, 1e-3, fix)
                yf = ops.sync_bn_infer_forward(xf, g, b, mm, mv, 1e-3, fix)
                assert yh.dtype == torch.float16 and _same_bits(yh, yf.half()), (shape, fix, offset)


@pytest.mark.gpu
def test_autograd_wrapper_against_torch_batch_norm_in_float64(ops):
    """torch.nn.functional.batch_norm(training=True) differentiated in float64 is the truth; T and the restatement's
    k_ref are those of tests/sync_bn_ref.py; the bound is that of the statistics test"""
    import torch
    rs = np.random.RandomState(14)
    for shape in ((6, 5), (3, 7, 5, 9), (6, 16, 8, 8), sr.SPLIT_SHAPE):
        c = sr.make_case(rs, shape, "random", False, 0.0, 1e-3)
        x = _cuda(c["x"]).requires_grad_()
        g, b = _cuda(c["gamma"]).requires_grad_(), _cuda(c["beta"]).requires_grad_()
        dy = _cuda(c["dy"])
        mm, mv = torch.zeros_like(g), torch.ones_like(g)
        y, mean, var = ops.sync_batch_norm(x, g, b, eps=1e-3, fix_gamma=False, moving_mean=mm, moving_var=mv,
                                           momentum=0.9, return_stats=True)
        assert not mean.requires_grad and not var.requires_grad
        assert torch.all(mm == 0) and torch.all(mv == 1)              # nothing moves in the forward
        dx, dgamma, dbeta = torch.autograd.grad(y, (x, g, b), dy)
        want_m = sr.bwd_contract32(c["dy"], c["x"], _np(mean), _np(var), c["gamma"], np.zeros((1, 2, shape[1]), F), 0,
                                   sr.count(c["x"]), 1e-3, False, np.zeros(shape[1], F), np.ones(shape[1], F), 0.9)
        assert _np_bits_equal(_np(mm), want_m["moving_mean"]) and _np_bits_equal(_np(mv), want_m["moving_var"])
        x64 = x.detach().double().requires_grad_()
        g64, b64 = g.detach().double().requires_grad_(), b.detach().double().requires_grad_()
        y64 = torch.nn.functional.batch_norm(x64, None, None, g64, b64, training=True, eps=float(F(1e-3)))
        dx64, dg64, db64 = torch.autograd.grad(y64, (x64, g64, b64), dy.double())
        truth, T, k_ref, mean32, var32 = sr.evaluate(c, 1)
        for o, got, want in (("y", y, y64), ("dx", dx, dx64), ("dgamma", dgamma, dg64), ("dbeta", dbeta, db64)):
            # torch's float64 result agrees with the restatement's truth: far below one float32 unit of T where the
            # truth takes no float32 input (y, dbeta); dx and dgamma of the restatement are formed about the float32
            # roundings of mean / var, which moves them by a fraction of a unit
            assert sr.k_of(_np(want), truth[o], T[o]) < (0.01 if o in ("y", "dbeta") else 2.0), (shape, o)
            k = sr.k_of(_np(got), _np(want), T[o])
            print("autograd %s %-6s k_gpu %.3f (k_ref %.3f)" % (shape, o, k, k_ref[o]))
            assert k <= 2 * k_ref[o] + 2, (shape, o, k, k_ref[o])
        only_y = ops.sync_batch_norm(x, g, b, eps=1e-3, fix_gamma=False)
        assert _same_bits(only_y.detach(), y.detach())
        dx2, = torch.autograd.grad(only_y, (x,), dy)                  # data gradient alone
        assert _same_bits(dx2, dx)
