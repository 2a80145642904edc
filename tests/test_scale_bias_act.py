"""The merged-BN affine (simpledet_amd/csrc/scale_bias_act.hip): fused scale, bias, residual add and relu, and
_contrib_BroadcastScale as its bare form, against the restatement of tests/merged_bn_ref.py.

  CPU: argument validation of the four C entry points (every case fails, or succeeds, before any launch); the
       workspace size is monotone in N and C; the fixtures tell per-step rounding from a contracted kernel (at least
       10 % of the elements differ: measured 16.8 % in float32 against a fused multiply-add, 37.9 % in float16
       against one final rounding, on the N(0,1) case with bias and residual).
  GPU: y, dx and dres BIT-EQUAL to the restatement (a NaN matches any NaN: the sign and payload of a generated NaN
       are the processor's) on every shape x form x dtype, at every pointer phase, in place, on the value edges,
       from a replayed graph and through autograd; on finite data bit-equal to the torch composition of the
       reference's nodes run on the device as well.  One mended detail there: torch's backward of where() SELECTS
       (a dead unit gets +0.0) where the reference MULTIPLIES ograd * relu_grad(out) (a dead unit under a negative
       dy gets -0.0, and dx the zero gamma's sign then gives); the two agree in value everywhere and in every bit
       but the sign of such a zero, so a zero is compared by value there and everything else by bits.
       dbeta: k_gpu <= 2 * k_ref + 2 per case (the margin rule of tests/test_group_norm.py: a factor 2 for the free
       summation order plus 2 units for the final roundings; k_ref is the float32 restatement's own k in the same
       run), exact where the sum is exact, equal bits between calls and pointer phases.
"""
import ctypes
import functools
import re

import numpy as np
import pytest

from simpledet_amd import _lib

from . import merged_bn_ref as mr

P = ctypes.c_void_p(256)   # never dereferenced: every CPU case returns before any launch
F, H = np.float32, np.float16


# ------------------------------------------------------------------------------------------ CPU --
def _wsb(N, C, HxW):
    return int(_lib.lib().cdll.sd_scale_bias_act_workspace_bytes(N, C, ctypes.c_long(HxW)))


def _fwd(sfx, N=2, C=8, HxW=16, act=1, ptr=P, skip=(), **_):
    a = [None if i in skip else ptr for i in range(5)]          # x, gamma, beta, residual, y
    return _lib.lib().call("sd_scale_bias_act_fwd" + sfx, *a, N, C, ctypes.c_long(HxW), act, None)


def _bwd(sfx, N=2, C=8, HxW=16, act=1, ptr=P, skip=(), dbeta=None, ws=None, wsb=0):
    a = [None if i in skip else ptr for i in range(5)]          # dy, y, gamma, dx, dres
    return _lib.lib().call("sd_scale_bias_act_bwd" + sfx, *a, dbeta, N, C, ctypes.c_long(HxW), act, ws,
                           ctypes.c_size_t(wsb), None)


CALLS = [(_fwd, "", (0, 1, 4)), (_fwd, "_f16", (0, 1, 4)), (_bwd, "", (0, 2, 3)), (_bwd, "_f16", (0, 2, 3))]


@pytest.mark.parametrize("call,sfx,required", CALLS, ids=["fwd", "fwd_f16", "bwd", "bwd_f16"])
def test_entry_points_reject_bad_arguments_without_a_gpu(call, sfx, required):
    E = _lib.SimpleDetOpsError
    for kw in (dict(N=-1), dict(C=-8), dict(HxW=-1)):
        with pytest.raises(E, match="negative dimension") as e:
            call(sfx, **kw)
        assert e.value.code == -1
    for act in (2, -1, 7):
        with pytest.raises(E, match="act=") as e:
            call(sfx, act=act)
        assert e.value.code == -1
    for i in required:
        with pytest.raises(E, match="null pointer") as e:
            call(sfx, skip=(i,))
        assert e.value.code == -1
    with pytest.raises(E, match="not aligned") as e:
        call(sfx, ptr=ctypes.c_void_p(257))
    assert e.value.code == -1
    # 2^31 - 1 elements is the stated limit: 2 x 1024 x 1048576 = 2^31
    with pytest.raises(E, match="exceed the limit") as e:
        call(sfx, N=2, C=1024, HxW=1 << 20)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(E, match="exceed the limit"):
        call(sfx, N=1 << 20, C=1 << 20, HxW=1 << 40)
    # empty problems succeed without touching the device (no pointer is looked at) ...
    for kw in (dict(N=0), dict(C=0), dict(HxW=0)):
        assert call(sfx, ptr=None, **kw) == 0
    # ... but their parameters are still checked
    with pytest.raises(E, match="act="):
        call(sfx, N=0, act=3, ptr=None)


@pytest.mark.parametrize("sfx", ["", "_f16"])
def test_backward_needs_y_under_act_and_a_workspace_for_dbeta(sfx):
    E = _lib.SimpleDetOpsError
    with pytest.raises(E, match="reads y") as e:
        _bwd(sfx, act=1, skip=(1,))
    assert e.value.code == -1
    need = _wsb(2, 8, 16)
    for kw in (dict(ws=None, wsb=need), dict(ws=P, wsb=need - 1), dict(ws=P, wsb=0)):
        with pytest.raises(E, match="workspace too small") as e:
            _bwd(sfx, dbeta=P, **kw)
        assert e.value.code == -4                                   # SD_ERR_WORKSPACE
    with pytest.raises(E, match="not aligned"):
        _bwd(sfx, dbeta=ctypes.c_void_p(258), ws=P, wsb=need)
    assert _bwd(sfx, N=0, dbeta=P, ptr=None) == 0                   # empty: no workspace either


def test_workspace_bytes_is_monotone_in_n_and_c():
    for HxW in (1, 49, 1050, 8192, 8193, 67200, 268800):
        prev = 0
        for N in (1, 2, 3, 8, 64, 1024):
            if N * 256 * HxW >= 1 << 31:      # (beyond the limit of the entry points the size is not defined)
                continue
            b = _wsb(N, 256, HxW)
            assert b >= prev
            prev = b
        prev = 0
        for C in (1, 3, 64, 256, 2048):
            b = _wsb(2, C, HxW)
            assert b >= prev
            prev = b
    assert _wsb(2, 256, 67200) >= 2 * 256 * 4
    assert 0 < _wsb(0, 256, 49) <= 4096 and 0 < _wsb(2, -1, 49) <= 4096


def test_fixtures_tell_per_step_rounding_from_a_contracted_kernel():
    """a kernel that fuses the multiply into the add (float32) or keeps the chain in float and rounds once
    (float16) must not pass the bit comparison: on the N(0,1) case at least 10 % of the elements differ"""
    for dt, floor in ((F, 0.10), (H, 0.10)):
        d = mr.make(np.random.RandomState(5), (3, 7, 13, 21), dt)
        want = mr.fwd(d["x"], d["gamma"], d["beta"], d["residual"])
        fused = mr.fwd_contracted(d["x"], d["gamma"], d["beta"], d["residual"])
        frac = float(np.mean(want != fused))
        print("%s: %.1f %% of the elements differ between per-step rounding and the contracted chain"
              % (np.dtype(dt).name, 100 * frac))
        assert frac >= floor, (dt, frac)


def test_all_forms_is_the_per_form_restatement():
    for dt in (F, H):
        d = mr.make(np.random.RandomState(6), (2, 3, 5, 4), dt)
        forms = mr.all_forms(d)
        assert sorted(forms) == sorted(mr.FORMS)
        for (hb, hr, act), got in forms.items():
            y = mr.fwd(d["x"], d["gamma"], d["beta"] if hb else None, d["residual"] if hr else None, act)
            b = mr.bwd(d["dy"], y, d["gamma"], act)
            assert mr.same_bits(got["y"], y) and mr.same_bits(got["dx"], b["dx"])
            assert mr.same_bits(got["dres"], b["dres"]) and mr.same_bits(got["dbeta"], b["dbeta"])


def test_restatement_known_answers():
    x = F([[[1.0, -2.0, 0.0, -0.0]]]).reshape(1, 1, 4)
    y = mr.fwd(x, F([2.0]), F([1.0]), F([[[-3.0, 1.0, -1.0, -1.0]]]).reshape(1, 1, 4), act=True)
    assert y.reshape(-1).tolist() == [0.0, 0.0, 0.0, 0.0] and not np.signbit(y).any()      # v = 0, -2, 0, 0
    y = mr.fwd(x, F([-1.0]))
    assert y.reshape(-1).tolist() == [-1.0, 2.0, 0.0, 0.0] and np.signbit(y).reshape(-1).tolist() == [1, 0, 1, 0]
    b = mr.bwd(F([[[np.inf, -1.0, 2.0, 3.0]]]).reshape(1, 1, 4), F([[[0.0, 0.0, 1.0, np.nan]]]).reshape(1, 1, 4),
               F([0.5]), act=True)
    assert np.isnan(b["dres"].reshape(-1)[0]) and np.signbit(b["dres"].reshape(-1)[1])     # inf * 0, -1 * 0
    assert b["dres"].reshape(-1)[2:].tolist() == [2.0, 0.0] and b["dx"].reshape(-1)[2] == 1.0
    # float16: every step rounds; 2049 is not a half, 2048 + 1 -> 2048 (ties to even), then + 1 again -> 2048
    y = mr.fwd(H([[[2048.0]]]), H([1.0]), H([1.0]), H([[[1.0]]]))
    assert y.item() == 2048.0 and mr.fwd_contracted(H([[[2048.0]]]), H([1.0]), H([1.0]), H([[[1.0]]])).item() == 2050.0


# ------------------------------------------------------------------------------------------ GPU --
SENTINEL = -777.5      # a half as well
PAD = 64               # elements in front of and behind every carved tensor: a multiple of 16 bytes in both dtypes


def _tdt(dt):
    import torch
    return torch.float32 if np.dtype(dt) == np.dtype(F) else torch.float16


def _dev(a, off=0):
    """a device copy of `a` (or an uninitialised tensor of shape `a` for a tuple) whose data pointer lies `off`
    elements behind a 16-byte boundary, carved from a sentinel-filled buffer -> (tensor, check)"""
    import torch
    if isinstance(a, tuple):
        shape, dt, src = a[0], a[1], None
    else:
        a = np.ascontiguousarray(a)
        shape, dt, src = a.shape, a.dtype, a
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD + 8,), SENTINEL, dtype=_tdt(dt), device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[PAD + off:PAD + off + n].view(shape)
    assert t.data_ptr() % 16 == (off * np.dtype(dt).itemsize) % 16
    if src is not None:
        t.copy_(torch.from_numpy(src))

    def intact():
        return bool(torch.all(buf[:PAD + off] == SENTINEL) and torch.all(buf[PAD + off + n:] == SENTINEL))
    return t, intact


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _dispatch():
    return (_lib.lib().cdll.sd_last_dispatch() or b"").decode()


def _composition(x, g, b, r, act):
    """the reference's nodes in torch: BroadcastScale, broadcast_add, the elemwise add, relu as where(v > 0, v, 0)"""
    import torch
    v = x * g.view(1, -1, 1, 1)
    if b is not None:
        v = v + b.view(1, -1, 1, 1)
    if r is not None:
        v = v + r
    return torch.where(v > 0, v, torch.zeros_like(v)) if act else v


def _bits_but_zero_signs(got, want):
    """equal bits, except that two zeros need not agree in sign (the docstring's mended detail)"""
    got, want = np.asarray(got), np.asarray(want)
    both_zero = (got == 0) & (want == 0)
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    return bool(np.array_equal(got.view(u)[~both_zero], want.view(u)[~both_zero]))


@functools.lru_cache(maxsize=None)
def _case(dtname, shape):
    d = mr.make(np.random.RandomState(1000 + sum(shape)), shape, np.dtype(dtname).type)
    return d, mr.all_forms(d)


def _dbeta_margin(got, ref, tag, failures):
    k = mr.k_of(got, ref["dbeta_truth"], ref["dbeta_T"])
    k_ref = mr.k_of(ref["dbeta"], ref["dbeta_truth"], ref["dbeta_T"])
    print("%s: dbeta k_gpu %.3f against k_ref %.3f" % (tag, k, k_ref))
    if not k <= 2 * k_ref + 2:
        failures.append("%s dbeta: k_gpu %.3f > 2 * %.3f + 2" % (tag, k, k_ref))


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", ["float32", "float16"])
@pytest.mark.parametrize("shape", mr.SHAPES + ("large",), ids=lambda s: s if s == "large" else "x".join(map(str, s)))
def test_hip_every_form_matches_the_restatement_and_the_torch_composition(ops, dtname, shape):
    import torch
    large = shape == "large"
    shape = mr.LARGE[dtname] if large else shape
    d, forms = _case(dtname, shape)
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    failures = []
    for hb, hr, act in mr.FORMS:
        ref, tag = forms[(hb, hr, act)], "%s %s bias=%d residual=%d act=%d" % (dtname, shape, hb, hr, act)
        b, r = (t["beta"] if hb else None), (t["residual"] if hr else None)
        y = ops.scale_bias_act_forward(t["x"], t["gamma"], b, r, "relu" if act else None)
        fdisp = _dispatch()
        dx, dres, dbeta = ops.scale_bias_act_backward(t["dy"], y if act else None, t["gamma"], "relu" if act else None,
                                                      need_dres=True, need_dbeta=True)
        bdisp = _dispatch()
        for name, got in (("y", y), ("dx", dx), ("dres", dres)):
            if not mr.same_bits(_np(got), ref[name]):
                failures.append("%s %s vs restatement: %s" % (tag, name, mr.mismatch(_np(got), ref[name])))
        _dbeta_margin(_np(dbeta), ref, tag, failures)
        # the torch composition on the device (finite data)
        xs = t["x"].clone().requires_grad_()
        rsd = None if r is None else r.clone().requires_grad_()
        yt = _composition(xs, t["gamma"], b, rsd, act)
        gr = torch.autograd.grad(yt, (xs,) + (() if rsd is None else (rsd,)), t["dy"])
        if not torch.equal(y.view(torch.int16 if dtname == "float16" else torch.int32),
                           yt.detach().view(torch.int16 if dtname == "float16" else torch.int32)):
            failures.append("%s y vs torch: %s" % (tag, mr.mismatch(_np(y), _np(yt))))
        if not _bits_but_zero_signs(_np(dx), _np(gr[0])):
            failures.append("%s dx vs torch: %s" % (tag, mr.mismatch(_np(dx), _np(gr[0]))))
        if rsd is not None and not _bits_but_zero_signs(_np(dres), _np(gr[1])):
            failures.append("%s dres vs torch: %s" % (tag, mr.mismatch(_np(dres), _np(gr[1]))))
        if large:
            for disp in (fdisp, bdisp):
                m = re.search(r"grid=(\d+) tiles=(\d+)", disp)
                assert m and int(m.group(1)) == 2048 and int(m.group(2)) > int(m.group(1)), disp
    assert not failures, "\n".join(failures[:20])


def _full(ops, t, off, act=True, with_dres=True, with_dbeta=True):
    """the full form (bias, residual, act) with every tensor carved at its own offset `off[name]`"""
    shape, dt = tuple(t["x"].shape), t["x"].dtype
    checks = []

    def carve(name, src):
        v, ok = _dev(src, off.get(name, 0))
        checks.append((name, ok))
        return v
    x, r = carve("x", t["x"]), carve("residual", t["residual"])
    y = carve("y", (shape, dt))
    ops.scale_bias_act_forward(x, carve("gamma", t["gamma"]), carve("beta", t["beta"]), r, "relu" if act else None,
                               out=y)
    fdisp = _dispatch()
    dy, yin = carve("dy", t["dy"]), carve("y_in", _np(y))
    dx, dres = carve("dx", (shape, dt)), (carve("dres", (shape, dt)) if with_dres else None)
    dbeta = carve("dbeta", ((shape[1],), F)) if with_dbeta else None
    ops.scale_bias_act_backward(dy, yin, carve("gamma2", t["gamma"]), "relu" if act else None, dx=dx, dres=dres,
                                dbeta=dbeta)
    bad = [n for n, ok in checks if not ok()]
    return dict(y=_np(y), dx=_np(dx), dres=_np(dres), dbeta=_np(dbeta)), bad, fdisp, _dispatch()


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", ["float32", "float16"])
def test_hip_every_tensor_at_every_phase_gives_the_same_bits_and_keeps_its_surroundings(ops, dtname):
    """x, residual, y (dy, y, dx, dres), and gamma / beta / dbeta, each on its own one element and three elements
    off a 16-byte boundary, then all of them at once on different phases"""
    for shape in ((3, 7, 13, 21), (2, 3, 5, 4), (1, 2, 1, 4099), (2, 5, 1, 3)):
        d, forms = _case(dtname, shape)
        ref = forms[(True, True, True)]
        base, bad, fd, bd = _full(ops, d, {})
        assert not bad, bad
        assert "x:vec residual:vec" in fd and "dy:vec y:vec dres:vec" in bd, (fd, bd)
        for name in ("y", "dx", "dres"):
            assert mr.same_bits(base[name], ref[name]), (shape, name, mr.mismatch(base[name], ref[name]))
        names = ("x", "residual", "y", "dy", "y_in", "dx", "dres", "gamma", "beta", "gamma2", "dbeta")
        offsets = [{n: o} for n in names for o in (1, 3)]
        offsets.append(dict(x=1, residual=3, y=2, dy=3, y_in=1, dx=1, dres=2, gamma=1, beta=3, gamma2=1, dbeta=1))
        offsets.append({n: 3 for n in names})
        for off in offsets:
            got, bad, fd, bd = _full(ops, d, off)
            assert not bad, (shape, off, bad)
            for name in ("y", "dx", "dres", "dbeta"):
                assert mr.same_bits(got[name], base[name]), (shape, off, name, mr.mismatch(got[name], base[name]))
            if set(off) == {"x"}:
                assert "x:narrow residual:vec" in fd, fd
            if set(off) == {"y"}:                   # the cut follows the OUTPUT: both inputs are then off it
                assert "x:narrow residual:narrow" in fd, fd
            if set(off) == {"dres"}:
                assert "dy:vec y:vec dres:narrow" in bd, bd


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", ["float32", "float16"])
def test_hip_in_place_forms(ops, dtname):
    """y is x, y is residual, dx is dy, dres is dy -- aligned and off the boundary"""
    for shape in ((3, 7, 13, 21), (1, 2, 1, 4099)):
        d, forms = _case(dtname, shape)
        ref = forms[(True, True, True)]
        for off in (0, 1, 3):
            for alias in ("x", "residual"):
                x, okx = _dev(d["x"], off)
                r, okr = _dev(d["residual"], off if alias == "residual" else 0)
                g, b = _dev(d["gamma"])[0], _dev(d["beta"])[0]
                out = x if alias == "x" else r
                y = ops.scale_bias_act_forward(x, g, b, r, "relu", out=out)
                assert y.data_ptr() == out.data_ptr() and okx() and okr()
                assert mr.same_bits(_np(y), ref["y"]), (shape, off, alias, mr.mismatch(_np(y), ref["y"]))
            for alias in ("dx", "dres"):
                dy, okd = _dev(d["dy"], off)
                y, g = _dev(ref["y"])[0], _dev(d["gamma"])[0]
                kw = {alias: dy}
                dx, dres, _ = ops.scale_bias_act_backward(dy, y, g, "relu", need_dres=True, **kw)
                assert okd() and (dx if alias == "dx" else dres).data_ptr() == dy.data_ptr()
                assert mr.same_bits(_np(dx), ref["dx"]), (shape, off, alias, mr.mismatch(_np(dx), ref["dx"]))
                assert mr.same_bits(_np(dres), ref["dres"]), (shape, off, alias)
        # BroadcastScale in place, both directions
        x = _dev(d["x"], 1)[0]
        g = _dev(d["gamma"])[0]
        assert mr.same_bits(_np(ops.scale_bias_act_forward(x, g, out=x)), forms[(False, False, False)]["y"])
        dy = _dev(d["dy"], 3)[0]
        assert mr.same_bits(_np(ops.scale_bias_act_backward(dy, None, g, dx=dy)[0]), forms[(False, False, False)]["dx"])


def _edge_case(dt):
    """(1, C, E, E): the first operand's edge values down the rows, the second's along the columns, a gamma and a
    beta per channel"""
    ev = mr.edge_values(dt)
    fi = np.finfo(dt)
    gam = np.array([1.0, 0.0, -0.0, -1.5, np.nan, 2.0, np.inf, fi.tiny / 2, 1.0, 1.0], dt)
    bet = np.array([0.0, 1.0, -0.0, 0.5, 1.0, fi.max, -1.0, 0.0, fi.max, -fi.max], dt)
    E, C = len(ev), len(gam)
    rows = np.broadcast_to(ev.reshape(1, 1, E, 1), (1, C, E, E)).copy()
    cols = np.broadcast_to(ev.reshape(1, 1, 1, E), (1, C, E, E)).copy()
    return dict(x=rows, residual=cols, dy=rows, y_in=cols, gamma=gam, beta=bet), ev


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", ["float32", "float16"])
def test_hip_value_edges(ops, dtname):
    """signed zeros, subnormals, infinities, NaN and the format's extremes in x, residual, dy and y; gamma 0, -0,
    negative, NaN, inf, subnormal; v exactly 0 and -0.0; an infinite dy over a dead unit; in float16 an overflow
    at each step's rounding"""
    import torch
    dt = np.dtype(dtname).type
    d, ev = _edge_case(dt)
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    idx = {("%r" % float(v)): i for i, v in enumerate(ev)}
    for hb, hr, act in mr.FORMS:
        want = mr.fwd(d["x"], d["gamma"], d["beta"] if hb else None, d["residual"] if hr else None, act)
        y = ops.scale_bias_act_forward(t["x"], t["gamma"], t["beta"] if hb else None, t["residual"] if hr else None,
                                       "relu" if act else None)
        assert mr.same_bits(_np(y), want), (dtname, hb, hr, act, mr.mismatch(_np(y), want))
        if act:
            assert not np.isnan(_np(y)).any() and not np.signbit(_np(y)).any()     # NaN and -0.0 give +0.0
        wb = mr.bwd(d["dy"], d["y_in"], d["gamma"], act)
        dx, dres, _ = ops.scale_bias_act_backward(t["dy"], t["y_in"], t["gamma"], "relu" if act else None,
                                                  need_dres=True)
        assert mr.same_bits(_np(dres), wb["dres"]), (dtname, act, mr.mismatch(_np(dres), wb["dres"]))
        assert mr.same_bits(_np(dx), wb["dx"]), (dtname, act, mr.mismatch(_np(dx), wb["dx"]))
    # what the grid holds, stated on the restatement (the device equals it bit for bit, above)
    full = mr.fwd(d["x"], d["gamma"], d["beta"], d["residual"], False)
    one, mone, mx = idx["1.0"], idx["-1.0"], idx["%r" % float(np.finfo(dt).max)]
    assert full[0, 0, one, mone] == 0 and not np.signbit(full[0, 0, one, mone])       # 1 * 1 + 0 + -1 = +0.0
    plain = mr.fwd(d["x"], d["gamma"])
    assert np.signbit(plain[0, 3, idx["0.0"], 0]) and plain[0, 3, idx["0.0"], 0] == 0   # 0 * -1.5 = -0.0
    assert np.isinf(plain[0, 5, mx, 0])                                               # overflow at the product
    assert np.isinf(mr.fwd(d["x"], d["gamma"], d["beta"])[0, 8, mx, 0])               # ... at the bias
    assert np.isfinite(mr.fwd(d["x"], d["gamma"], d["beta"])[0, 0, mx, 0]) and np.isinf(full[0, 0, mx, mx])   # ... at the add
    g1 = mr.bwd(d["dy"], d["y_in"], d["gamma"], True)["dres"]
    assert np.isnan(g1[0, 0, idx["inf"], idx["0.0"]]) and np.isnan(g1[0, 0, idx["-inf"], idx["-1.0"]])
    assert np.signbit(g1[0, 0, mone, idx["0.0"]]) and g1[0, 0, mone, idx["0.0"]] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", ["float32", "float16"])
def test_hip_dbeta_exact_sums_equal_bits_and_skipping(ops, dtname):
    import torch
    dt = np.dtype(dtname).type
    rs = np.random.RandomState(21)
    for shape in ((2, 3, 5, 4), (3, 7, 13, 21), (2, 4, 100, 168), (1, 2, 1, 20000)):
        N, C = shape[:2]
        count = N * int(np.prod(shape[2:]))
        assert count < 1 << 24
        g = torch.from_numpy((rs.standard_normal(C) + 1).astype(dt)).cuda()
        ones = torch.ones(shape, dtype=_tdt(dt), device="cuda")
        _, _, dbeta = ops.scale_bias_act_backward(ones, None, g, need_dbeta=True)
        assert "sba_dbeta_partial_kernel" in _dispatch() and "sba_dbeta_finish_kernel" in _dispatch()
        assert dbeta.dtype == torch.float32 and np.all(_np(dbeta) == F(count)), (shape, _np(dbeta)[:4], count)
        # small integers under a mask: every partial sum is an integer below 2^24
        dy = rs.randint(-8, 9, size=shape).astype(dt)
        y = rs.standard_normal(shape).astype(dt)
        want = np.where(y > 0, dy, 0).astype(np.float64).sum(axis=(0, 2, 3))
        tdy, ty = torch.from_numpy(dy).cuda(), torch.from_numpy(y).cuda()
        a = ops.scale_bias_act_backward(tdy, ty, g, "relu", need_dbeta=True)[2]
        assert np.array_equal(_np(a).astype(np.float64), want), shape
        # two calls on random data: equal bits
        dyr = torch.from_numpy(rs.standard_normal(shape).astype(dt)).cuda()
        p = _np(ops.scale_bias_act_backward(dyr, ty, g, "relu", need_dbeta=True)[2])
        q = _np(ops.scale_bias_act_backward(dyr, ty, g, "relu", need_dbeta=True)[2])
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), shape
        # not requested: neither dbeta kernel is launched, and no workspace is asked for
        dx, dres, none = ops.scale_bias_act_backward(dyr, ty, g, "relu")
        assert none is None and dres is None and "dbeta" not in _dispatch() and "sba_bwd_kernel" in _dispatch()


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", ["float32", "float16"])
def test_hip_a_replayed_graph_follows_its_inputs(ops, dtname):
    """forward + backward captured once, replayed on CHANGED inputs: the bits of eager calls on those inputs;
    the capture holds kernel nodes only"""
    import torch
    from .test_group_norm import _node_types
    shape = (3, 7, 13, 21)
    dt = np.dtype(dtname).type
    N, C = shape[:2]
    first = mr.make(np.random.RandomState(31), shape, dt)
    st = {k: torch.from_numpy(v).cuda() for k, v in first.items()}
    ws = torch.empty(ops.scale_bias_act_workspace_bytes(N, C, 273), dtype=torch.uint8, device="cuda")

    def both():
        y = ops.scale_bias_act_forward(st["x"], st["gamma"], st["beta"], st["residual"], "relu")
        dx, dres, dbeta = ops.scale_bias_act_backward(st["dy"], y, st["gamma"], "relu", need_dres=True,
                                                      need_dbeta=True, workspace=ws)
        return y, dx, dres, dbeta
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap = both()
    for seed in (32, 33):
        new = mr.make(np.random.RandomState(seed), shape, dt)
        for k, v in new.items():
            st[k].copy_(torch.from_numpy(v))
        for o in cap:
            o.fill_(float("nan"))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        got = [_np(o).copy() for o in cap]
        eager = [_np(o) for o in both()]
        ref = mr.all_forms(new)[(True, True, True)]
        for name, g_, e_ in zip(("y", "dx", "dres", "dbeta"), got, eager):
            assert mr.same_bits(g_, e_), (seed, name, mr.mismatch(g_, e_))
            if name != "dbeta":
                assert mr.same_bits(g_, ref[name]), (seed, name)
    kinds = _node_types(both)
    assert len(kinds) == 4 and all(k == 0 for k in kinds), kinds        # hipGraphNodeTypeKernel = 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", ["float32", "float16"])
def test_autograd_matches_the_compositions_autograd(ops, dtname):
    import torch
    shape = (3, 7, 13, 21)
    d, forms = _case(dtname, shape)
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    failures = []
    for hb, hr, act in mr.FORMS:
        ref = forms[(hb, hr, act)]

        def leaves():
            x = t["x"].clone().requires_grad_()
            g = t["gamma"].clone().requires_grad_()
            b = t["beta"].clone().requires_grad_() if hb else None
            r = t["residual"].clone().requires_grad_() if hr else None
            return x, g, b, r
        x, g, b, r = leaves()
        y = ops.scale_bias_act(x, g, b, r, "relu" if act else None)
        ins = [v for v in (x, g, b, r) if v is not None]
        grads = dict(zip([n for n, v in zip("xgbr", (x, g, b, r)) if v is not None],
                         torch.autograd.grad(y, ins, t["dy"], allow_unused=True)))
        assert grads["g"] is None                                          # no gradient for gamma
        x2, g2, b2, r2 = leaves()
        yt = _composition(x2, g2, b2, r2, act)
        ins2 = [v for v in (x2, b2, r2) if v is not None]
        tg = dict(zip([n for n, v in zip("xbr", (x2, b2, r2)) if v is not None], torch.autograd.grad(yt, ins2, t["dy"])))
        assert mr.same_bits(_np(y), ref["y"]) and mr.same_bits(_np(grads["x"]), ref["dx"])
        assert _bits_but_zero_signs(_np(y), _np(yt)) and _bits_but_zero_signs(_np(grads["x"]), _np(tg["x"]))
        if hr:
            assert mr.same_bits(_np(grads["r"]), ref["dres"]) and _bits_but_zero_signs(_np(grads["r"]), _np(tg["r"]))
        if hb:
            assert grads["b"].dtype == b.dtype and grads["b"].shape == b.shape
            if dtname == "float32":
                _dbeta_margin(_np(grads["b"]), ref, "autograd %s %s" % (dtname, (hb, hr, act)), failures)
            else:   # the float32 sum rounded once to the parameter's half
                want = ops.scale_bias_act_backward(t["dy"], y.detach(), t["gamma"], "relu" if act else None,
                                                   need_dbeta=True)[2]
                assert torch.equal(grads["b"], want.to(torch.float16))
    assert not failures, "\n".join(failures)
    # BroadcastScale, scaler (C,) and (1,C,1,1)
    for view in ((-1,), (1, -1, 1, 1)):
        x = t["x"].clone().requires_grad_()
        sc = t["gamma"].reshape(view).clone().requires_grad_()
        y = ops.broadcast_scale(x, sc)
        gx, gs = torch.autograd.grad(y, (x, sc), t["dy"], allow_unused=True)
        assert gs is None
        x2 = t["x"].clone().requires_grad_()
        yt = x2 * t["gamma"].view(1, -1, 1, 1)
        assert torch.equal(y.detach(), yt.detach()) and torch.equal(gx, torch.autograd.grad(yt, (x2,), t["dy"])[0])
        assert mr.same_bits(_np(y), forms[(False, False, False)]["y"])
        assert mr.same_bits(_np(gx), forms[(False, False, False)]["dx"])


@pytest.mark.gpu
def test_wrapper_refuses_what_the_kernels_do_not_take(ops):
    import torch
    x = torch.zeros((2, 4, 3, 3), device="cuda")
    g = torch.ones(4, device="cuda")
    with pytest.raises(ValueError, match="act must be"):
        ops.scale_bias_act_forward(x, g, act="sigmoid")
    with pytest.raises(ValueError, match="gamma must have shape"):
        ops.scale_bias_act_forward(x, torch.ones(5, device="cuda"))
    with pytest.raises(TypeError):
        ops.scale_bias_act_forward(x, g.half())
    with pytest.raises(TypeError):
        ops.scale_bias_act_forward(x.double(), g.double())
    with pytest.raises(ValueError, match="needs y"):
        ops.scale_bias_act_backward(x, None, g, "relu")
    with pytest.raises(RuntimeError, match="GPU"):
        ops.scale_bias_act_forward(x.cpu(), g.cpu())
    e = torch.zeros((0, 4, 3, 3), device="cuda")
    assert ops.scale_bias_act_forward(e, g, act="relu").shape == e.shape
    assert ops.scale_bias_act_backward(e, e, g, "relu", need_dbeta=True)[2].tolist() == [0.0] * 4
