"""The FPN top-down pathway (simpledet_amd/csrc/fpn_topdown.hip) against the restatement of tests/fpn_topdown_ref.py.

  CPU: argument validation of the four C entry points (every case fails, or succeeds, before any launch); the
       restatement's known answers by hand, against the torch CPU composition (forward bit-equal in both dtypes,
       float32 backward bit-equal) and against float64 autograd (k <= 2 (L-1) units of eps * T, T the same graph on
       the absolute gradients: every element passes at most 4 rounded adds per level, and half of the sum of their
       relative errors is the bound of a sum of non-negative terms); L levels equal chained two-level steps.
  GPU: every output BIT-EQUAL to the restatement (a NaN matches any NaN) on every chain x dtype, with NULL inner
       gradients, with each d_lateral left out, at pointers off the 16-byte boundary between sentinels, on the value
       edges, from a replayed graph, chained and through autograd; the forward bit-equal to the torch composition
       on the device; the backward against torch on the device is printed in k, not asserted by bits.
  One thing the contract itself decides: in float16 the fused backward rounds g_l + S_l ONCE (S_l stays float32),
  while a chain of two-level calls has to round S_l to half before an add outside it rounds again.  So the
  chained comparison is by bits in float32 and, in float16, in the forward and wherever the inner gradients are
  NULL; with inner gradients in float16 the chain is a different function and is not compared.
"""
import ctypes
import functools

import numpy as np
import pytest

from simpledet_amd import _lib

from . import fpn_topdown_ref as fr

F, H = fr.F, fr.H
DTYPES = ["float32", "float16"]
P = 4096           # never dereferenced: every CPU case returns before any launch
E = _lib.SimpleDetOpsError


# ------------------------------------------------------------------------------------------ CPU --
def _tab(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _call(name, N=2, C=3, hs=(2, 4), ws=(3, 6), L=None, top=P, ins="auto", outs="auto", tables=(True, True),
          hsws=(True, True)):
    """fwd: (top, lateral[], out[]); bwd: (g[], d_top, d_lateral[]).  Every tensor gets its own 1 MiB range."""
    L = len(hs) if L is None else L
    n = max(len(hs) - 1, 1)
    ins = [P + (1 + k) * (1 << 20) for k in range(n)] if ins == "auto" else list(ins)
    outs = [P + (9 + k) * (1 << 20) for k in range(n)] if outs == "auto" else list(outs)
    a = _tab(ins) if tables[0] else None
    b = _tab(outs) if tables[1] else None
    dims = (_ints(hs) if hsws[0] else None, _ints(ws) if hsws[1] else None)
    if "fwd" in name:
        return _lib.lib().call(name, top, a, b, N, C, dims[0], dims[1], L, None)
    return _lib.lib().call(name, a, top, b, N, C, dims[0], dims[1], L, None)


ENTRY = ["sd_fpn_topdown_fwd", "sd_fpn_topdown_fwd_f16", "sd_fpn_topdown_bwd", "sd_fpn_topdown_bwd_f16"]


@pytest.mark.parametrize("name", ENTRY)
def test_entry_points_reject_bad_arguments_without_a_gpu(name):
    fwd = "fwd" in name
    esz = 2 if name.endswith("f16") else 4
    assert_code = lambda e, c: e.value.code == c   # noqa: E731
    # L out of range
    for hs in ((2,), (1,) * 7):
        with pytest.raises(E, match="outside 2..6") as e:
            _call(name, hs=hs, ws=hs)
        assert assert_code(e, -1)
    with pytest.raises(E, match="outside 2..6"):
        _call(name, L=0)
    # sizes
    for kw in (dict(N=-1), dict(C=-3)):
        with pytest.raises(E, match="negative dimension") as e:
            _call(name, **kw)
        assert assert_code(e, -1)
    for kw in (dict(hs=(0, 0)), dict(ws=(3, 0)), dict(hs=(-2, 4)), dict(ws=(3, -6))):
        with pytest.raises(E, match="non-positive dimension") as e:
            _call(name, **kw)
        assert assert_code(e, -1)
    for kw in (dict(hs=(2, 5)), dict(ws=(3, 7)), dict(hs=(2, 4, 9), ws=(3, 6, 12)), dict(hs=(2, 4, 8), ws=(3, 6, 13))):
        with pytest.raises(E, match="larger than twice") as e:
            _call(name, **kw)
        assert assert_code(e, -1)
    # null pointers: the size tables, the pointer tables, top / d_top, a required entry
    for kw in (dict(hsws=(False, True)), dict(hsws=(True, False)), dict(top=None), dict(tables=(False, True))):
        with pytest.raises(E, match="null pointer") as e:
            _call(name, **kw)
        assert assert_code(e, -1)
    three = dict(hs=(2, 4, 8), ws=(3, 6, 12))
    if fwd:
        with pytest.raises(E, match="null pointer"):
            _call(name, tables=(True, False))
        for k in (0, 1):
            for which in ("ins", "outs"):
                tab = [P + (1 + j + (8 if which == "outs" else 0)) * (1 << 20) for j in range(2)]
                tab[k] = None
                with pytest.raises(E, match="null pointer") as e:
                    _call(name, **three, **{which: tab})
                assert assert_code(e, -1)
    else:
        # the finest gradient is required; inner gradients, every d_lateral and the d_lateral table are optional
        with pytest.raises(E, match="finest") as e:
            _call(name, **three, ins=[P + (1 << 20), None])
        assert assert_code(e, -1)
    # element alignment
    with pytest.raises(E, match="not aligned") as e:
        _call(name, top=P + 1)
    assert assert_code(e, -1)
    with pytest.raises(E, match="not aligned"):
        _call(name, ins=[P + (1 << 20) + 1])
    with pytest.raises(E, match="not aligned"):
        _call(name, outs=[P + (9 << 20) + esz // 2])
    # an output that overlaps an input: the same range, and by one element at either end
    n_top, n_fine = 2 * 3 * 2 * 3 * esz, 2 * 3 * 4 * 6 * esz
    base = P + (1 << 20)
    for out in (base, base + n_fine - esz, base - n_fine + esz):
        with pytest.raises(E, match="overlaps") as e:
            _call(name, outs=[out])
        assert assert_code(e, -1)
    if fwd:
        with pytest.raises(E, match="overlaps"):          # out_1 over top
            _call(name, outs=[P + n_top - esz])
    else:
        with pytest.raises(E, match="overlaps"):          # d_top over g_1
            _call(name, top=base + n_fine - esz)
    # more than 2^31 - 1 elements in one tensor: 2 x 1024 x 1024 x 1024 = 2^31 at the fine level only
    with pytest.raises(E, match="exceed the limit") as e:
        _call(name, N=2, C=1024, hs=(512, 1024), ws=(512, 1024))
    assert assert_code(e, _lib.SD_ERR_UNSUPPORTED)
    # N * C = 0 succeeds without touching the device, whatever the pointers; its L is still checked
    for kw in (dict(N=0), dict(C=0)):
        assert _call(name, top=None, tables=(False, False), **kw) == 0
    with pytest.raises(E, match="outside 2..6"):
        _call(name, N=0, L=7)


def test_restatement_known_answers_by_hand():
    for dt in (F, H):
        # 1x1 -> 2x2
        top = np.array([[[[3.0]]]], dt)
        lat = np.array([[[[1.0, 2.0], [4.0, 8.0]]]], dt)
        assert np.array_equal(fr.fwd(top, [lat])[0], np.array([[[[4.0, 5.0], [7.0, 11.0]]]], dt))
        d_top, d_lat = fr.bwd([lat], [top.shape, lat.shape])
        assert d_top.dtype == dt and np.array_equal(d_top, np.array([[[[15.0]]]], dt)) and d_lat[0] is lat
        # a cropped 1x2 window: 1x1 -> 1x2 keeps the window's first row
        lat = np.array([[[[1.0, 2.0]]]], dt)
        assert np.array_equal(fr.fwd(top, [lat])[0], np.array([[[[4.0, 5.0]]]], dt))
        assert np.array_equal(fr.bwd([lat], [top.shape, lat.shape])[0], np.array([[[[3.0]]]], dt))
        # 3x4 -> 4x5: the coarse row 2 and column 3 lose their whole window and get +0.0, written, not -0.0
        g = -np.ones((1, 1, 4, 5), dt)
        d_top = fr.bwd([g], [(1, 1, 3, 4), g.shape])[0]
        want = np.array([[-4, -4, -2, 0], [-4, -4, -2, 0], [0, 0, 0, 0]], dt)[None, None]
        assert np.array_equal(d_top, want) and not np.signbit(d_top[0, 0, 2]).any() and not np.signbit(d_top[0, 0, :, 3]).any()
        # a window of -0.0 sums to +0.0: the sum starts at +0.0
        z = np.full((1, 1, 2, 2), -0.0, dt)
        assert not np.signbit(fr.bwd([z], [(1, 1, 1, 1), z.shape])[0]).any()


def _torch_composition(top, lats, grads, device="cpu"):
    """interpolate(nearest) -> slice -> add with autograd, in the tensors' own dtype"""
    import torch
    import torch.nn.functional as Fn
    t = torch.from_numpy(top).to(device).requires_grad_(True)
    ls = [torch.from_numpy(x).to(device).requires_grad_(True) for x in lats]
    outs, p = [], t
    for lat in ls:
        p = Fn.interpolate(p, scale_factor=2, mode="nearest")[:, :, :lat.shape[2], :lat.shape[3]] + lat
        outs.append(p)
    live = [(o, torch.from_numpy(g).to(device)) for o, g in zip(outs, grads) if g is not None]
    torch.autograd.backward([o for o, _ in live], [g for _, g in live])
    return ([o.detach().cpu().numpy() for o in outs], t.grad.cpu().numpy(), [x.grad.cpu().numpy() for x in ls])


CPU_CHAINS = ["crop23", "ones", "crop1_mixed", "even_odd", "L5"]


@pytest.mark.parametrize("chain", CPU_CHAINS)
@pytest.mark.parametrize("dtname", DTYPES)
def test_restatement_against_the_torch_cpu_composition(chain, dtname):
    dt = np.dtype(dtname).type
    top, lats, grads = fr.make(np.random.RandomState(3), fr.CHAINS[chain], dt)
    outs, d_top, d_lat = _torch_composition(top, lats, grads)
    for l, (got, want) in enumerate(zip(fr.fwd(top, lats), outs)):
        assert fr.same_bits(got, want), (chain, dtname, "out", l + 1)
    if dt is F:   # (float16: torch accumulates wider; the half backward is held to the float64 truth instead)
        r_top, r_lat = fr.bwd(grads, [top.shape] + [x.shape for x in lats])
        assert fr.same_bits(r_top, d_top), (chain, "d_top")
        for l, (got, want) in enumerate(zip(r_lat, d_lat)):
            assert fr.same_bits(got, want), (chain, "d_lateral", l + 1)


@pytest.mark.parametrize("chain", CPU_CHAINS)
@pytest.mark.parametrize("dtname", DTYPES)
def test_restatement_against_float64_autograd(chain, dtname):
    dt = np.dtype(dtname).type
    top, lats, grads = fr.make(np.random.RandomState(4), fr.CHAINS[chain], dt)
    L = len(lats) + 1
    outs, d_top, d_lat, a_top, a_lat = fr.truth64(top, lats, grads)
    r_top, r_lat = fr.bwd(grads, [top.shape] + [x.shape for x in lats])
    ks = [fr.k_units(r_top, d_top, a_top, dt)] + [fr.k_units(g, w, s, dt) for g, w, s in zip(r_lat, d_lat, a_lat)]
    print("%s %s: backward k = %s (bound %d)" % (chain, dtname, ["%.2f" % k for k in ks], 2 * (L - 1)))
    assert max(ks) <= 2 * (L - 1), (chain, dtname, ks)
    # the forward adds once per level: half a unit of the result per level, relative to sum |terms|
    p = np.abs(top.astype(np.float64))
    for l, lat in enumerate(lats):
        p = fr.up_crop(p, lat.shape[2], lat.shape[3]) + np.abs(lat.astype(np.float64))
        k = fr.k_units(fr.fwd(top, lats)[l], outs[l], p, dt)
        assert k <= 0.5 * (l + 1) * (1 + np.finfo(dt).eps) ** (l + 1), (chain, dtname, "out", l + 1, k)


def _check_chained(fused, chained, dt, inner_given, what):
    """by bits -- but for float16 with inner gradients (module docstring), where nothing is compared: the two
    roundings of the chain are a different function, and a cancelling g_l + S_l magnifies the difference at will"""
    if dt is H and inner_given:
        return
    f_top, f_lat = fused
    c_top, c_lat = chained
    pairs = [("d_top", f_top, c_top)] + [("d_lateral_%d" % (l + 1), a, b) for l, (a, b) in enumerate(zip(f_lat, c_lat))]
    for name, a, b in pairs:
        assert fr.same_bits(a, b), (what, name)


@pytest.mark.parametrize("chain", ["crop1_mixed", "even_odd", "L5", "L6"])
@pytest.mark.parametrize("dtname", DTYPES)
def test_restatement_of_l_levels_equals_chained_two_level_steps(chain, dtname):
    dt = np.dtype(dtname).type
    top, lats, grads = fr.make(np.random.RandomState(5), fr.CHAINS[chain], dt)
    shapes = [top.shape] + [x.shape for x in lats]
    for a, b in zip(fr.fwd(top, lats), fr.fwd_chained(top, lats)):
        assert fr.same_bits(a, b)
    _check_chained(fr.bwd(grads, shapes), fr.bwd_chained(grads, shapes), dt, True, chain)
    inner_null = [None] * (len(grads) - 1) + [grads[-1]]
    _check_chained(fr.bwd(inner_null, shapes), fr.bwd_chained(inner_null, shapes), dt, False, chain)


# ------------------------------------------------------------------------------------------ GPU --
SENTINEL = -777.5      # a half as well
PAD = 64


def _tdt(dt):
    import torch
    return torch.float32 if np.dtype(dt) == np.dtype(F) else torch.float16


def _dev(a, off=0):
    """a device copy of `a` (an uninitialised, NaN-filled tensor for a (shape, dtype) tuple) whose data pointer lies
    `off` elements behind a 16-byte boundary, in the middle of a sentinel-filled buffer -> (tensor, intact)"""
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
    if src is not None:
        t.copy_(torch.from_numpy(src))
    else:
        t.fill_(float("nan"))

    def intact():
        return bool(torch.all(buf[:PAD + off] == SENTINEL) and torch.all(buf[PAD + off + n:] == SENTINEL))
    return t, intact


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(chain, dtname, N=2, C=3, seed=11):
    """inputs and the restatement's results, computed once and shared (read-only)"""
    dt = np.dtype(dtname).type
    spatial = fr.FPN_CHAIN if chain == "fpn" else fr.CHAINS[chain]
    top, lats, grads = fr.make(np.random.RandomState(seed), spatial, dt, N, C)
    shapes = [top.shape] + [x.shape for x in lats]
    d_top, d_lat = fr.bwd(grads, shapes)
    case = dict(top=top, lats=lats, grads=grads, shapes=shapes, outs=fr.fwd(top, lats), d_top=d_top, d_lat=d_lat)
    return case


def _run(ops, case, off=0, grads=None, d_laterals=None, want_finest=False):
    """forward and backward on the device at pointer phase `off`; returns numpy results and asserts the sentinels"""
    dt = case["top"].dtype
    checks = []

    def dev(a):
        t, chk = _dev(a, off)
        checks.append(chk)
        return t
    top, lats = dev(case["top"]), [dev(x) for x in case["lats"]]
    outs = ops.fpn_topdown_forward(top, lats, outs=[dev((x.shape, dt)) for x in case["lats"]])
    grads = case["grads"] if grads is None else grads
    g = [None if x is None else dev(x) for x in grads]
    if d_laterals is None:
        d_laterals = [dev((s, dt)) for s in case["shapes"][1:-1]] + [None]
    else:
        d_laterals = [dev((case["shapes"][k + 1], dt)) if v is True else v for k, v in enumerate(d_laterals)]
    d_top, d_lat = ops.fpn_topdown_backward(g, case["shapes"], d_top=dev((case["shapes"][0], dt)),
                                            d_laterals=d_laterals, want_finest=want_finest)
    import torch
    torch.cuda.synchronize()
    assert all(chk() for chk in checks), "a sentinel was overwritten"
    finest_is_input = d_lat[-1] is g[-1]
    return [_np(o) for o in outs], _np(d_top), [_np(x) for x in d_lat], finest_is_input


GPU_CHAINS = ["crop1_mixed", "crop23", "ones", "even_odd", "L5", "L6", "L6_wide", "L2_wide"]


@pytest.mark.gpu
@pytest.mark.parametrize("chain", GPU_CHAINS)
@pytest.mark.parametrize("dtname", DTYPES)
def test_hip_matches_the_restatement(ops, chain, dtname):
    """N = 2, C = 3 with odd plane sizes: plane starts fall on every alignment phase.  L6_wide and L2_wide are the
    shapes whose level-0 width exceeds the tile (16 columns at L = 6, 4096 at L = 2): three column tiles, the last
    partial."""
    N, C = (1, 1) if chain == "L2_wide" else (2, 3)
    case = _case(chain, dtname, N, C)
    outs, d_top, d_lat, alias = _run(ops, case)
    for l, (got, want) in enumerate(zip(outs, case["outs"])):
        assert fr.same_bits(got, want), (chain, dtname, "out", l + 1)
    assert fr.same_bits(d_top, case["d_top"]), (chain, dtname, "d_top")
    for l, (got, want) in enumerate(zip(d_lat, case["d_lat"])):
        assert fr.same_bits(got, want), (chain, dtname, "d_lateral", l + 1)
    assert alias                                              # the finest gradient came back as the input itself


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTYPES)
def test_hip_the_config_chain_spans_several_tiles(ops, dtname):
    """25x42 -> 50x84 -> 100x167 -> 200x334 at N = 1, C = 2 (0.5 MB): the level-0 tile is 6 rows x 42 columns at
    L = 4, so the 25 rows are five row tiles, the last of one row; the columns are not tiled here (L6_wide and
    L2_wide above tile them).  Forward also bit-equal to the torch composition on the device; the backward against
    torch on the device is printed in k."""
    case = _case("fpn", dtname, 1, 2)
    outs, d_top, d_lat, _ = _run(ops, case, want_finest=True)
    assert "tile=6x42 tiles=5x1" in (_lib.lib().cdll.sd_last_dispatch() or b"").decode()
    t_outs, t_top, t_lat = _torch_composition(case["top"], case["lats"], case["grads"], "cuda")
    for l in range(3):
        assert fr.same_bits(outs[l], case["outs"][l]) and fr.same_bits(outs[l], t_outs[l]), (dtname, "out", l + 1)
        assert fr.same_bits(d_lat[l], case["d_lat"][l]), (dtname, "d_lateral", l + 1)
    assert fr.same_bits(d_top, case["d_top"])
    _, w_top, w_lat, a_top, a_lat = fr.truth64(case["top"], case["lats"], case["grads"])
    dt = case["top"].dtype.type
    k_hip = [fr.k_units(d_top, w_top, a_top, dt)] + [fr.k_units(g, w, s, dt) for g, w, s in zip(d_lat, w_lat, a_lat)]
    k_torch = [fr.k_units(t_top, w_top, a_top, dt)] + [fr.k_units(g, w, s, dt) for g, w, s in zip(t_lat, w_lat, a_lat)]
    print("%s backward k against float64: hip %s, torch on the device %s; equal bits with torch: %s"
          % (dtname, ["%.2f" % k for k in k_hip], ["%.2f" % k for k in k_torch],
             [fr.same_bits(d_top, t_top)] + [fr.same_bits(a, b) for a, b in zip(d_lat, t_lat)]))
    assert max(k_hip) <= 2 * 3


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTYPES)
def test_hip_null_inner_gradients_and_left_out_laterals(ops, dtname):
    case = _case("even_odd", dtname)
    shapes, grads = case["shapes"], case["grads"]
    # every subset of the inner gradients NULL
    for mask in ((0, 0), (1, 0), (0, 1)):
        gs = [None if (k < 2 and not mask[k]) else g for k, g in enumerate(grads)]
        w_top, w_lat = fr.bwd(gs, shapes)
        _, d_top, d_lat, _ = _run(ops, case, grads=gs)
        assert fr.same_bits(d_top, w_top), (dtname, mask)
        for l in range(3):
            assert fr.same_bits(d_lat[l], w_lat[l]), (dtname, mask, l + 1)
    # each d_lateral left out in turn (False: not stored), the rest unchanged
    for skip in range(3):
        dl = [False if k == skip else True for k in range(3)]
        _, d_top, d_lat, alias = _run(ops, case, d_laterals=dl)
        assert d_lat[skip] is None and not alias
        assert fr.same_bits(d_top, case["d_top"]), (dtname, skip)
        for l in range(3):
            if l != skip:
                assert fr.same_bits(d_lat[l], case["d_lat"][l]), (dtname, skip, l + 1)
    # want_finest: a buffer of its own with the same bits
    _, _, d_lat, alias = _run(ops, case, want_finest=True)
    assert not alias and fr.same_bits(d_lat[2], grads[2])


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTYPES)
@pytest.mark.parametrize("chain", ["crop1_mixed", "even_odd"])
def test_hip_pointers_off_the_16_byte_boundary(ops, chain, dtname):
    """every tensor one element (4 bytes, 2 for half) behind a 16-byte boundary, and at every other phase of the
    output item: equal bits, sentinels untouched (checked inside _run)"""
    case = _case(chain, dtname)
    per16 = 16 // np.dtype(dtname).itemsize
    for off in (1, 2, 3, per16 - 1):
        outs, d_top, d_lat, _ = _run(ops, case, off=off, want_finest=True)
        for l in range(3):
            assert fr.same_bits(outs[l], case["outs"][l]), (chain, dtname, off, "out", l + 1)
            assert fr.same_bits(d_lat[l], case["d_lat"][l]), (chain, dtname, off, "d_lateral", l + 1)
        assert fr.same_bits(d_top, case["d_top"]), (chain, dtname, off)


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTYPES)
def test_hip_value_edges(ops, dtname):
    """+-inf, NaN and -0.0 windows; in float16 overflow to inf on the final rounding (65504 + 65504) and subnormals"""
    dt = np.dtype(dtname).type
    spatial = [(2, 3), (4, 5), (7, 10)]
    top, lats, grads = fr.make(np.random.RandomState(21), spatial, dt, 1, 2)
    inf, nan = float("inf"), float("nan")
    g = grads[1]
    g[0, 0, 0:2, 0:2] = [[inf, 1], [1, 1]]           # a window with +inf
    g[0, 0, 0:2, 2:4] = [[inf, -inf], [1, 1]]        # +inf and -inf: NaN
    g[0, 0, 2:4, 0:2] = [[nan, 1], [1, 1]]
    g[0, 0, 2:4, 2:4] = -0.0                         # a window of -0.0 sums to +0.0
    g[0, 1, 0:2, 0:2] = 0.0
    grads[0][0, 0, 1, 1] = -0.0                      # -0.0 + (+0.0) = +0.0
    grads[0][0, 1, 0, 0] = -0.0
    lats[0][0, 0, 0, 0], top[0, 0, 0, 0] = -0.0, -0.0  # -0.0 + -0.0 = -0.0 forward
    lats[1][0, 1, 0, 0] = inf
    top[0, 1, 1, 2] = nan
    if dt is H:
        top[0, 0, 1, 0] = 65504
        lats[0][0, 0, 2:4, 0:2] = 65504              # 65504 + 65504 overflows on the rounding
        g[0, 1, 4:6, 4:6] = 65504                    # the float32 window sum 262016 rounds to inf
        g[0, 1, 4:6, 6:8] = [[6e-8, 6e-8], [6e-8, 0]]   # subnormal halves sum exactly in float32
        lats[1][0, 1, 6, 0:4] = 6e-8
        grads[0][0, 1, 3, 3] = 6e-8
    shapes = [top.shape] + [x.shape for x in lats]
    case = dict(top=top, lats=lats, grads=grads, shapes=shapes)
    w_outs, (w_top, w_lat) = fr.fwd(top, lats), fr.bwd(grads, shapes)
    assert np.isnan(w_lat[0][0, 0, 0, 1]) and np.isnan(w_lat[0][0, 0, 1, 0]) and np.isinf(w_lat[0][0, 0, 0, 0])
    assert w_lat[0][0, 0, 1, 1] == 0 and not np.signbit(w_lat[0][0, 0, 1, 1])
    assert np.signbit(w_outs[0][0, 0, 0, 0])
    if dt is H:
        assert np.isinf(w_outs[0][0, 0, 2, 0]) and np.isinf(w_lat[0][0, 1, 2, 2])
    outs, d_top, d_lat, _ = _run(ops, case)
    for l in range(2):
        assert fr.same_bits(outs[l], w_outs[l]), (dtname, "out", l + 1)
        assert fr.same_bits(d_lat[l], w_lat[l]), (dtname, "d_lateral", l + 1)
    assert fr.same_bits(d_top, w_top)


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTYPES)
def test_hip_two_calls_give_equal_bits_and_l_levels_equal_chained_steps(ops, dtname):
    import torch
    dt = np.dtype(dtname).type
    case = _case("even_odd", dtname)
    first, second = _run(ops, case), _run(ops, case, off=1)
    for a, b in zip(first[0] + [first[1]] + first[2], second[0] + [second[1]] + second[2]):
        assert fr.same_bits(a, b)
    # chained two-level calls on the device
    top = torch.from_numpy(case["top"]).cuda()
    lats = [torch.from_numpy(x).cuda() for x in case["lats"]]
    p = top
    for l, lat in enumerate(lats):
        p = ops.fpn_topdown_forward(p, [lat])[0]
        assert fr.same_bits(_np(p), first[0][l]), (dtname, "out", l + 1)
    shapes = case["shapes"]
    for inner_given in (True, False):
        gs = [g if (inner_given or k == 2) else None for k, g in enumerate(case["grads"])]
        f_top, f_lat = ops.fpn_topdown_backward([None if g is None else torch.from_numpy(g).cuda() for g in gs], shapes)
        D = torch.from_numpy(gs[2]).cuda()
        c_lat = [None, None, D]
        for l in (2, 1, 0):
            S, _ = ops.fpn_topdown_backward([D], [shapes[l], shapes[l + 1]])
            if l == 0:
                c_top = S
                break
            D = S if gs[l - 1] is None else torch.from_numpy(gs[l - 1]).cuda() + S
            c_lat[l - 1] = D
        _check_chained((_np(f_top), [_np(x) for x in f_lat]), (_np(c_top), [_np(x) for x in c_lat]), dt, inner_given,
                       dtname)


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTYPES)
def test_hip_a_replayed_graph_follows_its_inputs(ops, dtname):
    """forward + backward captured once, replayed on CHANGED inputs: the restatement's bits on those inputs"""
    import torch
    dt = np.dtype(dtname).type
    spatial = fr.CHAINS["even_odd"]
    top, lats, grads = fr.make(np.random.RandomState(31), spatial, dt)
    shapes = [top.shape] + [x.shape for x in lats]
    st = [torch.from_numpy(x).cuda() for x in [top] + lats + grads]

    def both():
        outs = ops.fpn_topdown_forward(st[0], st[1:4])
        d_top, d_lat = ops.fpn_topdown_backward(st[4:7], shapes, want_finest=True)
        return outs + [d_top] + d_lat
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap = both()
    for seed in (32, 33):
        top, lats, grads = fr.make(np.random.RandomState(seed), spatial, dt)
        for t, v in zip(st, [top] + lats + grads):
            t.copy_(torch.from_numpy(v))
        for o in cap:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        w_top, w_lat = fr.bwd(grads, shapes)
        for name, got, want in zip("out1 out2 out3 d_top d_lat1 d_lat2 d_lat3".split(), cap,
                                   fr.fwd(top, lats) + [w_top] + w_lat):
            assert fr.same_bits(_np(got), want), (seed, name)


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTYPES)
def test_hip_autograd_wrapper(ops, dtname):
    """the wrapper's gradients are fpn_topdown_backward's; nothing is saved for the backward"""
    import torch
    case = _case("crop1_mixed", dtname)
    top = torch.from_numpy(case["top"]).cuda().requires_grad_(True)
    lats = [torch.from_numpy(x).cuda().requires_grad_(True) for x in case["lats"]]
    outs = ops.fpn_topdown(top, lats)
    assert outs[0].grad_fn is not None and len(outs[0].grad_fn.saved_tensors) == 0
    for l in range(3):
        assert fr.same_bits(_np(outs[l]), case["outs"][l])
    gs = [torch.from_numpy(g).cuda() for g in case["grads"]]
    torch.autograd.backward(outs, gs)
    assert fr.same_bits(_np(top.grad), case["d_top"])
    for l in range(3):
        assert fr.same_bits(_np(lats[l].grad), case["d_lat"][l]), (dtname, l + 1)
    # an output without a consumer: its gradient is NULL, not a tensor of zeros
    top2 = torch.from_numpy(case["top"]).cuda().requires_grad_(True)
    lats2 = [torch.from_numpy(x).cuda().requires_grad_(i != 1) for i, x in enumerate(case["lats"])]
    outs2 = ops.fpn_topdown(top2, lats2)
    torch.autograd.backward([outs2[0], outs2[2]], [gs[0], gs[2]])
    w_top, w_lat = fr.bwd([case["grads"][0], None, case["grads"][2]], case["shapes"])
    assert fr.same_bits(_np(top2.grad), w_top) and fr.same_bits(_np(lats2[0].grad), w_lat[0])
    assert lats2[1].grad is None and fr.same_bits(_np(lats2[2].grad), w_lat[2])


@pytest.mark.gpu
def test_hip_the_wrapper_refuses_bad_tensors(ops):
    import torch
    case = _case("crop23", "float32")
    top = torch.from_numpy(case["top"]).cuda()
    lat = torch.from_numpy(case["lats"][0]).cuda()
    with pytest.raises(E, match="overlaps"):                               # an output over an input
        ops.fpn_topdown_forward(top, [lat], outs=[lat])
    with pytest.raises(E, match="overlaps"):
        ops.fpn_topdown_backward([lat], case["shapes"], d_laterals=[lat])
    with pytest.raises(TypeError):                                         # dtypes
        ops.fpn_topdown_forward(top, [lat.half()])
    with pytest.raises(TypeError):
        ops.fpn_topdown_forward(top.double(), [lat.double()])
    with pytest.raises(TypeError):
        ops.fpn_topdown_backward([lat.half()], case["shapes"], d_top=torch.empty_like(top))
    with pytest.raises(ValueError, match="contiguous"):
        ops.fpn_topdown_forward(top, [lat.transpose(2, 3).contiguous().transpose(2, 3)])
    with pytest.raises(ValueError, match="contiguous"):
        ops.fpn_topdown_forward(top.transpose(2, 3).contiguous().transpose(2, 3), [lat])
    with pytest.raises(ValueError, match=r"\(N,C\)"):                      # mismatched N / C
        ops.fpn_topdown_forward(top, [lat[:1].contiguous()])
    with pytest.raises(ValueError, match=r"\(N,C\)"):
        ops.fpn_topdown_forward(top, [lat[:, :2].contiguous()])
    with pytest.raises(ValueError, match="larger than twice"):
        ops.fpn_topdown_forward(top[:, :, :1].contiguous(), [lat])
    with pytest.raises(ValueError, match="must have shape"):
        ops.fpn_topdown_backward([lat], [(2, 3, 3, 4), (2, 3, 4, 4)])
    with pytest.raises(ValueError, match="finest"):
        ops.fpn_topdown_backward([None], case["shapes"])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.fpn_topdown_forward(top.cpu(), [lat.cpu()])
