"""DeformableConvolution at non-square kernels and per-axis pad / stride / dilate.

Every other DCN test drives the op with kernel (k, k) and one scalar each for pad, stride and dilate, so a body
that reads pad_h for pad_w, decodes a tap as tap / kh, or sizes the offsets as 2*kh*kh would pass them all.  The
piece entry points (sd_deform_im2col / _col2im / _col2im_ws / _col2im_coord) take all six geometry values; here
they get values that differ per axis, on every kernel body the launchers of csrc/deform_sample.hip choose from.

CPU (unmarked): the C oracle at the new geometry against three statements that share no code with it --
torch.nn.functional.unfold (zero offsets, bit for bit), tests/dcn_torch_ref.py with autograd (random offsets), and
the transposition relation (the problem with both axes swapped gives the transposed col matrix) -- and the
argument refusals of make_geom(), which run before any device access.
GPU: the pieces against the oracle under the default knobs and with each kernel family switched off, and the
transposition relation on im2col and on the fused forward (which has no oracle pin of its own).

Bars (none is new): im2col bit-equal; col2im / col2im_coord rtol = atol = 1e-4 (test_deform_conv.py); oracle vs
fp64: 4e-6 x max(1, max|col|) and 1e-5 relative (test_deform_conv_autograd.py); `_bar` for the convolution.
The transposition bound is derived: swapping the axes swaps the two middle terms of the four-term bilinear sum
w1 v1 + w2 v2 + w3 v3 + w4 v4 (w2 = hh*lw <-> w3 = lh*hw; the products are commutative, so the same bits), hence
only the order of the sum changes; each order is at most 3 roundings of partial sums bounded by max|x| (the
weights are a convex combination) away from the exact value: |difference| <= 6 x 2^-24 x max|x|, asserted as
8 x 2^-24 x max|x|.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from . import dcn_torch_ref as R
from .test_deform_conv import _bar
from .test_deform_conv_autograd import _rel

# name -> kernel, pad (h, w), stride (h, w), dilate (h, w) [, C, H, W, N, scale]; default N=2, C=8, dg=2, H=12,
# W=16, offset scale 1.5.  The comment names the launcher conditions of sd_deform_im2col / col2im_impl /
# sd_deform_col2im_coord each row satisfies (P = Ho*Wo, cpg = C / dg = 4 unless said otherwise).
TABLE = {
    # kh*kw == 9 && kw == 3 && H*W % 4 == 0 && cpg >= 2 && P % 4 == 0: pipe im2col; cpg % 4 == 0 && P % 4 == 0:
    # four-channel col2im, fixed point with a workspace; coord <T,9>
    "A": dict(kernel=(3, 3), pad=(2, 1), stride=(1, 1), dil=(2, 1), out=(12, 16)),
    "B": dict(kernel=(3, 3), pad=(1, 2), stride=(1, 1), dil=(1, 2), out=(12, 16)),   # as A, other axis
    "C": dict(kernel=(3, 3), pad=(1, 1), stride=(2, 1), dil=(1, 1), out=(6, 16)),    # as A, P = 96
    "D": dict(kernel=(3, 3), pad=(1, 1), stride=(1, 2), dil=(1, 1), out=(12, 8)),    # as A, P = 96
    # P = 30, P % 4 != 0: im2col <T,9> without the pipe, one-channel col2im; coord <T,9>
    "E": dict(kernel=(3, 3), pad=(0, 3), stride=(2, 3), dil=(1, 2), out=(5, 6)),
    # kh*kw = 3 != 9: im2col <T,0>, coord <T,0>; four-channel col2im (P = 192)
    "F": dict(kernel=(1, 3), pad=(0, 1), stride=(1, 1), dil=(1, 1), out=(12, 16)),
    "G": dict(kernel=(3, 1), pad=(1, 0), stride=(1, 1), dil=(1, 1), out=(12, 16)),   # as F, other axis
    # six taps, P = 91: <T,0> twice, one-channel col2im
    "H": dict(kernel=(2, 3), pad=(1, 0), stride=(1, 2), dil=(1, 1), out=(13, 7)),
    # kh*kw = 15 > kDcnMaxTaps: per-lane im2col and coord; four-channel (chunk) col2im, P = 96
    "I": dict(kernel=(3, 5), pad=(1, 2), stride=(2, 1), dil=(1, 1), out=(6, 16)),
    "J": dict(kernel=(5, 3), pad=(2, 1), stride=(1, 1), dil=(1, 1), out=(12, 16)),   # as I, other axis, P = 192
    # kh*kw == 9 but kw != 3: im2col <T,9> (never the pipe, which decodes tap / 3), coord <T,9>; four-channel col2im
    "K": dict(kernel=(1, 9), pad=(0, 4), stride=(1, 1), dil=(1, 1), out=(12, 16)),
    "L": dict(kernel=(9, 1), pad=(4, 0), stride=(1, 1), dil=(1, 1), out=(12, 16)),   # as K, other axis
    # six taps, every pair differs: <T,0> twice, four-channel col2im (P = 96)
    "M": dict(kernel=(3, 2), pad=(2, 0), stride=(1, 2), dil=(2, 1), out=(12, 8)),
}
EXTRA = {
    # cpg = 1: cpg >= 2 fails -> im2col <T,9> without the pipe; cpg % 4 != 0 -> one-channel col2im
    "A_C2": dict(TABLE["A"], C=2),
    # H*W = 99, H*W % 4 != 0: scalar staging (vec = 0) -> no pipe; P = 99 -> one-channel col2im
    "B_9x11": dict(TABLE["B"], H=9, W=11, out=(9, 11)),
    # (H*W + W + 8) * 4 > 64 KB: per-lane im2col and coord; four planes of 67 KB -> four-channel fixed-point
    # col2im in 4 row bands of 25 rows
    "A_100x168": dict(TABLE["A"], H=100, W=168, N=1, scale=3.0, out=(100, 168)),
}
ROWS = dict(TABLE, **EXTRA)
WILD = ("A", "E", "I", "M")     # again with offsets of scale 40: whole-plane windows, most samples outside
GPU_CASES = [(r, None) for r in ROWS] + [(r, 40.0) for r in WILD]
DG = 2


def _geo(row):
    r = ROWS[row]
    return dict(kernel=r["kernel"], pad=r["pad"], stride=r["stride"], dil=r["dil"], dgroup=DG)


def _ops_geo(row):
    r = ROWS[row]
    return dict(kernel=r["kernel"], pad=r["pad"], stride=r["stride"], dilate=r["dil"], num_deformable_group=DG)


@functools.lru_cache(maxsize=None)
def _inputs(row, scale=None):
    """x (N,C,H,W), offset (N, dg*2*kh*kw, Ho, Wo), g (N, C*kh*kw, P): read-only, shared by the tests"""
    r = ROWS[row]
    N, C, H, W = r.get("N", 2), r.get("C", 8), r.get("H", 12), r.get("W", 16)
    kh, kw = r["kernel"]
    Ho, Wo = r["out"]
    scale = r.get("scale", 1.5) if scale is None else scale
    rs = np.random.RandomState(100 + sorted(ROWS).index(row))
    x = rs.standard_normal((N, C, H, W)).astype(np.float32)
    off = (rs.standard_normal((N, DG * 2 * kh * kw, Ho, Wo)) * scale).astype(np.float32)
    g = rs.standard_normal((N, C * kh * kw, Ho * Wo)).astype(np.float32)
    for a in (x, off, g):
        a.flags.writeable = False
    return x, off, g


@functools.lru_cache(maxsize=None)
def _want(row, scale=None):
    """the oracle's col, col2im(g) and col2im_coord(g) for _inputs(row, scale), computed once"""
    from oracle import pyoracle as oracle
    x, off, g = _inputs(row, scale)
    geo = _geo(row)
    n_ = range(x.shape[0])
    out = (np.stack([oracle.deform_im2col(x[n], off[n], **geo) for n in n_]),
           np.stack([oracle.deform_col2im(g[n], off[n], x[n].shape, **geo) for n in n_]),
           np.stack([oracle.deform_col2im_coord(g[n], x[n], off[n], **geo) for n in n_]))
    for a in out:
        a.flags.writeable = False
    return out


def _transposed(row, x, off):
    """the same problem with the two image axes swapped: x^T, kernel (kw, kh), pad / stride / dilate swapped,
    offset'[g, (j, i), 0] = offset[g, (i, j), 1]^T and offset'[g, (j, i), 1] = offset[g, (i, j), 0]^T"""
    r = ROWS[row]
    kh, kw = r["kernel"]
    N, _, Ho, Wo = off.shape
    o = off.reshape(N, DG, kh, kw, 2, Ho, Wo).transpose(0, 1, 3, 2, 4, 6, 5)[:, :, :, :, ::-1]
    geo = dict(kernel=(kw, kh), pad=r["pad"][::-1], stride=r["stride"][::-1], dil=r["dil"][::-1], dgroup=DG)
    return (np.ascontiguousarray(x.transpose(0, 1, 3, 2)),
            np.ascontiguousarray(o).reshape(N, DG * 2 * kh * kw, Wo, Ho), geo)


def _check_transposition(row, col, col_t, x):
    """col'[(c, j, i), (wo, ho)] == col[(c, i, j), (ho, wo)] within the derived bound"""
    kh, kw = ROWS[row]["kernel"]
    Ho, Wo = ROWS[row]["out"]
    N, C = x.shape[:2]
    back = col_t.reshape(N, C, kw, kh, Wo, Ho).transpose(0, 1, 3, 2, 5, 4).reshape(col.shape)
    bound = 8 * 2.0 ** -24 * float(np.abs(x).max())
    err = float(np.abs(back.astype(np.float64) - col.astype(np.float64)).max())
    share = float((col != 0).mean())
    print("transposition %s: err %.3g, bound %.3g, non-zero share %.2f" % (row, err, bound, share))
    assert share >= 0.5, "the relation would hold trivially"
    assert err <= bound, (row, err, bound)


# ------------------------------------------------------------------------------------------ CPU --
def test_the_table_is_what_the_geometry_gives(oracle):
    for row, r in ROWS.items():
        H, W = r.get("H", 12), r.get("W", 16)
        assert oracle._out_hw(H, W, *r["kernel"], r["pad"], r["stride"], r["dil"]) == r["out"], row
    assert oracle._out_hw(9, 11, 3, 3, 1, 2, 1) == oracle._out_hw(9, 11, 3, 3, (1, 1), (2, 2), (1, 1)) == (5, 6)


@pytest.mark.parametrize("row", list(TABLE))
def test_oracle_zero_offsets_is_unfold(oracle, row):
    x, off, _ = _inputs(row)
    r = ROWS[row]
    want = torch.nn.functional.unfold(torch.tensor(x), kernel_size=r["kernel"], dilation=r["dil"],
                                      padding=r["pad"], stride=r["stride"]).numpy()
    zero = np.zeros_like(off[0])
    for n in range(x.shape[0]):
        col = oracle.deform_im2col(x[n], zero, **_geo(row))
        assert col.shape == want[n].shape
        np.testing.assert_array_equal(col, want[n])
    assert float(np.abs(want).max()) > 0


@pytest.mark.parametrize("row", list(TABLE))
def test_oracle_pieces_against_autograd(oracle, row):
    x, off, g = _inputs(row)
    r = ROWS[row]
    geo = (r["kernel"], r["pad"], r["stride"], r["dil"], DG)
    H, W = x.shape[2:]
    off = R.keep_off_the_kinks(torch.tensor(off), H, W, *geo).numpy()
    xt = torch.tensor(x).double().requires_grad_(True)
    ot = torch.tensor(off).double().requires_grad_(True)
    col = R.dcn_col(xt, ot, *geo)
    (col.reshape(g.shape) * torch.tensor(g).double()).sum().backward()
    col = col.detach().numpy().reshape(g.shape)
    ocol = np.stack([oracle.deform_im2col(x[n], off[n], **_geo(row)) for n in range(x.shape[0])])
    odx = np.stack([oracle.deform_col2im(g[n], off[n], x[n].shape, **_geo(row)) for n in range(x.shape[0])])
    odo = np.stack([oracle.deform_col2im_coord(g[n], x[n], off[n], **_geo(row)) for n in range(x.shape[0])])
    err = float(np.abs(ocol - col).max())
    print("row %s: col %.3g, dX %.3g, dOffset %.3g" % (row, err, _rel(odx, xt.grad.numpy()),
                                                      _rel(odo, ot.grad.numpy())))
    assert err <= 4e-6 * max(1.0, float(np.abs(col).max()))
    assert _rel(odx, xt.grad.numpy()) <= 1e-5, "d_data (deformable_col2im)"
    assert _rel(odo, ot.grad.numpy()) <= 1e-5, "d_offset (deformable_col2im_coord)"
    assert float(np.abs(odo).max()) > 0 and float(np.abs(odx).max()) > 0


@pytest.mark.parametrize("row", list(TABLE))
def test_oracle_transposition_relation(oracle, row):
    x, off, _ = _inputs(row)
    col = _want(row)[0]
    xt, offt, geo = _transposed(row, x, off)
    col_t = np.stack([oracle.deform_im2col(xt[n], offt[n], **geo) for n in range(x.shape[0])])
    _check_transposition(row, col, col_t, x)


def _piece_calls(cdll):
    """the four piece entry points with null tensors: f(geometry...) -> return code"""
    def tail(dims, geom):
        return list(dims) + list(geom) + [DG]
    return {
        "sd_deform_im2col": lambda d, q: cdll.sd_deform_im2col(None, None, None, *tail(d, q), None),
        "sd_deform_col2im": lambda d, q: cdll.sd_deform_col2im(None, None, None, 1, *tail(d, q), None),
        "sd_deform_col2im_ws": lambda d, q: cdll.sd_deform_col2im_ws(None, None, None, 1, *tail(d, q), None,
                                                                    ctypes.c_size_t(0), None),
        "sd_deform_col2im_coord": lambda d, q: cdll.sd_deform_col2im_coord(None, None, None, None, 1, *tail(d, q),
                                                                          None),
    }


@pytest.mark.parametrize("entry", ["sd_deform_im2col", "sd_deform_col2im", "sd_deform_col2im_ws",
                                   "sd_deform_col2im_coord"])
def test_per_axis_arguments_are_refused_per_axis(entry):
    """make_geom() runs before any device access: with null tensors a good geometry gets as far as the pointer
    check, a bad value on ONE axis is refused with its own message"""
    from simpledet_amd._lib import lib
    cdll = lib().cdll
    call = _piece_calls(cdll)[entry]
    msg = lambda: (cdll.sd_last_error() or b"").decode()
    # dims: N, C, H, W, kh, kw; geometry: pad_h, pad_w, stride_h, stride_w, dil_h, dil_w
    assert call((1, 8, 12, 16, 3, 5), (1, 2, 2, 1, 1, 1)) == -1 and "null tensor pointer" in msg()   # row I: accepted
    assert call((1, 8, 12, 2, 3, 5), (0, 0, 1, 1, 1, 1)) == -1 and "kernel size exceed input" in msg()   # Wo <= 0 < Ho
    assert call((1, 8, 2, 12, 5, 3), (0, 0, 1, 1, 1, 1)) == -1 and "kernel size exceed input" in msg()   # Ho <= 0 < Wo
    # the same with a stride of 2 on the short axis: C's division rounds (2 - 3) / 2 to 0, an output size of 1 where
    # the wrappers' floor division gives 0 and allocates nothing -- refused on the extent, not on Ho / Wo
    assert call((1, 8, 12, 2, 3, 3), (0, 0, 1, 2, 1, 1)) == -1 and "kernel size exceed input" in msg()
    assert call((1, 8, 2, 12, 3, 3), (0, 0, 2, 1, 1, 1)) == -1 and "kernel size exceed input" in msg()
    assert call((1, 8, 12, 3, 3, 3), (0, 0, 1, 2, 1, 1)) == -1 and "null tensor pointer" in msg()    # extent == input: fine
    assert call((1, 8, 12, 16, 3, 1), (0, 0, 1, 1, 1, 6)) == -1 and "null tensor pointer" in msg()   # dil_w idle: kw = 1
    assert call((1, 8, 12, 16, 3, 1), (0, 0, 1, 1, 6, 1)) == -1 and "kernel size exceed input" in msg()  # dil_h is not
    assert call((1, 8, 12, 16, 3, 3), (1, 1, 1, 0, 1, 1)) == -1 and "bad kernel/stride/dilate" in msg()  # stride_w = 0
    assert call((1, 8, 12, 16, 3, 3), (1, 1, 1, 1, 0, 1)) == -1 and "bad kernel/stride/dilate" in msg()  # dil_h = 0
    assert call((1, 8, 12, 16, 3, 3), (1, -1, 1, 1, 1, 1)) == -1 and "negative pad" in msg()             # pad_w = -1


# ------------------------------------------------------------------------------------------ GPU --
def _t(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()   # a copy: the shared inputs stay read-only


def _with(knob, fn):
    """fn() with one kernel family switched off; the knob goes back to what it was whatever happens"""
    from simpledet_amd._lib import lib
    with lib().tuned(**{knob: 0}):
        return fn()


@pytest.mark.gpu
@pytest.mark.parametrize("row,scale", GPU_CASES)
def test_pieces_match_the_oracle(ops, row, scale):
    x, off, g = _inputs(row, scale)
    wcol, wdx, wdo = _want(row, scale)
    a = _ops_geo(row)
    tx, to, tg = _t(x), _t(off), _t(g)
    # im2col: the same float operations in the same order as the oracle -- the same bits, from every family
    col = ops.deform_im2col(tx, to, **a)
    np.testing.assert_array_equal(col.cpu().numpy(), wcol)
    for knob in ("dcn_im2col", "dcn_window", "dcn_im2col_pipe"):
        assert torch.equal(_with(knob, lambda: ops.deform_im2col(tx, to, **a)), col), knob
    # col2im: fixed-point sums (workspace), fp32 compare-and-swap adds (none), four-channel float, one-channel
    runs = {("default", ws): ops.deform_col2im(tg, to, x.shape, workspace=ws, **a) for ws in (True, False)}
    for knob in ("dcn_col2im", "dcn_col2im_fx"):
        for ws in (True, False):
            runs[knob, ws] = _with(knob, lambda: ops.deform_col2im(tg, to, x.shape, workspace=ws, **a))
    for key, dx in runs.items():
        np.testing.assert_allclose(dx.cpu().numpy(), wdx, rtol=1e-4, atol=1e-4, err_msg=str(key))
    if (x.shape[1] // DG) % 4 == 0 and wcol.shape[2] % 4 == 0:   # the fixed-point kernel: order independent
        assert torch.equal(ops.deform_col2im(tg, to, x.shape, workspace=True, **a), runs["default", True])
    # col2im_coord: a per-lane reduction in the oracle's channel order -- LDS and per-lane forms, same bits
    do = ops.deform_col2im_coord(tg, tx, to, **a)
    np.testing.assert_allclose(do.cpu().numpy(), wdo, rtol=1e-4, atol=1e-4)
    assert torch.equal(_with("dcn_coord", lambda: ops.deform_col2im_coord(tg, tx, to, **a)), do)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["A", "E", "I", "K", "M"])
def test_im2col_transposition_relation(ops, row):
    x, off, _ = _inputs(row)
    xt, offt, geo = _transposed(row, x, off)
    col = ops.deform_im2col(_t(x), _t(off), **_ops_geo(row)).cpu().numpy()
    col_t = ops.deform_im2col(_t(xt), _t(offt), kernel=geo["kernel"], pad=geo["pad"], stride=geo["stride"],
                              dilate=geo["dil"], num_deformable_group=DG).cpu().numpy()
    _check_transposition(row, col, col_t, x)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [0, 37])
@pytest.mark.parametrize("cfg", [dict(pad=1, stride=1, dilate=1), dict(pad=1, stride=2, dilate=1),
                                 dict(pad=2, stride=1, dilate=2)])
def test_fused_forward_transposition_relation(ops, cfg, tile):
    """The col-free forward (3x3, 16 channels per group, H*W % 4 == 0) on a 12 x 20 plane and on the transposed
    problem (20 x 12, weight transposed in its last two axes, offsets rearranged): y' == y^T within `_bar`.  A row /
    column mix-up inside the fused kernel cannot cancel between the two runs."""
    from simpledet_amd._lib import lib
    N, C, F, H, W = 1, 32, 8, 12, 20
    Ho, Wo = ops._dcn_out_hw(H, W, 3, 3, cfg["pad"], cfg["stride"], cfg["dilate"])
    rs = np.random.RandomState(77)
    x = rs.standard_normal((N, C, H, W)).astype(np.float32)
    off = (rs.standard_normal((N, DG * 18, Ho, Wo)) * 1.5).astype(np.float32)
    w = (rs.standard_normal((F, C, 3, 3)) * 0.2).astype(np.float32)
    offt = np.ascontiguousarray(off.reshape(N, DG, 3, 3, 2, Ho, Wo).transpose(0, 1, 3, 2, 4, 6, 5)[:, :, :, :, ::-1])
    offt = offt.reshape(N, DG * 18, Wo, Ho)
    with lib().tuned(dcn_fused_tile=tile):
        y = ops.deform_conv_forward(_t(x), _t(off), _t(w), num_deformable_group=DG, **cfg).cpu().numpy()
        yt = ops.deform_conv_forward(_t(x.transpose(0, 1, 3, 2)), _t(offt), _t(w.transpose(0, 1, 3, 2)),
                                     num_deformable_group=DG, **cfg).cpu().numpy()
    assert y.shape == (N, F, Ho, Wo) and yt.shape == (N, F, Wo, Ho)
    assert float(np.abs(y).max()) > 1.0
    err = float(np.abs(yt.transpose(0, 1, 3, 2) - y).max())
    print("fused transposition", cfg, tile, "err %.3g" % err, "bar %.3g" % _bar(y))
    assert err <= _bar(y)
