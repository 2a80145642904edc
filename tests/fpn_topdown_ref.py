"""numpy restatement of the FPN top-down pathway's contract (include/simpledet_ops.h, sd_fpn_topdown_*), float32 and
float16, and the cases the tests share.

  forward   out_l = up2(p_{l-1})[:H_l, :W_l] + lateral_l, p_0 = top, p_l = out_l: nearest neighbour (y >> 1, x >> 1),
            the crop from the origin; the add is the dtype's own (numpy's float16 add is the float sum rounded once).
  backward  D_{L-1} = g_{L-1}; D_l = g_l + S_l; d_top = S_0; d_lateral_l = D_l.  S_l starts at +0.0f and adds
            D_{l+1}[2i+a, 2j+b] in the order (0,0), (0,1), (1,0), (1,1) in float32, positions beyond the fine level
            left out; float16: one rounding per stored element, the next level reads the rounded half.
Upstream MXNet's UpSampling / slice_like / add_n are not in the reference tree; this is their arithmetic restated
(mshadow's pool<red::sum> for the UpSampling backward).
"""
import numpy as np

F, H = np.float32, np.float16

# spatial chains, level 0 (the coarsest) first
CHAINS = {
    "crop1_mixed": [(2, 3), (3, 5), (6, 9), (11, 18)],
    "crop23": [(3, 4), (4, 5)],
    "ones": [(1, 1), (1, 1), (2, 2)],
    "even_odd": [(4, 6), (7, 11), (13, 22), (26, 43)],
    "L5": [(2, 3), (4, 5), (7, 10), (14, 19), (27, 38)],
    "L6": [(1, 2), (2, 3), (4, 6), (7, 11), (14, 21), (27, 41)],
    # the level-0 tile is 16 elements wide at L = 6: 40 columns are three column tiles, the last partial
    "L6_wide": [(2, 40), (3, 79), (6, 158), (11, 315), (22, 629), (43, 1257)],
    # the level-0 tile is 4096 elements wide at L = 2: 9000 columns are three column tiles, the last partial
    "L2_wide": [(1, 9000), (2, 17999)],
}
FPN_CHAIN = [(25, 42), (50, 84), (100, 167), (200, 334)]     # faster_r50v1_fpn_1x at 800 x 1333
RETINA_CHAIN = [(25, 42), (50, 84), (100, 167)]


def shapes_of(chain, N=2, C=3):
    return [(N, C, h, w) for h, w in chain]


def make(rs, chain, dt, N=2, C=3):
    """top, laterals, grads: N(0,1) values of dtype dt"""
    sh = shapes_of(chain, N, C)
    top = rs.standard_normal(sh[0]).astype(dt)
    lats = [rs.standard_normal(s).astype(dt) for s in sh[1:]]
    grads = [rs.standard_normal(s).astype(dt) for s in sh[1:]]
    return top, lats, grads


def check_chain(shapes):
    for l in range(1, len(shapes)):
        assert shapes[l][:2] == shapes[0][:2]
        assert shapes[l][2] <= 2 * shapes[l - 1][2] and shapes[l][3] <= 2 * shapes[l - 1][3], shapes


def up_crop(p, h, w):
    return np.repeat(np.repeat(p, 2, axis=2), 2, axis=3)[:, :, :h, :w]


def fwd(top, laterals):
    check_chain([top.shape] + [t.shape for t in laterals])
    outs, p = [], top
    with np.errstate(all="ignore"):
        for lat in laterals:
            p = (up_crop(p, lat.shape[2], lat.shape[3]) + lat).astype(top.dtype)
            outs.append(p)
    return outs


def window_sum(D, h, w):
    """S[i,j] over the 2 x 2 window of D above it, float32, row-major from +0.0, cropped positions left out"""
    S = np.zeros(D.shape[:2] + (h, w), F)
    Df = D.astype(F)
    with np.errstate(all="ignore"):
        for a in (0, 1):
            for b in (0, 1):
                part = Df[:, :, a::2, b::2]
                S[:, :, :part.shape[2], :part.shape[3]] += part
    return S


def bwd(grads, shapes):
    """grads [g_1 .. g_{L-1}] (inner ones may be None) -> d_top, [d_lateral_1 .. d_lateral_{L-1}]"""
    check_chain(shapes)
    L = len(shapes)
    dt = grads[-1].dtype
    D = grads[-1]
    d_lat = [None] * (L - 1)
    d_lat[L - 2] = D
    for l in range(L - 2, -1, -1):
        S = window_sum(D, shapes[l][2], shapes[l][3])
        if l == 0:
            with np.errstate(all="ignore"):
                return S.astype(dt), d_lat
        g = grads[l - 1]
        with np.errstate(all="ignore"):
            D = (S if g is None else g.astype(F) + S).astype(dt)
        d_lat[l - 1] = D


def fwd_chained(top, laterals):
    outs, p = [], top
    for lat in laterals:
        p = fwd(p, [lat])[0]
        outs.append(p)
    return outs


def bwd_chained(grads, shapes):
    """L - 1 two-level calls: the incoming gradient of level l is g_l plus what the finer step sent down -- formed
    by the step itself, which takes D_{l+1} as its finest gradient"""
    L = len(shapes)
    D = grads[-1]
    d_lat = [None] * (L - 1)
    d_lat[L - 2] = D
    for l in range(L - 2, -1, -1):
        S, _ = bwd([D], [shapes[l], shapes[l + 1]])
        if l == 0:
            return S, d_lat
        g = grads[l - 1]
        D = S if g is None else (g.astype(F) + S.astype(F)).astype(S.dtype)
        d_lat[l - 1] = D


def same_bits(a, b):
    """equal bit patterns; a NaN matches any NaN (the sign and payload of a generated NaN are the processor's)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def truth64(top, laterals, grads):
    """float64 truth by autograd of the torch composition; returns outs, d_top, d_laterals and the same backward on
    the absolute values of the gradients (the scale T of the error measure k = |err| / (eps * T))"""
    import torch
    import torch.nn.functional as Fn

    def run(gs):
        t = torch.from_numpy(top.astype(np.float64)).requires_grad_(True)
        ls = [torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in laterals]
        outs, p = [], t
        for lat in ls:
            p = Fn.interpolate(p, scale_factor=2, mode="nearest")[:, :, :lat.shape[2], :lat.shape[3]] + lat
            outs.append(p)
        live = [(o, torch.from_numpy(g.astype(np.float64))) for o, g in zip(outs, gs) if g is not None]
        torch.autograd.backward([o for o, _ in live], [g for _, g in live])
        return [o.detach().numpy() for o in outs], t.grad.numpy(), [x.grad.numpy() for x in ls]
    outs, d_top, d_lat = run(grads)
    _, a_top, a_lat = run([None if g is None else np.abs(g) for g in grads])
    return outs, d_top, d_lat, a_top, a_lat


def k_units(got, want64, scale64, dt):
    """max |got - want| / (eps * T); an element whose scale is 0 must be exact"""
    eps = float(np.finfo(dt).eps)
    err = np.abs(got.astype(np.float64) - want64)
    zero = scale64 == 0
    assert np.all(err[zero] == 0), "error where the scale is zero"
    if zero.all():
        return 0.0
    return float((err[~zero] / (eps * scale64[~zero])).max())
