"""Geometries, inputs and numpy restatements for tests/test_roi_align_fp16_edges.py (a plain module, not a conftest).

fwd_band_plan: launch_fwd's band plan of the band-resident forward (simpledet_amd/csrc/roi_align_fwd.hip): bands, owned
    rows, resident rows and planes per fill (`P.g[l]`) of every level.
fwd_planes:    every (level, band, image, channel) plane of a geometry with the displacement its fp16 fill lands at in
    LDS, `((b C + c) H W + row0 W) mod 8` halves (the feature pointers are 16-byte aligned), the band length and the
    plane's position in its fill.
bwd_bands:     the backward's write-out per (level, band, image, channel): element offset and element count, from
    fx_verdict.band_plan; the kernel takes its `__half2` path when `((off | count) & 3) == 0`.
"""
import collections

import numpy as np

from simpledet_amd import synth

from . import fx_verdict

STRIDES = list(synth.FPN_STRIDES)

# csrc/roi_align_common.h
BAND_BUF_FLOATS, BAND_HALO, BAND_MAX_BANDS, BAND_NP, BAND_WAVES, WAVE = 16896, 8, 16, 4, 16, 64

Geom = collections.namedtuple("Geom", "name image B C R pooled degenerate round4")

ODD_A = (196, 388)     # (49,97) (25,49) (13,25) (7,13): every H W odd
ODD_B = (260, 516)     # (65,129) (33,65) (17,33) (9,17): every H W odd, the finest level is two backward bands
CORNER = (212, 396)    # (53,99) (27,50) (14,25) (7,13): with two forward bands (R = 300) the finest level's first band
#                        is 38 rows = 3762 = 8 k + 2 halves, at displacements 0..7: the other corner of the LDS stride
EVEN = (200, 296)      # (50,74) = 4 mod 8, (25,37), (13,19), (7,10) = 2 mod 4: the __half2 write-out at a small size

GEOMS = [
    Geom("a_c1_r1", ODD_A, 1, 1, 1, 7, False, False),
    Geom("a_c3_r77_int", ODD_A, 3, 3, 77, 7, True, True),
    Geom("a_c6_r77_p14", ODD_A, 2, 6, 77, 14, True, False),
    Geom("a_c12_r7", ODD_A, 1, 12, 7, 7, True, False),
    Geom("a_c8_r7", ODD_A, 2, 8, 7, 7, True, False),
    Geom("b_c33_r7_p14", ODD_B, 1, 33, 7, 14, True, False),
    Geom("b_c8_r300", ODD_B, 1, 8, 300, 7, True, False),
    Geom("b_c12_r77", ODD_B, 3, 12, 77, 7, True, False),
    Geom("b_c6_r1", ODD_B, 2, 6, 1, 7, False, False),
    Geom("c_c8_r300", CORNER, 1, 8, 300, 7, True, False),
    Geom("c_c3_r77_p14", CORNER, 3, 3, 77, 14, True, False),
    Geom("e_c8_r77", EVEN, 2, 8, 77, 7, True, False),
    Geom("e_c3_r7_p14", EVEN, 1, 3, 7, 14, True, True),
]
BY_NAME = {g.name: g for g in GEOMS}
ODD_IMAGES = (ODD_A, ODD_B)


def shapes_of(image):
    return [(-(-image[0] // s), -(-image[1] // s)) for s in STRIDES]


# ------------------------------------------------------------------------------------------------ plans
def fwd_band_plan(shapes, C, R, pooled, half=True):
    """-> per level dict(nbands, owned, rows, halo, g, bstride): launch_fwd with the packed arg-max"""
    out = []
    for (H, W) in shapes:
        halo = BAND_HALO
        if H <= 128:
            halo = max(BAND_HALO, min((H + pooled - 1) // pooled + 2, 12))
        rb = (BAND_BUF_FLOATS - 16) // W
        assert rb >= halo + 4
        nbn = 1 if H <= rb else -(-H // (rb - halo))
        cap = BAND_NP * BAND_WAVES * (WAVE // pooled)
        est = R * pooled // len(shapes)
        by_items = (est * 5 + 4 * cap - 1) // (4 * cap)
        nbn = min(max(nbn, by_items), H, BAND_MAX_BANDS)
        owned = -(-H // nbn)
        if nbn > 1:
            for o in range(owned, owned + 4):
                if o + halo > rb:
                    break
                if (o * W) % 4 == 0:
                    owned = o
                    break
        if owned + halo > rb:
            owned = rb - halo
        nbn = -(-H // owned)
        assert nbn <= BAND_MAX_BANDS
        rows = H if nbn == 1 else min(owned + halo, H)
        bstride = ((rows * W + 14) >> 3) * 8 if half else (rows * W + 4 + 3) & ~3
        assert bstride <= BAND_BUF_FLOATS
        g = 1
        for c in (2, 4, 8):
            if C % c == 0 and c * bstride <= BAND_BUF_FLOATS:
                g = c
        out.append(dict(nbands=nbn, owned=H if nbn == 1 else owned, rows=rows, halo=halo, g=g, bstride=bstride))
    return out


def fwd_planes(geom):
    """-> list of dict(level, band, b, c, disp, blen, g, pos): one per plane the fp16 forward may fill"""
    shapes = shapes_of(geom.image)
    res = []
    for l, ((H, W), p) in enumerate(zip(shapes, fwd_band_plan(shapes, geom.C, geom.R, geom.pooled))):
        for band in range(p["nbands"]):
            r0 = band * p["owned"]
            blen = min(H - r0, p["rows"]) * W
            for b in range(geom.B):
                for c in range(geom.C):
                    res.append(dict(level=l, band=band, b=b, c=c, disp=((b * geom.C + c) * H * W + r0 * W) % 8,
                                    blen=blen, g=p["g"], pos=c % p["g"], bstride=((blen + 14) >> 3) * 8))
    return res


def bwd_bands(geom):
    """-> list of dict(level, band, off, count, half2): the write-out of every workgroup of the fp16 backward"""
    shapes = shapes_of(geom.image)
    nbands, rows, _ = fx_verdict.band_plan(shapes)
    res = []
    for l, (H, W) in enumerate(shapes):
        for band in range(nbands[l]):
            row0 = band * rows[l]
            count = (min(row0 + rows[l], H) - row0) * W
            for b in range(geom.B):
                for c in range(geom.C):
                    off = ((b * geom.C + c) * H + row0) * W
                    res.append(dict(level=l, band=band, off=off, count=count, half2=((off | count) & 3) == 0))
    return res


# ------------------------------------------------------------------------------------------------ inputs
def _seed(geom):
    return 7000 + 17 * GEOMS.index(BY_NAME[geom.name])


def make_rois(geom):
    """random boxes (degenerate ones included where the geometry says so) plus, from R = 7 on, one box per image sized
    for each pyramid level, so that every level has work; round4: coordinates on multiples of 4 (coincident taps)"""
    ih, iw = geom.image
    rois = synth.random_rois(_seed(geom), geom.B, geom.R, ih, iw, degenerate=geom.degenerate, min_size=4.0,
                             max_size=float(max(ih, iw)))
    if geom.R >= 7:
        rs = np.random.RandomState(_seed(geom) + 1)
        for b in range(geom.B):
            # (sqrt(area) below 112, in [112, 224) and in [224, 448))
            for l, (w, h) in enumerate(((30.0, 30.0), (150.0, 140.0), (0.95 * iw, 0.95 * ih))):
                x, y = rs.uniform(0, iw - w - 1), rs.uniform(0, ih - h - 1)
                rois[b, geom.R - 4 + l] = [x, y, x + w + rs.uniform(0, 1), y + h + rs.uniform(0, 1)]
            # the coarsest level takes boxes of sqrt(area) >= 448: larger than these images, clamped by the kernel
            rois[b, geom.R - 1] = [-140.3, -130.7, iw + 150.4, ih + 140.6]
            rois[b, geom.R - 5] = [-300.2, 20.3, 250.1, ih + 200.9]
    if geom.round4:
        rois = (np.round(rois / 4) * 4).astype(np.float32)
    return rois


def make_feats16(geom, kind="normal"):
    """fp16 maps.  normal: N(0,1); subnormal: N(0,1) 2^-20 (subnormal halves); max: a third of the pixels +-65504;
    zeros: relu-style runs of zeros of either sign; nonfinite: N(0,1) with a handful of +inf / -inf / NaN per level"""
    rs = np.random.RandomState(_seed(geom) + 2)
    feats = []
    for f in synth.feature_maps(_seed(geom) + 3, geom.B, geom.C, shapes_of(geom.image)):
        if kind == "subnormal":
            f = f * np.float32(2.0 ** -20)
        f = f.astype(np.float16)
        flat = f.reshape(-1)
        if kind == "max":
            pick = rs.randint(0, 6, flat.size)
            flat[pick == 0] = np.float16(65504)
            flat[pick == 1] = np.float16(-65504)
        elif kind == "zeros":
            run = np.repeat(rs.randint(0, 2, -(-flat.size // 5)), 5)[:flat.size].astype(bool)
            zero = np.where(rs.randint(0, 2, flat.size) == 1, np.float16(-0.0), np.float16(0.0))
            flat[run | (flat < 0)] = zero[run | (flat < 0)]
        elif kind == "nonfinite":
            n = max(3, flat.size // 200)
            pos = rs.choice(flat.size, n, replace=False)
            flat[pos] = np.array([np.inf, -np.inf, np.nan], np.float16)[np.arange(n) % 3]
        feats.append(f)
    return feats


# ------------------------------------------------------------------------------------------------ comparisons
def bits16(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float16
    return a.view(np.uint16)


def assert_same_half_bits(got, want, what):
    """equal bits (the sign of zero counts); at NaN positions only NaN-ness has to agree"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float16 and want.dtype == np.float16 and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN masks differ at %d positions" % (what, int((gn != wn).sum()))
    bad = (bits16(got) != bits16(want)) & ~wn
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d halves differ, first at %s: got %r (0x%04x) want %r (0x%04x)" % (
            what, int(bad.sum()), bad.size, i, float(got[i]), int(bits16(got)[i]), float(want[i]), int(bits16(want)[i])))


def half_step(w):
    """one fp16 step at the magnitude of w (the floor is the subnormal step)"""
    return np.maximum(np.abs(w) * 2.0 ** -10, 2.0 ** -24)


def mass_bar(got16, want32, mass32, dy32):
    """the bar of test_crowded_band_14x14_fp16_io_against_the_oracle: excess over one fp16 step of the rounded oracle
    sum, relative to max(median |dY|, gradient mass that reaches the pixel)"""
    w16 = want32.astype(np.float16).astype(np.float64)
    got = got16.astype(np.float64)
    excess = np.maximum(np.abs(got - w16) - half_step(w16), 0.0)
    return float((excess / np.maximum(float(np.median(np.abs(dy32))), mass32.astype(np.float64))).max())
