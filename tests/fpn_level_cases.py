"""RoIs at which one ulp of log2 decides the FPN level (models/FPN/assign_layer_fpn.py:26-32):

    t = floor(lvl0 + log2(sqrt(area) / scale0 + 1e-6))        in float32

floor() turns a last-bit difference of log2 into another pyramid level, but only where lvl0 + log2(z) is an exact
tie of the float32 add.  With lvl0 = 4: at z = 2 - 3 ulp the correctly rounded log2f(z) is 1 - 4 * 2^-24, the sum
lies half way between 5 - 2^-21 and 5 and rounds to 5; a log2f one ulp lower gives level 4.  The same happens just
under z = 0.5 and z = 4; around z = 1 the sum is exact and nothing is sensitive.  At those z the spec is the
correctly rounded log2f: glibc's, i.e. the oracle's, and numpy's, i.e. the fixture's
(tests/golden/fpn_assign_thresholds.npz, written by tests/golden/make_golden.py from the reference's own class).

The sweep, per pyramid and per level threshold c = 2^j inside it: the 801 consecutive float32 areas around
a0 = float32((scale0 * (c - 1e-6))^2), each as the RoI (0, 0, w - 1, a / w - 1) with w a power of two, so that
(x2 - x1 + 1) * (y2 - y1 + 1) gives the area back bit for bit.  After the sweeps come the rows the rule treats
specially (SPECIAL).  conditions() checks what the tests rely on -- properties of these inputs, not of any code
under test.  Only the SHA-256 of the RoIs is stored in the fixture; rois() regenerates them.
"""
import hashlib

import numpy as np

F = np.float32
HALF = 400             # ulps of area on either side of a0
NEAR = 16              # the neighbourhood the RoIAlign tests run on

# name -> rcnn_stride, roi_canonical_scale, roi_canonical_level, ((threshold c, RoI width w), ...): h ~ 0.77 w
PYRAMIDS = {
    "p2_p5": ((4, 8, 16, 32), 224, 4, ((0.5, 128), (1.0, 256), (2.0, 512))),
    "p3_p6": ((8, 16, 32, 64), 224, 4, ((1.0, 256), (2.0, 512), (4.0, 1024))),
}
# thresholds where moving log2f's result by one ulp moves some area of the sweep to another level (c = 1 has none)
SENSITIVE = (0.5, 2.0, 4.0)

SPECIAL = (
    ("area_zero", (10, 10, 9, 40)),             # sqrt(0) = 0 -> log2(1e-6) -> clipped to k_min
    ("area_negative", (50, 50, 10, 200)),       # sqrt(< 0) = NaN -> matches no stride: level -1
    ("area_inf", (0, 0, np.inf, 10)),           # log2(inf) = inf -> clipped to k_max
    ("one_by_one", (7, 7, 7, 7)),
    ("above_top", (0, 0, 1999, 1999)),          # past the top threshold of both pyramids: clipped to k_max
    ("below_bottom", (30, 30, 49, 49)),         # under the bottom threshold of both pyramids: clipped to k_min
)


def a0(c, scale0=224):
    return F((float(scale0) * (float(c) - 1e-6)) ** 2)


def sweep_areas(c, scale0=224, half=HALF):
    """the 2 * half + 1 consecutive float32 values centred on a0(c), ascending"""
    bits = a0(c, scale0).view(np.int32) + np.arange(-half, half + 1, dtype=np.int32)
    a = bits.view(F)
    assert np.all(np.diff(a) > 0) and np.all(np.diff(np.frexp(a)[1]) == 0)     # one binade: steps of one ulp
    return a


def rois_for_areas(areas, w):
    """(n, 4): (0, 0, w - 1, a / w - 1); the rule's float32 area expression reproduces `areas` exactly"""
    areas = np.asarray(areas, F)
    h = (areas / F(w)).astype(F)
    r = np.zeros((len(areas), 4), F)
    r[:, 2] = F(w) - F(1)
    r[:, 3] = h - F(1)
    assert np.array_equal(area_of(r), areas), "the RoIs do not reproduce their areas"
    return r


def area_of(rois):
    r = np.asarray(rois, F)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((r[..., 2] - r[..., 0] + F(1)) * (r[..., 3] - r[..., 1] + F(1))).astype(F)


def z_of(areas, scale0=224):
    with np.errstate(invalid="ignore"):
        return (np.sqrt(np.asarray(areas, F)) / F(scale0) + F(1e-6)).astype(F)


def level_from_log2(lg, strides, lvl0=4):
    """the rest of the rule given float32 log2(z): floor, clip, 2 ** t as uint8, the stride's index or -1"""
    strides = list(strides)
    k_min, k_max = F(np.log2(min(strides))), F(np.log2(max(strides)))
    with np.errstate(invalid="ignore"):
        t = np.floor((F(lvl0) + np.asarray(lg, F)).astype(F))
        t = np.where(t < k_min, k_min, np.where(t > k_max, k_max, t))     # NaN passes through (mx.nd.clip)
    out = np.full(t.shape, -1, np.int8)
    ok = t == t
    ts = np.zeros(t.shape, np.int64)
    ts[ok] = (2 ** t[ok].astype(np.int64)) & 255                          # .astype('uint8')
    for l in reversed(range(len(strides))):
        out[ok & (ts == strides[l])] = l
    return out


def level_f64(areas, strides, scale0=224, lvl0=4):
    """the level with log2 correctly rounded by construction: (float)log2((double)z)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        lg = np.log2(z_of(areas, scale0).astype(np.float64)).astype(F)
    return level_from_log2(lg, strides, lvl0)


def sensitive(areas, strides, scale0=224, lvl0=4):
    """mask: areas whose level changes when log2f's result moves by one ulp either way"""
    with np.errstate(invalid="ignore", divide="ignore"):
        lg = np.log2(z_of(areas, scale0).astype(np.float64)).astype(F)
    base = level_from_log2(lg, strides, lvl0)
    up = level_from_log2(np.nextafter(lg, F(np.inf)), strides, lvl0)
    dn = level_from_log2(np.nextafter(lg, F(-np.inf)), strides, lvl0)
    return (up != base) | (dn != base)


def segments(name, half=HALF):
    """[(label, c or None, ulp offsets or None, rois (n, 4))]: the sweeps of a pyramid, then SPECIAL"""
    strides, scale0, lvl0, thr = PYRAMIDS[name]
    out = []
    for c, w in thr:
        out.append(("c=%g" % c, c, np.arange(-half, half + 1), rois_for_areas(sweep_areas(c, scale0, half), w)))
    out.append(("special", None, None, np.array([r for _, r in SPECIAL], F)))
    return out


def rois(name, half=HALF):
    """(1, n, 4) float32"""
    return np.concatenate([s[3] for s in segments(name, half)], 0)[None]


def describe(name, rows, half=HALF):
    """row indices of rois(name, half) -> 'c=2 -3 ulp' / the special row's name, for failure messages"""
    labels = []
    for label, c, offs, r in segments(name, half):
        labels += ["%s %+d ulp" % (label, o) for o in offs] if c is not None else [n for n, _ in SPECIAL]
    return [labels[int(i)] for i in rows]


def near_rois(name="p2_p5", finite=True):
    """the +-NEAR ulp neighbourhood of every threshold of a pyramid plus the (finite) special rows: (1, n, 4)"""
    r = rois(name, NEAR)[0]
    if finite:
        r = r[np.isfinite(r).all(1)]
    return np.ascontiguousarray(r[None])


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, F).tobytes()).hexdigest()


def conditions(name, oracle_level):
    """oracle_level: int levels of rois(name)[0] from the implementation that serves as the spec.  Asserts the
    properties the tests rely on and returns {c: number of sensitive areas}."""
    strides, scale0, lvl0, thr = PYRAMIDS[name]
    oracle_level = np.asarray(oracle_level).reshape(-1)
    counts, at = {}, 0
    for label, c, offs, r in segments(name):
        lv = oracle_level[at:at + len(r)]
        at += len(r)
        if c is None:
            continue
        a = area_of(r)
        assert len(set(lv.tolist())) == 2, "%s %s: the sweep holds levels %s" % (name, label, sorted(set(lv.tolist())))
        assert np.all(np.diff(lv) >= 0), "%s %s: level not monotone in the area" % (name, label)
        assert np.array_equal(lv, level_f64(a, strides, scale0, lvl0)), \
            "%s %s: the oracle's log2f is not the correctly rounded one" % (name, label)
        counts[c] = int(sensitive(a, strides, scale0, lvl0).sum())
        assert (counts[c] >= 1) == (c in SENSITIVE), "%s %s: %d sensitive areas" % (name, label, counts[c])
    assert at == len(oracle_level)
    return counts


def boundary_rows(name):
    """per threshold: (c, last RoI below it, first RoI at or above it), by the correctly rounded rule"""
    strides, scale0, lvl0, thr = PYRAMIDS[name]
    out = []
    for label, c, offs, r in segments(name):
        if c is None:
            continue
        lv = level_f64(area_of(r), strides, scale0, lvl0)
        first = int(np.argmax(lv == lv.max()))
        out.append((c, r[first - 1], r[first], int(lv[first - 1]), int(lv[first])))
    return out
