"""numpy restatement of _contrib_DeformablePSROIPooling (DESIGN.md 4.15 is the spec) and of TSD's
get_roi_feature composition (models/TSD/poolings.py:12-174: masks, four operator calls, add_n).

Every function takes `dt`: np.float32 restates the operator's own arithmetic operation by operation (its
error against the truth is k_ref), np.float64 evaluates the same formulas on the same float32 inputs (the
truth).  With `info` a dict, the float64 evaluation also records how close a sample came to a skip boundary
or to an integer coordinate, and whether any was clamped: the fixtures are conditioned on those.

  k = |got - truth| / (eps32 * T + tiny),  T = the sum of the absolute values of the terms of an element.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
TINY = 1e-30


def c_round(x):
    """C round(): half away from zero (numpy's round is half-to-even)"""
    return np.sign(x) * np.floor(np.abs(x) + type(x)(0.5))


def k_of(got, truth, T):
    got = np.asarray(got, np.float64)
    return float(np.max(np.abs(got - truth) / (EPS32 * T + TINY))) if got.size else 0.0


def params(spatial_scale, output_dim, group_size, pooled_size, part_size=0, sample_per_part=4, trans_std=0.1,
           no_trans=False):
    return dict(spatial_scale=spatial_scale, output_dim=output_dim, group_size=group_size, pooled_size=pooled_size,
                part_size=part_size, sample_per_part=sample_per_part, trans_std=trans_std, no_trans=no_trans)


def _dims(prm, trans):
    P = prm["pooled_size"]
    part = prm["part_size"] or P
    ncls = 1 if prm["no_trans"] else trans.shape[1] // 2
    assert prm["output_dim"] % ncls == 0
    return P, part, ncls, prm["output_dim"] // ncls


def _note(info, key, v, fn=min):
    if info is not None:
        info[key] = fn(info.get(key, v), v)


def unit_taps(roi, tr, H, W, ph, pw, prm, part, dt, info=None):
    """the samples of one (RoI, class, bin): roi = (x1, y1, x2, y2), tr = (trans_x, trans_y) raw offsets.
    Returns ([(y0, y1, x0, x1, dx, dy)], roi_w, roi_h)."""
    P, S = prm["pooled_size"], prm["sample_per_part"]
    scale, half, one = dt(prm["spatial_scale"]), dt(0.5), dt(1)
    x1, y1, x2, y2 = [dt(v) for v in roi]
    rsw = c_round(x1) * scale - half
    rsh = c_round(y1) * scale - half
    rew = (c_round(x2) + one) * scale - half
    reh = (c_round(y2) + one) * scale - half
    rw = max(rew - rsw, dt(0.1))
    rh = max(reh - rsh, dt(0.1))
    bin_w, bin_h = rw / dt(P), rh / dt(P)
    sub_w, sub_h = bin_w / dt(S), bin_h / dt(S)
    trans_x = dt(tr[0]) * dt(prm["trans_std"])
    trans_y = dt(tr[1]) * dt(prm["trans_std"])
    wstart = dt(pw) * bin_w + rsw
    wstart = wstart + trans_x * rw
    hstart = dt(ph) * bin_h + rsh
    hstart = hstart + trans_y * rh
    wlim, hlim = dt(W) - half, dt(H) - half
    taps = []
    for ih in range(S):
        for iw in range(S):
            w = wstart + dt(iw) * sub_w
            h = hstart + dt(ih) * sub_h
            _note(info, "skip_margin", float(min(abs(w + half), abs(w - wlim), abs(h + half), abs(h - hlim))))
            if w < -half or w > wlim or h < -half or h > hlim:
                continue
            wc = min(max(w, dt(0)), dt(W) - one)
            hc = min(max(h, dt(0)), dt(H) - one)
            if info is not None and (wc != w or hc != h):
                info["clamped"] = True
            _note(info, "int_margin", float(min(abs(wc - np.round(wc)), abs(hc - np.round(hc)))))
            x0, xb, y0, yb = int(np.floor(wc)), int(np.ceil(wc)), int(np.floor(hc)), int(np.ceil(hc))
            taps.append((y0, yb, x0, xb, wc - dt(x0), hc - dt(y0)))
    return taps, rw, rh


def _bin_geom(prm, part, ph, pw, dt):
    P, G = prm["pooled_size"], prm["group_size"]
    part_h = int(np.floor(dt(ph) / dt(P) * dt(part)))
    part_w = int(np.floor(dt(pw) / dt(P) * dt(part)))
    gw = min(max(int(np.floor(dt(pw) * dt(G) / dt(P))), 0), G - 1)
    gh = min(max(int(np.floor(dt(ph) * dt(G) / dt(P))), 0), G - 1)
    return part_h, part_w, gh, gw


def _walk(data, rois, trans, prm, dt, info):
    """yields (n, batch, cls, ctops, channels, ph, pw, part_h, part_w, taps, roi_w, roi_h) per (RoI, class, bin)"""
    B, C, H, W = data.shape
    P, part, ncls, cpc = _dims(prm, trans)
    G = prm["group_size"]
    assert C == prm["output_dim"] * G * G
    for n in range(rois.shape[0]):
        b = int(rois[n, 0])
        for cls in range(ncls):
            ctops = np.arange(cls * cpc, (cls + 1) * cpc)
            for ph in range(P):
                for pw in range(P):
                    part_h, part_w, gh, gw = _bin_geom(prm, part, ph, pw, dt)
                    tr = (0.0, 0.0) if prm["no_trans"] else (trans[n, 2 * cls, part_h, part_w],
                                                             trans[n, 2 * cls + 1, part_h, part_w])
                    taps, rw, rh = unit_taps(rois[n, 1:5], tr, H, W, ph, pw, prm, part, dt, info)
                    if not 0 <= b < B:
                        taps = []
                    yield n, b, cls, ctops, (ctops * G + gh) * G + gw, ph, pw, part_h, part_w, taps, rw, rh


def forward(data, rois, trans, prm, dt=np.float32, info=None):
    """-> out, top_count, T (K, output_dim, P, P); T = sum of |terms| / count"""
    P = prm["pooled_size"]
    K, OD = rois.shape[0], prm["output_dim"]
    out = np.zeros((K, OD, P, P), dt)
    T = np.zeros((K, OD, P, P), np.float64)
    cnt = np.zeros((K, OD, P, P), np.float32)
    D = data.astype(dt)
    one = dt(1)
    for n, b, cls, ctops, ch, ph, pw, _, _, taps, _, _ in _walk(data, rois, trans, prm, dt, info):
        if not taps:
            continue
        s = np.zeros(len(ctops), dt)
        t = np.zeros(len(ctops), np.float64)
        for y0, yb, x0, xb, dx, dy in taps:
            v00, v01, v10, v11 = D[b, ch, y0, x0], D[b, ch, yb, x0], D[b, ch, y0, xb], D[b, ch, yb, xb]
            q00, q01, q10, q11 = (one - dx) * (one - dy), (one - dx) * dy, dx * (one - dy), dx * dy
            s = s + (q00 * v00 + q01 * v01 + q10 * v10 + q11 * v11)
            t += np.abs(q00 * v00) + np.abs(q01 * v01) + np.abs(q10 * v10) + np.abs(q11 * v11)
        out[n, ctops, ph, pw] = s / dt(len(taps))
        T[n, ctops, ph, pw] = t / len(taps)
        cnt[n, ctops, ph, pw] = len(taps)
    return out, cnt, T


def backward(dy_, data, rois, trans, prm, dt=np.float32, info=None):
    """-> d_data, d_trans, T_data, T_trans"""
    D = data.astype(dt)
    G_ = dy_.astype(dt)
    dd = np.zeros(data.shape, dt)
    Td = np.zeros(data.shape, np.float64)
    dtr = np.zeros(trans.shape, dt)
    Tt = np.zeros(trans.shape, np.float64)
    one, std = dt(1), dt(prm["trans_std"])
    for n, b, cls, ctops, ch, ph, pw, part_h, part_w, taps, rw, rh in _walk(data, rois, trans, prm, dt, info):
        if not taps:
            continue
        g = G_[n, ctops, ph, pw] / dt(len(taps))
        for y0, yb, x0, xb, dx, dy in taps:
            for (y, x, q) in ((y0, x0, (one - dx) * (one - dy)), (yb, x0, (one - dx) * dy),
                              (y0, xb, dx * (one - dy)), (yb, xb, dx * dy)):
                np.add.at(dd, (b, ch, y, x), g * q)
                np.add.at(Td, (b, ch, y, x), np.abs(g * q))
            if prm["no_trans"]:
                continue
            u00, u01, u10, u11 = D[b, ch, y0, x0], D[b, ch, yb, x0], D[b, ch, y0, xb], D[b, ch, yb, xb]
            gx = (u11 * dy + u10 * (one - dy) - u01 * dy - u00 * (one - dy)) * std * g * rw
            gy = (u11 * dx + u01 * (one - dx) - u10 * dx - u00 * (one - dx)) * std * g * rh
            ax = (np.abs(u11 * dy) + np.abs(u10 * (one - dy)) + np.abs(u01 * dy) + np.abs(u00 * (one - dy))) * np.abs(std * g * rw)
            ay = (np.abs(u11 * dx) + np.abs(u01 * (one - dx)) + np.abs(u10 * dx) + np.abs(u00 * (one - dx))) * np.abs(std * g * rh)
            for v in gx:
                dtr[n, 2 * cls, part_h, part_w] += v
            for v in gy:
                dtr[n, 2 * cls + 1, part_h, part_w] += v
            Tt[n, 2 * cls, part_h, part_w] += float(np.sum(ax, dtype=np.float64))
            Tt[n, 2 * cls + 1, part_h, part_w] += float(np.sum(ay, dtype=np.float64))
    return dd, dtr, Td, Tt


# ----------------------------------------------------------------------------------------------- TSD --
def assign_levels(rois, strides, scale0=224, lvl0=4, dt=np.float32, info=None):
    """fpn_roi_assign_offset (models/TSD/poolings.py:12-33): rois (B,R,4) -> target stride (B,R) as uint8"""
    r = rois.astype(dt)
    x1, y1, x2, y2 = r[..., 0], r[..., 1], r[..., 2], r[..., 3]
    k_min, k_max = np.log2(min(strides)), np.log2(max(strides))
    area = (x2 - x1 + dt(1)) * (y2 - y1 + dt(1))
    arg = dt(lvl0) + np.log2(np.sqrt(area) / dt(scale0) + dt(1e-6))
    if info is not None and arg.size:
        _note(info, "level_margin", float(np.min(np.abs(arg - np.round(arg)))))
    lv = np.clip(np.floor(arg), dt(k_min), dt(k_max))
    return np.power(dt(2), lv).astype(np.uint8)


def _masked_inputs(rois, trans, strides, P, form, scale0, lvl0, dt, info=None):
    """the eight tensors the reference feeds its operator calls: per stride (rois (B*R,5), trans (B*R,2,P,P), own)"""
    B, R = rois.shape[:2]
    target = assign_levels(rois, strides, scale0, lvl0, dt, info)
    batch_pad = np.repeat(np.arange(B), R).astype(np.float32).reshape(-1, 1)
    tr = trans.reshape(B, R, -1)
    per = []
    for s in strides:
        own = target == s
        lr = np.where(own[..., None], rois, np.float32(-1)).reshape(-1, 4)
        lo = np.where(own[..., None], tr, np.float32(0))
        if form == "C":
            lo = lo.reshape(-1, 2, P, P)
        else:
            lo = np.tile(lo.reshape(-1, 2, 1, 1), (1, 1, P, P))
        per.append((np.concatenate([batch_pad, lr], 1).astype(np.float32), np.ascontiguousarray(lo, np.float32),
                    own.reshape(-1)))
    return per


def _tsd_prm(C, P, S, stride, dt, trans_std):
    return params(dt(1.0) / dt(stride), C, 1, P, 0, S, trans_std, False)


def tsd_forward(feats, rois, trans, strides, P, form, S=4, trans_std=0.1, scale0=224, lvl0=4, dt=np.float32,
                info=None):
    """FPNRoIAlign_DeltaC ("C": trans (B*R,2,P,P)) / DeltaR ("R": trans (B*R,2)).get_roi_feature
    -> out (B*R,C,P,P), top_count (B*R,nlvl,P,P), T"""
    C = feats[0].shape[1]
    out = T = None
    cnts = []
    for f, s, (lr, lo, _) in zip(feats, strides, _masked_inputs(rois, trans, strides, P, form, scale0, lvl0, dt, info)):
        o, c, t = forward(f, lr, lo, _tsd_prm(C, P, S, s, dt, trans_std), dt, info)
        out = o if out is None else out + o          # add_n
        T = t if T is None else T + t
        cnts.append(c[:, 0])
    return out, np.stack(cnts, 1), T


def tsd_backward(dy_, feats, rois, trans, strides, P, form, S=4, trans_std=0.1, scale0=224, lvl0=4, dt=np.float32):
    """-> [d_feat per level], d_trans (shape of trans), [T per level], T_trans"""
    C = feats[0].shape[1]
    dfs, Tfs = [], []
    dtr = np.zeros(trans.shape, dt)
    Ttr = np.zeros(trans.shape, np.float64)
    for f, s, (lr, lo, own) in zip(feats, strides, _masked_inputs(rois, trans, strides, P, form, scale0, lvl0, dt)):
        dd, dl, Td, Tl = backward(dy_, f, lr, lo, _tsd_prm(C, P, S, s, dt, trans_std), dt)
        dfs.append(dd)
        Tfs.append(Td)
        if form == "R":                               # the gradient of tile: summed over the bins
            dl = dl.reshape(dl.shape[0], 2, -1)
            acc = np.zeros(dl.shape[:2], dt)
            for i in range(dl.shape[2]):
                acc = acc + dl[:, :, i]
            dl, Tl = acc, Tl.reshape(Tl.shape[0], 2, -1).sum(2)
        m = own.reshape((-1,) + (1,) * (dl.ndim - 1))
        dtr = dtr + np.where(m, dl, dt(0)).reshape(trans.shape)     # where's gradient: the own level's only
        Ttr = Ttr + np.where(m, Tl, 0.0).reshape(trans.shape)
    return dfs, dtr, Tfs, Ttr


def quirk_bins(H, W, stride, P=7, S=4, dt=np.float32):
    """bins (ph, pw) of the masked RoI (-1,-1,-1,-1) with zero offsets that keep a sample on a level, with the
    pixels they read"""
    prm = _tsd_prm(1, P, S, stride, dt, 0.1)
    bins, pixels = [], set()
    for ph in range(P):
        for pw in range(P):
            taps, _, _ = unit_taps((-1, -1, -1, -1), (0, 0), H, W, ph, pw, prm, P, dt)
            if taps:
                bins.append((ph, pw))
                for y0, yb, x0, xb, dx, dy in taps:
                    pixels |= {(y0, x0)} | ({(yb, x0)} if dy else set()) | ({(y0, xb)} if dx else set())
    return bins, pixels
