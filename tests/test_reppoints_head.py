"""RepPoints training head: sd_reppoints_target, sd_reppoints_box_loss_fwd / _bwd (simpledet_amd/csrc/reppoints_head.hip).

CPU: the numpy restatement (tests/reppoints_ref.py) equal BIT FOR BIT to tests/golden/reppoints_head.npz -- the
     reference's own point_ops.py functions run on the evaluating stand-in (tests/golden/make_golden_reppoints.py) --
     on every stored array; the reference's own known answers (point_ops.py:280-322) through the restatement;
     argument validation of every entry point.
GPU: targets bit-equal to the fixture on every element of every case; losses with an exact zero pattern and every
     forward value, gradient element and d_moment_transfer within the house margin
     k = |got - truth| / (eps32 * T + tiny),  max k_gpu <= 2 * k_ref + 2,  k_ref the float32 restatement's own
     maximum on the same cases; exact cases equal to the restatement (tied min / max, nine coincident points, all
     weights zero, req add); equal bits over calls and under graph replay on changed inputs; pointers 4 bytes off a
     16-byte boundary; red zones around every output and the workspaces; L = 1.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from simpledet_amd import _lib
from . import reppoints_ref as rr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reppoints_head.npz")
F32 = np.float32


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def target_cases():
    return rr.target_cases()


@functools.lru_cache(maxsize=None)
def loss_refs():
    """[(name, case, targets, float32 restatement, float64 truth)], computed once"""
    out = []
    for name, c in rr.loss_cases():
        tg = rr.targets_f32(c)
        out.append((name, c, tg, rr.losses_f32(c, tg), rr.losses_truth(c, tg)))
    return out


@functools.lru_cache(maxsize=None)
def k_ref():
    ks = [rr.k_all(r, t) for _, _, _, r, t in loss_refs()]
    return tuple(max(k[i] for k in ks) for i in range(3))


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


# ------------------------------------------------------------------------------------------------ CPU --
def test_restatement_equals_the_reference_fixture_bit_for_bit():
    g = golden()
    mname, mcase = rr.margin_target_case()
    assert list(g["target_cases"]) == [n for n, _ in target_cases()] + [mname]
    assert list(g["loss_cases"]) == [n for n, _ in rr.loss_cases()]
    for name, c in target_cases():
        assert np.array_equal(g["t/%s/gt_bbox" % name], c["gt_bbox"])
        tg = rr.targets_f32(c)
        for key in ("label_init", "label_refine"):
            assert np.array_equal(g["t/%s/%s" % (name, key)].astype(F32), tg[key]), (name, key)
        for key in ("gt_init", "gt_refine", "boxes"):
            a = g["t/%s/%s" % (name, key)]
            assert a.dtype == F32 and a.shape == tg[key].shape and np.array_equal(_bits(a), _bits(tg[key])), (name, key)
    tg = rr.targets_f32(mcase)
    for key in ("label_init", "label_refine", "gt_init", "gt_refine"):
        assert np.array_equal(g["t/%s/%s" % (mname, key)].astype(F32), tg[key]), key
    for name, c, tg, r32, _ in loss_refs():
        for key in ("loss_init", "loss_refine"):
            a = g["l/%s/%s" % (name, key)]
            assert a.shape == r32[key].shape
            if not c["mt"].any():
                assert np.array_equal(_bits(a), _bits(r32[key])), (name, key)
            else:       # exp(moment_transfer) is the library's: a few ulp of the box, nothing more
                assert np.allclose(a, r32[key], rtol=1e-5, atol=1e-6), (name, key)
    # the cases do what their names say
    q = g["t/max-fg-quirk-threshold-equality-degenerate/label_refine"]
    assert q[0, 0] == 7 and (q[0, 1:] == 0).all()          # best box of gt 1 (class 3), labelled by its own arg-max (7)
    assert q[1, 0] == 4 and q[1, 4 * 12 + 8] == -1 and (np.delete(q[1], [0, 56]) == 0).all()
    assert (g["t/band/label_refine"] == -1).any() and (g["t/no-valid-gt/label_init"][0] == -1).all()
    d = g["t/duplicates-and-centre-ties/label_init"]
    assert d[0, 0] == 3 and (d[0] == 9).sum() == 0 and (d[0] == 5).sum() == 1 and (d[0] == 2).sum() == 0


def test_the_reference_known_answers_pass_through_the_restatement():
    """the asserts of point_ops.py:280-322"""
    offs = np.array([-1, -1, -1, 0, -1, 1, 0, -1, 0, 0, 0, 1, 1, -1, 1, 0, 1, 1], F32).reshape(1, 18, 1, 1)
    assert np.array_equal(rr.gen_offsets(3, 1), offs)
    pts = rr.gen_points([(2, 3)], [8])
    assert np.array_equal(pts.reshape(1, 2, 3, 3),
                          np.array([0, 0, 8, 8, 0, 8, 16, 0, 8, 0, 8, 8, 8, 8, 8, 16, 8, 8], F32).reshape(1, 2, 3, 3))
    y, x = rr.split_yx(np.arange(36, dtype=F32).reshape(1, 18, 2, 1))
    box = rr.points2bbox(x, y, "minmax", None)                       # (1, 2, 4) -> (1, 4, 2, 1)
    assert np.array_equal(box.transpose(0, 2, 1).reshape(1, 4, 2, 1), np.array([2, 3, 0, 1, 34, 35, 32, 33], F32).reshape(1, 4, 2, 1))
    points = rr.gen_points([(2, 4), (1, 2)], [32, 64])
    gt = F32([[63, 923, 123, 1800, 2], [200, 50, 600, 120, 3], [21, 456, 123, 712, 4], [325, 123, 523, 612, 5], [-1, -1, 5000, 5000, 6]])
    lab, box = rr.point_assign_f32(points, gt, 4, 1)
    assert list(lab) == [-1, -1, -1, -1, -1, -1, 4, 3, -1, 6]
    assert np.array_equal(box[6], F32([21, 456, 123, 712])) and np.array_equal(box[7], F32([200, 50, 600, 120]))
    assert np.array_equal(box[9], F32([-1, -1, 5000, 5000])) and not box[[0, 1, 2, 3, 4, 5, 8]].any()
    props = F32([[45, 23, 452, 45], [12, 798, 45, 902], [103, 563, 345, 609], [34, 452, 123, 623], [12, 23, 43, 134], [341, 78, 587, 102]])
    lab, box, _ = rr.iou_assign_f32(props, gt[:3], 0.5, 0.4, 0.0)
    assert list(lab) == [0, 0, 0, 4, 0, 3]
    assert np.array_equal(box[3], F32([21, 456, 123, 712])) and np.array_equal(box[5], F32([200, 50, 600, 120]))
    assert not box[[0, 1, 2, 4]].any()


def test_restatements_agree_and_k_ref():
    kf, kg, km = k_ref()
    print("reppoints k_ref: forward %.3f  gradients %.3f  d_moment_transfer %.3f" % (kf, kg, km))
    assert kf < 64 and kg < 64 and km < 64
    for name, c, tg, r32, t in loss_refs():
        for s in ("init", "refine"):
            assert np.array_equal(r32["loss_" + s] == 0, t["loss_" + s] == 0), name
            assert (tg["label_" + s] > 0).any(), name


def _i(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    l = _lib.lib()
    P = ctypes.c_void_p(4096)       # never dereferenced: every check comes before the first launch
    tab, H, W, S = _ptrs([4096] * 5), _i([8, 4, 2, 1, 1]), _i([12, 6, 3, 2, 1]), _i(rr.STRIDES)
    ws = ctypes.c_size_t(1 << 20)

    def target(pts=tab, H=H, W=W, S=S, L=5, gt=P, mt=P, li=P, gi=P, lr=P, gr=P, state=P, N=2, M=8, K=9, tr=2,
               scale=4.0, num_pos=1, pos=0.5, neg=0.5, minpos=0.0, wsp=P, wsb=ws):
        return l.call("sd_reppoints_target", pts, H, W, S, L, gt, mt, li, gi, lr, gr, state, N, M, K, tr, scale,
                      num_pos, pos, neg, minpos, wsp, wsb, None)

    def fwd(pi=tab, pr=tab, H=H, W=W, S=S, L=5, mt=P, li=P, gi=P, lr=P, gr=P, oi=P, orf=P, N=2, K=9, tr=2, scale=4.0):
        return l.call("sd_reppoints_box_loss_fwd", pi, pr, H, W, S, L, mt, li, gi, lr, gr, oi, orf, N, K, tr, scale, None)

    def bwd(pi=tab, pr=tab, H=H, W=W, S=S, L=5, mt=P, li=P, gi=P, lr=P, gr=P, state=P, di=tab, dr=tab, dmt=P, N=2,
            K=9, tr=2, scale=4.0, gsi=0.5, gsr=1.0, req=1, wsp=P, wsb=ws):
        return l.call("sd_reppoints_box_loss_bwd", pi, pr, H, W, S, L, mt, li, gi, lr, gr, state, di, dr, dmt, N, K, tr,
                      scale, gsi, gsr, req, wsp, wsb, None)

    def raises(f, match, code=-1, **kw):
        with pytest.raises(_lib.SimpleDetOpsError, match=match) as e:
            f(**kw)
        assert e.value.code == code, (match, kw)

    for f in (target, fwd, bwd):
        raises(f, "negative dimension", N=-1)
        raises(f, "negative dimension", L=-1)
        raises(f, "negative size", H=_i([8, -4, 2, 1, 1]))
        raises(f, "not positive", S=_i([8, 0, 32, 64, 128]))
        raises(f, "null level table", H=None)
        raises(f, "transform=3", tr=3)
        raises(f, "partial_minmax", tr=1, K=1)
        raises(f, "must be positive", scale=0.0)
        raises(f, "must be positive|NaN", scale=float("nan"))
        raises(f, "moment_transfer", mt=None)
        raises(f, "exceed the limit 8", code=_lib.SD_ERR_UNSUPPORTED, L=9, H=_i([1] * 9), W=_i([1] * 9), S=_i([8] * 9),
               **({"pts": _ptrs([4096] * 9)} if f is target else {"pi": _ptrs([4096] * 9), "pr": _ptrs([4096] * 9)}))
        for K in (0, 4, 16, 49):
            raises(f, "num_points=%d" % K, code=_lib.SD_ERR_UNSUPPORTED, K=K)
        raises(f, "images exceed the limit 65535", code=_lib.SD_ERR_UNSUPPORTED, N=65536, L=1, H=_i([1]), W=_i([1]), S=_i([8]))
        raises(f, "elements exceed the limit", code=_lib.SD_ERR_UNSUPPORTED, N=64, L=1, H=_i([4096]), W=_i([4096]), S=_i([8]))
        raises(f, "beyond 2\\^24", code=_lib.SD_ERR_UNSUPPORTED, L=1, H=_i([1]), W=_i([40000]), S=_i([1024]))
        for name in ("li", "gi", "lr", "gr"):
            raises(f, "null pointer", **{name: None})
        # empty problems succeed without touching the device
        assert f(N=0, li=None) == 0 and f(L=0, H=None, W=None, S=None, gi=None) == 0
        assert f(H=_i([0] * 5), lr=None) == 0
    raises(target, "null pointer in level 2", pts=_ptrs([4096, 4096, 0, 4096, 4096]))
    raises(target, "null level table", pts=None)
    raises(target, "null pointer", gt=None)
    raises(target, "null pointer", state=None)
    raises(target, "negative dimension", M=-1)
    raises(target, "M=0", M=0)
    raises(target, "M=129", code=_lib.SD_ERR_UNSUPPORTED, M=129)
    raises(target, "num_pos=0", code=_lib.SD_ERR_UNSUPPORTED, num_pos=0)
    raises(target, "num_pos=17", code=_lib.SD_ERR_UNSUPPORTED, num_pos=17)
    raises(target, "NaN", pos=float("nan"))
    raises(target, "NaN", minpos=float("nan"))
    raises(target, "workspace too small", code=-4, wsb=ctypes.c_size_t(64))
    raises(target, "workspace too small", code=-4, wsp=None)
    raises(fwd, "null pointer in level 4", pr=_ptrs([4096, 4096, 4096, 4096, 0]))
    raises(fwd, "null pointer", oi=None)
    raises(bwd, "null pointer", state=None)
    raises(bwd, "null pointer", dmt=None)
    raises(bwd, "null level table", di=None)
    raises(bwd, "null pointer in level 0", dr=_ptrs([0, 4096, 4096, 4096, 4096]))
    raises(bwd, "req=2", req=2)
    raises(bwd, "NaN", gsi=float("nan"))
    raises(bwd, "workspace too small", code=-4, wsb=ctypes.c_size_t(16))
    assert l.cdll.sd_reppoints_target_workspace_bytes(2, 100, ctypes.c_long(22300)) >= 2 * 22300 * 24 + 800
    assert l.cdll.sd_reppoints_target_workspace_bytes(-1, 1, ctypes.c_long(5)) == 0
    assert l.cdll.sd_reppoints_box_loss_workspace_bytes(2, ctypes.c_long(22300)) >= 175 * 16
    assert l.cdll.sd_reppoints_box_loss_workspace_bytes(2, ctypes.c_long(-1)) == 0


# ------------------------------------------------------------------------------------------------ GPU --
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tbits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _kw_t(c):
    return dict(transform=c["transform"], target_scale=c["target_scale"], num_pos=c["num_pos"],
                pos_iou_thr=c["pos_iou_thr"], neg_iou_thr=c["neg_iou_thr"], min_pos_iou=c["min_pos_iou"])


def _run_target(ops, c, **kw):
    return ops.reppoints_target([_dev(p) for p in c["pts_init"]], _dev(c["gt_bbox"]), c["strides"],
                                moment_transfer=_dev(c["mt"]), **_kw_t(c), **kw)


@pytest.mark.gpu
def test_hip_targets_equal_the_reference_fixture(ops):
    g = golden()
    for name, c in target_cases():
        t = _run_target(ops, c)
        for key in ("label_init", "label_refine"):
            want = g["t/%s/%s" % (name, key)].astype(F32)
            assert np.array_equal(_bits(getattr(t, key).cpu().numpy()), _bits(want)), (name, key)
        for key in ("gt_init", "gt_refine"):
            assert np.array_equal(_bits(getattr(t, key).cpu().numpy()), _bits(g["t/%s/%s" % (name, key)])), (name, key)
        state = t.state.cpu().numpy()
        ci, cr = int((g["t/%s/label_init" % name] >= 1).sum()), int((g["t/%s/label_refine" % name] >= 1).sum())
        assert list(state[:2]) == [ci, cr] and list(state[2:].view(F32)) == [ci + 1.0, cr + 1.0], name
    # a non-zero moment_transfer: the labels (and with them the boxes taken from gt rows) are equal, nothing left out
    name, c = rr.margin_target_case()
    t = _run_target(ops, c)
    for key in ("label_init", "label_refine", "gt_init", "gt_refine"):
        assert np.array_equal(getattr(t, key).cpu().numpy(), g["t/%s/%s" % (name, key)].astype(F32)), key


def _targets_of(tg):
    import torch
    from simpledet_amd import ops
    state = np.array([tg["count"][0], tg["count"][1], 0, 0], np.int32)
    state[2:] = np.array([tg["count"][0] + 1.0, tg["count"][1] + 1.0], F32).view(np.int32)
    return ops.RepPointsTargets(_dev(tg["label_init"]), _dev(tg["gt_init"]), _dev(tg["label_refine"]),
                                _dev(tg["gt_refine"]), torch.from_numpy(state).cuda())


def _kw_l(c):
    return dict(transform=c["transform"], scale=c["scale"])


def _run_losses(ops, c, tg, **kw):
    pi, pr, mt = [_dev(p) for p in c["pts_init"]], [_dev(p) for p in c["pts_refine"]], _dev(c["mt"])
    t = _targets_of(tg)
    li, lr = ops.reppoints_box_loss_forward(pi, pr, t, c["strides"], moment_transfer=mt, **_kw_l(c))
    di, dr, dmt = ops.reppoints_box_loss_backward(pi, pr, t, c["strides"], moment_transfer=mt, **_kw_l(c), **kw)
    return dict(loss_init=li.cpu().numpy(), loss_refine=lr.cpu().numpy(), d_init=[d.cpu().numpy() for d in di],
                d_refine=[d.cpu().numpy() for d in dr], d_mt=dmt.cpu().numpy())


@pytest.mark.gpu
def test_hip_losses_margin_and_zero_patterns(ops):
    ref = k_ref()
    gpu = [0.0, 0.0, 0.0]
    for name, c, tg, r32, truth in loss_refs():
        got = _run_losses(ops, c, tg)
        # the device's own targets are the restatement's (the losses above ran on the latter)
        t = _run_target(ops, c)
        for key in ("label_init", "gt_init", "label_refine", "gt_refine"):
            assert np.array_equal(getattr(t, key).cpu().numpy(), tg[key]), (name, key)
        for s in ("init", "refine"):
            assert np.array_equal(got["loss_" + s] == 0, truth["loss_" + s] == 0), (name, s)     # the zero pattern is exact
            for a, b in zip(got["d_" + s], truth["d_" + s]):
                assert np.array_equal(a == 0, b == 0), (name, s)
        k = rr.k_all(got, truth)
        print("%s: k_gpu forward %.3f gradients %.3f d_moment_transfer %.3f" % ((name,) + k))
        gpu = [max(a, b) for a, b in zip(gpu, k)]
    print("reppoints margins: forward k_ref %.3f k_gpu %.3f; gradients k_ref %.3f k_gpu %.3f; d_moment_transfer "
          "k_ref %.3f k_gpu %.3f" % (ref[0], gpu[0], ref[1], gpu[1], ref[2], gpu[2]))
    for kg, kr in zip(gpu, ref):
        assert kg <= 2 * kr + 2


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["tied-minmax", "coincident-points", "all-weights-zero"])
def test_hip_exact_cases_equal_the_restatement(ops, which):
    c = dict(rr.exact_loss_cases())[which]
    tg = rr.targets_f32(c)
    want, got = rr.losses_f32(c, tg), _run_losses(ops, c, tg)
    for key in ("loss_init", "loss_refine", "d_mt"):
        assert _same(got[key], want[key]), (which, key)
    for s in ("d_init", "d_refine"):
        for a, b in zip(got[s], want[s]):
            assert _same(a, b), (which, s)
    if which == "tied-minmax":          # every tied point holds the gradient: more non-zeros than positive sides
        w = tg["label_refine"] > 0
        assert w.any() and sum(int((d != 0).sum()) for d in got["d_refine"]) > 4 * int(w.sum())
    if which == "coincident-points":    # std = 0: the expression as written is 0 * inf
        assert np.isnan(got["d_init"][0][0, :, 2, 3]).all() and np.isnan(got["d_refine"][0][0, :, 2, 3]).all()
        assert np.isfinite(got["d_init"][0][1]).all() and np.isfinite(got["loss_init"]).all()
    if which == "all-weights-zero":
        assert not got["loss_init"].any() and not got["loss_refine"].any() and not got["d_mt"].any()
        assert all(not d.any() for d in got["d_init"] + got["d_refine"])


@pytest.mark.gpu
def test_hip_req_add_accumulates(ops):
    name, c, tg, r32, _ = loss_refs()[0]
    rs = np.random.RandomState(5)
    base = ([rs.standard_normal(p.shape).astype(F32) for p in c["pts_init"]],
            [rs.standard_normal(p.shape).astype(F32) for p in c["pts_refine"]], F32([0.5, -2.0]))
    plain = _run_losses(ops, c, tg)
    got = _run_losses(ops, c, tg, req="add", d_init=[_dev(a) for a in base[0]], d_refine=[_dev(a) for a in base[1]],
                      d_moment_transfer=_dev(base[2]))
    for s, b in (("d_init", base[0]), ("d_refine", base[1])):
        for a, x, p in zip(got[s], b, plain[s]):
            assert np.array_equal(_bits(a), _bits(x + p)), s
    assert np.array_equal(_bits(got["d_mt"]), _bits(base[2] + plain["d_mt"]))


def _chain(ops, c, b):
    t = ops.reppoints_target(b["pi"], b["gt"], c["strides"], moment_transfer=b["mt"], **_kw_t(c), label_init=b.get("li"),
                             gt_init=b.get("gi"), label_refine=b.get("lr"), gt_refine=b.get("gr"), state=b.get("state"),
                             workspace=b.get("ws_t"))
    li, lr = ops.reppoints_box_loss_forward(b["pi"], b["pr"], t, c["strides"], moment_transfer=b["mt"], **_kw_l(c),
                                            loss_init=b.get("oi"), loss_refine=b.get("or"))
    di, dr, dmt = ops.reppoints_box_loss_backward(b["pi"], b["pr"], t, c["strides"], moment_transfer=b["mt"], **_kw_l(c),
                                                  d_init=b.get("di"), d_refine=b.get("dr"),
                                                  d_moment_transfer=b.get("dmt"), workspace=b.get("ws_l"))
    return list(t) + [li, lr] + list(di) + list(dr) + [dmt]


def _inputs(c):
    return dict(pi=[_dev(p) for p in c["pts_init"]], pr=[_dev(p) for p in c["pts_refine"]], gt=_dev(c["gt_bbox"]),
                mt=_dev(c["mt"]))


@pytest.mark.gpu
def test_hip_chain_repeats_and_replays_on_changed_inputs(ops):
    import torch
    (_, c), (_, c2) = rr.loss_cases()[3], rr.loss_cases()[3]          # several workgroups per image, M = 100
    c2 = dict(c2, gt_bbox=np.roll(c["gt_bbox"], 3, axis=1) + F32([4, 2, 4, 2, 0]),
              pts_init=[p * F32(0.75) for p in c["pts_init"]], pts_refine=[p * F32(1.25) for p in c["pts_refine"]],
              mt=F32([-0.5, 0.125]))
    want = []
    for case in (c, c2, c):
        b = _inputs(case)
        first = [t.clone() for t in _chain(ops, case, b)]
        for x, y in zip(first, _chain(ops, case, b)):
            assert torch.equal(_tbits(x), _tbits(y))
        want.append(first)
    assert not torch.equal(want[0][0], want[1][0])
    b = _inputs(c)
    N, P = want[0][0].shape
    M = c["gt_bbox"].shape[1]
    E = lambda *shape, dt=torch.float32: torch.empty(shape, device="cuda", dtype=dt)
    b.update(li=E(N, P), gi=E(N, P, 4), lr=E(N, P), gr=E(N, P, 4), state=E(4, dt=torch.int32), oi=E(N, P, 4),
             dmt=E(2), di=[torch.empty_like(t) for t in b["pi"]], dr=[torch.empty_like(t) for t in b["pr"]],
             ws_t=E(ops.reppoints_target_workspace_bytes(N, M, P), dt=torch.uint8),
             ws_l=E(ops.reppoints_box_loss_workspace_bytes(N, P), dt=torch.uint8))
    b["or"] = E(N, P, 4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _chain(ops, c, b)                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _chain(ops, c, b)
    for case, first in zip((c, c2, c), want):
        fresh = _inputs(case)
        for dst, src in zip(b["pi"] + b["pr"] + [b["gt"], b["mt"]], fresh["pi"] + fresh["pr"] + [fresh["gt"], fresh["mt"]]):
            dst.copy_(src)
        for t in out:
            t.zero_() if t.dtype == torch.int32 else t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(first, out):
            assert torch.equal(_tbits(x), _tbits(y))


@pytest.mark.gpu
@pytest.mark.parametrize("skew", [0, 4])
def test_hip_red_zones_and_pointers_off_their_16_byte_boundary(ops, skew):
    """every input, output and workspace sits in one arena filled with a sentinel, 4 KB guards around each; with
    skew = 4 every pointer is 4 bytes past a 16-byte boundary.  Equal bits to the plain run, no guard byte changed."""
    import torch
    _, c = rr.loss_cases()[0]
    plain = _inputs(c)
    want = _chain(ops, c, plain)
    N, P = want[0].shape
    M = c["gt_bbox"].shape[1]
    arena = torch.full((4 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
    spans, off = [], 0

    def carve(shape, dt=torch.float32):
        nonlocal off
        n = int(np.prod(shape)) * 4
        start = (off + 4096 + 255) // 256 * 256 + skew
        spans.append((start, start + n))
        off = start + n
        return arena[start:start + n].view(dt).reshape(shape)

    def put(t):
        v = carve(tuple(t.shape), t.dtype)
        v.copy_(t)
        return v
    b = dict(pi=[put(t) for t in plain["pi"]], pr=[put(t) for t in plain["pr"]], gt=put(plain["gt"]), mt=put(plain["mt"]))
    b.update(li=carve((N, P)), gi=carve((N, P, 4)), lr=carve((N, P)), gr=carve((N, P, 4)), state=carve((4,), torch.int32),
             oi=carve((N, P, 4)), dmt=carve((2,)), di=[carve(tuple(t.shape)) for t in plain["pi"]],
             dr=[carve(tuple(t.shape)) for t in plain["pr"]])
    b["or"] = carve((N, P, 4))
    b["ws_t"] = carve(((ops.reppoints_target_workspace_bytes(N, M, P) + 3) // 4,), torch.int32).view(torch.uint8)
    b["ws_l"] = carve(((ops.reppoints_box_loss_workspace_bytes(N, P) + 3) // 4,), torch.int32).view(torch.uint8)
    got = _chain(ops, c, b)
    torch.cuda.synchronize()
    for x, y in zip(want, got):
        assert y.data_ptr() % 16 == skew and torch.equal(_tbits(x), _tbits(y))
    keep = torch.ones(arena.numel(), dtype=torch.bool, device="cuda")
    for s, e in spans:
        keep[s:e] = False
    assert bool((arena[keep] == 0xA5).all()), "a store outside the buffers the library was given"


@pytest.mark.gpu
def test_autograd_function_and_empty_problem(ops):
    import torch
    name, c, tg, _, _ = loss_refs()[1]
    b = _inputs(c)
    t = _targets_of(tg)
    req = [[x.clone().requires_grad_(True) for x in b["pi"]], [x.clone().requires_grad_(True) for x in b["pr"]]]
    li, lr = ops.reppoints_box_loss(req[0], req[1], t, c["strides"], **_kw_l(c))
    (li.sum() * 3.0 + lr.sum()).backward()        # the incoming gradient is ignored, as MakeLoss does
    di, dr, _ = ops.reppoints_box_loss_backward(b["pi"], b["pr"], t, c["strides"], **_kw_l(c))
    for a, w in zip(req[0] + req[1], di + dr):
        assert torch.equal(_tbits(a.grad), _tbits(w))
    empty = [torch.empty(2, 18, 0, 3, device="cuda")]
    t0 = ops.reppoints_target(empty, b["gt"], (8,), transform="minmax")
    assert t0.label_init.shape == (2, 0) and list(t0.state.cpu().numpy()) == [0, 0, 0x3f800000, 0x3f800000]
