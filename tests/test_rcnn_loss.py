"""The Faster / Mask R-CNN loss heads on the device against tests/rcnn_loss_ref.py.

  prob, reg_loss, both gradients, reg_sum   k_gpu <= 2 k_ref + 2 against the float64 truth (k_ref = the float32 host
                                            restatement's own k on that case; both are printed)
  valid, correct, fg                        exact against the restatement's metrics() on the DEVICE'S OWN prob
  zeros of the gradients                    exact: ignored rows, weight 0
  equal bits                                a second call, pointers 4 bytes off their 16-byte boundary, a call with both
                                            halves against the two half calls, graph replay on changed inputs, the
                                            L = 5 call against five L = 1 calls (class gradients, valid handed in)
"""
import ctypes

import numpy as np
import pytest

from tests import rcnn_loss_ref as rl

F = rl.F
SENT = -12345.0
RPN_NAMES = [c[0] for c in rl.RPN_CASES]
RCNN_CASES = [(R, K, ag) for R, K in rl.RCNN_SHAPES for ag in (False, True)]


class Guarded:
    """a device tensor of `shape` with sentinel floats on either side; offset: its data pointer sits 4 bytes off its
    16-byte boundary"""

    def __init__(self, shape, offset=False, src=None, dtype=None):
        import torch
        n = int(np.prod(shape))
        self.lead = 5 if offset else 4
        self.buf = torch.full((n + 12,), SENT, dtype=torch.float32, device="cuda")
        self.t = self.buf[self.lead:self.lead + n].view(tuple(shape))
        if src is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(src, F)).view(tuple(shape)))
        else:
            self.t.fill_(float("nan"))
        if dtype is not None:
            self.t = self.t.view(dtype)
        assert self.t.data_ptr() % 16 == (4 if offset else 0)

    def check(self, what):
        n = self.t.numel()
        g = self.buf.cpu().numpy()
        assert np.all(g[:self.lead] == F(SENT)) and np.all(g[self.lead + n:] == F(SENT)), what + ": sentinel overwritten"
        return g[self.lead:self.lead + n].reshape(tuple(self.t.shape))


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def _same_bits(a, b, what):
    if isinstance(a, list):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            _same_bits(x, y, "%s[%d]" % (what, i))
    else:
        assert np.array_equal(_bits(a), _bits(b)), what


def _state_of(words):
    """{valid, correct, fg, reg_sum} of the four words read back as floats' bits"""
    w = _bits(words)
    return dict(valid=int(w[0]), correct=int(w[1]), fg=int(w[2]), reg_sum=w[3:4].view(F)[0])


# ------------------------------------------------------------------------------------------- RPN --
def _run_rpn(ops, c, offset=False, half="both", valid=None):
    """forward and backward on guarded buffers -> dict of numpy arrays (lists for the per-level gradients).
    half: 'both', 'cls' or 'box'.  valid: the normaliser handed to the backward instead of the forward's."""
    import torch
    N, A, HW = c["N"], c["A"], c["HW"]
    do_cls, do_box = half in ("both", "cls"), half in ("both", "box")
    gi = dict(label=Guarded(c["label"].shape, offset, c["label"]), target=Guarded(c["target"].shape, offset, c["target"]),
              weight=Guarded(c["weight"].shape, offset, c["weight"]))
    cls = [Guarded(t.shape, offset, t) for t in c["cls"]]
    delta = [Guarded(t.shape, offset, t) for t in c["delta"]]
    o = dict(state=Guarded((4,), offset, dtype=torch.int32))
    if do_cls:
        o["prob"] = Guarded((N, 2, A, HW), offset)
    if do_box:
        o["reg_loss"] = Guarded((N, 4 * A, HW), offset)
    d_cls = [Guarded(t.shape, offset) for t in c["cls"]] if do_cls else None
    d_delta = [Guarded(t.shape, offset) for t in c["delta"]] if do_box else None
    args = ([g.t for g in cls] if do_cls else None, [g.t for g in delta] if do_box else None,
            gi["label"].t, gi["target"].t, gi["weight"].t)
    ops.rpn_loss_forward(*args, sigma=c["sigma"], prob=o["prob"].t if do_cls else None,
                         reg_loss=o["reg_loss"].t if do_box else None, state=o["state"].t)
    state = o["state"].t
    if valid is not None:
        state = torch.tensor([valid, 0, 0, 0], dtype=torch.int32, device="cuda")
    ops.rpn_loss_backward(*args, state, cls_grad_scale=c["cls_gs"], reg_grad_scale=c["reg_gs"], sigma=c["sigma"],
                          d_cls=[g.t for g in d_cls] if do_cls else None,
                          d_delta=[g.t for g in d_delta] if do_box else None)
    res = {k: g.check(k) for k, g in o.items()}
    if do_cls:
        res["d_cls"] = [g.check("d_cls") for g in d_cls]
    if do_box:
        res["d_delta"] = [g.check("d_delta") for g in d_delta]
    for k, g in gi.items():
        assert np.array_equal(_bits(g.check(k)), _bits(c[k])), k + " was written"
    for lst, src in ((cls, c["cls"]), (delta, c["delta"])):
        for g, s in zip(lst, src):
            assert np.array_equal(_bits(g.check("level")), _bits(s)), "an input level was written"
    res.update(_state_of(res.pop("state")))
    return res


def _against_truth(got, tr, T, f32, what):
    k_ref = rl.k_all(f32, tr, T)
    k_gpu = rl.k_all(got, tr, T)
    for o in k_ref:
        print("%s %s: k_gpu %.3f k_ref %.3f" % (what, o, k_gpu[o], k_ref[o]))
    for o in k_ref:
        assert k_gpu[o] <= 2 * k_ref[o] + 2, (what, o, k_gpu[o], k_ref[o])


@pytest.mark.gpu
@pytest.mark.parametrize("name", RPN_NAMES)
def test_hip_rpn_loss_against_the_truth(ops, name):
    c = rl.make_rpn_case(name)
    got = _run_rpn(ops, c)
    tr, T = rl.rpn_case_fn(rl.rows_truth, c)
    f32 = rl.rpn_case_fn(rl.rows_f32, c)
    assert np.isfinite(got["prob"]).all() and np.isfinite(got["reg_loss"]).all()       # the +-1e4 logits included
    _against_truth(got, tr, T, f32, "rpn " + name)
    # the state block: exact against the metrics of the device's own prob
    correct, valid, _, fg = rl.metrics(got["prob"].reshape(c["N"], 2, -1), c["label"], None, ignore=-1)
    assert (got["correct"], got["valid"], got["fg"]) == (correct, valid, fg)
    k = c["label"].astype(np.int32)
    assert valid == int((k != -1).sum()) and fg == int(((k != -1) & (k != 0)).sum())
    if c["tie_row"] is not None and name not in ("all_ignored",):
        # the one-ulp tie: the probabilities tie on the device too, so the row is a miss (its label is the class
        # the logits prefer)
        row = got["prob"].reshape(c["N"], 2, -1).transpose(0, 2, 1).reshape(-1, 2)[c["tie_row"]]
        assert row[0] == row[1] == 0.5
    # zeros, exactly: the class gradient of ignored rows, the box gradient under weight 0
    ign = (k == -1).reshape(c["N"], 1, c["A"], c["HW"])
    g = rl.rpn_concat(got["d_cls"], None)[0]
    assert not g[np.broadcast_to(ign, g.shape)].any()
    assert np.array_equal(g == 0, rl.rpn_concat(f32["d_cls"], None)[0] == 0)
    gd = rl.rpn_concat(None, got["d_delta"])[1]
    assert not gd[c["weight"] == 0].any()
    assert np.array_equal(gd == 0, rl.rpn_concat(None, f32["d_delta"])[1] == 0)
    if name == "all_ignored":
        assert got["valid"] == 0 and not g.any()           # norm 1, every class gradient exactly 0
    if name == "none_ignored":
        assert got["valid"] == c["label"].size
    # equal bits: a second call, pointers 4 bytes off their 16-byte boundary, the two half calls
    for other in (_run_rpn(ops, c), _run_rpn(ops, c, offset=True)):
        for key in got:
            _same_bits(got[key], other[key], key)
    hc, hb = _run_rpn(ops, c, half="cls"), _run_rpn(ops, c, half="box")
    for key in ("prob", "d_cls", "valid", "correct", "fg"):
        _same_bits(got[key], hc[key], "cls half " + key)
    for key in ("reg_loss", "d_delta", "reg_sum"):
        _same_bits(got[key], hb[key], "box half " + key)
    assert (hb["valid"], hb["correct"], hb["fg"]) == (0, 0, 0) and _bits(hc["reg_sum"])[0] == 0


@pytest.mark.gpu
def test_hip_rpn_loss_five_levels_equal_five_single_level_calls(ops):
    c = rl.make_rpn_case("fpn5")
    got = _run_rpn(ops, c)
    N, A, HW = c["N"], c["A"], c["HW"]
    o = 0
    for l, (h, w) in enumerate(c["sizes"]):
        sub = dict(c, HW=h * w, sizes=(c["sizes"][l],), cls=[c["cls"][l]], delta=[c["delta"][l]],
                   label=np.ascontiguousarray(c["label"].reshape(N, A, HW)[:, :, o:o + h * w]).reshape(N, -1),
                   target=np.ascontiguousarray(c["target"][:, :, o:o + h * w]),
                   weight=np.ascontiguousarray(c["weight"][:, :, o:o + h * w]))
        one = _run_rpn(ops, sub, valid=got["valid"])
        _same_bits(got["d_cls"][l], one["d_cls"][0], "d_cls of level %d" % l)
        _same_bits(got["d_delta"][l], one["d_delta"][0], "d_delta of level %d" % l)
        _same_bits(got["prob"][..., o:o + h * w], one["prob"], "prob of level %d" % l)
        o += h * w


@pytest.mark.gpu
def test_hip_rpn_loss_weight_zero_against_a_nan_delta(ops):
    c, cn = rl.make_rpn_case("fpn5"), rl.make_rpn_case("fpn5", nan=True)
    got, gn = _run_rpn(ops, c), _run_rpn(ops, cn)
    f32 = rl.rpn_case_fn(rl.rows_f32, cn)
    assert np.isnan(f32["reg_loss"].reshape(-1)[cn["nan_at"]])            # the product form: 0 * NaN
    assert np.array_equal(np.isnan(gn["reg_loss"]), np.isnan(f32["reg_loss"])) and np.isnan(gn["reg_loss"]).sum() == 1
    assert np.isnan(gn["reg_sum"])
    # every other element, and the class half, as without the NaN
    keep = ~np.isnan(f32["reg_loss"])
    changed = np.zeros(keep.shape, bool)
    changed.reshape(-1)[cn["nan_at"]] = True
    assert np.array_equal(_bits(gn["reg_loss"])[~changed], _bits(got["reg_loss"])[~changed])
    for key in ("prob", "d_cls", "valid", "correct", "fg"):
        _same_bits(got[key], gn[key], key)


@pytest.mark.gpu
def test_hip_rpn_loss_graph_replay_on_changed_inputs_gives_equal_bits(ops):
    import torch
    cases = [rl.make_rpn_case("fpn5", seed=0), rl.make_rpn_case("fpn5", seed=1)]
    N, A, HW = cases[0]["N"], cases[0]["A"], cases[0]["HW"]
    L = len(cases[0]["cls"])

    def tensors(c):
        return [torch.from_numpy(t).cuda() for t in c["cls"] + c["delta"] + [c["label"], c["target"], c["weight"]]]

    def chain(t, ws=None):
        out = ops.rpn_loss_forward(t[:L], t[L:2 * L], *t[2 * L:], workspace=ws)
        d_cls, d_delta = ops.rpn_loss_backward(t[:L], t[L:2 * L], *t[2 * L:], out.state, cls_grad_scale=128.0,
                                               reg_grad_scale=0.25)
        return [out.prob, out.reg_loss, out.state] + d_cls + d_delta
    eager = [[e.clone() for e in chain(tensors(c))] for c in cases]
    static = tensors(cases[0])
    ws = torch.empty(ops.rpn_loss_workspace_bytes(N, A, HW), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap = chain(static, ws)
    for i in (1, 0, 1):
        for t, src in zip(static, tensors(cases[i])):
            t.copy_(src)
        for o in cap:
            o.fill_(-1)
        ws.fill_(0xFF)                                   # nothing is expected of the workspace: no memset
        graph.replay()
        torch.cuda.synchronize()
        for e, o in zip(eager[i], cap):
            assert torch.equal(e.view(torch.int32), o.view(torch.int32))


@pytest.mark.gpu
def test_hip_rpn_anchor_target_chain_as_a_graph_equals_the_eager_calls(ops):
    import torch
    from simpledet_amd import synth
    cfg = dict(stride=(16, 32), short=(50, 25), long=(84, 42), scales=(8,), aspects=(0.5, 1.0, 2.0),
               allowed_border=0, pos_thr=0.7, neg_thr=0.3, min_pos_thr=0.0, image_anchor=64, pos_fraction=0.5)
    prm = ops.rpn_target_param(**cfg)
    B, A = 2, 3
    rs = np.random.RandomState(5)
    im_info = torch.from_numpy(np.array([[800, 1333, 1.0]] * B, F)).cuda()
    gt = torch.from_numpy(np.ascontiguousarray(synth.gt_boxes(3, B, 20))).cuda()
    cls = [torch.from_numpy((rs.standard_normal((B, 2 * A, h, w)) * 2).astype(F)).cuda() for h, w in ((50, 84), (25, 42))]
    delta = [torch.from_numpy(rs.standard_normal((B, 4 * A, h, w)).astype(F)).cuda() for h, w in ((50, 84), (25, 42))]

    def chain(st):
        label, target, weight = ops.rpn_anchor_target(im_info, gt, prm, st, layout=1)
        out = ops.rpn_loss_forward(cls, delta, label, target, weight)
        d_cls, d_delta = ops.rpn_loss_backward(cls, delta, label, target, weight, out.state, cls_grad_scale=1.0,
                                               reg_grad_scale=1.0 / (B * 64))
        return [label, out.prob, out.reg_loss, out.state] + d_cls + d_delta
    st = ops.mt19937_state(seed=7)
    eager = [e.clone() for e in chain(st)]
    words = _state_of(eager[3].view(torch.float32).cpu().numpy())
    lab = eager[0].cpu().numpy().astype(np.int32)
    assert words["valid"] == int((lab != -1).sum()) == B * 64 and words["fg"] == int((lab == 1).sum()) > 0
    st2 = ops.mt19937_state(seed=7)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap = chain(st2)
    st2.copy_(ops.mt19937_state(seed=7))
    graph.replay()
    torch.cuda.synchronize()
    for e, o in zip(eager, cap):
        assert torch.equal(e.view(torch.int32), o.view(torch.int32))


@pytest.mark.gpu
def test_hip_rpn_loss_autograd_against_torch_float64(ops):
    import torch
    c = rl.make_rpn_case("a1")
    c["label"] = np.where(c["label"] > 1, F(1), c["label"]).astype(F)      # nll_loss takes no label outside the classes
    N, A, HW = c["N"], c["A"], c["HW"]
    cls = [torch.from_numpy(t).cuda().requires_grad_(True) for t in c["cls"]]
    delta = [torch.from_numpy(t).cuda().requires_grad_(True) for t in c["delta"]]
    fixed = [torch.from_numpy(c[k]).cuda() for k in ("label", "target", "weight")]
    out = ops.rpn_loss(cls, delta, *fixed, cls_grad_scale=c["cls_gs"], reg_grad_scale=c["reg_gs"], sigma=3.0)
    (out.prob.sum() + out.reg_loss.sum()).backward()
    # the reference's graph in float64: reshape, concat, softmax cross-entropy with ignore_index, the smooth-L1 chain
    cls64 = [torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in c["cls"]]
    delta64 = [torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in c["delta"]]
    x = torch.cat([t.reshape(N, 2, A, -1) for t in cls64], dim=-1).reshape(N, 2, A * HW)
    d = torch.cat([t.reshape(N, 4 * A, -1) for t in delta64], dim=2)
    label = torch.from_numpy(c["label"]).long()
    norm = max(1, int((label != -1).sum()))
    ce = torch.nn.functional.cross_entropy(x, label, ignore_index=-1, reduction="sum") * (c["cls_gs"] / norm)
    v = d - torch.from_numpy(c["target"].astype(np.float64))
    ib = float(rl.IBSQ[3.0])
    bsq = float(F(3) * F(3))
    sl1 = torch.where(v.abs() > ib, v.abs() - 0.5 * ib, 0.5 * bsq * v * v)
    reg = (torch.from_numpy(c["weight"].astype(np.float64)) * sl1).sum() * float(F(c["reg_gs"]))
    (ce + reg).backward()
    tr, T = rl.rpn_case_fn(rl.rows_truth, c)
    k_ref = rl.k_all(rl.rpn_case_fn(rl.rows_f32, c), tr, T)
    for l in range(len(cls)):
        np.testing.assert_allclose(cls64[l].grad.numpy(), tr["d_cls"][l], rtol=1e-9, atol=1e-13)   # the truth is that graph
        np.testing.assert_allclose(delta64[l].grad.numpy(), tr["d_delta"][l], rtol=1e-9, atol=1e-13)
        kc = rl.k_of(cls[l].grad.cpu().numpy(), cls64[l].grad.numpy(), T["d_cls"][l])
        kd = rl.k_of(delta[l].grad.cpu().numpy(), delta64[l].grad.numpy(), T["d_delta"][l])
        print("rpn autograd level %d: d_cls k %.3f (k_ref %.3f), d_delta k %.3f (k_ref %.3f)"
              % (l, kc, k_ref["d_cls"], kd, k_ref["d_delta"]))
        assert kc <= 2 * k_ref["d_cls"] + 2 and kd <= 2 * k_ref["d_delta"] + 2


# ----------------------------------------------------------------------------------------- R-CNN --
def _run_rcnn(ops, c, offset=False, half="both"):
    import torch
    R, K, D = c["R"], c["K"], c["D"]
    do_cls, do_box = half in ("both", "cls"), half in ("both", "box")
    names = ("x", "label", "delta", "target", "weight")
    gi = {k: Guarded(c[k].shape, offset, c[k]) for k in names}
    o = dict(state=Guarded((4,), offset, dtype=torch.int32))
    if do_cls:
        o.update(prob=Guarded((R, K), offset), d_cls=Guarded((R, K), offset))
    if do_box:
        o.update(reg_loss=Guarded((R, D), offset), d_delta=Guarded((R, D), offset))
    args = (gi["x"].t if do_cls else None, gi["label"].t, gi["delta"].t if do_box else None, gi["target"].t,
            gi["weight"].t)
    ops.rcnn_loss_forward(*args, smooth_l1_scalar=c["sigma"], prob=o["prob"].t if do_cls else None,
                          reg_loss=o["reg_loss"].t if do_box else None, state=o["state"].t)
    ops.rcnn_loss_backward(*args, o["state"].t, cls_grad_scale=c["cls_gs"], reg_grad_scale=c["reg_gs"],
                           smooth_l1_scalar=c["sigma"], d_cls_logit=o["d_cls"].t if do_cls else None,
                           d_bbox_delta=o["d_delta"].t if do_box else None)
    res = {k: g.check(k) for k, g in o.items()}
    for k in names:
        assert np.array_equal(_bits(gi[k].check(k)), _bits(c[k])), k + " was written"
    res.update(_state_of(res.pop("state")))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("R,K,agnostic", RCNN_CASES)
def test_hip_rcnn_loss_against_the_truth(ops, R, K, agnostic):
    c = rl.make_rcnn_case(R, K, agnostic)
    got = _run_rcnn(ops, c)
    tr, T = rl.rcnn_case_fn(rl.rows_truth, c)
    f32 = rl.rcnn_case_fn(rl.rows_f32, c)
    assert np.isfinite(got["prob"]).all() and np.isfinite(got["reg_loss"]).all()
    _against_truth(got, tr, T, f32, "rcnn %dx%d D=%d" % (R, K, c["D"]))
    correct, valid, _, fg = rl.metrics(got["prob"], c["label"], None, ignore=None)
    assert (got["correct"], got["valid"], got["fg"]) == (correct, valid, fg) and valid == R
    if c["tie_row"] is not None:
        row, lab = got["prob"][c["tie_row"]], int(c["label"][c["tie_row"]])
        assert row[lab] == row.max() and int(np.argmax(row)) < lab        # tied on the device too: the lower class wins
    assert not got["d_delta"][c["weight"] == 0].any()
    assert np.array_equal(got["d_delta"] == 0, f32["d_delta"] == 0)
    # a label that names no class (-1, K, beyond): the gradient is p * scale, nothing subtracted
    k = c["label"].astype(np.int32)
    out = (k < 0) | (k >= K)
    scale = F(c["cls_gs"]) / F(R)
    assert np.array_equal(_bits(got["d_cls"][out]), _bits((got["prob"][out] * scale).astype(F)))
    for other in (_run_rcnn(ops, c), _run_rcnn(ops, c, offset=True)):
        for key in got:
            _same_bits(got[key], other[key], key)
    hc, hb = _run_rcnn(ops, c, half="cls"), _run_rcnn(ops, c, half="box")
    for key in ("prob", "d_cls", "valid", "correct", "fg"):
        _same_bits(got[key], hc[key], "cls half " + key)
    for key in ("reg_loss", "d_delta", "reg_sum"):
        _same_bits(got[key], hb[key], "box half " + key)


@pytest.mark.gpu
def test_hip_rcnn_loss_weight_zero_against_a_nan_delta(ops):
    c, cn = rl.make_rcnn_case(7, 81, False), rl.make_rcnn_case(7, 81, False, nan=True)
    got, gn = _run_rcnn(ops, c), _run_rcnn(ops, cn)
    f32 = rl.rcnn_case_fn(rl.rows_f32, cn)
    assert np.isnan(f32["reg_loss"].reshape(-1)[cn["nan_at"]])
    assert np.array_equal(np.isnan(gn["reg_loss"]), np.isnan(f32["reg_loss"])) and np.isnan(gn["reg_loss"]).sum() == 1
    assert np.isnan(gn["reg_sum"])
    changed = np.zeros(gn["reg_loss"].shape, bool)
    changed.reshape(-1)[cn["nan_at"]] = True
    assert np.array_equal(_bits(gn["reg_loss"])[~changed], _bits(got["reg_loss"])[~changed])
    for key in ("prob", "d_cls", "valid", "correct", "fg"):
        _same_bits(got[key], gn[key], key)


@pytest.mark.gpu
def test_hip_proposal_target_chain_as_a_graph_and_replay_on_changed_inputs(ops):
    import torch
    from simpledet_amd import synth
    B, S, K = 2, 64, 81
    prois, gt = synth.proposal_target_inputs(0, B, 400, 30)
    rois, gts = torch.from_numpy(prois).cuda(), torch.from_numpy(gt).cuda()
    rs = np.random.RandomState(9)
    xs = [torch.from_numpy((rs.standard_normal((B * S, K)) * 2).astype(F)).cuda() for _ in range(2)]
    ds = [torch.from_numpy(rs.standard_normal((B * S, 4 * K)).astype(F)).cuda() for _ in range(2)]

    def chain(x, d, rng, ws=None):
        pt = ops.proposal_target(rois, gts, K, B, S, rng_state=rng)
        label, target, weight = pt[1].reshape(-1), pt[2].reshape(B * S, -1), pt[3].reshape(B * S, -1)
        out = ops.rcnn_loss_forward(x, label, d, target, weight, workspace=ws)
        gx, gd = ops.rcnn_loss_backward(x, label, d, target, weight, out.state, cls_grad_scale=1.0,
                                        reg_grad_scale=1.0 / (B * S))
        return [label, out.prob, out.reg_loss, out.state, gx, gd]
    eager = [[e.clone() for e in chain(xs[i], ds[i], ops.glibc_rand_state(1))] for i in range(2)]
    words = _state_of(eager[0][3].view(torch.float32).cpu().numpy())
    assert words["valid"] == B * S and words["fg"] == int((eager[0][0] != 0).sum()) > 0
    sx, sd, rng = xs[0].clone(), ds[0].clone(), ops.glibc_rand_state(1)
    ws = torch.empty(ops.rcnn_loss_workspace_bytes(B * S), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap = chain(sx, sd, rng, ws)
    for i in (1, 0, 1):
        sx.copy_(xs[i])
        sd.copy_(ds[i])
        rng.copy_(ops.glibc_rand_state(1))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        for e, o in zip(eager[i], cap):
            assert torch.equal(e.view(torch.int32), o.view(torch.int32))


@pytest.mark.gpu
def test_hip_rcnn_loss_autograd_against_torch_float64(ops):
    import torch
    c = rl.make_rcnn_case(130, 81, False)
    K = c["K"]
    x = torch.from_numpy(c["x"]).cuda().requires_grad_(True)
    d = torch.from_numpy(c["delta"]).cuda().requires_grad_(True)
    fixed = [torch.from_numpy(c[k]).cuda() for k in ("label", "target", "weight")]
    out = ops.rcnn_loss(x, fixed[0], d, fixed[1], fixed[2], cls_grad_scale=c["cls_gs"], reg_grad_scale=c["reg_gs"],
                        smooth_l1_scalar=c["sigma"])
    (out.prob.sum() + out.reg_loss.sum()).backward()
    x64 = torch.from_numpy(c["x"].astype(np.float64)).requires_grad_(True)
    d64 = torch.from_numpy(c["delta"].astype(np.float64)).requires_grad_(True)
    k = torch.from_numpy(c["label"].astype(np.int32).astype(np.int64))
    hit = (k >= 0) & (k < K)
    # SoftmaxOutput's gradient is that of sum over the rows of -log p[label]; a label outside the classes adds
    # log sum exp alone (no class is subtracted)
    lse = torch.logsumexp(x64, dim=1)
    picked = torch.where(hit, x64.gather(1, k.clamp(0, K - 1)[:, None])[:, 0], torch.zeros_like(lse))
    ce = (lse - picked).sum() * (c["cls_gs"] / c["R"])
    v = d64 - torch.from_numpy(c["target"].astype(np.float64))
    bsq = float(F(c["sigma"]) * F(c["sigma"]))
    ib = float(F(1) / F(bsq))
    sl1 = torch.where(v.abs() > ib, v.abs() - 0.5 * ib, 0.5 * bsq * v * v)
    reg = (torch.from_numpy(c["weight"].astype(np.float64)) * sl1).sum() * float(F(c["reg_gs"]))
    (ce + reg).backward()
    tr, T = rl.rcnn_case_fn(rl.rows_truth, c)
    k_ref = rl.k_all(rl.rcnn_case_fn(rl.rows_f32, c), tr, T)
    np.testing.assert_allclose(x64.grad.numpy(), tr["d_cls"], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(d64.grad.numpy(), tr["d_delta"], rtol=1e-9, atol=1e-13)
    kc = rl.k_of(x.grad.cpu().numpy(), x64.grad.numpy(), T["d_cls"])
    kd = rl.k_of(d.grad.cpu().numpy(), d64.grad.numpy(), T["d_delta"])
    print("rcnn autograd: d_cls k %.3f (k_ref %.3f), d_delta k %.3f (k_ref %.3f)" % (kc, k_ref["d_cls"], kd, k_ref["d_delta"]))
    assert kc <= 2 * k_ref["d_cls"] + 2 and kd <= 2 * k_ref["d_delta"] + 2


# ------------------------------------------------------------------------------- without a device --
def test_the_cases_hold_what_they_are_named_for():
    c = rl.make_rpn_case("fpn5")
    assert c["HW"] == 53 and [h * w for h, w in c["sizes"]].count(1) == 2 and c["N"] * c["A"] * c["HW"] > 256
    assert rl.make_rpn_case("span3")["sizes"][0][0] * rl.make_rpn_case("span3")["sizes"][0][1] >= 3 * 256
    s2 = rl.make_rpn_case("stride2")
    assert s2["N"] * s2["A"] * s2["HW"] > 1024 * 256
    assert (rl.make_rpn_case("all_ignored")["label"] == -1).all()
    assert not (rl.make_rpn_case("none_ignored")["label"] == -1).any()
    k = c["label"].astype(np.int32)
    assert (k >= 2).any() and (k == -1).any()
    rows = rl.rpn_concat(c["cls"], None)[0].reshape(c["N"], 2, -1).transpose(0, 2, 1).reshape(-1, 2)
    assert (rows[:, 0] == rows[:, 1]).any() and (np.abs(rows) == 1e4).any()
    # the one-ulp tie really ties in the restatement, and the label is the class the LOGITS prefer
    p = rl.softmax_rows_f32(rows[c["tie_row"]][None])[0]
    assert rows[c["tie_row"], 1] == np.nextafter(rows[c["tie_row"], 0], F(1)) and p[0] == p[1]
    assert int(c["label"].reshape(-1)[c["tie_row"]]) == 1
    # v exactly at +-1 / sigma^2 and one ulp to either side; weights other than 0 / 1
    v = (np.concatenate([t.reshape(c["N"], 4 * c["A"], -1) for t in c["delta"]], axis=2) - c["target"]).reshape(-1)
    ib = rl.IBSQ[3.0]
    for want in (ib, -ib, np.nextafter(ib, F(1)), np.nextafter(ib, F(0)), -np.nextafter(ib, F(1)), -np.nextafter(ib, F(0))):
        assert (v == want).any()
    assert set(np.unique(c["weight"])) >= {F(0), F(0.25), F(1), F(2.5)}
    r = rl.make_rcnn_case(130, 81, False)
    k = r["label"].astype(np.int32)
    assert (k == -1).any() and (k >= 81).any() and r["label"][1] == F(2.7)
    p = rl.softmax_rows_f32(r["x"][r["tie_row"]][None])[0]
    assert p[3] == p[5] == p.max() and r["x"][r["tie_row"], 5] > r["x"][r["tie_row"], 3] and k[r["tie_row"]] == 5
    assert rl.make_rcnn_case(3, 200, True)["K"] > 128 and rl.make_rcnn_case(4100, 3, True)["R"] > 4096


def test_python_rejects_what_is_not_built():
    from simpledet_amd import ops
    for kw in (dict(normalization="batch"), dict(normalization="null"), dict(smooth_alpha=0.1), dict(out_grad=True)):
        with pytest.raises(NotImplementedError):
            ops.rpn_loss_forward(None, None, None, None, None, **kw)
    for kw in (dict(normalization="valid"), dict(normalization="null"), dict(smooth_alpha=0.1), dict(out_grad=True)):
        with pytest.raises(NotImplementedError):
            ops.rcnn_loss_forward(None, None, None, None, None, **kw)
        with pytest.raises(NotImplementedError):
            ops.rcnn_loss_backward(None, None, None, None, None, None, **kw)


def test_entry_points_reject_bad_arguments_before_the_device():
    from simpledet_amd._lib import lib
    cd = lib().cdll
    one = (ctypes.c_void_p * 1)(256)
    hw = (ctypes.c_long * 1)(4)
    p = ctypes.c_void_p(256)
    z = ctypes.c_size_t(0)

    def rpn(L=1, N=1, A=1, ignore=-1.0, sigma=3.0, cls=one, delta=one, ws=None, wsb=z):
        return cd.sd_rpn_loss_fwd(cls, delta, hw, L, p, p, p, N, A, ignore, sigma, p, p, p, ws, wsb, None)
    assert rpn(L=0) == -1 and rpn(L=9) == -1 and rpn(A=0) == -1 and rpn(N=-1) == -1
    assert rpn(sigma=0.0) == -1 and rpn(ignore=-0.5) == -1 and rpn(cls=None, delta=None) == -1
    assert rpn() == -4                                         # a NULL workspace
    assert rpn(N=0) == 0                                       # an empty problem: no launch
    assert cd.sd_rpn_loss_workspace_bytes(2, 3, ctypes.c_long(89023)) >= 1024 * 16
    assert cd.sd_rpn_loss_workspace_bytes(0, 3, ctypes.c_long(5)) == 256

    def rcnn(R=4, K=81, D=324, sigma=1.0, x=p, d=p):
        return cd.sd_rcnn_loss_fwd(x, p, d, p, p, R, K, D, sigma, p, p, p, None, z, None)
    assert rcnn(K=0) == -1 and rcnn(R=-1) == -1 and rcnn(sigma=-1.0) == -1 and rcnn(x=None, d=None) == -1
    assert rcnn(K=1025) == -2
    assert rcnn() == -4 and rcnn(R=0) == 0
    assert cd.sd_rcnn_loss_bwd(p, p, p, p, p, 4, 81, 324, 1.0, 1.0, 1.0, None, p, p, None) == -1      # no state
