"""The CrowdHuman double-prediction head (simpledet_amd/csrc/crowdhuman_head.hip).

  RoI targets  against tests/golden/crowdhuman_target.npz, what the reference's own bbox_target.py / bbox_sec_target.py
               gave on the cases of tests/crowdhuman_ref.target_cases() with the real np.random (the generator,
               tests/golden/make_golden_crowdhuman.py, asserts that every such case fills all its rows).
               exact -- sampled_proposal, both labels, both weights, the dx / dy columns of both targets, count, and
               all 625 words of the generator state.
               within a margin -- the dw / dh columns: numpy's float32 log is not correctly rounded and depends on the
               host's SIMD dispatch, so both sides are measured against the float64 truth of the same float32 operands,
                   k = |got - truth| / (eps32 * T + tiny)                         (tests/crowdhuman_ref.py)
               and k on the GPU must not exceed 2 * k_ref + 2, k_ref = the recorded reference's own k on that case.
  EMD loss     R in {37, 1024}, K in {2, 3}: forward and the four gradients against the float64 truth by the same rule
               (k_ref = the float32 host restatement's k), the pairing exact; equal bits over repeated calls, graph
               replay and pointers 4 bytes off their 16-byte boundary; the softmax-entropy terms against what the
               reference's own softmax_entropy_op.py gave (tests/golden/crowdhuman_softmax_entropy.npz).
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from simpledet_amd import _lib

from . import crowdhuman_ref as cr
from .test_sigmoid_ce import Guarded, _bits, P256

F = np.float32
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ("sampled_proposal", "bbox_cls", "bbox_target", "bbox_target_weight", "bbox_sec_cls", "bbox_sec_target",
         "bbox_sec_target_weight")


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(GOLDEN, "crowdhuman_target.npz"))


@functools.lru_cache(maxsize=None)
def _cases():
    return {c["name"]: c for c in cr.target_cases()}


@functools.lru_cache(maxsize=None)
def _loss_cases():
    return cr.loss_cases()


CASE_NAMES = [c["name"] for c in cr.target_cases(full=False)] + ["full-m0", "full-m1"]


# ------------------------------------------------------------------------------------------ CPU --
def test_the_fixture_holds_the_inputs_the_cases_build():
    g = _golden()
    for name, c in _cases().items():
        assert np.array_equal(_bits(g[name + "/proposal"]), _bits(c["proposal"])), name
        assert np.array_equal(_bits(g[name + "/gt"]), _bits(c["gt"])), name
        S = c["cfg"]["image_rois"]
        assert g[name + "/sampled_proposal"].shape == c["proposal"].shape[:1] + (S, 4), name   # every row filled


def test_the_cases_cover_what_they_are_named_for():
    g = _golden()
    # list sizes: n = 1 (no draw) and 2; the quota; the segment edges -- read off the fixture's foreground rows
    fg = lambda name: [(g[name + "/bbox_cls"][b] > 0).sum() for b in range(g[name + "/bbox_cls"].shape[0])]
    assert fg("n1-n2-m1") == [1, 2] and fg("quota-m1") == [16, 10, 16]
    assert fg("half-even-17-m0") == [8, 8] and fg("half-even-19-m0") == [10, 10]              # 8.5 -> 8, 9.5 -> 10
    # a single gt in the class: no second foreground; duplicates: every foreground has a second one
    assert not g["single-gt-m1/bbox_sec_cls"].any() and g["single-gt-m1/bbox_cls"].any()
    d = g["duplicate-gt-m1/bbox_cls"] > 0
    assert np.array_equal(g["duplicate-gt-m1/bbox_sec_cls"][d], g["duplicate-gt-m1/bbox_cls"][d])
    assert set(np.unique(g["three-classes-m1/bbox_cls"])) == {0.0, 1.0, 2.0}


def test_loss_inputs_are_ties_by_construction_or_clearly_apart():
    for c in _loss_cases().values():
        cr.check_loss_inputs(c)
        r = cr.emd_f32(c)
        assert set(np.unique(r["pairing"])) == {1, 2}
        s2 = c["sigma"] ** 2
        v = np.abs(c["d1"] - c["t1"])[c["w1"] > 0]
        assert (v < 1 / s2).any() and (v >= 1 / s2).any()                    # both smooth-L1 branches
        assert (c["w1"].sum(1) == 0).any() and "observable-tie" in c["recipes"]
        tie = [i for i, w in enumerate(c["recipes"]) if w == "observable-tie"]
        assert (r["pairing"][tie] == 1).all()


def test_softmax_entropy_restatement_equals_the_reference_op():
    fx = np.load(os.path.join(GOLDEN, "crowdhuman_softmax_entropy.npz"))
    for name, x, y, og in cr.ce_fixture_inputs():
        ce, p, _ = cr.softmax_entropy(x, y)
        fwd, bwd = fx[name + "/forward"], fx[name + "/backward"]
        np.testing.assert_array_equal(fwd.sum(1), ce, err_msg=name)
        oh = (np.arange(x.shape[1])[None] == y.astype(np.int64)[:, None]).astype(F)
        np.testing.assert_array_equal(bwd, ((p - oh) * F(og)).astype(F), err_msg=name)
        assert fwd[0, 1] == F(-np.log(F(1e-10)))                              # the 1e-10 decides this element


def _tgt_call(ptrs=None, B=2, P=8, M=4, mode=1, cfg=None, ws=P256, wsb=1 << 24, mt=P256):
    from simpledet_amd import ops
    prm = ops.CrowdHumanTargetParam()
    c = dict(cr.CONFIG, **(cfg or {}))
    prm.num_reg_class, prm.add_gt_to_proposal, prm.image_rois = c["num_reg_class"], 1, c["image_rois"]
    prm.fg_fraction, prm.fg_thresh, prm.bg_thresh_hi, prm.bg_thresh_lo = 0.5, 0.5, 0.5, 0.0
    for i, v in enumerate(c["bbox_target_std"]):
        prm.bbox_target_std[i] = v
    p = [P256] * 10 if ptrs is None else ptrs
    return _lib.lib().call("sd_crowdhuman_target", p[0], p[1], B, P, M, mode, ctypes.byref(prm), mt, *p[2:], ws,
                           ctypes.c_size_t(wsb), None)


def test_entry_points_reject_bad_arguments():
    for kw, msg in ((dict(mode=2), "mode"), (dict(M=0), "bad B"), (dict(M=1025), "M=1025"), (dict(P=4000, M=100), "P \\+ M"),
                    (dict(cfg=dict(image_rois=1025)), "image_rois"), (dict(cfg=dict(num_reg_class=1)), "num_reg_class"),
                    (dict(cfg=dict(bbox_target_std=(0.1, 0.0, 0.2, 0.2))), "bbox_target_std"), (dict(mt=None), "null"),
                    (dict(ws=None), "workspace too small"), (dict(wsb=8), "workspace too small")):
        with pytest.raises(_lib.SimpleDetOpsError, match=msg):
            _tgt_call(**kw)
    for i in (1, 2, 3, 4, 5, 9):
        with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
            _tgt_call(ptrs=[None if j == i else P256 for j in range(10)])
    with pytest.raises(_lib.SimpleDetOpsError, match="second outputs"):
        _tgt_call(ptrs=[P256] * 6 + [None] * 3 + [P256])
    assert _tgt_call(B=0, ptrs=[None] * 10, ws=None, wsb=0, mt=None) == 0
    l = _lib.lib()
    l.cdll.sd_crowdhuman_target_workspace_bytes.restype = ctypes.c_size_t
    sizes = [l.cdll.sd_crowdhuman_target_workspace_bytes(2, P, 500) for P in (0, 300, 2000, 3596)]
    assert sizes == sorted(sizes) and sizes[0] >= 256
    fwd = lambda **kw: l.call("sd_emd_loss_fwd", *kw.get("p", [P256] * 10), kw.get("R", 4), kw.get("K", 2), kw.get("D", 8),
                              kw.get("s", 1.0), kw.get("loss", P256), None, None)
    bwd = lambda **kw: l.call("sd_emd_loss_bwd", *kw.get("p", [P256] * 10), kw.get("R", 4), kw.get("K", 2), kw.get("D", 8),
                              kw.get("s", 1.0), 1.0, *kw.get("g", [P256] * 4), None)
    for fn in (fwd, bwd):
        for kw, msg in ((dict(R=-1), "bad R"), (dict(K=0), "bad R"), (dict(s=0.0), "smooth_l1_scalar"),
                        (dict(p=[None] + [P256] * 9), "null pointer"), (dict(p=[P256] * 9 + [None]), "null pointer")):
            with pytest.raises(_lib.SimpleDetOpsError, match=msg):
                fn(**kw)
        with pytest.raises(_lib.SimpleDetOpsError, match="2\\^31") as e:
            fn(R=1 << 28, K=2, D=8)
        assert e.value.code == _lib.SD_ERR_UNSUPPORTED
        assert fn(R=0, p=[None] * 10, loss=None, g=[None] * 4) == 0
    with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
        fwd(loss=None)
    with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
        bwd(g=[P256, None, P256, P256])


# ------------------------------------------------------------------------------------------ GPU --
def _state(ops, seed):
    return ops.mt19937_state(seed=int(seed))


def _run_target(ops, c, st, workspace=None, tensors=None):
    import torch
    t = tensors or (torch.from_numpy(c["proposal"]).cuda(), torch.from_numpy(c["gt"]).cuda())
    return ops.crowdhuman_target(t[0], t[1], st, double=c["mode"] == 1, workspace=workspace, **c["cfg"])


def _check_state(st, g, name):
    s = st.cpu().numpy()
    assert np.array_equal(s[:624].view(np.uint32), g[name + "/mt_key"]), name + ": MT19937 key words"
    assert int(s[624]) == int(g[name + "/mt_pos"][0]), name + ": MT19937 position"


def _check_targets(res, g, name, mode, nrc):
    got = [None if t is None else t.cpu().numpy() for t in res]
    B, S = got[1].shape
    assert np.array_equal(got[7], np.full(B, S, np.int32)), name + ": count"
    heads = ((1, 2, 3, ""),) + (((4, 5, 6, "sec_"),) if mode == 1 else ())
    assert np.array_equal(_bits(got[0]), _bits(g[name + "/sampled_proposal"])), name + ": sampled_proposal"
    for ic, it, iw, pre in heads:
        assert np.array_equal(_bits(got[ic]), _bits(g["%s/%s" % (name, NAMES[ic])])), name + ": " + NAMES[ic]
        assert np.array_equal(_bits(got[iw]), _bits(g["%s/%s" % (name, NAMES[iw])])), name + ": " + NAMES[iw]
        want = g["%s/%s" % (name, NAMES[it])]
        xy = (np.arange(4 * nrc) % 4) < 2
        assert np.array_equal(_bits(got[it][..., xy]), _bits(want[..., xy])), name + ": dx / dy of " + NAMES[it]
        truth, T = g["%s/%starget_truth" % (name, pre)], g["%s/%starget_T" % (name, pre)]
        k_ref = cr.k_of(want[..., ~xy], truth[..., ~xy], T[..., ~xy])
        k_gpu = cr.k_of(got[it][..., ~xy], truth[..., ~xy], T[..., ~xy])
        print("%s %sdw/dh: k_gpu %.3f k_ref %.3f" % (name, pre, k_gpu, k_ref))
        assert k_gpu <= 2 * k_ref + 2, (name, NAMES[it], k_gpu, k_ref)
    if mode == 0:
        assert got[4] is None and got[5] is None and got[6] is None


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_hip_targets_equal_the_reference(ops, name):
    g, c = _golden(), _cases()[name]
    st = _state(ops, g[name + "/seed"][0])
    res = _run_target(ops, c, st)
    _check_targets(res, g, name, c["mode"], c["cfg"]["num_reg_class"])
    _check_state(st, g, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["config-small-m1", "n1-n2-m0", "n127-128-129-m1", "bg-above-1024-m0", "full-m1"])
def test_hip_lds_replay_variant_gives_the_same_bits(ops, name):
    """tuning crowdhuman_front = 1: the front of the permutations from a replay of all swaps in LDS"""
    g, c = _golden(), _cases()[name]
    l = _lib.lib()
    with l.tuned(crowdhuman_front=1):
        st = _state(ops, g[name + "/seed"][0])
        res = _run_target(ops, c, st)
        _check_targets(res, g, name, c["mode"], c["cfg"]["num_reg_class"])
        _check_state(st, g, name)


@pytest.mark.gpu
def test_hip_two_calls_continue_one_generator_stream(ops):
    g = _golden()
    st = _state(ops, g["two-calls/0/seed"][0])
    for i, c in enumerate((_cases()["config-small-m1"], cr.two_call_inputs())):
        name = "two-calls/%d" % i
        assert np.array_equal(_bits(g[name + "/proposal"]), _bits(c["proposal"]))
        res = _run_target(ops, c, st)
        _check_targets(res, g, name, 1, 2)
        _check_state(st, g, name)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (0, 1))
def test_hip_short_image_reports_its_count_and_zero_rows(ops, mode):
    g, c = _golden(), cr.short_case(mode)
    name = c["name"]
    assert np.array_equal(_bits(g[name + "/proposal"]), _bits(c["proposal"]))
    st = _state(ops, 77 + mode)
    res = _run_target(ops, c, st)
    got = [None if t is None else t.cpu().numpy() for t in res]
    xy = (np.arange(8) % 4) < 2
    for b in range(2):
        n = len(g["%s/%d/sampled_proposal" % (name, b)])
        assert got[7][b] == n and (n < 32) == (b == 0)
        for i in range(7 if mode == 1 else 4):
            want = g["%s/%d/%s" % (name, b, NAMES[i])]
            if i in (2, 5):
                # targets: dx / dy exactly.  dw / dh = iw log(q): either side lies within 2 eps32 T of the truth,
                # T = |iw| (1 + |log q|) (the quotient's rounding, a log good to an ulp, the product's rounding), so
                # they differ by at most 4 eps32 (|iw| + |dw|), |iw| <= 1 / 0.2 = 5
                assert np.array_equal(_bits(got[i][b, :n][:, xy]), _bits(want[:, xy])), (b, NAMES[i])
                np.testing.assert_allclose(got[i][b, :n], want, rtol=4 * 2.0 ** -23, atol=4 * 2.0 ** -23 * 5)
            else:
                assert np.array_equal(_bits(got[i][b, :n]), _bits(want)), (b, NAMES[i])
            assert not _bits(got[i][b, n:]).any(), (b, NAMES[i], "rows behind count are +0.0")
    _check_state(st, g, name)


@pytest.mark.gpu
def test_hip_target_graph_replay_on_changed_inputs_gives_equal_bits(ops):
    import torch
    g = _golden()
    cases = [_cases()["config-small-m1"], cr.two_call_inputs()]
    seeds = (11, 12)
    eager = []
    for c, seed in zip(cases, seeds):
        st = _state(ops, seed)
        eager.append([t.clone() for t in _run_target(ops, c, st)] + [st.clone()])
    static = (torch.from_numpy(cases[0]["proposal"]).cuda(), torch.from_numpy(cases[0]["gt"]).cuda())
    st = _state(ops, seeds[0])
    ws = torch.empty(ops.crowdhuman_target_workspace_bytes(2, 300, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap = _run_target(ops, cases[0], st, workspace=ws, tensors=static)
    for i in (1, 0, 1):
        static[0].copy_(torch.from_numpy(cases[i]["proposal"]))
        static[1].copy_(torch.from_numpy(cases[i]["gt"]))
        st.copy_(_state(ops, seeds[i]))
        for o in cap[:7]:
            o.fill_(float("nan"))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        for e, o in zip(eager[i], list(cap) + [st]):
            assert torch.equal(e.view(torch.int32), o.view(torch.int32))


LOSS_IN = ("x1", "x2", "y1", "y2", "d1", "d2", "t1", "t2", "w1", "w2")


def _run_loss(ops, c, offset=False):
    """forward and backward on guarded buffers -> dict of numpy arrays"""
    import torch
    gi = [Guarded(c[k].shape, offset, c[k]) for k in LOSS_IN]
    R, K = c["x1"].shape
    o = dict(loss=Guarded((1,), offset), g1=Guarded((R, K), offset), g2=Guarded((R, K), offset),
             gd1=Guarded((R, 4 * K), offset), gd2=Guarded((R, 4 * K), offset))
    pairing = torch.full((R + 2,), -7, dtype=torch.int32, device="cuda")
    ops.emd_loss_forward(*[t.t for t in gi], c["sigma"], loss=o["loss"].t, pairing=pairing[1:R + 1])
    ops.emd_loss_backward(*[t.t for t in gi], c["sigma"], c["scale"], d_cls_logit=o["g1"].t, d_cls_sec_logit=o["g2"].t,
                          d_bbox_delta=o["gd1"].t, d_bbox_sec_delta=o["gd2"].t)
    res = {k: v.check(k) for k, v in o.items()}
    p = pairing.cpu().numpy()
    assert p[0] == -7 and p[-1] == -7
    res["pairing"] = p[1:-1]
    for k, t in zip(LOSS_IN, gi):
        assert np.array_equal(_bits(t.check(k)), _bits(c[k])), k + " was written"
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("R,K", cr.LOSS_SHAPES)
def test_hip_emd_loss_against_the_truth(ops, R, K):
    c = _loss_cases()[R, K]
    got = _run_loss(ops, c)
    tr, T = cr.emd_truth(c)
    k_ref = cr.emd_k_ref(c)
    assert np.array_equal(got["pairing"], tr["pairing"]) and np.array_equal(got["pairing"], cr.emd_f32(c)["pairing"])
    tie = [i for i, w in enumerate(c["recipes"]) if w == "observable-tie"]
    assert (got["pairing"][tie] == 1).all()
    for o in cr.OUTS:
        k_gpu = cr.k_of(got[o], tr[o], T[o])
        print("R %d K %d %s: k_gpu %.3f k_ref %.3f" % (R, K, o, k_gpu, k_ref[o]))
        assert k_gpu <= 2 * k_ref[o] + 2, (o, k_gpu, k_ref[o])
    # a weight of 0 gives a gradient of exactly 0; the tie row's heads get different gradients (pairing 1 is visible)
    assert not got["gd1"][(c["w1"] == 0) & (c["w2"] == 0)].any()
    assert not np.array_equal(got["g1"][tie[0]], got["g2"][tie[0]])
    # equal bits: a second call, and pointers 4 bytes off their 16-byte boundary
    for other in (_run_loss(ops, c), _run_loss(ops, c, offset=True)):
        for k in got:
            assert np.array_equal(got[k].view(np.int32), other[k].view(np.int32)), k


@pytest.mark.gpu
def test_hip_emd_loss_softmax_entropy_terms_equal_the_reference_op(ops):
    """identical heads and labels, weights 0: L1 = L2 = 2 ce(x, y), so the loss is 2 mean(ce) and the gradient of either
    head is the reference op's backward with out_grad = grad_scale / R"""
    import torch
    fx = np.load(os.path.join(GOLDEN, "crowdhuman_softmax_entropy.npz"))
    for name, x, y, og in cr.ce_fixture_inputs():
        R, K = x.shape
        z = np.zeros((R, 4 * K), F)
        t = [torch.from_numpy(a).cuda() for a in (x, x, y, y, z, z, z, z, z, z)]
        loss = ops.emd_loss_forward(*t, 1.0).cpu().numpy()
        g1, g2, gd1, gd2 = [a.cpu().numpy() for a in ops.emd_loss_backward(*t, 1.0, og * R)]
        ce64, p64, Tce = cr.softmax_entropy(x, y, np.float64)
        fwd, bwd = fx[name + "/forward"].sum(1), fx[name + "/backward"]
        k_ref = cr.k_of(2 * fwd.astype(np.float64).mean(), 2 * ce64.mean(), 2 * Tce.mean())
        k_gpu = cr.k_of(loss[0], 2 * ce64.mean(), 2 * Tce.mean())
        oh = (np.arange(K)[None] == y.astype(np.int64)[:, None])
        mx = x.astype(np.float64).max(1, keepdims=True)
        ls = np.abs(np.log(np.exp(x - mx).sum(1, keepdims=True)))
        Tg = (p64 * (np.abs(x - mx) + ls + 2) + oh) * og
        kg_ref, kg_gpu = cr.k_of(bwd, (p64 - oh) * og, Tg), max(cr.k_of(g1, (p64 - oh) * og, Tg), cr.k_of(g2, (p64 - oh) * og, Tg))
        print("%s: loss k_gpu %.3f k_ref %.3f, gradient k_gpu %.3f k_ref %.3f" % (name, k_gpu, k_ref, kg_gpu, kg_ref))
        assert k_gpu <= 2 * k_ref + 2 and kg_gpu <= 2 * kg_ref + 2
        assert np.array_equal(g1, g2) and not gd1.any() and not gd2.any()


@pytest.mark.gpu
def test_hip_emd_loss_graph_replay_and_autograd(ops):
    import torch
    cases = [_loss_cases()[37, 3], cr.make_loss_case(37, 3, seed=5, scale=128.0, sigma=3.0)]

    def chain(t):
        loss, pairing = ops.emd_loss_forward(*t, 3.0, return_pairing=True)
        return (loss, pairing) + tuple(ops.emd_loss_backward(*t, 3.0, 128.0))
    eager = []
    for c in cases:
        eager.append([e.clone() for e in chain([torch.from_numpy(c[k]).cuda() for k in LOSS_IN])])
    static = [torch.from_numpy(cases[0][k]).cuda() for k in LOSS_IN]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap = chain(static)
    for i in (1, 0, 1):
        for t, k in zip(static, LOSS_IN):
            t.copy_(torch.from_numpy(cases[i][k]))
        for o in cap:
            o.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for e, o in zip(eager[i], cap):
            assert torch.equal(e.view(torch.int32), o.view(torch.int32))
    # autograd through ops.emd_loss against a float64 torch composition of the reference's graph
    c = cases[0]
    R, K = c["x1"].shape
    t32 = {k: torch.from_numpy(c[k]).cuda() for k in LOSS_IN}
    for k in ("x1", "x2", "d1", "d2"):
        t32[k].requires_grad_(True)
    loss = ops.emd_loss(t32["x1"], t32["x2"], t32["y1"], t32["y2"], t32["d1"], t32["d2"], t32["t1"], t32["t2"],
                        t32["w1"], t32["w2"], 3.0, 128.0)
    loss.backward()
    t64 = {k: torch.from_numpy(c[k].astype(np.float64)).requires_grad_(k in ("x1", "x2", "d1", "d2")) for k in LOSS_IN}

    class SoftmaxEntropy(torch.autograd.Function):
        """softmax_entropy_op.py: the forward, and the backward the operator DEFINES, (softmax - onehot) * out_grad --
        not the derivative of its forward (the 1e-10 is left out, and a label outside [0, K) still gets softmax)"""

        @staticmethod
        def forward(ctx, x, y):
            oh = (torch.arange(K)[None] == y[:, None]).double()     # mx.nd.one_hot: no column outside [0, K)
            p = torch.softmax(x, -1)
            ctx.save_for_backward(p, oh)
            return -oh * torch.log(p + 1e-10)

        @staticmethod
        def backward(ctx, og):
            p, oh = ctx.saved_tensors
            return (p - oh) * og, None

    def ce(x, y):
        return SoftmaxEntropy.apply(x, y).sum(-1)

    def sl1(v):
        return torch.where(v.abs() > 1 / 9.0, v.abs() - 0.5 / 9.0, 0.5 * 9.0 * v * v)
    L1 = ce(t64["x1"], t64["y1"]) + ce(t64["x2"], t64["y2"]) + (t64["w1"] * sl1(t64["d1"] - t64["t1"])
                                                              + t64["w2"] * sl1(t64["d2"] - t64["t2"])).sum(-1)
    L2 = ce(t64["x1"], t64["y2"]) + ce(t64["x2"], t64["y1"]) + (t64["w2"] * sl1(t64["d1"] - t64["t2"])
                                                              + t64["w1"] * sl1(t64["d2"] - t64["t1"])).sum(-1)
    ref = torch.where(L1 <= L2, L1, L2).mean()
    (ref * 128.0).backward()
    tr, T = cr.emd_truth(c)
    k_ref = cr.emd_k_ref(c)
    assert cr.k_of(float(loss.detach()), float(ref.detach()), T["loss"]) <= 2 * k_ref["loss"] + 2
    for k, o in (("x1", "g1"), ("x2", "g2"), ("d1", "gd1"), ("d2", "gd2")):
        np.testing.assert_allclose(t64[k].grad.numpy(), tr[o], rtol=1e-12, atol=1e-14)         # the truth is that graph
        k_gpu = cr.k_of(t32[k].grad.cpu().numpy(), t64[k].grad.numpy(), T[o])
        assert k_gpu <= 2 * k_ref[o] + 2, (o, k_gpu, k_ref[o])
