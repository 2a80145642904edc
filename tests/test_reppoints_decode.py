"""sd_reppoints_decode (simpledet_amd/csrc/reppoints_decode.hip): RepPointsHead.get_prediction in one call.

The reference is the spec: tests/golden/reppoints_decode.npz holds what the reference's own, unmodified
get_prediction gave (tests/golden/make_golden_reppoints_decode.py) for the cases of tests/reppoints_decode_ref.py, and
the device must give the same BITS on every element of both outputs.  The fixture feeds probabilities and
moment_transfer = 0, so no libm is in those bits; the device's expf enters in two tests of their own:
  * a non-zero moment_transfer: cls_score stays bit-equal (the selection does not look at the boxes); each box
    coordinate is held to |gpu - ref| <= 8 * 2^-23 * (s * (|mean| + half) + |point|), in float64 from the
    restatement's intermediates.  Derivation: two expf within 2 ulp of the truth give at most 4 eps on half * s; three
    later roundings (the product by s, mean -+ half, the add of the point) of at most eps / 2 each act on that
    magnitude; the clip does not expand a difference.  A derived envelope, not a measured one.
  * the fused sigmoid: input_logits = 1 equals sd_fcos_sigmoid followed by input_logits = 0, bit for bit."""
import ctypes
import functools
import os

import numpy as np
import pytest

from simpledet_amd import _lib

from . import reppoints_decode_ref as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reppoints_decode.npz")
KEYS = ("cls_score", "bbox_xyxy")
F32 = np.float32


@functools.lru_cache(maxsize=None)
def _cases():
    return dict(dr.cases())


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _want(name):
    g = _golden()
    return {k: g["%s/%s" % (name, k)] for k in KEYS}


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _known_case(k):
    """C = 2, H = 1, W = 2, stride 8, four points, moment with moment_transfer = 0, image 12 x 20.
    Location 0 at (0, 0): x = (-1, 1, -1, 1): mean 0, std 1; y = (0, 2, 0, 2): mean 1, std 1
        -> box (-1, 0, 1, 2) * 8 + (0, 0, 0, 0) = (-8, 0, 8, 16) -> clipped to (0, 0, 8, 11)
    Location 1 at (8, 0): x = (.5, 1.5, .5, 1.5): mean 1, std .5; y = (-1, -1, -1, -1): mean -1, std 0
        -> box (.5, -1, 1.5, -1) * 8 + (8, 0, 8, 0) = (12, -8, 20, -8) -> clipped to (12, 0, 19, 0)
    Scores: location 0 (0.25, 0.5), location 1 (0.75, 0.125): maxima 0.5 and 0.75, so location 1 comes first."""
    cls = F32([[0.25, 0.75], [0.5, 0.125]]).reshape(1, 2, 1, 2)
    x0, y0, x1, y1 = (-1, 1, -1, 1), (0, 2, 0, 2), (.5, 1.5, .5, 1.5), (-1, -1, -1, -1)
    pts = np.zeros((1, 8, 1, 2), F32)
    pts[0, 0::2, 0, 0], pts[0, 1::2, 0, 0] = y0, x0
    pts[0, 0::2, 0, 1], pts[0, 1::2, 0, 1] = y1, x1
    c = dict(cls=[cls], pts=[pts], im_info=F32([[12, 20, 1]]), strides=[8], ks=[k], transform="moment", mt=F32([0, 0]),
             num_points=4)
    score = F32([[[0, 0.75, 0.125], [0, 0.25, 0.5]]])
    box = F32([[[12, 0, 19, 0], [0, 0, 8, 11]]])
    n = k if k > 0 else 2
    return c, score[:, :n], box[:, :n]


# ------------------------------------------------------------------------------------------ CPU --
def _tab(n, v=64):
    return (ctypes.c_void_p * n)(*([v] * n))


def _iarr(v):
    return (ctypes.c_int * len(v))(*v)


def _decode_args(**kw):
    a = dict(L=2, N=1, C=3, K=9, tr=2, logits=0, H=(7, 4), W=(11, 6), stride=(8, 64), k=(8, -1), cls=None, pts=None,
             info=64, mt=64, score=64, box=64, ws=256, ws_bytes=1 << 30)
    a.update(kw)
    L = max(a["L"], 1) if a["L"] <= 8 else a["L"]
    tab = lambda key: a[key] if a[key] is not None else _tab(L)
    fit = lambda v: _iarr((list(v) * L)[:L])
    return (tab("cls"), tab("pts"), ctypes.c_void_p(a["info"]), ctypes.c_void_p(a["mt"]), fit(a["H"]), fit(a["W"]),
            fit(a["stride"]), fit(a["k"]), a["L"], a["N"], a["C"], a["K"], a["tr"], a["logits"],
            ctypes.c_void_p(a["score"]), ctypes.c_void_p(a["box"]), ctypes.c_void_p(a["ws"]),
            ctypes.c_size_t(a["ws_bytes"]), None)


def test_decode_rejects_bad_arguments_without_a_gpu():
    l = _lib.lib()

    def bad(match, code, **kw):
        with pytest.raises(_lib.SimpleDetOpsError, match=match) as e:
            l.call("sd_reppoints_decode", *_decode_args(**kw))
        assert e.value.code == code, (kw, e.value.code)

    bad("expected 1..8", -1, L=0)
    bad("expected 1..8", -1, L=9)
    bad("bad dimensions", -1, C=0)
    bad("bad dimensions", -1, N=-1)
    bad("num_points=0", -1, K=0)
    bad("first four points, num_points=3", -1, K=3, tr=1)
    bad("level 1 is", -1, H=(7, 0))
    bad("level 0 is", -1, W=(0, 6))
    bad("stride 0 of level 1", -1, stride=(8, 0))
    bad("level 1 keeps k = 25 of 24", -1, k=(8, 25))
    bad("transform=3", -1, tr=3)
    bad("transform=-1", -1, tr=-1)
    bad("needs moment_transfer", -1, mt=None)
    bad("input_logits=2", -1, logits=2)
    bad("input_logits=-1", -1, logits=-1)
    bad("null tensor pointer", -1, info=None)
    bad("null tensor pointer", -1, score=None)
    bad("null tensor pointer", -1, box=None)
    nul = _tab(2)
    nul[1] = None
    bad("null pointer in level 1", -1, pts=nul)
    bad("null pointer in level 1", -1, cls=nul)
    bad("16-byte aligned", -1, ws=260)
    bad("keeps 16385 rows, more than 16384", -2, H=(129, 4), W=(128, 6), k=(16385, -1))
    bad("keeps 16512 rows, more than 16384", -2, H=(129, 4), W=(128, 6), k=(-1, -1))
    bad("more than 2\\^24", -2, H=(4097, 4), W=(4096, 6))
    bad("N=65536 images", -2, N=65536)
    bad("N\\*C\\*H\\*W = .* more than 2\\^31 - 1", -2, N=2, C=80, H=(4096, 4), W=(4096, 6))
    bad("N\\*R\\*\\(C\\+1\\) = .* more than 2\\^31 - 1", -2, N=65535, C=1, H=(128, 128), W=(128, 128), k=(-1, -1))
    bad("null workspace", -4, ws=None)
    bad("workspace too small", -4, ws_bytes=256)
    # minmax and partial_minmax do not need moment_transfer; N = 0 is valid: nothing to write, nothing touched
    assert l.call("sd_reppoints_decode", *_decode_args(N=0, tr=0, mt=None, info=None, score=None, box=None, ws=None)) == 0
    assert l.call("sd_reppoints_decode", *_decode_args(N=0, tr=1, K=4, mt=None, ws=None)) == 0


def test_workspace_query():
    q = _lib.lib().cdll.sd_reppoints_decode_workspace_bytes
    hw = lambda *v: (ctypes.c_long * len(v))(*v)
    base = q(1, 3, 2, hw(77, 24), _iarr((8, -1)))
    assert base > 256 and base % 256 == 0
    # grows with what sizes a buffer: images, locations, rows kept; not with the classes
    assert q(2, 3, 2, hw(77, 24), _iarr((8, -1))) > base and q(1, 3, 2, hw(770, 24), _iarr((8, -1))) > base
    assert q(1, 3, 2, hw(77, 24), _iarr((77, -1))) > base and q(1, 80, 2, hw(77, 24), _iarr((8, -1))) == base
    # holds the documented buffers: the maxima (N, P) and the selected locations (N, R)
    sizes = [(100, 167), (50, 84), (25, 42), (13, 21), (7, 11)]
    hws = [h * w for h, w in sizes]
    ks = dr.topk_table((8, 16, 32, 64, 128), 1000)
    R = sum(k if k > 0 else n for k, n in zip(ks, hws))
    assert R == 3350
    need = 2 * sum(hws) * 4 + 2 * R * 4
    got = q(2, 80, 5, hw(*hws), _iarr(ks))
    assert need <= got <= need + 4 * 256
    # invalid dimensions and N = 0: the minimum
    for args in ((0, 3, 2, hw(77, 24), _iarr((8, -1))), (1, 0, 2, hw(77, 24), _iarr((8, -1))),
                 (1, 3, 9, hw(*[4] * 9), _iarr([1] * 9)), (1, 3, 2, hw(77, 24), _iarr((8, 25))),
                 (1, 3, 2, hw(77, 0), _iarr((8, -1))), (1, 3, 2, None, _iarr((8, -1))), (1, 3, 2, hw(77, 24), None),
                 (1, 3, 2, hw(77, 20000), _iarr((8, -1)))):
        assert q(*args) == 256


def test_topk_table_is_the_references_rule():
    from simpledet_amd import ops
    assert ops.reppoints_topk_table((8, 16, 32, 64, 128), 1000) == [1000, 1000, 1000, -1, -1]
    assert ops.reppoints_topk_table((8, 16, 32, 64, 128), 1000) == dr.topk_table((8, 16, 32, 64, 128), 1000)


def test_restatement_equals_the_reference_fixture():
    g = _golden()
    assert list(g["cases"]) == list(_cases()) == list(dr.CASE_NAMES)
    for name, c in _cases().items():
        got = dr.run(c)
        for k in KEYS:
            assert _same_bits(got[k], g["%s/%s" % (name, k)]), (name, k)
        if name in dr.HAND_MADE:                                   # the stored inputs are the ones regenerated here
            for l, (x, p) in enumerate(zip(c["cls"], c["pts"])):
                assert _same_bits(x, g["%s/cls%d" % (name, l)]) and _same_bits(p, g["%s/pts%d" % (name, l)]), name
            assert _same_bits(c["im_info"], g["%s/im_info" % name])


def test_known_answer_two_locations():
    for k in (-1, 2, 1):
        c, score, box = _known_case(k)
        got = dr.run(c)
        assert _same_bits(got["cls_score"], score) and _same_bits(got["bbox_xyxy"], box), k


# ------------------------------------------------------------------------------------------ GPU --
def _dev(a, skew=0):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not skew:
        return t.cuda()
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
    start = (-(buf.data_ptr() // 4) % 4) + skew // 4
    v = buf[start:start + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == skew
    return v


def _inputs(c, skew=0):
    return ([_dev(x, skew) for x in c["cls"]], [_dev(x, skew) for x in c["pts"]], _dev(c["im_info"], skew),
            _dev(c["mt"], skew))


def _run(ops, c, ins=None, logits=False, **kw):
    cls, pts, info, mt = ins or _inputs(c)
    out = ops.reppoints_decode(cls, pts, info, c["strides"], c["ks"], transform=c["transform"],
                               moment_transfer=mt if c["transform"] == "moment" else None, input_logits=logits, **kw)
    return dict(zip(KEYS, out))


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", dr.CASE_NAMES)
def test_hip_decode_equals_the_reference_fixture(ops, name):
    c, want = _cases()[name], _want(name)
    got = _np(_run(ops, c))
    for k in KEYS:
        assert got[k].shape == want[k].shape, (k, got[k].shape)
        bad = np.nonzero(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert _same_bits(got[k], want[k]), "%s/%s: %d elements differ, first at %s" % (
            name, k, len(bad[0]), [int(b[0]) for b in bad])


@pytest.mark.gpu
def test_hip_known_answer_two_locations(ops):
    """the hand-worked numbers of test_known_answer_two_locations, on the device"""
    for k in (-1, 2, 1):
        c, score, box = _known_case(k)
        got = _np(_run(ops, c))
        assert _same_bits(got["cls_score"], score) and _same_bits(got["bbox_xyxy"], box), (k, got)


@pytest.mark.gpu
def test_hip_nonzero_moment_transfer_within_the_derived_envelope(ops):
    c = dr.mt_case()
    want, got = dr.run(c, detail=True), _np(_run(ops, c))
    assert _same_bits(got["cls_score"], want["cls_score"])
    f64 = lambda k: want[k].astype(np.float64)
    bound = 8 * 2.0 ** -23 * (f64("stride") * (np.abs(f64("mean")) + f64("half")) + np.abs(f64("point")))
    err = np.abs(got["bbox_xyxy"].astype(np.float64) - f64("bbox_xyxy"))
    print("moment_transfer %s: max |gpu - ref| / bound = %.4f" % (c["mt"], float((err / bound).max())))
    assert (bound > 0).all() and (err <= bound).all()
    # the exp matters here: with moment_transfer = 0 the boxes would be others
    assert not np.array_equal(want["bbox_xyxy"], dr.run(dict(c, mt=F32([0, 0])))["bbox_xyxy"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["five_levels", "multi_wg", "saturated"])
def test_hip_fused_sigmoid_equals_sigmoid_then_decode(ops, name):
    import torch
    c = dr.logits_case(_cases()["multi_wg" if name == "saturated" else name], 7, saturate=name == "saturated")
    cls, pts, info, mt = _inputs(c)
    fused = _run(ops, c, (cls, pts, info, mt), logits=True)
    probs = [ops.fcos_sigmoid(x) for x in cls]
    plain = _run(ops, c, (probs, pts, info, mt), logits=False)
    for k in KEYS:
        assert torch.equal(_bits(fused[k]), _bits(plain[k])), (name, k)
    if name == "saturated":
        # more maxima than rows kept share the probability 1.0f, and their logits differ: the selection among them
        # is by location, which a sigmoid of the maximum logit would not reproduce
        p, x = probs[0].cpu().numpy(), c["cls"][0]
        m, top = p.max(1).reshape(p.shape[0], -1), x.max(1).reshape(x.shape[0], -1)
        for i in range(p.shape[0]):
            one = m[i] == 1
            assert one.sum() > c["ks"][0] and len(np.unique(top[i][one])) > c["ks"][0]
    else:
        assert all(0 < float(p.min()) and float(p.max()) < 1 for p in probs)


@pytest.mark.gpu
def test_hip_empty_batch(ops):
    c = _cases()["exact_k"]
    empty = dict(c, cls=[x[:0] for x in c["cls"]], pts=[x[:0] for x in c["pts"]], im_info=c["im_info"][:0])
    out = _run(ops, empty)
    assert out["cls_score"].shape == (0, 16, 5) and out["bbox_xyxy"].shape == (0, 16, 4)


def _buffers(ops, c):
    import torch
    N, C = c["cls"][0].shape[:2]
    hws = [x.shape[2] * x.shape[3] for x in c["cls"]]
    R = sum(k if k > 0 else hw for k, hw in zip(c["ks"], hws))
    wsb = ops.reppoints_decode_workspace_bytes(N, C, hws, c["ks"])
    return N, C, R, wsb, dict(cls_score=torch.empty(N, R, C + 1, device="cuda"), bbox_xyxy=torch.empty(N, R, 4, device="cuda"),
                              workspace=torch.empty(wsb, device="cuda", dtype=torch.uint8))


@pytest.mark.gpu
def test_hip_repeats_and_replays_on_changed_inputs_with_equal_bits(ops):
    import torch
    for name in ("five_levels", "multi_wg"):
        c = _cases()[name]
        other = dict(c, cls=[np.ascontiguousarray(x[::-1, :, ::-1]) for x in c["cls"]],
                     pts=[np.ascontiguousarray(-x[::-1]) for x in c["pts"]], im_info=c["im_info"] - F32(7))
        ins = _inputs(c)
        first = {k: v.clone() for k, v in _run(ops, c, ins).items()}
        second = _run(ops, c, ins)
        for k in KEYS:
            assert torch.equal(_bits(first[k]), _bits(second[k])), (name, k)
        eager_other = {k: v.clone() for k, v in _run(ops, other).items()}
        assert not torch.equal(_bits(first["bbox_xyxy"]), _bits(eager_other["bbox_xyxy"]))
        _, _, _, _, bufs = _buffers(ops, c)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _run(ops, c, ins, **bufs)                             # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = _run(ops, c, ins, **bufs)
        for want, src in ((first, c), (eager_other, other), (first, c)):
            for dst, a in zip(ins[0] + ins[1] + [ins[2]], src["cls"] + src["pts"] + [src["im_info"]]):
                dst.copy_(torch.from_numpy(a))
            for t in out.values():
                t.fill_(float("nan"))
            bufs["workspace"].fill_(0xFF)                         # the workspace needs no clearing
            graph.replay()
            torch.cuda.synchronize()
            for k in KEYS:
                assert torch.equal(_bits(want[k]), _bits(out[k])), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("skew", [0, 4])
def test_hip_red_zones_and_pointers_off_their_16_byte_boundary(ops, skew):
    """both outputs and the workspace sit in one arena filled with a sentinel, 4 KB guards around each; with skew = 4
    every tensor pointer -- inputs included -- is 4 bytes past a 16-byte boundary (the workspace stays aligned, as
    the entry point demands).  The results equal the fixture and no guard byte changes."""
    import torch
    for name in ("five_levels", "multi_wg", "four_points_moment"):
        c, want = _cases()[name], _want(name)
        N, C, R, wsb, _ = _buffers(ops, c)
        arena = torch.full((4 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
        spans, off = [], 0

        def carve(nbytes, dtype, shape, sk):
            nonlocal off
            start = (off + 4096 + 255) // 256 * 256 + sk
            off = start + nbytes
            spans.append((start, off))
            return arena[start:off].view(dtype).reshape(shape)

        E = lambda *shape: carve(4 * int(np.prod(shape)), torch.float32, shape, skew)
        bufs = dict(cls_score=E(N, R, C + 1), bbox_xyxy=E(N, R, 4), workspace=carve(wsb, torch.uint8, (wsb,), 0))
        assert off + 4096 <= arena.numel()
        got = _run(ops, c, _inputs(c, skew), **bufs)
        torch.cuda.synchronize()
        for k in KEYS:
            assert got[k].data_ptr() % 16 == skew and _same_bits(got[k].cpu().numpy(), want[k]), (name, k)
        keep = torch.ones(arena.numel(), dtype=torch.bool, device="cuda")
        for s, e in spans:
            keep[s:e] = False
        assert bool((arena[keep] == 0xA5).all()), "a store outside the buffers the library was given"
