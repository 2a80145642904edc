"""sd_fcos_decode / sd_fcos_sigmoid (simpledet_amd/csrc/fcos_decode.hip): FCOSFPNHead.get_all_proposal in one call.

The reference is the spec: tests/golden/fcos_decode.npz holds what the reference's own two CustomOps gave
(tests/golden/make_golden_fcos_decode.py) for the cases of tests/fcos_decode_ref.py, and the device must give the same
on every element (np.array_equal: the sign of a zero is not pinned).  The tie cases are checked against the float32
restatement only, because the order among equal scores is the project's choice.

sd_fcos_sigmoid is held to the house margin of tests/test_focal_loss.py: k = |got - truth| / (eps32 * |truth| +
tiny32) against a float64 truth, k_gpu <= 2 * k_ref + 2 with k_ref the float32 numpy restatement's own k on the same
inputs (three roundings: exp, +, / -- under 3 ulp)."""
import ctypes
import functools
import os

import numpy as np
import pytest

from simpledet_amd import _lib

from . import fcos_decode_ref as dr
from . import focal_ref as fr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcos_decode.npz")
KEYS = ("stage", "bbox", "score", "cls_id")
F32 = np.float32


@functools.lru_cache(maxsize=None)
def _cases():
    return dict(dr.cases())


@functools.lru_cache(maxsize=None)
def _ties():
    return dict(dr.tie_cases())


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _want(name):
    g = _golden()
    return {k: g["%s/%s" % (name, k)] for k in KEYS}


def _restate(c):
    return dr.decode(c["cls"], c["ctr"], c["off"], c["im_info"], c["strides"], c["top_n"], c["thresh"])


# ------------------------------------------------------------------------------------------ CPU --
def _tab(n, v=64):
    return (ctypes.c_void_p * n)(*([v] * n))


def _iarr(v):
    return (ctypes.c_int * len(v))(*v)


def _decode_args(**kw):
    a = dict(L=2, N=1, C=3, top_n=8, thresh=0.05, logits=0, H=(7, 4), W=(11, 6), stride=(8, 16), cls=None, ctr=None,
             off=None, info=64, bbox=64, score=64, cls_id=64, stage=None, ws=256, ws_bytes=1 << 30)
    a.update(kw)
    L = max(a["L"], 1) if a["L"] <= 8 else a["L"]
    tab = lambda k: a[k] if a[k] is not None else _tab(L)
    fit = lambda v: _iarr((list(v) * L)[:L])
    return (tab("cls"), tab("ctr"), tab("off"), ctypes.c_void_p(a["info"]), fit(a["H"]), fit(a["W"]), fit(a["stride"]),
            a["L"], a["N"], a["C"], a["top_n"], a["thresh"], a["logits"], ctypes.c_void_p(a["bbox"]),
            ctypes.c_void_p(a["score"]), ctypes.c_void_p(a["cls_id"]), ctypes.c_void_p(a["stage"]),
            ctypes.c_void_p(a["ws"]), ctypes.c_size_t(a["ws_bytes"]), None)


def test_decode_rejects_bad_arguments_without_a_gpu():
    l = _lib.lib()

    def bad(match, code, **kw):
        with pytest.raises(_lib.SimpleDetOpsError, match=match) as e:
            l.call("sd_fcos_decode", *_decode_args(**kw))
        assert e.value.code == code, (kw, e.value.code)

    bad("expected 1..8", -1, L=0)
    bad("expected 1..8", -1, L=9)
    bad("top_n=0", -1, top_n=0)
    bad("bad dimensions", -1, N=-1)
    bad("bad dimensions", -1, C=0)
    bad("level 1 is", -1, H=(7, 0))
    bad("stride 0 of level 1", -1, stride=(8, 0))
    bad("NaN", -1, thresh=float("nan"))
    bad("input_logits=2", -1, logits=2)
    bad("null tensor pointer", -1, info=None)
    bad("null tensor pointer", -1, score=None)
    nul = _tab(2)
    nul[1] = None
    bad("null pointer in level 1", -1, off=nul)
    bad("misaligned|16-byte aligned", -1, ws=260)
    bad("C=81 classes exceed", -2, C=81)
    bad("more than 2\\^24", -2, C=80, H=(500, 4), W=(500, 6))
    bad("R = L\\*top_n = 16392 rows exceed the limit 16384", -2, top_n=8196)
    bad("N=65536 images", -2, N=65536)
    bad("null workspace", -4, ws=None)
    bad("workspace too small", -4, ws_bytes=1024)
    # N = 0 is valid: nothing to write, nothing touched
    assert l.call("sd_fcos_decode", *_decode_args(N=0, info=None, bbox=None, score=None, cls_id=None, ws=None)) == 0
    # the sigmoid
    with pytest.raises(_lib.SimpleDetOpsError, match="negative"):
        l.call("sd_fcos_sigmoid", ctypes.c_void_p(64), ctypes.c_void_p(64), -1, None)
    with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
        l.call("sd_fcos_sigmoid", None, ctypes.c_void_p(64), 4, None)
    assert l.call("sd_fcos_sigmoid", None, None, 0, None) == 0


def test_workspace_query():
    q = _lib.lib().cdll.sd_fcos_decode_workspace_bytes
    hw = lambda *v: (ctypes.c_long * len(v))(*v)
    base = q(1, 3, 2, hw(77, 24), 8)
    assert base > 256 and base % 256 == 0
    # grows with every argument that sizes a buffer
    assert q(2, 3, 2, hw(77, 24), 8) > base and q(1, 4, 2, hw(77, 24), 8) > base
    assert q(1, 3, 2, hw(77, 240), 8) > base and q(1, 3, 2, hw(77, 24), 1000) > base
    # holds at least the documented buffers: counters, sparse list, candidate words, fused scores, stage rows, values
    N, C, L, t, tot = 2, 80, 5, 1000, sum(h * w for h, w in dr.CONFIG_SIZES)
    need = N * L * (4096 + 4) * 4 + N * L * t * 4 + N * L * 16384 * 8 + N * C * tot * 4 + N * L * t * 7 * 4
    got = q(N, C, L, hw(*[h * w for h, w in dr.CONFIG_SIZES]), t)
    assert need <= got <= need + 8 * 256
    # invalid dimensions and N = 0: the minimum
    for args in ((0, 3, 2, hw(77, 24), 8), (1, 81, 2, hw(77, 24), 8), (1, 3, 9, hw(*[4] * 9), 8), (1, 3, 2, hw(77, 24), 0),
                 (1, 3, 2, hw(77, 0), 8), (1, 3, 2, None, 8)):
        assert q(*args) == 256


def test_the_build_rounds_sqrt_and_divide_correctly():
    """score = sqrtf(...) and the sigmoid's divide must be IEEE: the Makefile asks for it"""
    mk = open(os.path.join(os.path.dirname(_lib.HEADER), "..", "simpledet_amd", "csrc", "Makefile")).read()
    assert "-fhip-fp32-correctly-rounded-divide-sqrt" in mk and "-ffp-contract=off" in mk
    assert "-ffast-math" not in mk


def test_restatement_equals_the_reference_fixture():
    g = _golden()
    assert list(g["cases"]) == list(_cases()) == list(dr.CASE_NAMES) and list(_ties()) == list(dr.TIE_NAMES)
    for name, c in _cases().items():
        got = _restate(c)
        for k in KEYS:
            w = g["%s/%s" % (name, k)]
            assert w.dtype == np.float32 and got[k].shape == w.shape and np.array_equal(got[k], w), (name, k)


def test_known_answer_two_locations():
    """C = 1, H = 1, W = 2, stride 8: locations at cx = 4 and 12, cy = 4; all offsets 1."""
    cls = F32([0.5, 0.25]).reshape(1, 1, 1, 2)
    ctr = F32([0.5, 0.5]).reshape(1, 1, 1, 2)
    off = np.ones((1, 4, 1, 2), F32)
    info = F32([[100, 100, 1]])
    got = dr.decode([cls], [ctr], [off], info, [8], 2)            # count == top_n: dense
    assert np.array_equal(got["stage"][0], F32([[1, 0.25, 3, 3, 5, 5], [1, 0.125, 11, 3, 13, 5]]))
    assert np.array_equal(got["bbox"][0], F32([[3, 3, 5, 5], [11, 3, 13, 5]]))
    assert np.array_equal(got["cls_id"][0], F32([1, 1]))
    want = np.zeros((2, 81), F32)
    want[0, 1], want[1, 1] = 0.5, np.sqrt(F32(0.125))
    assert np.array_equal(got["score"][0], want)
    got = dr.decode([cls], [ctr], [off], info, [8], 3)            # count < top_n: sparse, one padding row
    assert np.array_equal(got["stage"][0, :2], F32([[1, 0.25, 3, 3, 5, 5], [1, 0.125, 11, 3, 13, 5]]))
    assert np.array_equal(got["stage"][0, 2], F32([-1] * 6)) and got["cls_id"][0, 2] == -1
    assert got["score"][0, 2, 80] == np.sqrt(F32(1e-20)) and not got["score"][0, 2, :80].any()
    # image smaller than the boxes: x2 clips to 12; a box with x1 = 0 <= cls and y1 = 0 <= fused is removed
    off2 = off.copy()
    off2[0, :2, 0, 0] = 9
    got = dr.decode([cls], [ctr], [off2], F32([[100, 12, 1]]), [8], 2)
    assert np.array_equal(got["stage"][0], F32([[-1] * 6, [1, 0.125, 11, 3, 12, 5]]))
    assert np.array_equal(got["bbox"][0], F32([[11, 3, 12, 5], [-1] * 4]))


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
    return ([_dev(x, skew) for x in c["cls"]], [_dev(x, skew) for x in c["ctr"]], [_dev(x, skew) for x in c["off"]],
            _dev(c["im_info"], skew))


def _run(ops, c, ins=None, logits=False, want_stage=True, **kw):
    cls, ctr, off, info = ins or _inputs(c)
    out = ops.fcos_decode(cls, ctr, off, info, c["strides"], c["top_n"], c["thresh"], input_logits=logits,
                          return_stage=want_stage, **kw)
    return dict(zip(("bbox", "score", "cls_id", "stage"), out))


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
        bad = np.nonzero(~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))))
        assert np.array_equal(got[k], want[k]), "%s/%s: %d elements differ, first at %s" % (
            name, k, len(bad[0]), [int(b[0]) for b in bad])


@pytest.mark.gpu
def test_hip_known_answer_two_locations(ops):
    """the hand-worked numbers of test_known_answer_two_locations, on the device"""
    cls = F32([0.5, 0.25]).reshape(1, 1, 1, 2)
    ctr = F32([0.5, 0.5]).reshape(1, 1, 1, 2)
    off = np.ones((1, 4, 1, 2), F32)
    c = dict(cls=[cls], ctr=[ctr], off=[off], im_info=F32([[100, 100, 1]]), strides=[8], top_n=2, thresh=dr.THRESH)
    got = _np(_run(ops, c))
    assert np.array_equal(got["stage"][0], F32([[1, 0.25, 3, 3, 5, 5], [1, 0.125, 11, 3, 13, 5]]))
    assert np.array_equal(got["bbox"][0], F32([[3, 3, 5, 5], [11, 3, 13, 5]]))
    want = np.zeros((2, 81), F32)
    want[0, 1], want[1, 1] = 0.5, np.sqrt(F32(0.125))
    assert np.array_equal(got["score"][0], want) and np.array_equal(got["cls_id"][0], F32([1, 1]))
    got = _np(_run(ops, dict(c, top_n=3)))                        # sparse, one padding row
    assert np.array_equal(got["stage"][0], F32([[1, 0.25, 3, 3, 5, 5], [1, 0.125, 11, 3, 13, 5], [-1] * 6]))
    assert got["score"][0, 2, 80] == np.sqrt(F32(1e-20)) and not got["score"][0, 2, :80].any()
    off2 = off.copy()
    off2[0, :2, 0, 0] = 9
    got = _np(_run(ops, dict(c, off=[off2], im_info=F32([[100, 12, 1]]))))
    assert np.array_equal(got["stage"][0], F32([[-1] * 6, [1, 0.125, 11, 3, 12, 5]]))
    assert np.array_equal(got["bbox"][0], F32([[11, 3, 12, 5], [-1] * 4]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", dr.TIE_NAMES)
def test_hip_tie_rule_equals_the_restatement(ops, name):
    c = _ties()[name]
    want, got = _restate(c), _np(_run(ops, c))
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (name, k)


@pytest.mark.gpu
def test_hip_stage_out_null_and_empty_batch(ops):
    import torch
    c = _cases()["branches"]
    with_stage, without = _run(ops, c), _run(ops, c, want_stage=False)
    assert set(without) == {"bbox", "score", "cls_id"}
    for k in without:
        assert torch.equal(_bits(with_stage[k]), _bits(without[k]))
    # N = 0: valid, every output empty
    empty = dict(c, cls=[x[:0] for x in c["cls"]], ctr=[x[:0] for x in c["ctr"]], off=[x[:0] for x in c["off"]],
                 im_info=c["im_info"][:0])
    out = _run(ops, empty)
    R = len(c["strides"]) * c["top_n"]
    assert out["bbox"].shape == (0, R, 4) and out["score"].shape == (0, R, 81) and out["stage"].shape == (0, R, 6)


@pytest.mark.gpu
def test_hip_repeats_and_replays_with_equal_bits(ops):
    import torch
    for name in ("branches", "multi_wg"):
        c = _cases()[name]
        ins = _inputs(c)
        N, R = c["im_info"].shape[0], len(c["strides"]) * c["top_n"]
        first = {k: v.clone() for k, v in _run(ops, c, ins).items()}
        second = _run(ops, c, ins)
        for k in first:
            assert torch.equal(_bits(first[k]), _bits(second[k])), (name, k)
        C = c["cls"][0].shape[1]
        hws = [x.shape[2] * x.shape[3] for x in c["cls"]]
        bufs = dict(bbox=torch.empty(N, R, 4, device="cuda"), score=torch.empty(N, R, 81, device="cuda"),
                    cls_id=torch.empty(N, R, device="cuda"), stage=torch.empty(N, R, 6, device="cuda"),
                    workspace=torch.empty(ops.fcos_decode_workspace_bytes(N, C, hws, c["top_n"]), device="cuda",
                                          dtype=torch.uint8))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _run(ops, c, ins, **bufs)                             # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = _run(ops, c, ins, **bufs)
        for _ in range(2):
            for t in out.values():
                t.fill_(float("nan"))
            bufs["workspace"].fill_(0xFF)                         # the call clears its own counters
            graph.replay()
            torch.cuda.synchronize()
            for k in first:
                assert torch.equal(_bits(first[k]), _bits(out[k])), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("skew", [0, 4])
def test_hip_red_zones_and_pointers_off_their_16_byte_boundary(ops, skew):
    """every output and the workspace sit in one arena filled with a sentinel, 4 KB guards around each; with skew = 4
    every tensor pointer -- inputs included -- is 4 bytes past a 16-byte boundary (the workspace stays aligned, as
    the entry point demands).  The results equal the fixture and no guard byte changes."""
    import torch
    for name in ("branches", "small_level"):
        c, want = _cases()[name], _want(name)
        N, R = c["im_info"].shape[0], len(c["strides"]) * c["top_n"]
        C = c["cls"][0].shape[1]
        hws = [x.shape[2] * x.shape[3] for x in c["cls"]]
        arena = torch.full((8 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
        spans, off = [], 0

        def carve(nbytes, dtype, shape, sk):
            nonlocal off
            start = (off + 4096 + 255) // 256 * 256 + sk
            off = start + nbytes
            spans.append((start, off))
            return arena[start:off].view(dtype).reshape(shape)

        E = lambda *shape: carve(4 * int(np.prod(shape)), torch.float32, shape, skew)
        wsb = ops.fcos_decode_workspace_bytes(N, C, hws, c["top_n"])
        bufs = dict(bbox=E(N, R, 4), score=E(N, R, 81), cls_id=E(N, R), stage=E(N, R, 6),
                    workspace=carve(wsb, torch.uint8, (wsb,), 0))
        got = _run(ops, c, _inputs(c, skew), **bufs)
        torch.cuda.synchronize()
        for k in KEYS:
            assert got[k].data_ptr() % 16 == skew and np.array_equal(got[k].cpu().numpy(), want[k]), (name, k)
        keep = torch.ones(arena.numel(), dtype=torch.bool, device="cuda")
        for s, e in spans:
            keep[s:e] = False
        assert bool((arena[keep] == 0xA5).all()), "a store outside the buffers the library was given"


def _logits_of(c, seed):
    """logits in the shapes of case c: level 0 spreads around the threshold (sigmoid(-2.94) = 0.05; top-k branch), every
    other level holds three planted candidates per image (nonzero branch)"""
    rs = np.random.RandomState(seed)
    cls = []
    for l, x in enumerate(c["cls"]):
        if l == 0:
            cls.append((rs.standard_normal(x.shape) * 1.5 - 3.0).astype(F32))
        else:
            v = (rs.standard_normal(x.shape) * 0.5 - 8.0).astype(F32)
            flat = v.reshape(x.shape[0], -1)
            flat[:, rs.permutation(flat.shape[1])[:3]] = F32(1.0)
            cls.append(v)
    return dict(c, cls=cls, ctr=[rs.standard_normal(x.shape).astype(F32) for x in c["ctr"]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["branches", "small_level", "multi_wg"])
def test_hip_fused_sigmoid_equals_sigmoid_then_decode(ops, name):
    import torch
    c = _logits_of(_cases()[name], 7)
    cls, ctr, off, info = _inputs(c)
    fused = _run(ops, c, (cls, ctr, off, info), logits=True)
    probs = ([ops.fcos_sigmoid(x) for x in cls], [ops.fcos_sigmoid(x) for x in ctr], off, info)
    plain = _run(ops, c, probs, logits=False)
    for k in KEYS:
        assert torch.equal(_bits(fused[k]), _bits(plain[k])), (name, k)
    # both branches were exercised
    counts = [[int((p[i] > c["thresh"]).sum()) for i in range(p.shape[0])] for p in probs[0]]
    assert all(n >= c["top_n"] for n in counts[0]) and all(0 < n < c["top_n"] for lv in counts[1:] for n in lv), counts


@pytest.mark.gpu
def test_hip_sigmoid_margin(ops):
    x = fr.logits(np.random.RandomState(5), (4099, 16))
    k_ref = fr.k_sigmoid(dr.sigmoid32(x), x)
    assert 0 < k_ref <= 3.0
    k_gpu = 0.0
    for skew in (0, 4):
        for a in (x, x.reshape(-1)[:4097], x.reshape(-1)[:3]):
            got = ops.fcos_sigmoid(_dev(a, skew)).cpu().numpy()
            assert got.shape == a.shape
            np.testing.assert_array_equal(got[(np.abs(a) >= 30) & (a > 0)], 1.0)
            np.testing.assert_array_equal(got[a <= -100], 0.0)
            assert np.all(got[a == 0] == 0.5)
            k_gpu = max(k_gpu, fr.k_sigmoid(got, a))
    print("fcos sigmoid: k_ref %.3f  k_gpu %.3f  bound %.3f" % (k_ref, k_gpu, 2 * k_ref + 2))
    assert k_gpu <= 2 * k_ref + 2
