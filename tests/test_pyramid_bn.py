"""Pyramid batch norm (simpledet_amd/csrc/pyramid_bn.hip, simpledet_amd/pyramid_bn.py) against the reference's graph
as tests/pyramid_bn_ref.py composes it from tests/sync_bn_ref.py: concat, SyncBatchNorm, split, ReLU.

  CPU: every entry point rejects bad arguments before any launch; the CustomOp's lists, shapes and kAddTo refusal.
  GPU, over dtype {f32, f16} x relu {0, 1} and the cases A, B, C1, C8, D of pyramid_bn_ref.SHAPES:
       1. mean, var, bpart against the float64 truth under test_sync_bn.py's bound k_gpu <= 2 * k_ref + 2, k_ref what
          fwd_ref32 / bwd_ref32 reach on the concatenated tensor; the constant channel exactly;
       2. y_l, dx_l, dgamma, dbeta and the moving statistics bit for bit against *_contract32 fed with the device's
          own partials and then masked; W = 2 on two rank slices of the N = 4 variant of A;
       3. the fp16 mask: in A's channel of gamma = 1e-7 between 10 % and 90 % of the stored y are 0 (62 % with this
          seed), and dx is 0 exactly there;
       4. every level pointer one element off its 16-byte boundary gives the same bits; the _f16 entry points give
          the bits of cast -> fp32 entry point -> cast.  Under relu the mask is taken on the STORED type, so the two
          part where a positive z underflows in fp16: that comparison runs with fix_gamma on under relu, which
          takes A's tiny gamma out; every other comparison has it off;
       5. the autograd wrapper against torch.nn.functional.batch_norm + relu on the concatenated tensor in float64,
          under the bound of test_sync_bn.py's wrapper test.
  B's level of 16800 is 3 x 2100 = 6300 items per channel: 7 chunks of 1024.
"""
import ctypes
import functools

import numpy as np
import pytest

from simpledet_amd import _lib

from . import mx_stub, pyramid_bn_ref as pr, sync_bn_ref as sr

F = np.float32
CASES = ("A", "B", "C1", "C8", "D")
ENTRIES = ("stats", "apply", "infer_fwd", "bwd_stats", "bwd_apply")


# ------------------------------------------------------------------------------------------ CPU --
def _entry(entry, f16, N=2, C=8, hxw=(16, 5), L=None, ptr=256, table=True, skip=None, wsb=None, ws=256, W=1, rank=0):
    """calls an entry point with pointers that are never dereferenced: every case returns before any launch"""
    L = len(hxw) if L is None else L
    tab = lambda: (ctypes.c_void_p * max(len(hxw), 1))(*[ptr] * len(hxw)) if table else None    # noqa: E731
    H = (ctypes.c_long * max(len(hxw), 1))(*hxw)
    cdll = _lib.lib().cdll
    need = int(cdll.sd_pyramid_bn_workspace_bytes(N, C, H, L))
    tail_ws = [ctypes.c_void_p(ws) if ws else None, ctypes.c_size_t(need if wsb is None else wsb), None]
    v = [ctypes.c_void_p(ptr) if ptr else None] * 9
    geo, flt = [N, C, H, L], [ctypes.c_float(1e-3), 1, 1]
    args = {"stats": [tab(), v[0]] + geo + tail_ws,
            "apply": [tab(), v[0], W, v[1], v[2], tab(), v[3], v[4]] + geo + flt + tail_ws,
            "infer_fwd": [tab(), v[0], v[1], v[2], v[3], tab()] + geo + flt + [None],
            "bwd_stats": [tab(), tab(), v[0], v[1], v[2], v[3], v[4]] + geo + flt + tail_ws,
            "bwd_apply": [tab(), tab(), v[0], v[1], v[2], v[3], v[4], W, rank, tab(), v[5], v[6], v[7], v[8],
                          ctypes.c_float(0.9)] + geo + flt + tail_ws}[entry]
    if skip is not None:
        args[skip] = None
    return _lib.lib().call("sd_pyramid_bn_" + entry + ("_f16" if f16 else ""), *args)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_points_reject_bad_arguments_without_a_gpu(entry, f16):
    E = _lib.SimpleDetOpsError
    call = functools.partial(_entry, entry, f16)
    for kw in (dict(N=-1), dict(C=-8), dict(hxw=(16, -1)), dict(L=-1)):
        with pytest.raises(E, match="negative dimension") as e:
            call(**kw)
        assert e.value.code == -1
    npointers = {"stats": 2, "apply": 8, "infer_fwd": 6, "bwd_stats": 7, "bwd_apply": 10}[entry]
    for i in range(npointers):                   # the leading arguments: tables and vectors (W and rank excepted)
        if entry in ("apply", "bwd_apply") and i in {"apply": (2,), "bwd_apply": (7, 8)}[entry]:
            continue
        with pytest.raises(E, match="null pointer") as e:
            call(skip=i)
        assert e.value.code == -1
    with pytest.raises(E, match="null pointer"):     # an entry of a table
        call(ptr=0)
    with pytest.raises(E, match="not aligned") as e:
        call(ptr=257)
    assert e.value.code == -1
    with pytest.raises(E, match="at most 8") as e:
        call(hxw=(4,) * 9)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(E, match="exceed the limit") as e:      # 2 x 1024 x (2^19 + 2^19) = 2^31
        call(N=2, C=1024, hxw=(1 << 19, 1 << 19), wsb=1 << 30)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    if entry != "infer_fwd":
        need = int(_lib.lib().cdll.sd_pyramid_bn_workspace_bytes(2, 8, (ctypes.c_long * 2)(16, 5), 2))
        with pytest.raises(E, match="workspace too small") as e:
            call(wsb=need - 1)
        assert e.value.code == -4
        with pytest.raises(E, match="workspace too small"):
            call(ws=0)
    # L = 0 or an empty tensor: nothing is done, no pointer is looked at
    for kw in (dict(hxw=(), table=False), dict(N=0), dict(C=0), dict(hxw=(0, 0))):
        assert call(ptr=0, ws=0, wsb=0, **kw) == 0
    if entry == "bwd_apply":
        with pytest.raises(E, match="rank="):
            call(W=2, rank=2)


def test_custom_op_lists_shapes_and_kaddto():
    from simpledet_amd import mxnet_plugin, pyramid_bn
    mx = mx_stub.make_stub()
    P = pyramid_bn.install(mx)["pyramid_bn"]
    assert "sd_pyramid_bn" in mx.registry and "pyramid_bn" not in mxnet_plugin.FEATURE_FLAGS
    levels = [(4, 256, 100, 167), (4, 256, 50, 84), (4, 256, 25, 42), (4, 256, 13, 21), (4, 256, 7, 11)]
    for L in (1, 5):
        p = P(num_levels=str(L), act_type="relu")
        assert p.list_arguments() == ["data%d" % l for l in range(L)] + ["gamma", "beta"]
        assert p.list_outputs() == ["output%d" % l for l in range(L)] + ["mean", "var"]
        assert p.list_auxiliary_states() == ["moving_mean", "moving_var"] and p.num_visible_outputs == L
        c = (256,)
        assert p.infer_shape(levels[:L] + [(), ()]) == (levels[:L] + [c, c], levels[:L] + [c, c], [c, c])
        assert p.infer_type([np.float16] * (L + 2))[0] == [np.float16] * L + [np.float32] * 2
    with pytest.raises(ValueError, match="num_levels"):
        P(num_levels="9")
    with pytest.raises(ValueError, match="act_type"):
        P(act_type="sigmoid")
    with pytest.raises(ValueError, match="data1"):
        P(num_levels="2").infer_shape([(4, 256, 8, 8), (4, 128, 4, 4), (), ()])
    op = P(num_levels="2").create_operator(None, None, [None])
    with pytest.raises(RuntimeError, match="add"):
        op.forward(True, ["add"] * 4, [], [], [])
    with pytest.raises(RuntimeError, match="kWriteTo"):
        op.backward(["write", "add", "write", "write"], [], [], [], [], [])
    fms = [mx.sym.Variable("p%d" % l) for l in range(3)]
    outs = pyramid_bn.ibn(fms, "sepc0_ibn", ndev=8)
    node = outs[0][1]
    assert [o[2] for o in outs] == [0, 1, 2] and node.nout == 5 and node.params["act_type"] == "relu"
    assert [i.op_type for i in node.inputs[3:]] == ["var:sepc0_ibn_" + k for k in ("gamma", "beta", "moving_mean",
                                                                                   "moving_var")]


# ------------------------------------------------------------------------------------------ GPU --
def _cuda(a, half, offset=False):
    """a device copy; offset: the data pointer sits one element off a 16-byte boundary"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    t = t.half() if half else t
    if not offset:
        return t.cuda()
    buf = torch.empty(t.numel() + 17, dtype=t.dtype, device="cuda")
    start = 1 + (16 - buf.data_ptr() % 16) % 16 // t.element_size()
    o = buf[start:start + t.numel()].view(t.shape)
    o.copy_(t)
    assert o.data_ptr() % 16 == t.element_size()
    return o


def _np(t):
    return t.detach().float().cpu().numpy()


def _bits(got, want):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def _run(pb, c, half, relu, fix, offset=False, parts=None, bparts=None, rank=0, as_float=False):
    """the four phased calls -> dict of numpy arrays (levels concatenated); parts / bparts: the ranks' blocks, this
    rank's own computed here when None.  as_float: halves are cast to float32 first and the results back."""
    import torch
    f = lambda v: torch.from_numpy(v).cuda()                                                # noqa: E731
    g, b, mm, mv = f(c["gamma"]), f(c["beta"]), f(c["mm0"].copy()), f(c["mv0"].copy())
    xs = [_cuda(a, half and not as_float, offset) for a in c["xs"]]
    dys = [_cuda(a, half and not as_float, offset) for a in c["dys"]]
    kw = dict(eps=c["eps"], fix_gamma=fix, relu=relu)
    part = pb.stats(xs)
    ys, mean, var = pb.apply(xs, part[None] if parts is None else f(parts), g, b, **kw)
    bpart = pb.bwd_stats(dys, xs, mean, var, g, b, **kw)
    dxs, dgamma, dbeta = pb.bwd_apply(dys, xs, mean, var, g, b, bpart[None] if bparts is None else f(bparts), rank,
                                      moving_mean=mm, moving_var=mv, momentum=0.9, **kw)
    torch.cuda.synchronize()
    if as_float and half:
        ys, dxs = [t.half() for t in ys], [t.half() for t in dxs]
    return dict(part=_np(part), mean=_np(mean), var=_np(var), bpart=_np(bpart), y=pr.concat([_np(t) for t in ys]),
                dx=pr.concat([_np(t) for t in dxs]), dgamma=_np(dgamma), dbeta=_np(dbeta), mm=_np(mm), mv=_np(mv))


def _check_behind(c, d, parts, bparts, rank, fix, relu, half):
    """assertion 2 for one rank -> the stored y and dx of the reference"""
    m, v = sr.combine_contract(parts)
    assert _bits(d["mean"], m) and _bits(d["var"], v)
    y = pr.forward(c, m, v, fix, relu, half)
    assert _bits(d["y"], y), "y"
    want = pr.backward(c, y, m, v, bparts, rank, fix, relu, half)
    for o, k in (("dx", "dx"), ("dgamma", "dgamma"), ("dbeta", "dbeta"), ("mm", "moving_mean"), ("mv", "moving_var")):
        assert _bits(d[o], want[k]), o
    return y, want["dx"]


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("name", CASES)
def test_hip_statistics_margin_and_the_rest_bit_for_bit(name, half, relu):
    from simpledet_amd import pyramid_bn as pb
    c = pr.make_case(name, half)
    fix = name == "B"
    d = _run(pb, c, half, relu, fix)
    x, eps = pr.concat(c["xs"]), c["eps"]
    # 1. the statistics
    ft, fT = sr.fwd_truth(x, c["gamma"], c["beta"], eps, fix)
    f32 = sr.fwd_ref32(x, c["gamma"], c["beta"], eps, fix)
    assert _bits(d["part"][0], d["mean"]) and _bits(d["part"][1], d["var"])
    assert d["mean"][1] == 1.5 and d["var"][1] == 0.0
    # 2. behind them, from the device's own partials
    y, dx = _check_behind(c, d, d["part"][None], d["bpart"][None], 0, fix, relu, half)
    dy = pr.masked(pr.concat(c["dys"]), y, relu)
    bt, bT = sr.bwd_truth(dy, x, d["mean"], d["var"], c["gamma"], eps, fix)
    b32 = sr.bwd_ref32(dy, x, d["mean"], d["var"], c["gamma"], eps, fix)
    for o, got, truth, T, ref in (("mean", d["mean"], ft, fT, f32), ("var", d["var"], ft, fT, f32),
                                  ("bpart", d["bpart"][None], bt, bT, b32)):
        k, k_ref = sr.k_of(got, truth[o], T[o]), sr.k_of(ref[o], truth[o], T[o])
        print("pyramid_bn %s %s relu=%d %-5s k_gpu %.3f k_ref %.3f" % (name, "f16" if half else "f32", relu, o, k, k_ref))
        assert k <= 2 * k_ref + 2, (o, k, k_ref)
    # 3. the fp16 mask
    if name == "A" and half and relu:
        zero = y[:, pr.TINY] == 0
        assert 0.1 < zero.mean() < 0.9, zero.mean()
        assert np.all(d["dx"][:, pr.TINY][zero] == 0) and np.any(d["dx"][:, pr.TINY][~zero] != 0)


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_hip_two_rank_slices_combine(half, relu):
    from simpledet_amd import pyramid_bn as pb
    c = pr.make_case("A4", half)
    ranks = [dict(c, xs=[a[2 * r:2 * r + 2] for a in c["xs"]], dys=[a[2 * r:2 * r + 2] for a in c["dys"]], N=2,
                  n=c["n"] // 2) for r in range(2)]
    own = [_run(pb, rc, half, relu, False) for rc in ranks]
    parts = np.stack([o["part"] for o in own])
    mean, var = sr.combine_contract(parts)
    # the backward partials about the COMBINED mean: a second pass with the gathered parts
    mid = [_run(pb, rc, half, relu, False, parts=parts) for rc in ranks]
    bparts = np.stack([o["bpart"] for o in mid])
    for r, rc in enumerate(ranks):
        d = _run(pb, rc, half, relu, False, parts=parts, bparts=bparts, rank=r)
        assert _bits(d["bpart"], bparts[r])
        _check_behind(rc, d, parts, bparts, r, False, relu, half)


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("name", CASES)
def test_hip_bit_stability_offsets_and_f16_equals_cast(name, half, relu):
    from simpledet_amd import pyramid_bn as pb
    c = pr.make_case(name, half)
    base, off = _run(pb, c, half, relu, False), _run(pb, c, half, relu, False, offset=True)
    for o in base:
        assert _bits(base[o], off[o]), o
    if half:
        fix = bool(relu)
        h, f = _run(pb, c, True, relu, fix), _run(pb, c, True, relu, fix, as_float=True)
        for o in h:
            assert _bits(h[o], f[o]), o


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [0, 1])
def test_autograd_wrapper_against_torch_batch_norm_in_float64(relu):
    import torch
    from simpledet_amd import pyramid_bn as pb
    c = pr.make_case("A", False)
    f = lambda v: torch.from_numpy(v).cuda()                                                # noqa: E731
    xs = [f(a).requires_grad_() for a in c["xs"]]
    g, b = f(c["gamma"]).requires_grad_(), f(c["beta"]).requires_grad_()
    mm, mv = f(c["mm0"].copy()), f(c["mv0"].copy())
    ys = pb.pyramid_bn(xs, g, b, mm, mv, eps=1e-3, momentum=0.9, fix_gamma=False, relu=bool(relu))
    assert torch.equal(mm, f(c["mm0"]))                              # nothing moves in the forward
    grads = torch.autograd.grad(ys, xs + [g, b], [f(a) for a in c["dys"]])
    assert not torch.equal(mm, f(c["mm0"]))
    x64 = torch.cat([x.detach().flatten(2) for x in xs], 2).double().requires_grad_()
    g64, b64 = g.detach().double().requires_grad_(), b.detach().double().requires_grad_()
    y64 = torch.nn.functional.batch_norm(x64, None, None, g64, b64, training=True, eps=float(F(1e-3)))
    y64 = torch.relu(y64) if relu else y64
    dyc = f(pr.concat(c["dys"]))
    want = torch.autograd.grad(y64, (x64, g64, b64), dyc.double())
    x = pr.concat(c["xs"])
    ft, fT = sr.fwd_truth(x, c["gamma"], c["beta"], 1e-3, False)
    mean32, var32 = ft["mean"].astype(F), ft["var"].astype(F)
    dy = pr.masked(pr.concat(c["dys"]), _np(y64), relu)
    bt, bT = sr.bwd_truth(dy, x, mean32, var32, c["gamma"], 1e-3, False)
    ref = dict(sr.fwd_ref32(x, c["gamma"], c["beta"], 1e-3, False), **sr.bwd_ref32(dy, x, mean32, var32, c["gamma"],
                                                                                  1e-3, False))
    truth, T = dict(ft, **bt), dict(fT, **bT)
    truth["y"] = pr.relu(truth["y"], relu)
    got = dict(y=pr.concat([_np(t) for t in ys]), dx=pr.concat([_np(t) for t in grads[:-2]]), dgamma=_np(grads[-2]),
               dbeta=_np(grads[-1]))
    w64 = dict(y=y64, dx=want[0], dgamma=want[1], dbeta=want[2])
    for o in ("y", "dx", "dgamma", "dbeta"):
        k_ref = sr.k_of(pr.relu(ref[o], relu) if o == "y" else ref[o], truth[o], T[o])
        k = sr.k_of(got[o], w64[o].detach().cpu().numpy(), T[o])
        print("pyramid_bn autograd relu=%d %-6s k_gpu %.3f (k_ref %.3f)" % (relu, o, k, k_ref))
        assert k <= 2 * k_ref + 2, (o, k, k_ref)
