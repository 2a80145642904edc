"""The FreeAnchor training head on the device against tests/free_anchor_ref.py.

  bags                      equal to the float32 restatement's in the rows of valid gts (the case builder asserts that
                            the inputs make this a fair demand), -1 elsewhere
  both losses, all gradients  k_gpu <= 2 k_ref + 2 against the float64 truth, k = |got - truth| / (eps32 * T + tiny),
                            k_ref the float32 restatement's own k on the same case; both are printed.  The +-30 logits
                            of the kinks cases are held element by element (free_anchor_ref.k_all says why)
  equal bits                a second call with unaligned anchors, and a graph replay on changed inputs
  adapter                   install / patch_builders / unpatch_builders on the stubs, the CustomOp against the torch path
"""
import ctypes
import functools
import importlib
import os
import sys

import numpy as np
import pytest

from . import free_anchor_ref as fr
from . import mx_stub
from . import ref_stubs as RS

CASES = ("small", "prune", "ties", "shared", "row0", "kinks2.0", "kinks1.5", "lds128")
REF = "/root/reference"


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    return fr.make_case(name, seed)


def _kw(c):
    return {k: c[k] for k in ("top_n", "bbox_thr", "alpha", "gamma", "mean", "std")}


def _device(c):
    import torch
    lists = [[torch.from_numpy(t).cuda() for t in c[k]] for k in ("cls", "delta", "anchors")]
    return lists + [torch.from_numpy(c["gt"]).cuda(), torch.from_numpy(c["im_info"]).cuda()]


def _chain(fa, t, c, ws=None):
    """forward and backward through the functional calls: [loss, bags] + d_cls + d_delta"""
    loss, bags, ws = fa.free_anchor_loss_forward(*t, workspace=ws, **_kw(c))
    d_cls, d_delta = fa.free_anchor_loss_backward(*t, ws, grad_scale=c["grad_scale"], **_kw(c))
    return [loss, bags] + d_cls + d_delta


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_free_anchor_against_the_truth(ops, name):
    import torch
    from simpledet_amd import free_anchor as fa
    c = case(name)
    truth, ref = c["truth"], c["ref"]
    cls, delta, anchors, gt, im_info = _device(c)
    for t in cls + delta:
        t.requires_grad_()
    pos, neg = fa.free_anchor_loss(cls, delta, anchors, gt, im_info, grad_scale=c["grad_scale"], **_kw(c))
    (pos + neg).backward()
    bags = fa.free_anchor_loss_forward([t.detach() for t in cls], [t.detach() for t in delta], anchors, gt, im_info,
                                       **_kw(c))[1].cpu().numpy()
    assert np.array_equal(bags[truth["valid"]], ref["bags"][truth["valid"]])
    assert np.all(bags[~truth["valid"]] == -1)
    got = dict(pos=pos.item(), neg=neg.item(), grads=[t.grad.cpu().numpy() for t in cls + delta])
    k_gpu, k_ref = fr.k_all(got, truth, c), fr.k_all(ref, truth, c)
    print("free_anchor %s: k_gpu loss %.3f grad %.3f, k_ref loss %.3f grad %.3f" % ((name,) + k_gpu[:2] + k_ref[:2]))
    assert k_gpu[0] <= 2 * k_ref[0] + 2 and k_gpu[1] <= 2 * k_ref[1] + 2
    assert np.all(k_gpu[2] <= 2 * k_ref[2] + 2)          # the saturated logits of the kinks cases, element by element
    if name == "row0":   # the image without a valid gt: nothing counts, no gradient
        assert all(not g[1].any() for g in got["grads"]) and any(g[0].any() for g in got["grads"])
    # a second call, the anchors 4 bytes off their 16-byte boundary (element loads): equal bits
    off = [torch.cat([a.new_zeros(1), a.flatten()])[1:].view(a.shape) for a in anchors]
    assert all(o.data_ptr() % 16 == 4 for o in off)
    again = _chain(fa, [[t.detach() for t in cls], [t.detach() for t in delta], off, gt, im_info], c)
    assert torch.equal(again[0], torch.stack([pos, neg]).detach()) and np.array_equal(again[1].cpu().numpy(), bags)
    for a, t in zip(again[2:], cls + delta):
        assert torch.equal(a.view(torch.int32), t.grad.view(torch.int32))


@pytest.mark.gpu
def test_hip_free_anchor_graph_replay_on_changed_inputs_gives_equal_bits(ops):
    import torch
    from simpledet_amd import free_anchor as fa
    cases = [case("small", 0), case("small", 1)]
    flat = lambda t: t[0] + t[1] + t[2] + t[3:]
    eager = [[e.clone() for e in _chain(fa, _device(c), c)] for c in cases]
    static = _device(cases[0])
    ws = torch.empty(fa.workspace_bytes(2, [96, 24], 9, 3, 4, 5), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap = _chain(fa, static, cases[0], ws)
    for i in (1, 0, 1):
        for t, src in zip(flat(static), flat(_device(cases[i]))):
            t.copy_(src)
        for o in cap:
            o.fill_(-1)
        ws.fill_(0xFF)                                   # nothing is expected of the workspace: no memset
        graph.replay()
        torch.cuda.synchronize()
        for e, o in zip(eager[i], cap):
            assert torch.equal(e.view(torch.int32), o.view(torch.int32))


def test_entry_points_reject_bad_arguments_before_the_device():
    from simpledet_amd._lib import lib
    cd = lib().cdll
    tab, p, f4 = (ctypes.c_void_p * 2)(256, 256), ctypes.c_void_p(256), (ctypes.c_float * 4)(1, 1, 1, 1)
    hw, w = (ctypes.c_long * 2)(96, 24), (ctypes.c_long * 2)(12, 6)

    def fwd(L=2, N=1, A=9, K=3, M=4, top_n=5, cls=tab, pitch=w, std=f4, ws=p, wsb=1 << 30):
        return cd.sd_free_anchor_loss_fwd(cls, tab, tab, pitch, p, p, N, L, hw, w, A, K, M, top_n, 0.6, 0.5, 2.0, f4,
                                          std, p, None, ws, ctypes.c_size_t(wsb), None)
    assert fwd(L=0) == -1 and fwd(L=9) == -1 and fwd(A=0) == -1 and fwd(K=0) == -1 and fwd(N=-1) == -1
    assert fwd(top_n=0) == -1 and fwd(A=1, top_n=121) == -1                 # more than the 120 anchors
    assert fwd(cls=None) == -1 and fwd(cls=(ctypes.c_void_p * 2)(256, None)) == -1
    assert fwd(pitch=(ctypes.c_long * 2)(11, 6)) == -1 and fwd(std=(ctypes.c_float * 4)(1, 0, 1, 1)) == -1
    assert fwd(M=257) == -2 and fwd(top_n=513) == -2
    assert fwd(ws=None) == -4 and fwd(wsb=1024) == -4
    assert b"workspace" in cd.sd_last_error()
    assert fwd(N=0) == 0                                                 # an empty problem: no launch
    need = cd.sd_free_anchor_workspace_bytes(2, 2, hw, 9, 3, 4, 5)
    assert need >= 2 * 1080 * 8 + 2 * 4 * 5 * 24 and cd.sd_free_anchor_workspace_bytes(0, 2, hw, 9, 3, 4, 5) == 256
    assert cd.sd_free_anchor_loss_bwd(tab, tab, tab, w, p, p, 1, 2, hw, w, 9, 3, 4, 5, 0.6, 0.5, 2.0, f4, f4, p,
                                      ctypes.c_size_t(1 << 30), 1.0, None, tab, None) == -1


@pytest.fixture()
def plug():
    from simpledet_amd import free_anchor, mxnet_plugin
    saved = dict(mxnet_plugin._state)
    yield free_anchor, mxnet_plugin
    free_anchor._own.update(installed=False, props={})
    mxnet_plugin._state.clear()
    mxnet_plugin._state.update(saved)
    mxnet_plugin._state.update(registered=False)


def test_install_registers_one_op_and_patching_needs_it(plug):
    fa, _ = plug
    with pytest.raises(RuntimeError):
        fa.patch_builders()
    mx = mx_stub.make_stub()
    props = fa.install(mx)
    assert list(props) == ["free_anchor_loss"] and "sd_free_anchor_loss" in mx.registry
    P = props["free_anchor_loss"](num_level="2", top_n="5", std="(0.1, 0.1, 0.2, 0.2)", grad_scale="128.0")
    assert P.need_top_grad_ is False and P.list_outputs() == ["positive_loss", "negative_loss"]
    assert P.list_arguments() == ["cls_logit0", "cls_logit1", "bbox_delta0", "bbox_delta1", "anchor0", "anchor1",
                                  "gt_bbox", "im_info"]
    shapes = [(2, 27, 8, 12), (2, 27, 4, 6), (2, 36, 8, 12), (2, 36, 4, 6), (1, 1, 13, 13, 36), (1, 1, 8, 8, 36)]
    assert P.infer_shape(shapes + [(2, 4, 5), ()])[:2] == (shapes + [(2, 4, 5), (2, 3)], [(1,), (1,)])
    with pytest.raises(ValueError):
        P.infer_shape(shapes[:4] + [(1, 1, 13, 11, 36), (1, 1, 8, 8, 36), (2, 4, 5), ()])    # anchors narrower than W
    with pytest.raises(ValueError):
        props["free_anchor_loss"](std="(1, 0, 1, 1)")


@pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")
def test_patched_get_loss_emits_one_node_under_the_reference_output_names(plug):
    fa, _ = plug
    with RS.reference_modules() as R:
        fa.install(R.mx)
        FB = importlib.import_module("models.FreeAnchor.builder")
        reference = FB.FreeAnchorRetinaNetHead.get_loss

        def heads():
            for mod in [m for m in sys.modules if m.startswith("config.")]:
                del sys.modules[mod]
            cfg = importlib.import_module("config.FreeAnchor.free_anchor_r50v1_fpn_1x")
            sym = next(s for s in (getattr(o, "train_symbol", None) for o in cfg.get_config(True))
                       if isinstance(s, RS.Symbol))
            return sym, [RS.source(h) for h in (sym.inputs if sym.op_type == "Group" else list(sym))]
        native = heads()[1]
        assert fa.patch_builders() is True and fa.patch_builders() is True
        assert FB.FreeAnchorRetinaNetHead._sd_reference_get_loss is reference
        sym, patched = heads()
        # the heads keep the reference's names (-> positive_loss_output, negative_loss_output) and type
        assert [(h.name, h.op_type) for h in patched] == [(h.name, h.op_type) for h in native]
        assert [h.name for h in patched] == ["positive_loss", "negative_loss"]
        nodes = [n for n in RS.walk(sym, {}).values() if n.op_type == "sd_free_anchor_loss"]
        assert len(nodes) == 1 and nodes[0].nout == 2
        assert [RS.source(h.inputs[0]) for h in patched] == nodes * 2 and [h.inputs[0].index for h in patched] == [0, 1]
        assert nodes[0].params == dict(num_level="5", top_n="50", bbox_thr="0.6", alpha="0.5", gamma="2.0",
                                       mean="(0.0, 0.0, 0.0, 0.0)", std="(0.1, 0.1, 0.2, 0.2)", grad_scale="1.0")
        assert [i.name for i in nodes[0].inputs[10:]] == ["anchor_stride%d" % s for s in (8, 16, 32, 64, 128)] + \
            ["gt_bbox", "im_info"]
        kinds = [n.op_type for n in RS.walk(sym, {}).values()]
        assert "concat" not in kinds and "topk" not in kinds and "one_hot" not in kinds
        assert fa.unpatch_builders() is True and FB.FreeAnchorRetinaNetHead.get_loss is reference
        assert "_sd_reference_get_loss" not in FB.FreeAnchorRetinaNetHead.__dict__ and fa.unpatch_builders() is False


@pytest.mark.gpu
def test_adapter_round_trip_equals_the_torch_path(plug):
    import torch
    fa, _ = plug
    c = case("small")
    props = fa.install(mx_stub.make_stub())
    t = _device(c)
    want = _chain(fa, t, c)
    ins = t[0] + t[1] + t[2] + t[3:]
    P = props["free_anchor_loss"](num_level="2", grad_scale=repr(c["grad_scale"]),
                                  **{k: str(v) for k, v in _kw(c).items()})
    ishape, oshape, _ = P.infer_shape([tuple(x.shape) for x in ins])
    op = P.create_operator(None, ishape, None)
    out = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in oshape]
    nd = [mx_stub.wrap(x) for x in ins]
    op.forward(True, ["write"] * 2, nd, out, [])
    assert torch.equal(torch.cat([o.t for o in out]).view(torch.int32), want[0].view(torch.int32))
    grads = [mx_stub.wrap(torch.full(tuple(x.shape), 7.0, device="cuda")) for x in ins]
    op.backward(["write"] * len(ins), [], nd, out, grads, [])
    for g, x in zip(grads[:4], want[2:]):
        assert torch.equal(g.t.view(torch.int32), x.view(torch.int32))
    assert all(not g.t.any() for g in grads[4:]) and any(bool(x.any()) for x in want[2:])
    with pytest.raises(RuntimeError):
        op.backward(["add"] + ["write"] * (len(ins) - 1), [], nd, out, grads, [])
    with pytest.raises(RuntimeError):
        op.forward(True, ["add", "write"], nd, out, [])
