"""The merged-BN affine behind the reference's names: `_contrib_BroadcastScale`, the fused node
`sd_scale_bias_act`, and a drop-in for `utils/graph_optimize.py:merge_bn` that emits it.

Every training and test run of the reference passes its graph through merge_bn (detection_train.py:154-155,
detection_test.py:129-130, mask_test.py:101-103).  With fixbn that turns each Convolution -> BatchNorm(
use_global_stats) pair into Convolution -> _contrib_BroadcastScale(gamma) -> broadcast_add(beta) [-> the shortcut's
add] -> relu: two to four element-wise nodes at full resolution.  This module

  1. registers two CustomOps, `sd__contrib_BroadcastScale` (the reference operator, broadcast_scale-inl.h:57-221)
     and `sd_scale_bias_act` (the whole chain in one node), and `install()` aliases `mx.sym.contrib.BroadcastScale`
     to the first;
  2. `plan_fusion(jgraph)` finds the chains in the dictionary `json.loads(sym.tojson())` gives;
  3. `merge_bn(symbol, args, auxs, symbol_only=False)` does what the reference's function does to the parameter
     dictionaries and rebuilds the symbol with the fused nodes of the plan; `patch_merge_bn()` rebinds
     `utils.graph_optimize.merge_bn` to it (the three scripts import the function at call time).

It stays out of mxnet_plugin's tables on purpose: it is no flag of `mxnet_plugin.install()`, has its own entry
points, and shares only what _mx_adapter.py holds (the pointer path, the alias path, the stream / sync state -- one
for both: the last install() call of either module sets it).  `import mxnet` happens inside the entry points.
"""
import ctypes
import importlib
import json
import logging

from ._mx_adapter import ADD_OPS, REQ, _PREFIX, _attrs, _bool, _call, _constructor, _is_f16, _mx, _no_add, _numel, \
    _ptr, _req, _require_write, _scratch, _state, _sync, _wait, _ws, drop_alias, prop_base, put_alias, register_ops

BROADCAST_SCALE = "_contrib_BroadcastScale"
SCALE_BIAS_ACT = "scale_bias_act"
_own = {"installed": False, "props": {}}


def _param_shape(given, data, name):
    """gamma / beta: (C,) or (1,C,1,...); an unknown shape becomes the broadcastable form merge_bn stores"""
    C = int(data[1])
    given = tuple(int(s) for s in given) if given else ()
    if not given or 0 in given:
        return (1, C) + (1,) * (len(data) - 2)
    if _numel(given) != C or (len(given) > 1 and given[1] != C):
        raise ValueError("%s should have shape (%d,) or (1,%d,1,...), got %s" % (name, C, C, given))
    return given


# ---------------------------------------------------------------------------------- operators ----
def _build_ops(mx):
    CustomOp, Prop = mx.operator.CustomOp, prop_base(mx)

    class ScaleBiasAct(CustomOp):
        """forward / backward of both nodes: BroadcastScale is the form without bias, residual and act"""

        def __init__(self, act, with_bias, with_residual, f16, what):
            super().__init__()
            self.act, self.with_bias, self.with_residual, self.what = int(act), with_bias, with_residual, what
            self.sfx = "_f16" if f16 else ""
            self.f16 = f16

        @staticmethod
        def _dims(shape):
            N, C = int(shape[0]), int(shape[1])
            return N, C, (_numel(shape) // (N * C) if N * C else 0)

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            if _req(req[0]) == REQ["null"]:
                return
            data, gamma = in_data[0], in_data[1]
            beta = in_data[2] if self.with_bias else None
            residual = in_data[2 + self.with_bias] if self.with_residual else None
            _wait(data, gamma, beta, residual)
            N, C, HxW = self._dims(data.shape)
            _call("sd_scale_bias_act_fwd" + self.sfx, _ptr(data), _ptr(gamma), _ptr(beta), _ptr(residual),
                  _ptr(out_data[0]), N, C, ctypes.c_long(HxW), self.act, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # BroadcastScaleOp::Backward checks req[kData] == kWriteTo (broadcast_scale-inl.h:95); so do the rest here
            names = ["data", "gamma"] + ["beta"] * self.with_bias + ["residual"] * self.with_residual
            _require_write(req, ["%s %s gradient" % (self.what, n) for n in names])
            dy = out_grad[0]
            gamma = in_data[1]
            y = out_data[0] if self.act else None
            _wait(dy, gamma, y)
            want = [_req(r) != REQ["null"] for r in req]
            want_x, want_g = want[0], want[1]
            want_b = self.with_bias and want[2]
            want_r = self.with_residual and want[2 + self.with_bias]
            # (in_data[0] is never touched: declare_backward_dependency does not name it)
            N, C, HxW = self._dims(dy.shape)
            if want_x or want_b or want_r:
                esz = 2 if self.f16 else 4
                dx = in_grad[0] if want_x else _scratch(dy, esz * _numel(dy.shape))
                dres = in_grad[2 + self.with_bias] if want_r else None
                dbeta = ws = wsp = None
                wsn = ctypes.c_size_t(0)
                if want_b:
                    ws, wsp, wsn = _ws(dy, "sd_scale_bias_act_workspace_bytes", N, C, ctypes.c_long(HxW))
                    # the sum is float32; a half graph gets it rounded once into its beta gradient
                    dbeta = _scratch(dy, 4 * C) if self.f16 else in_grad[2]
                _call("sd_scale_bias_act_bwd" + self.sfx, _ptr(dy), _ptr(y), _ptr(gamma), _ptr(dx), _ptr(dres),
                      _ptr(dbeta), N, C, ctypes.c_long(HxW), self.act, wsp, wsn, None)
                if want_b and self.f16:
                    _call("sd_cast_f32_to_f16", _ptr(dbeta), _ptr(in_grad[2]), ctypes.c_size_t(C), REQ["write"], None)
            _sync()
            if want_g:
                # the reference leaves the scaler's gradient buffer unwritten (broadcast_scale-inl.h:83-103 has no
                # store to it); zeros are what a buffer that was cleared once holds, and what fixed_param implies
                self.assign(in_grad[1], req[1], 0)

    class _Base(Prop):
        what = ""
        act, with_bias, with_residual = 0, False, False

        def __init__(self):
            super().__init__(need_top_grad=True)

        def infer_shape(self, in_shape):
            d = tuple(int(s) for s in in_shape[0])
            if len(d) < 2:
                raise ValueError("%s: data should be (batch, channel, ...), got %s" % (self.what, d))
            names = self.list_arguments()
            shapes = [d]
            for i, n in enumerate(names[1:], 1):
                given = in_shape[i] if i < len(in_shape) else ()
                if n == "residual":
                    if given and tuple(int(s) for s in given) != d and 0 not in tuple(given):
                        raise ValueError("%s: residual %s does not match data %s" % (self.what, tuple(given), d))
                    shapes.append(d)
                else:
                    shapes.append(_param_shape(given, d, "%s: %s" % (self.what, n)))
            return shapes, [d], []

        def infer_type(self, in_type):
            t = in_type[0]
            return [t] * len(self.list_arguments()), [t], []

        def create_operator(self, ctx, shapes, dtypes):
            return ScaleBiasAct(self.act, self.with_bias, self.with_residual, _is_f16(dtypes), self.what)

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            # the scaler and the output gradient (broadcast_scale-inl.h:185-190), and the output under relu
            # (ograd * relu_grad(out)) -- never in_data[0]: the convolution's output may be freed after the forward
            return [out_grad[0], in_data[1]] + ([out_data[0]] if self.act else [])

    class BroadcastScaleProp(_Base):
        what = "BroadcastScale"
        ARGS = ("data", "scaler")

    class ScaleBiasActProp(_Base):
        what = "scale_bias_act"

        def __init__(self, act="relu", with_bias="True", with_residual="False"):
            super().__init__()
            a = str(act).strip().lower()
            if a not in ("relu", "none", ""):
                raise ValueError("scale_bias_act: act must be 'relu' or 'none', got %r" % (act,))
            self.act = int(a == "relu")
            self.with_bias, self.with_residual = _bool(with_bias), _bool(with_residual)

        def list_arguments(self):
            return ["data", "gamma"] + ["beta"] * self.with_bias + ["residual"] * self.with_residual

    return {BROADCAST_SCALE: BroadcastScaleProp, SCALE_BIAS_ACT: ScaleBiasActProp}


# ------------------------------------------------------------------------------- registration ----
def register(mx=None):
    """Register `sd__contrib_BroadcastScale` and `sd_scale_bias_act`.  Returns {name: PropClass}."""
    mx = _mx(mx)
    return register_ops(mx, _build_ops(mx), _own)


def _broadcast_scale_ctor(mx, original):
    def BroadcastScale(*args, **kwargs):
        kwargs = {k: v for k, v in kwargs.items() if v is not None}
        name = kwargs.pop("name", None)
        inputs = dict(zip(("data", "scaler"), args))
        for k in ("data", "scaler"):
            if k in kwargs:
                if k in inputs:
                    raise TypeError("BroadcastScale: input '%s' given positionally and by keyword" % k)
                inputs[k] = kwargs.pop(k)
        if len(args) > 2 or kwargs:
            raise TypeError("BroadcastScale takes data and scaler (got %d positional, keywords %s)"
                            % (len(args), sorted(kwargs)))
        return mx.sym.Custom(op_type=_PREFIX + BROADCAST_SCALE, name=name, **inputs)
    BroadcastScale._sd_alias = True
    BroadcastScale._sd_original = original
    return BroadcastScale


def install(mx=None, stream=None, sync=True):
    """register() + alias `BroadcastScale` in every contrib namespace the plugin knows to the device op.  The
    native constructor is kept as `<namespace>._sd_reference_BroadcastScale`; uninstall() puts it back.
    `stream` / `sync` are the plugin's (mxnet_plugin.install has the ordering contract)."""
    mx = _mx(mx)
    props = register(mx)
    _state["stream"], _state["sync"] = stream, bool(sync)
    put_alias(mx, "contrib", "BroadcastScale", lambda original: _broadcast_scale_ctor(mx, original))
    _own["installed"] = True
    return props


def uninstall(mx=None):
    """Put the native `BroadcastScale` constructors back.  (MXNet has no way to drop a registered CustomOp: the two
    op types stay known, and nothing builds them any more.)"""
    drop_alias(_mx(mx), "contrib", "BroadcastScale")
    _own["installed"] = False


def scale_bias_act(data, gamma, beta=None, residual=None, act=None, name=None, mx=None):
    """The fused node as a symbol: act((data * gamma + beta) + residual)."""
    mx = _mx(mx)
    if not _own["props"]:
        raise RuntimeError("sd_scale_bias_act is not registered: call merged_bn.install() or register() first")
    inputs = dict(data=data, gamma=gamma)
    if beta is not None:
        inputs["beta"] = beta
    if residual is not None:
        inputs["residual"] = residual
    return mx.sym.Custom(op_type=_PREFIX + SCALE_BIAS_ACT, name=name, act="relu" if act in ("relu", True, 1) else "none",
                         with_bias=str(beta is not None), with_residual=str(residual is not None), **inputs)


# ------------------------------------------------------------------------------------ fusion ----
def _is_relu(node):
    return node["op"] == "relu" or (node["op"] == "Activation" and _attrs(node).get("act_type") == "relu")


def plan_fusion(jgraph):
    """Find every `_contrib_BroadcastScale -> broadcast_add [-> two-input add] [-> relu]` chain of a graph dictionary
    (MXNet's schema: nodes with op / name / attrs / inputs as [node, output, version], heads).  Pure: the dictionary
    is not changed.  Returns a list, in node order of `out`, of
        dict(out, scale, bias, add, relu, data, gamma, beta, residual, act, folded)
    out: the chain's last node, whose output the fused node replaces and whose name it takes; scale / bias / add /
    relu: the node ids of the links (add / relu None where absent); data / gamma / beta / residual: the input entries
    [node, output, version] (residual None where absent; it names another plan's `out` for a projection shortcut);
    act: whether a relu ends the chain; folded: the links in front of `out`, which no longer exist afterwards.
    A link is folded into the next only if its output has exactly one consumer and is no head of the graph, so
    whoever reads an inner node (get_internals() users, a second branch) keeps it; the add is `elemwise_add`, `_Plus`,
    `_plus`, or `add_n` / `ElementWiseSum` with two inputs, in either operand order; the relu is
    `Activation(act_type=relu)` or `relu`.  Where both operands of the add are such chains, the first absorbs the add
    and the second stays a fused node without activation and is the first's residual.  Nothing else moves."""
    nodes = jgraph["nodes"]
    consumers = {}
    for nid, node in enumerate(nodes):
        for e in node["inputs"]:
            consumers.setdefault(e[0], []).append(nid)
    heads = {e[0] for e in jgraph.get("heads", [])}

    def sole_consumer(nid):
        c = consumers.get(nid, [])
        return c[0] if len(c) == 1 and nid not in heads else None

    chains = {}       # bias node id -> plan
    for nid, node in enumerate(nodes):
        if node["op"] != "broadcast_add" or len(node["inputs"]) != 2:
            continue
        for k in (0, 1):
            s, b = node["inputs"][k], node["inputs"][1 - k]
            sn = nodes[s[0]]
            if (sn["op"] == BROADCAST_SCALE and len(sn["inputs"]) == 2 and sole_consumer(s[0]) == nid
                    and nodes[b[0]]["op"] == "null" and nodes[sn["inputs"][1][0]]["op"] == "null"):
                chains[nid] = dict(out=nid, scale=s[0], bias=nid, add=None, relu=None, data=list(sn["inputs"][0]),
                                   gamma=list(sn["inputs"][1]), beta=list(b), residual=None, act=False,
                                   folded=[s[0]])
                break
    tail = {nid: p for nid, p in chains.items()}     # current last node -> plan
    for nid, node in enumerate(nodes):
        if node["op"] not in ADD_OPS or len(node["inputs"]) != 2:
            continue
        cand = [k for k in (0, 1) if node["inputs"][k][0] in tail and tail[node["inputs"][k][0]]["add"] is None
                and tail[node["inputs"][k][0]]["relu"] is None and sole_consumer(node["inputs"][k][0]) == nid]
        if not cand:
            continue
        k = cand[0]
        p = tail.pop(node["inputs"][k][0])
        p["folded"].append(p["out"])
        p.update(out=nid, add=nid, residual=list(node["inputs"][1 - k]))
        tail[nid] = p
    for nid, node in enumerate(nodes):
        if not _is_relu(node) or len(node["inputs"]) != 1:
            continue
        src = node["inputs"][0][0]
        if src in tail and tail[src]["relu"] is None and sole_consumer(src) == nid:
            p = tail.pop(src)
            p["folded"].append(p["out"])
            p.update(out=nid, relu=nid, act=True)
            tail[nid] = p
    return sorted(chains.values(), key=lambda p: p["out"])


def _merged_bn_nodes(jgraph):
    """ids of the BatchNorm nodes merge_bn turns into the affine: use_global_stats behind a Convolution"""
    nodes = jgraph["nodes"]
    out = []
    for nid, node in enumerate(nodes):
        if node["op"] == "BatchNorm" and _bool(_attrs(node).get("use_global_stats", "False")):
            e = node["inputs"][0]
            if nodes[e[0]]["op"] == "Convolution" and e[1] == 0:
                out.append(nid)
    return out


def _expand_bn(jgraph, merged, shape_of):
    """The graph with every BatchNorm of `merged` written as the reference writes it: fresh variables <name>_gamma /
    <name>_beta, _contrib_BroadcastScale(data, gamma) named <name>_scale and broadcast_add(., beta) carrying the
    BatchNorm's own name, so that whatever read <name>_output still finds it.  Node ids are renumbered."""
    merged = set(merged)
    new_nodes, new_id, fresh = [], {}, {}

    def entry(e):
        return [new_id[e[0]], e[1], e[2] if len(e) > 2 else 0]

    def var(name):
        if name not in fresh:
            attrs = {}
            shape = shape_of(name)
            if shape is not None:
                attrs["__shape__"] = str(tuple(int(s) for s in shape))
            new_nodes.append(dict(op="null", name=name, inputs=[], **({"attrs": attrs} if attrs else {})))
            fresh[name] = len(new_nodes) - 1
        return [fresh[name], 0, 0]

    for nid, node in enumerate(jgraph["nodes"]):
        if nid in merged:
            name = node["name"]
            g, b = var(name + "_gamma"), var(name + "_beta")
            new_nodes.append(dict(op=BROADCAST_SCALE, name=name + "_scale", inputs=[entry(node["inputs"][0]), g]))
            new_nodes.append(dict(op="broadcast_add", name=name, inputs=[[len(new_nodes) - 1, 0, 0], b]))
        else:
            n = dict(node)
            n["inputs"] = [entry(e) for e in node["inputs"]]
            new_nodes.append(n)
        new_id[nid] = len(new_nodes) - 1
    out = {k: v for k, v in jgraph.items() if k not in ("nodes", "heads", "arg_nodes", "node_row_ptr")}
    out["nodes"] = new_nodes
    out["heads"] = [entry(e) for e in jgraph.get("heads", [])]
    out["arg_nodes"] = [i for i, n in enumerate(new_nodes) if n["op"] == "null"]
    return out


def _build_symbol(mx, jgraph, plans):
    """symbols from a graph dictionary, node by node in its order, the plans' chains as one fused node each"""
    by_out = {p["out"]: p for p in plans}
    gone = {n for p in plans for n in p["folded"]}
    built = {}

    def get(e):
        return built[e[0]][e[1]]

    for nid, node in enumerate(jgraph["nodes"]):
        if nid in gone:
            continue
        attrs, name, op = dict(_attrs(node)), node["name"], node["op"]
        if nid in by_out:
            p = by_out[nid]
            built[nid] = scale_bias_act(get(p["data"]), get(p["gamma"]), get(p["beta"]),
                                        None if p["residual"] is None else get(p["residual"]),
                                        "relu" if p["act"] else None, name=name, mx=mx)
        elif op == "null":
            built[nid] = mx.sym.var(name, **{k: v for k, v in attrs.items() if k.startswith("__")})
        else:
            built[nid] = _constructor(mx, op)(*[get(e) for e in node["inputs"]], **attrs, name=name)
    outs = [get(e) for e in jgraph["heads"]]
    return outs[0] if len(outs) == 1 else mx.sym.Group(outs)


def merge_bn(symbol, args, auxs, symbol_only=False):
    """Drop-in for utils/graph_optimize.py:merge_bn (same signature, same return value (symbol, args, auxs)).
    For every BatchNorm(use_global_stats=True) whose data comes from a Convolution, the statistics are folded into
    the affine parameters in place, in the dictionaries the caller passed:
        beta -= gamma * mean / sqrt(eps + var);   gamma /= sqrt(eps + var)
    the four arrays become (1, C, 1, 1), the moving mean and variance are reset to 0 and 1 (a shared BatchNorm is
    then folded once, however many nodes use it), and args[<node>_gamma] / args[<node>_beta] name the folded
    arrays per node.  symbol_only=True, or a node whose moving mean is not in auxs, leaves the dictionaries alone.
    The symbol is rebuilt with the fused `sd_scale_bias_act` nodes of plan_fusion() in place of the reference's
    BroadcastScale / broadcast_add / add / relu chains; a chain that cannot be folded keeps its nodes (BroadcastScale
    is then the aliased device operator).  Needs install()."""
    assert symbol is not None
    if not _own["installed"]:
        raise RuntimeError("merged_bn.merge_bn needs merged_bn.install(): the fused node is not registered")
    mx = _mx()
    jgraph = json.loads(symbol.tojson())
    nodes = jgraph["nodes"]
    merged = _merged_bn_nodes(jgraph)
    for nid in merged:
        node = nodes[nid]
        name = node["name"]
        g_name, b_name, m_name, v_name = [nodes[e[0]]["name"] for e in node["inputs"][1:5]]
        for part, got in (("gamma", g_name), ("beta", b_name), ("moving_mean", m_name), ("moving_var", v_name)):
            assert part in got, "%s: input %r is not its %s" % (name, got, part)
        if symbol_only:
            continue
        if m_name not in auxs:
            logging.info("Can not find %s, merge the symbol only", m_name)
            continue
        logging.info("Merging %s", name)
        eps = float(_attrs(node)["eps"])
        # beta first: it needs the gamma of before
        args[b_name] -= args[g_name] * auxs[m_name] / mx.nd.sqrt(eps + auxs[v_name])
        args[g_name] /= mx.nd.sqrt(eps + auxs[v_name])
        if args[g_name].ndim == 1:
            for d, k in ((args, g_name), (args, b_name), (auxs, m_name), (auxs, v_name)):
                d[k] = d[k].expand_dims(axis=0).expand_dims(axis=-1).expand_dims(axis=-1)
        auxs[m_name][:] = mx.nd.zeros_like(auxs[m_name])
        auxs[v_name][:] = mx.nd.ones_like(auxs[v_name])
        args[name + "_gamma"] = args[g_name]
        args[name + "_beta"] = args[b_name]

    def shape_of(var_name):
        return args[var_name].shape if args is not None and var_name in args else None
    expanded = _expand_bn(jgraph, merged, shape_of)
    return _build_symbol(mx, expanded, plan_fusion(expanded)), args, auxs


def patch_merge_bn(module=None):
    """Rebind `utils.graph_optimize.merge_bn` (or `module.merge_bn`) to this module's; the original is kept on the
    module as `_sd_reference_merge_bn` (a second call keeps the first).  Returns the module."""
    module = importlib.import_module("utils.graph_optimize") if module is None else module
    if not hasattr(module, "_sd_reference_merge_bn"):
        module._sd_reference_merge_bn = module.merge_bn
    module.merge_bn = merge_bn
    return module


def unpatch_merge_bn(module=None):
    """Put the reference's merge_bn back."""
    module = importlib.import_module("utils.graph_optimize") if module is None else module
    if hasattr(module, "_sd_reference_merge_bn"):
        module.merge_bn = module._sd_reference_merge_bn
        del module._sd_reference_merge_bn
    return module
