"""The FPN top-down pathway behind MXNet: the CustomOp `sd_fpn_topdown`, a planner that finds the chains in a graph
dictionary, and a wrapper of `utils.graph_optimize.merge_bn` that rewrites the symbol every script builds.

Every FPN-style neck of the reference merges a coarse level into the next finer one with
    UpSampling(scale=2, sample_type="nearest", num_args=1) -> slice_like(., lateral) -> add_n(., lateral)
(models/FPN/builder.py:444-524 three times in a row, models/retinanet/builder.py:498-543 twice, FCOS, RepPoints and
NASFPN's FPN variant alike).  The sums feed each other and nothing else lies between them, so the whole pathway is
one operator: inputs (top, lateral_1 .. lateral_{L-1}), outputs (out_1 .. out_{L-1}), one launch each way
(simpledet_amd/csrc/fpn_topdown.hip), and a backward that needs the output gradients only.  This module

  1. registers the CustomOp `sd_fpn_topdown(num_levels=L)` (`register()` / `install()`; there is no native operator
     to alias);
  2. `plan_topdown(jgraph)` finds the chains in the dictionary `json.loads(sym.tojson())` gives -- a pure function;
  3. `rewrite(symbol)` rebuilds a symbol with one fused node per chain;
  4. `patch_merge_bn()` wraps whatever `utils.graph_optimize.merge_bn` currently is -- the reference's own or
     `merged_bn.merge_bn` -- so that the symbol it returns is rewritten.  All three scripts pass their graph through
     that function (detection_train.py:154-155, detection_test.py:129-130, mask_test.py:101-103).
     APPLY IT LAST: `merged_bn.patch_merge_bn()` (and `merged_bn.unpatch_merge_bn()`) rebind the function and drop
     a wrapper installed before them.

Like merged_bn it stays out of mxnet_plugin's tables: no flag of `mxnet_plugin.install()`, its own entry points, and
only what _mx_adapter.py holds shared (the pointer path, the stream / sync state -- one state for all: the last
install() call of any of the modules sets it).  `import mxnet` happens inside the entry points.

Limits: scale 2 and nearest only, NCHW, kWriteTo only, and the sums' node names are not kept by
rewrite() (the fused node has L-1 outputs under one name, `<last sum>_topdown`).
"""
import importlib
import json

from ._mx_adapter import ADD_OPS, REQ, _PREFIX, _attrs, _call, _constructor, _iarr, _is_f16, _mx, _no_add, _ptr, _req, \
    _require_write, _scratch, _state, _sync, _table, _wait, prop_base, register_ops

FPN_TOPDOWN = "fpn_topdown"
MAX_LEVELS = 6
_own = {"installed": False, "props": {}}


def _check_levels(shapes, what="fpn_topdown"):
    """(N,C,H,W) per level, level 0 the coarsest, each level at most twice the one before"""
    shapes = [tuple(int(v) for v in s) for s in shapes]
    for l, s in enumerate(shapes):
        if len(s) != 4:
            raise ValueError("%s: level %d should be (N,C,H,W), got %s" % (what, l, s))
        if s[:2] != shapes[0][:2]:
            raise ValueError("%s: level %d has (N,C) = %s, the top %s" % (what, l, s[:2], shapes[0][:2]))
        if l and (s[2] > 2 * shapes[l - 1][2] or s[3] > 2 * shapes[l - 1][3]):
            raise ValueError("%s: level %d (%d x %d) is larger than twice level %d (%d x %d)"
                             % (what, l, s[2], s[3], l - 1, shapes[l - 1][2], shapes[l - 1][3]))
    return shapes


# ---------------------------------------------------------------------------------- operators ----
def _build_ops(mx):
    CustomOp, Prop = mx.operator.CustomOp, prop_base(mx)

    class FpnTopdown(CustomOp):
        def __init__(self, L, f16):
            super().__init__()
            self.L, self.f16 = L, f16
            self.sfx = "_f16" if f16 else ""

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            if all(_req(r) == REQ["null"] for r in req):
                return
            _wait(*in_data)
            shapes = _check_levels([a.shape for a in in_data])
            _call("sd_fpn_topdown_fwd" + self.sfx, _ptr(in_data[0]), _table(in_data[1:]), _table(out_data),
                  shapes[0][0], shapes[0][1], _iarr([s[2] for s in shapes]), _iarr([s[3] for s in shapes]), self.L, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # the kernels overwrite: kAddTo is refused loudly (as for scale_bias_act)
            names = ["top"] + ["lateral%d" % l for l in range(1, self.L)]
            _require_write(req, ["fpn_topdown %s gradient" % n for n in names])
            want = [_req(r) != REQ["null"] for r in req]
            if not any(want):
                return
            _wait(*out_grad)
            # (in_data is never touched: declare_backward_dependency names the output gradients only)
            shapes = _check_levels([g.shape for g in in_grad])
            esz = 2 if self.f16 else 4
            numel = shapes[0][0] * shapes[0][1] * shapes[0][2] * shapes[0][3]
            d_top = in_grad[0] if want[0] else _scratch(out_grad[0], esz * numel)
            d_lat = [in_grad[l] if want[l] else None for l in range(1, self.L)]
            _call("sd_fpn_topdown_bwd" + self.sfx, _table(out_grad), _ptr(d_top), _table(d_lat), shapes[0][0],
                  shapes[0][1], _iarr([s[2] for s in shapes]), _iarr([s[3] for s in shapes]), self.L, None)
            _sync()

    class FpnTopdownProp(Prop):
        def __init__(self, num_levels="4"):
            super().__init__(need_top_grad=True)
            self.L = int(num_levels)
            if not 2 <= self.L <= MAX_LEVELS:
                raise ValueError("fpn_topdown: num_levels must be 2..%d, got %r" % (MAX_LEVELS, num_levels))

        def list_arguments(self):
            return ["top"] + ["lateral%d" % l for l in range(1, self.L)]

        def list_outputs(self):
            return ["out%d" % l for l in range(1, self.L)]

        def infer_shape(self, in_shape):
            if len(in_shape) != self.L:
                raise ValueError("fpn_topdown: %d inputs for num_levels=%d" % (len(in_shape), self.L))
            shapes = _check_levels(in_shape)
            return shapes, shapes[1:], []

        def infer_type(self, in_type):
            import numpy as np
            t = next((x for x in in_type if x is not None), None)
            if t is not None and np.dtype(t) not in (np.dtype(np.float32), np.dtype(np.float16)):
                raise TypeError("fpn_topdown: float32 or float16, got %s" % np.dtype(t))
            return [t] * self.L, [t] * (self.L - 1), []

        def create_operator(self, ctx, shapes, dtypes):
            return FpnTopdown(self.L, _is_f16(dtypes))

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            # the output gradients alone: no input and no output of the forward is kept alive for the backward
            return list(out_grad)

    return {FPN_TOPDOWN: FpnTopdownProp}


# ------------------------------------------------------------------------------- registration ----
def register(mx=None):
    """Register `sd_fpn_topdown`.  Returns {name: PropClass}."""
    mx = _mx(mx)
    return register_ops(mx, _build_ops(mx), _own)


def install(mx=None, stream=None, sync=True):
    """register() + the plugin's `stream` / `sync` state (mxnet_plugin.install has the ordering contract).  There is
    no native constructor to alias: the node enters a graph through rewrite() or fpn_topdown()."""
    mx = _mx(mx)
    props = register(mx)
    _state["stream"], _state["sync"] = stream, bool(sync)
    _own["installed"] = True
    return props


def uninstall(mx=None):
    """(MXNet has no way to drop a registered CustomOp: the op type stays known, and rewrite() refuses to emit it.)"""
    _own["installed"] = False


def fpn_topdown(top, laterals, name=None, mx=None):
    """The fused node as a symbol; its outputs are out_1 .. out_{L-1}, coarse to fine."""
    mx = _mx(mx)
    if not _own["props"]:
        raise RuntimeError("sd_fpn_topdown is not registered: call fpn_topdown.install() or register() first")
    laterals = list(laterals)
    inputs = dict(top=top)
    for l, s in enumerate(laterals, 1):
        inputs["lateral%d" % l] = s
    return mx.sym.Custom(op_type=_PREFIX + FPN_TOPDOWN, name=name, num_levels=str(len(laterals) + 1), **inputs)


# ----------------------------------------------------------------------------------- planning ----
def _all_axes(attrs):
    return str(attrs.get("axes", "()")).replace(" ", "") in ("()", "None", "[]", "")


def _is_up2_nearest(node):
    a = _attrs(node)
    try:
        return (node["op"] == "UpSampling" and len(node["inputs"]) == 1 and a.get("sample_type") == "nearest"
                and int(a.get("scale", 0)) == 2 and int(a.get("num_args", 1)) == 1)
    except (TypeError, ValueError):
        return False


def plan_topdown(jgraph):
    """Find the top-down chains of a graph dictionary (MXNet's schema: nodes with op / name / attrs / inputs as
    [node, output, version], heads).  Pure: the dictionary is not changed.  A step is
        UpSampling(sample_type=nearest, scale=2, num_args=1) -> slice_like over all axes -> a two-input add
    (`add_n`, `ElementWiseSum`, `elemwise_add`, `_Plus`, `_plus`, either operand order) whose other operand is the
    slice_like's shape reference.  The UpSampling's and the slice_like's outputs must each have exactly one consumer
    and be no head of the graph (whoever reads them keeps them); the sum may have any consumers.  Steps join into
    one chain where a sum feeds the next step's UpSampling -- the first such step in node order where several do, and
    only while the next lateral does not itself depend on a sum of the chain (the fused node needs every lateral
    before it gives any output), up to 6 levels.  scale=4, bilinear, a slice_like with `axes`, a third addend: left.
    Returns a list, in node order of the first sum, of
        dict(L, top, laterals, sums, ups, clips, folded)
    top / laterals: input entries [node, output, version]; sums / ups / clips: node ids per step, coarse to fine;
    folded: every node that no longer exists afterwards (output l-1 of the fused node replaces sums[l-1])."""
    nodes = jgraph["nodes"]
    consumers = {}
    for nid, node in enumerate(nodes):
        for e in node["inputs"]:
            consumers.setdefault(e[0], []).append(nid)
    heads = {e[0] for e in jgraph.get("heads", [])}

    def sole_consumer(nid):
        c = consumers.get(nid, [])
        return c[0] if len(c) == 1 and nid not in heads else None

    steps = {}     # sum node id -> step
    for nid, node in enumerate(nodes):
        if node["op"] not in ADD_OPS or len(node["inputs"]) != 2:
            continue
        for k in (0, 1):
            s, o = node["inputs"][k], node["inputs"][1 - k]
            clip = nodes[s[0]]
            if not (clip["op"] == "slice_like" and len(clip["inputs"]) == 2 and s[1] == 0 and _all_axes(_attrs(clip))
                    and sole_consumer(s[0]) == nid and list(clip["inputs"][1][:2]) == list(o[:2])):
                continue
            u = clip["inputs"][0]
            if u[1] == 0 and _is_up2_nearest(nodes[u[0]]) and sole_consumer(u[0]) == s[0]:
                steps[nid] = dict(sum=nid, up=u[0], clip=s[0], coarse=list(nodes[u[0]]["inputs"][0]), lateral=list(o))
                break

    def depends_on(entry, targets):
        seen, stack = set(), [entry[0]]
        while stack:
            n = stack.pop()
            if n in targets:
                return True
            if n in seen:
                continue
            seen.add(n)
            stack.extend(e[0] for e in nodes[n]["inputs"])
        return False

    follower = {}  # sum id -> the step that continues its chain
    for nid in sorted(steps):
        c = steps[nid]["coarse"]
        if c[0] in steps and c[1] == 0 and c[0] not in follower:
            follower[c[0]] = nid
    continued = set(follower.values())
    plans, used = [], set()

    def grow(nid):
        chain = [steps[nid]]
        used.add(nid)
        while len(chain) < MAX_LEVELS - 1:
            nxt = follower.get(chain[-1]["sum"])
            if nxt is None or nxt in used or depends_on(steps[nxt]["lateral"], {s["sum"] for s in chain}):
                break
            chain.append(steps[nxt])
            used.add(nxt)
        ids = lambda k: [s[k] for s in chain]   # noqa: E731
        return dict(L=len(chain) + 1, top=chain[0]["coarse"], laterals=ids("lateral"), sums=ids("sum"), ups=ids("up"),
                    clips=ids("clip"), folded=sorted(ids("up") + ids("clip") + ids("sum")))
    for nid in sorted(steps):
        if nid not in continued:
            plans.append(grow(nid))
    # a step left behind by a chain that broke off (too long, or a lateral that depends on the chain) starts its own
    for nid in sorted(steps):
        if nid not in used:
            plans.append(grow(nid))
    return sorted(plans, key=lambda p: p["sums"][0])


# ------------------------------------------------------------------------------------ rewrite ----
def _build_symbol(mx, jgraph, plans):
    """symbols from a graph dictionary with the plans' chains as one fused node each.  The fused node needs all its
    laterals, so nodes are built on demand from the heads (an explicit stack: graphs are hundreds of nodes deep)."""
    nodes = jgraph["nodes"]
    by_sum = {}
    for pi, p in enumerate(plans):
        for l, s in enumerate(p["sums"]):
            by_sum[s] = (pi, l)
    built, fused = {}, {}

    def deps(key):
        if key[0] == "plan":
            p = plans[key[1]]
            return [p["top"]] + p["laterals"]
        return nodes[key[1]]["inputs"]

    def key_of(e):
        return ("plan", by_sum[e[0]][0]) if e[0] in by_sum else ("node", e[0])

    def get(e):
        if e[0] in by_sum:
            pi, l = by_sum[e[0]]
            return fused[pi][l]
        return built[e[0]][e[1]]

    def make(key):
        if key[0] == "plan":
            p = plans[key[1]]
            fused[key[1]] = fpn_topdown(get(p["top"]), [get(e) for e in p["laterals"]],
                                        name=nodes[p["sums"][-1]]["name"] + "_topdown", mx=mx)
            return
        node = nodes[key[1]]
        attrs, name, op = dict(_attrs(node)), node["name"], node["op"]
        if op == "null":
            built[key[1]] = mx.sym.var(name, **{k: v for k, v in attrs.items() if k.startswith("__")})
        else:
            built[key[1]] = _constructor(mx, op)(*[get(e) for e in node["inputs"]], **attrs, name=name)

    done = set()
    for h in jgraph["heads"]:
        stack = [(key_of(h), False)]
        while stack:
            key, ready = stack.pop()
            if key in done:
                continue
            if ready:
                make(key)
                done.add(key)
                continue
            stack.append((key, True))
            stack.extend((key_of(e), False) for e in reversed(deps(key)) if key_of(e) not in done)
    outs = [get(e) for e in jgraph["heads"]]
    return outs[0] if len(outs) == 1 else mx.sym.Group(outs)


def rewrite(symbol, mx=None):
    """The symbol with every chain plan_topdown() finds replaced by one `sd_fpn_topdown` node; the symbol itself,
    untouched, where there is none (so a second rewrite() is a no-op).  Every other node is rebuilt with its own
    name, attributes and inputs; heads keep their order.  Needs install()."""
    if not _own["installed"]:
        raise RuntimeError("fpn_topdown.rewrite needs fpn_topdown.install(): the fused node is not registered")
    jgraph = json.loads(symbol.tojson())
    plans = plan_topdown(jgraph)
    if not plans:
        return symbol
    return _build_symbol(_mx(mx), jgraph, plans)


def patch_merge_bn(module=None):
    """Wrap `utils.graph_optimize.merge_bn` (or `module.merge_bn`) as it is NOW -- the reference's, or
    merged_bn.merge_bn after merged_bn.patch_merge_bn() -- so that the symbol it returns passes through rewrite().
    Idempotent: a function that is already the wrapper is left alone.  Apply it LAST: merged_bn.patch_merge_bn() and
    merged_bn.unpatch_merge_bn() rebind the function and so drop the wrapper.  Returns the module."""
    module = importlib.import_module("utils.graph_optimize") if module is None else module
    inner = module.merge_bn
    if getattr(inner, "_sd_topdown_inner", None) is not None:
        return module

    def merge_bn(symbol, args, auxs, symbol_only=False):
        symbol, args, auxs = inner(symbol, args, auxs, symbol_only)
        return rewrite(symbol), args, auxs
    merge_bn._sd_topdown_inner = inner
    merge_bn.__doc__ = "fpn_topdown.rewrite() behind %s.%s" % (getattr(inner, "__module__", "?"), inner.__name__)
    module.merge_bn = merge_bn
    return module


def unpatch_merge_bn(module=None):
    """Put back the function patch_merge_bn() wrapped."""
    module = importlib.import_module("utils.graph_optimize") if module is None else module
    inner = getattr(module.merge_bn, "_sd_topdown_inner", None)
    if inner is not None:
        module.merge_bn = inner
    return module
