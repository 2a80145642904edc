"""What the MXNet adapter modules share: mxnet_plugin and its satellites merged_bn, rcnn_loss, sync_bn, fpn_topdown.

  * the one state dictionary (`_state`: the MXNet module, the stream / sync contract, the per-device random states)
    and the data path every operator uses: NDArray -> raw device pointer, `_call` on the adapter's stream, `_sync`;
  * parameter parsing (`_tuple`, `_bool`, ...) and the req rules (`_no_add`, `_require_write`);
  * `_ws`: a workspace sized by the library's own `*_workspace_bytes` query;
  * `prop_base(mx)`: the CustomOpProp base whose constant answers are class attributes, and `op_base(mx)`;
  * registration and aliasing: `register_ops`, `put_alias` / `drop_alias`, `alias_ctor`;
  * the graph-dictionary helpers the two symbol rewriters (merged_bn, fpn_topdown) share.

Importing this module needs neither MXNet nor torch; mxnet_plugin's docstring has the ordering contract.
"""
import ctypes
from ast import literal_eval

from ._lib import lib

REQ = {"null": 0, "write": 1, "inplace": 2, "add": 3}
_PREFIX = "sd_"
_state = {"mx": None, "registered": False, "rng": {}, "stream": None, "sync": True}


# ---------------------------------------------------------------------------------- data path ----
def _mx(mx=None):
    """the MXNet module: the one given, the one an earlier register() left, or `import mxnet` (lazy: only here)"""
    if mx is not None:
        return mx
    if _state.get("mx") is not None:
        return _state["mx"]
    import mxnet
    return mxnet


def _ptr(nd):
    """Raw device pointer of an mx.nd.NDArray (MXNDArrayGetData), or of any object that exposes
    `data_ptr()` (the test stub wraps torch tensors)."""
    if nd is None:
        return None
    if hasattr(nd, "data_ptr"):
        return ctypes.c_void_p(nd.data_ptr())
    mx = _state["mx"]
    p = ctypes.c_void_p()
    rc = mx.base._LIB.MXNDArrayGetData(nd.handle, ctypes.byref(p))
    if rc != 0:
        raise RuntimeError("MXNDArrayGetData failed")
    return p


def _table(arrs):
    """void*[] of the arrays' device pointers (None stays a null pointer)"""
    return (ctypes.c_void_p * len(arrs))(*[None if a is None else _ptr(a).value for a in arrs])


def _wait(*arrs):
    for a in arrs:
        if a is not None and hasattr(a, "wait_to_read"):
            a.wait_to_read()


def _req(r):
    return REQ[r] if isinstance(r, str) else int(r)


def _stream():
    """hipStream_t the adapter launches on: install(stream=...) -- None = the NULL stream, an int / c_void_p, or
    a callable evaluated per call (e.g. `lambda: torch.cuda.current_stream().cuda_stream`)."""
    st = _state.get("stream")
    if callable(st):
        st = st()
    if st is None or isinstance(st, ctypes.c_void_p):
        return st
    return ctypes.c_void_p(int(st))


def _call(name, *args):
    """lib().call with the adapter's stream in place of a trailing None where the entry point's last parameter is
    `void* stream` (read off include/simpledet_ops.h)."""
    proto = lib().protos.get(name)
    if args and args[-1] is None and proto and proto[1] and proto[1][-1][0] == "stream":
        args = args[:-1] + (_stream(),)
    return lib().call(name, *args)


def _sync():
    if _state.get("sync", True):
        lib().call("sd_stream_synchronize", _stream())


def _scratch(like, nbytes):
    """Device scratch owned by MXNet (an NDArray on the same context)."""
    mx = _state["mx"]
    return mx.nd.empty(((int(nbytes) + 3) // 4,), ctx=like.context, dtype="float32")


def _ws(like, query, *args):
    """The workspace an entry point asks for: `query` is its size function (`sd_*_workspace_bytes`, return type as
    include/simpledet_ops.h declares it) and `args` that function's arguments.  Returns (the scratch array on
    `like`'s context -- keep it referenced until the call is issued --, its pointer, its size as c_size_t): the last
    two are what the entry point takes."""
    nbytes = int(getattr(lib().cdll, query)(*args))
    ws = _scratch(like, nbytes)
    return ws, _ptr(ws), ctypes.c_size_t(nbytes)


# ------------------------------------------------------------------- parameters and req rules ----
def _tuple(v, n=None, typ=float):
    t = literal_eval(v) if isinstance(v, str) else v
    if not isinstance(t, (tuple, list)):
        t = (t,) * (n or 1)
    return tuple(typ(x) for x in t)


def _bool(v):
    if isinstance(v, str):
        return v.strip().lower() in ("1", "true", "yes")
    return bool(v)


def _iarr(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _darr(vals):
    return (ctypes.c_double * len(vals))(*[float(v) for v in vals])


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _is_f16(dtypes):
    import numpy as np
    return bool(dtypes) and dtypes[0] is not None and np.dtype(dtypes[0]) == np.float16


def _no_add(req):
    """forward outputs: kWriteTo / kWriteInplace / kNullOp only.  The kernels overwrite their
    outputs, so honouring kAddTo would need a temporary; no graph of the reference requests it
    (MXNet uses kAddTo for gradients), hence it is refused loudly instead of silently ignored."""
    for r in req:
        if _req(r) == REQ["add"]:
            raise RuntimeError("forward outputs do not support req='add' (kAddTo)")


def _require_write(req, names):
    for r, n in zip(req, names):
        if _req(r) not in (REQ["write"], REQ["null"]):
            raise RuntimeError("%s requires kWriteTo (got req=%s)" % (n, r))


def _param_str(v):
    """keyword argument -> the string MXNet's front end would send (str(value)); numpy scalars
    are unwrapped first (numpy 2 prints np.float32(0.25) for repr)."""
    if isinstance(v, str):
        return v
    if isinstance(v, (tuple, list)):
        return "(" + ", ".join(_param_str(x) for x in v) + ("," if len(v) == 1 else "") + ")"
    if hasattr(v, "item") and not isinstance(v, (bool, int, float)):
        v = v.item()
    return repr(v) if isinstance(v, float) else str(v)


def _is_symbol(mx, v):
    sym_t = getattr(getattr(mx, "sym", None), "Symbol", None)
    return sym_t is not None and isinstance(v, sym_t)


# -------------------------------------------------------------------------- operator and prop base ----
def op_base(mx):
    """The CustomOp of an operator whose state is the dictionary its prop parsed the parameters into: `self.g`."""
    class Op(mx.operator.CustomOp):
        def __init__(self, g):
            super().__init__()
            self.g = g

    return Op


# what declare_backward_dependency is handed, as the first item of a DEPS entry
OUT_GRAD, IN_DATA, OUT_DATA = 0, 1, 2


def prop_base(mx):
    """The CustomOpProp the adapter's props derive from (made per `mx`, as the operators are).  What a prop answers
    with a constant is a class attribute:
        ARGS, OUTS, AUX   list_arguments / list_outputs / list_auxiliary_states
        OP, OP_ARGS       create_operator: OP(*[the prop's attributes named by OP_ARGS])
        DEPS              declare_backward_dependency: (OUT_GRAD | IN_DATA | OUT_DATA, index) pairs
    and a prop overrides the method where the answer depends on its parameters.  `need_top_grad` goes to
    CustomOpProp.__init__ from the prop's own __init__, and `num_visible_outputs` exists only on the props that set
    it (install() reads it with a default)."""
    class Prop(mx.operator.CustomOpProp):
        ARGS, OUTS, AUX = (), ("output",), ()
        OP, OP_ARGS = None, ("g",)
        DEPS = ()

        def list_arguments(self):
            return list(self.ARGS)

        def list_outputs(self):
            return list(self.OUTS)

        def list_auxiliary_states(self):
            return list(self.AUX)

        def create_operator(self, ctx, shapes, dtypes):
            return self.OP(*[getattr(self, a) for a in self.OP_ARGS])

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            return [(out_grad, in_data, out_data)[which][i] for which, i in self.DEPS]

    return Prop


# ------------------------------------------------------------------- registration and aliases ----
def register_ops(mx, table, own=None):
    """Register {name: PropClass} under sd_<name>; returns {name: the registered class} (and leaves it in
    own["props"])."""
    lib()  # fail loudly now if the HIP library is missing
    _state["mx"] = mx
    props = {name: mx.operator.register(_PREFIX + name)(prop) for name, prop in table.items()}
    if own is not None:
        own["props"] = props
    return props


def _namespaces(mx, ns):
    """Every namespace object the reference reaches an operator through: `mx.sym` (= `mx.symbol`) or
    `mx.sym.contrib`, and for contrib operators also the old `mx.contrib.symbol` / `mx.contrib.sym`
    module, which MXNet 1.x still fills with the same constructors as separate attributes
    (models/tridentnet/resnet_v1.py:85 builds its DeformableConvolution through it)."""
    out = []

    def add(t):
        if t is not None and all(t is not o for o in out):
            out.append(t)
    for root in (getattr(mx, "sym", None), getattr(mx, "symbol", None)):
        if root is not None:
            add(getattr(root, ns) if ns else root)
    if ns == "contrib":
        old = getattr(mx, "contrib", None)
        for a in ("symbol", "sym"):
            add(getattr(old, a, None) if old is not None else None)
    return out


def put_alias(mx, ns, attr, ctor_for):
    """Set `attr` in every namespace of _namespaces(mx, ns) to ctor_for(the constructor it replaces) and keep that
    constructor as `_sd_reference_<attr>`.  A second install keeps the first one's original."""
    for target in _namespaces(mx, ns):
        cur = getattr(target, attr, None)
        original = cur._sd_original if getattr(cur, "_sd_alias", False) else cur
        setattr(target, attr, ctor_for(original))
        setattr(target, "_sd_reference_" + attr, original)


def drop_alias(mx, ns, attr):
    """The inverse of put_alias: the constructor an alias replaced is put back (the attribute deleted if there was
    none) and `_sd_reference_<attr>` removed."""
    for target in _namespaces(mx, ns):
        cur = getattr(target, "__dict__", {}).get(attr)
        if getattr(cur, "_sd_alias", False):
            if cur._sd_original is None:
                delattr(target, attr)
            else:
                setattr(target, attr, cur._sd_original)
        if "_sd_reference_" + attr in getattr(target, "__dict__", {}):
            delattr(target, "_sd_reference_" + attr)


def alias_ctor(mx, name, prop, original, record, label=None, aux_inputs=False, positionals="mixed",
               unknown_inputs="keep", native_drop=(), group_all=False):
    """The symbol constructor that stands for a reference operator: builds mx.sym.Custom(op_type=sd_<name>) and
    returns its visible outputs; a parameter set the prop's `sd_supports` does not take goes back to `original`
    (the constructor the alias replaces) after record(name, node name, why).
        label           what error messages and the constructor's __name__ call the operator (default: name)
        aux_inputs      the auxiliary states are inputs too, after the arguments
        positionals     "mixed": positional inputs get their argument names only when keyword symbols come with
                        them (else they stay positional); "always": every positional input is named
        unknown_inputs  a keyword symbol that is no input name: "keep" it after the named ones, or "error"
        native_drop     keywords of this adapter's own that `original` must not see
        group_all       where every output is visible: the node itself, or (True) the Group of its outputs"""
    label = label or name

    def ctor(*args, **kwargs):
        # MXNet's generated constructors skip inputs / attributes given as None
        # (models/sepc/sepc_dconv.py:13: `bias=bias if not no_bias else None`)
        kwargs = {k: v for k, v in kwargs.items() if v is not None}
        name_kw = kwargs.pop("name", None)
        params = {k: _param_str(v) for k, v in kwargs.items() if not _is_symbol(mx, v)}
        inputs = {k: v for k, v in kwargs.items() if _is_symbol(mx, v)}
        supports = getattr(prop, "sd_supports", None)
        why = supports(params) if supports is not None else ""
        if why:
            if original is None:
                raise ValueError("%s: %s (and no native constructor to fall back to)" % (label, why))
            record(name, name_kw, why)
            native = {k: v for k, v in kwargs.items() if k not in native_drop}
            if name_kw is not None:
                native["name"] = name_kw
            return original(*args, **native)
        p = prop(**params)
        if positionals == "always" or (args and inputs):
            # MXNet composes a variadic operator (Custom is `*data`) from positional OR keyword Symbols, never
            # both (Symbol._compose raises TypeError) -- and the reference mixes them for the built-in it
            # believes it is calling (models/sepc/sepc_dconv.py:12-16: DeformableConvolution(x, offset,
            # weight=weight, bias=bias, ...)): positional inputs take the operator's argument names in order
            names = list(p.list_arguments()) + (list(p.list_auxiliary_states()) if aux_inputs else [])
            if len(args) > len(names):
                raise TypeError("%s takes %d inputs (%s), %d given positionally"
                                % (label, len(names), names, len(args)))
            for k, v in zip(names, args):
                if k in inputs:
                    raise TypeError("%s: input '%s' given positionally and by keyword" % (label, k))
                inputs[k] = v
            unknown = {k: v for k, v in inputs.items() if k not in names}
            if unknown and unknown_inputs == "error":
                raise TypeError("%s: unknown inputs %s" % (label, list(unknown)))
            # keyword composition matches by name; keep the operator's own order for readability of the graph
            inputs = {k: inputs[k] for k in names if k in inputs} | unknown
            args = ()
        sym = mx.sym.Custom(*args, op_type=_PREFIX + name, name=name_kw, **inputs, **params)
        nout = len(p.list_outputs())
        nvis = getattr(p, "num_visible_outputs", nout)
        if nvis == nout and not group_all:
            return sym
        return sym[0] if nvis == 1 else mx.sym.Group([sym[i] for i in range(nvis)])
    ctor.__name__ = label
    ctor._sd_alias = True
    ctor._sd_original = original
    return ctor


# ----------------------------------------------------------------- graph-dictionary helpers ----
ADD_OPS = ("elemwise_add", "_Plus", "_plus", "add_n", "ElementWiseSum")


def _attrs(node):
    return node.get("attrs") or node.get("attr") or node.get("param") or {}


def _constructor(mx, op):
    if op.startswith("_contrib_"):
        return getattr(mx.sym.contrib, op[len("_contrib_"):])
    if op.startswith("_"):
        return getattr(mx.sym._internal, op)
    return getattr(mx.sym, op)
