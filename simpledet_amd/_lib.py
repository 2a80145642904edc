"""ctypes binding of libsimpledet_ops_hip.so (the C ABI in include/simpledet_ops.h).

The argtypes are generated from the header itself, so the header is the single source of truth for
the boundary.  There is NO CPU fallback: if the shared library is missing or a symbol is absent the
import fails loudly.
"""
import contextlib
import ctypes
import operator
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "simpledet_ops.h")
# SIMPLEDET_AMD_LIB: load another build of the same ABI (tools/ use the -DSD_PROFILING build)
LIB_PATH = os.environ.get("SIMPLEDET_AMD_LIB") or os.path.join(_HERE, "libsimpledet_ops_hip.so")

_SCALARS = {
    "int": ctypes.c_int,
    "long": ctypes.c_long,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
    "size_t": ctypes.c_size_t,
    "int32_t": ctypes.c_int32,
    "uint32_t": ctypes.c_uint32,
    "uint8_t": ctypes.c_uint8,
    "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64,
    "unsigned": ctypes.c_uint,
}


_FLOATS = (ctypes.c_float, ctypes.c_double)
_INTS = tuple(set(_SCALARS.values()) - set(_FLOATS))


class _Bound:
    """One symbol, bound: the foreign function and its marshalling, laid out once from the prototype -- which
    parameters are pointers, which floats, which integers (`const char*` needs nothing).  Calling it converts
    each argument by its parameter's kind and makes the foreign call:
      pointer   anything with data_ptr() (a tensor; duck-typed, this module needs no torch) becomes its address;
                None stays NULL; everything else -- an int, a c_void_p, a ctypes array, a byref -- passes as it is
      float     float(v)
      integer   an int passes; anything else goes through __index__ (numpy / torch integer scalars, bools), so
                a float is refused with TypeError
    A ctypes scalar (c_size_t(n), c_float(x), ...) passes through the last two untouched.  The slots are walked
    kind by kind, inline: a Python-level converter call per argument cost the 21-argument forward 1.3 us."""
    __slots__ = ("name", "fn", "names", "pointers", "floats", "ints", "stream")

    def __init__(self, name, fn, args):
        self.name, self.fn = name, fn
        self.names = tuple(n for n, _ in args)
        self.pointers = tuple(i for i, (_, t) in enumerate(args) if t is ctypes.c_void_p)
        self.floats = tuple(i for i, (_, t) in enumerate(args) if t in _FLOATS)
        self.ints = tuple(i for i, (_, t) in enumerate(args) if t in _INTS)
        self.stream = bool(args) and args[-1] == ("stream", ctypes.c_void_p)

    def __call__(self, args):
        if len(args) != len(self.names):
            raise TypeError("%s takes %d arguments (%s), got %d"
                            % (self.name, len(self.names), ", ".join(self.names), len(args)))
        a = list(args)
        for i in self.pointers:
            v = a[i]
            if v is not None:
                ptr = getattr(v, "data_ptr", None)
                if ptr is not None:
                    a[i] = ptr()
        for i in self.floats:
            v = a[i]
            if v.__class__ is not float and not isinstance(v, ctypes._SimpleCData):
                a[i] = float(v)
        for i in self.ints:
            v = a[i]
            if v.__class__ is not int and not isinstance(v, ctypes._SimpleCData):
                a[i] = operator.index(v)
        return self.fn(*a)


def parse_header(path=HEADER):
    """Return {symbol: (restype, [(argname, ctype)])} for every function the header declares."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(sd_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if "*" in ret:
            restype = ctypes.c_char_p if "char" in ret else ctypes.c_void_p
        else:
            restype = _SCALARS.get(ret.replace("const", "").strip(), ctypes.c_int)
        argl = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                mm = re.match(r"(.*?)(\w+)$", a)
                typ, an = mm.group(1).strip(), mm.group(2)
                if "*" in typ:
                    ct = ctypes.c_char_p if re.match(r"(const\s+)?char\s*\*$", typ) else ctypes.c_void_p
                else:
                    ct = _SCALARS[typ.replace("const", "").strip()]
                argl.append((an, ct))
        protos[name] = (restype, argl)
    return protos


def header_abi_version(path=HEADER):
    m = re.search(r"^\s*#define\s+SD_ABI_VERSION\s+(\d+)", open(path).read(), flags=re.M)
    if not m:
        raise ImportError("SD_ABI_VERSION missing from %s" % path)
    return int(m.group(1))


class SimpleDetOpsError(RuntimeError):
    """code: the SD_ERR_* value the entry point returned (include/simpledet_ops.h)."""
    code = 0


SD_ERR_UNSUPPORTED = -2


class _Lib:
    def __init__(self, cdll=None):
        """cdll: a library that is loaded already (the marshaller's test binds a recording stand-in);
        None loads LIB_PATH and checks its ABI version."""
        if cdll is not None:
            self._bind(cdll)
            return
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "simpledet_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C simpledet_amd/csrc` (needs hipcc, gfx950). There is no CPU "
                "fallback." % LIB_PATH)
        # torch ships its own libamdhip64.so.7; import it first so this library binds to the SAME
        # HIP runtime (one runtime per process: streams and device pointers are shared with torch)
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for pure-C users
            pass
        self._bind(ctypes.CDLL(LIB_PATH))
        # buffer layouts and size contracts are part of the ABI: a library older or newer than the
        # header this wrapper marshals for is refused
        want = header_abi_version()
        got = int(self.cdll.sd_abi_version())
        if got != want:
            raise ImportError("simpledet_amd: %s has ABI version %d, include/simpledet_ops.h %d: rebuild "
                              "(`make -C simpledet_amd/csrc`)" % (LIB_PATH, got, want))

    def _bind(self, cdll):
        """restype, argtypes and the marshalling (_Bound) of every symbol, all from the header's prototypes"""
        self.cdll = cdll
        self.protos = parse_header()
        self.bound = {}
        for name, (restype, args) in self.protos.items():
            try:
                fn = getattr(cdll, name)
            except AttributeError as e:
                raise ImportError("simpledet_amd: %s does not export %s (header/library mismatch)"
                                  % (LIB_PATH, name)) from e
            fn.restype = restype
            fn.argtypes = [t for _, t in args]
            self.bound[name] = _Bound(name, fn, args)

    def entry(self, name):
        """the _Bound of a symbol the header declares: entry(name)(args) marshals `args` and calls it"""
        try:
            return self.bound[name]
        except KeyError:
            raise AttributeError("include/simpledet_ops.h declares no %s" % name) from None

    def check(self, name, rc):
        """raise SimpleDetOpsError for the non-zero code `rc` an entry point returned"""
        if rc != 0:
            msg = self.cdll.sd_last_error()
            err = SimpleDetOpsError("%s failed (%d): %s" % (name, rc, (msg or b"").decode()))
            err.code = int(rc)
            raise err
        return rc

    def call(self, name, *args):
        """Call an int-returning entry point, its arguments marshalled by the prototype (_Bound: tensors and
        plain numbers go in as they are); raise SimpleDetOpsError on a non-zero code."""
        return self.check(name, self.entry(name)(args))

    def set_tuning(self, key, value):
        self.call("sd_set_tuning", key.encode(), int(value))

    def get_tuning(self, key):
        """the value a kernel-variant knob holds: the library's default until someone sets it"""
        v = ctypes.c_int()
        self.call("sd_get_tuning", key.encode(), ctypes.byref(v))
        return int(v.value)

    def tuning_keys(self):
        """the keys of the library's knob list, in its order"""
        keys = []
        while (key := self.entry("sd_tuning_key")((len(keys),))) is not None:
            keys.append(key.decode())
        return keys

    @contextlib.contextmanager
    def tuned(self, **knobs):
        """Run a block under these knob values and put the previous ones back after it, in reverse order, however
        the block ends.  An unknown key raises before anything is changed."""
        before = [(key, self.get_tuning(key)) for key in knobs]
        try:
            for key, value in knobs.items():
                self.set_tuning(key, value)
            yield
        finally:
            for key, value in reversed(before):
                self.set_tuning(key, value)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _Lib()
    return _lib
