"""The public interface of simpledet_amd.ops, pinned to a recorded snapshot.

tests/golden/ops_interface.json holds, for every public name of the module: the signature of each function
(parameter names, order, defaults, keyword-only markers), the forward / backward signatures of each autograd
Function, the fields of each namedtuple, the field names and ctypes types of each Structure, and the value of each
constant.  How the module marshals its calls may change; none of this may -- a default or a keyword silently
altered is what no other test would see.

The snapshot is produced by this file (`python -m tests.test_ops_interface <out.json>`, run from the repository
root) by introspection alone -- no library and no device -- so the same file runs on any commit.
"""
import ctypes
import inspect
import json
import os
import sys
import types

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_interface.json")


def _ctype_name(t):
    """c_int -> "c_int", c_float * 4 -> "c_float*4" (ctypes names its array types c_float_Array_4)"""
    if isinstance(t, type) and issubclass(t, ctypes.Array):
        return "%s*%d" % (_ctype_name(t._type_), t._length_)
    return t.__name__


def _describe(obj):
    import torch
    if isinstance(obj, type):
        if issubclass(obj, ctypes.Structure):
            return dict(kind="structure", fields=[[n, _ctype_name(t)] for n, t in obj._fields_])
        if issubclass(obj, tuple) and hasattr(obj, "_fields"):
            return dict(kind="namedtuple", fields=list(obj._fields))
        if issubclass(obj, torch.autograd.Function):
            return dict(kind="autograd", forward=str(inspect.signature(obj.forward)),
                        backward=str(inspect.signature(obj.backward)))
        return dict(kind="class", bases=[b.__name__ for b in obj.__bases__])
    if callable(obj):
        return dict(kind="function", signature=str(inspect.signature(obj)))
    return dict(kind="constant", value=obj)


def snapshot():
    """{public name: its description}, in sorted order; modules the file imports are not its interface"""
    from simpledet_amd import ops
    return {name: _describe(obj) for name, obj in sorted(vars(ops).items())
            if not name.startswith("_") and not isinstance(obj, types.ModuleType)}


def test_ops_interface_matches_snapshot():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(snapshot()))      # tuples -> lists, as the file holds them
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(snapshot(), f, indent=1, sort_keys=True)
        f.write("\n")
