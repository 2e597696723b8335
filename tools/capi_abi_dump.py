#!/usr/bin/env python3
"""What the ctypes binding tells ctypes about the C ABI, as text: one line per function (restype, the kind of every argument), per
struct field (name, ctype, offset) and per public constant.  Two commits' dumps are compared with diff; the library must be built.

  python tools/capi_abi_dump.py            data pointers with their pointee: ptr<float64>
  python tools/capi_abi_dump.py --coarse   every data pointer as `ptr`, the way a binding that declares them void* sees them
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from path_optimizer_2_amd import capi  # noqa: E402


def kind(t, coarse):
    if t in (C.c_int, C.c_double, C.c_void_p):
        return {C.c_int: "int", C.c_double: "double", C.c_void_p: "ptr"}[t]
    if isinstance(t, type) and issubclass(t, C._Pointer):
        if issubclass(t._type_, C.Structure):
            return f"struct {t._type_.__name__}*"
        if t._type_ is C.c_void_p:
            return "ptr*"
        return "ptr" if coarse else f"ptr<{t._type_.__name__}>"
    if hasattr(t, "from_param") and hasattr(t, "dtype"):
        return "ptr" if coarse else f"ptr<{t.dtype}>"
    raise SystemExit(f"argtype not understood: {t!r}")


def main():
    coarse = "--coarse" in sys.argv[1:]
    lib = capi.load_library(with_torch=False)
    for name in sorted(capi.EXPORTS):
        fn = getattr(lib, name)
        args = "(no argtypes)" if fn.argtypes is None else ", ".join(kind(t, coarse) for t in fn.argtypes)
        print(f"function {name}: {getattr(fn.restype, '__name__', None)} <- {args}")
    structs = [v for v in vars(capi).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]
    for s in sorted(structs, key=lambda s: s.__name__):
        print(f"struct {s.__name__}: size {C.sizeof(s)}")
        for f, t in s._fields_:
            print(f"  {s.__name__}.{f}: {t.__name__} at {getattr(s, f).offset}")
    for k, v in sorted(vars(capi).items()):
        if k.isupper() and isinstance(v, int) and not isinstance(v, bool):
            print(f"constant {k} = {v}")


if __name__ == "__main__":
    main()
