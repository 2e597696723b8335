"""The ctypes binding against include/pqp.h, with the C compiler as the judge: capi.py builds its classes, constants and argtypes from what
pqp_header reads in the header, and these tests hold that reading against gcc's (prototypes, struct layouts), against the header's
text (nothing skipped) and against what the typed data pointers must refuse.  No device is needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from build_util import declared as _declared
from path_optimizer_2_amd import capi, pqp_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = capi.HEADER


def _gcc(args, cwd):
    return subprocess.run(["gcc", "-Wall", "-Werror", "-I", INCLUDE, *args], cwd=cwd, capture_output=True, text=True)


def _pointer_line(k, f, params=None):
    params = [p.type for p in f.params] if params is None else params
    return f"{f.ret} (*f_{k})({', '.join(params) or 'void'}) = {f.name};"


def test_prototypes_agree_with_the_compiler(tmp_path):
    """One function pointer per declared function, typed from the reader's output and initialised with the function itself: a wrong
    count, type or const is an incompatible-pointer-types error.  A mutated line must fail, so the check cannot pass vacuously."""
    fns = list(HEADER.functions.values())
    lines = [_pointer_line(k, f) for k, f in enumerate(fns)]
    (tmp_path / "protos.c").write_text('#include "pqp.h"\n' + "\n".join(lines) + "\n")
    r = _gcc(["-c", "protos.c", "-o", "protos.o"], tmp_path)
    assert r.returncode == 0, r.stderr[:4000]
    k = [f.name for f in fns].index("pqp_create")
    params = [p.type for p in fns[k].params]
    assert params[-1] == "int"
    lines[k] = _pointer_line(k, fns[k], params[:-1] + ["double"])
    (tmp_path / "mutated.c").write_text('#include "pqp.h"\n' + "\n".join(lines) + "\n")
    r = _gcc(["-c", "mutated.c", "-o", "mutated.o"], tmp_path)
    assert r.returncode != 0 and "pqp_create" in r.stderr and "incompatible" in r.stderr, r.stderr[:4000]


def test_struct_layouts_agree_with_the_compiler(tmp_path):
    """sizeof of every struct, offsetof and size of every field, as gcc lays the header out, against the generated ctypes classes"""
    prints = []
    for s in HEADER.structs.values():
        prints.append(f'printf("{s.name} %zu\\n", sizeof({s.name}));')
        prints += [f'printf("{s.name}.{f} %zu %zu\\n", offsetof({s.name}, {f}), sizeof((({s.name}*)0)->{f}));' for f, _ in s.fields]
    (tmp_path / "layout.c").write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pqp.h"\nint main(void) {\n' + "\n".join(prints)
                                       + "\nreturn 0;\n}\n")
    r = _gcc(["layout.c", "-o", "layout"], tmp_path)
    assert r.returncode == 0, r.stderr[:4000]
    got = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    want = []
    for s in HEADER.structs.values():
        cls = capi.STRUCTS[s.name]
        assert cls is getattr(capi, pqp_header.class_name(s.name)) and [f for f, _ in cls._fields_] == [f for f, _ in s.fields]
        want.append(f"{s.name} {C.sizeof(cls)}")
        want += [f"{s.name}.{f} {getattr(cls, f).offset} {getattr(cls, f).size}" for f, _ in s.fields]
    assert len(HEADER.structs) == 10 and len(got) == len(want)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]


def test_reader_skips_nothing():
    """every function, struct, #define and enumerator of the header's text is in the binding, under the names it has always had"""
    names = _declared()
    assert len(HEADER.functions) == len(names) and sorted(HEADER.functions) == names == sorted(capi.EXPORTS)
    text = pqp_header.strip_comments(open(os.path.join(INCLUDE, "pqp.h")).read())
    defines = dict(re.findall(r"#define (PQP_[A-Z_0-9]+)[ \t]+(-?\d+)", text))
    enumerators = dict(re.findall(r"\b(PQP_[A-Z_0-9]+)\s*=\s*(-?\d+)", text))
    assert len(defines) >= 11 and len(enumerators) >= 51 and not set(defines) & set(enumerators)
    for k, v in {**defines, **enumerators}.items():
        assert getattr(capi, k[len("PQP_"):]) == int(v) == HEADER.constants[k], k
    assert len(HEADER.constants) == len(defines) + len(enumerators)
    structs = re.findall(r"typedef struct (\w+)\s*\{", text)
    assert structs == list(HEADER.structs) and len(structs) == 10
    assert [capi.STRUCTS[s].__name__ for s in structs[:3]] == ["PqpParams", "PqpSizes", "PqpGridGeometry"]
    assert (capi.OPT_STORE_WARM, capi.OPT_LONG_LINES, capi.KERNEL_LANE_PER_QP, capi.SCORE_STRIDE, capi.PROJECT_TILE_SAMPLES,
            capi.SPEED_NOT_FINITE, capi.TRAJ_STRIDE, capi.PROJ_NOT_FINITE) == (1, 8, 2, 8, 1024, 16, 8, 8)


_SMALL = """#ifndef PQP_H_
#define PQP_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PQP_N 3   /* a count */
typedef struct pqp_handle pqp_handle;
typedef struct pqp_a { double x, y; int32_t n; } pqp_a;
typedef struct pqp_b { pqp_a a; %s } pqp_b;
enum { PQP_ONE = 1, PQP_MINUS = -2 };
%s
int pqp_f(pqp_handle* h, const pqp_b* b,
          const float* data, double* const* rows, int n);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_refuses_what_it_does_not_know():
    h = pqp_header.parse(_SMALL % ("int32_t k;", "const char* pqp_name(void);"))
    assert h.constants == {"PQP_N": 3, "PQP_ONE": 1, "PQP_MINUS": -2} and h.opaque == ["pqp_handle"]
    assert h.structs["pqp_b"].fields == (("a", "pqp_a"), ("k", "int32_t")) and h.structs["pqp_a"].fields[1] == ("y", "double")
    assert h.functions["pqp_name"] == pqp_header.Function("pqp_name", "const char*", ())
    assert [p.type for p in h.functions["pqp_f"].params] == ["pqp_handle*", "const pqp_b*", "const float*", "double* const*", "int"]
    for field, decl in (("float k;", ""),                                 # a field type the ABI does not use
                        ("pqp_c c;", ""),                                 # a struct that was not declared
                        ("", "double pqp_g(int n);"),                     # a return type
                        ("", "int pqp_g(long n);"),                       # a parameter type
                        ("", "int pqp_g(int (*cb)(int));"),               # a callback
                        ("", "int pqp_g(const pqp_b b);"),                # a struct by value
                        ("", "enum { PQP_AUTO };"),                       # an enumerator without a value
                        ("", "#define PQP_F 1.5"),
                        ("", "#pragma once"),
                        ("", "static inline int pqp_g(int n) { return n; }"),
                        ("", "extern int pqp_counter;")):
        with pytest.raises(pqp_header.HeaderError):
            pqp_header.parse(_SMALL % (field, decl))


def _sizes_call(lib, s):
    sizes, p = capi.PqpSizes(), capi.default_params(lib)
    rc = lib.pqp_path_sizes(C.byref(p), 80, s, C.byref(sizes))
    return rc, (sizes.vars, sizes.cons, sizes.nnz_a, sizes.nnz_p)


def test_typed_data_pointers_refuse_the_wrong_array(hip_lib):
    ok = (0, (479, 482, 1355, 319))                                      # test_sizes_is_pure_host_logic's
    s64 = np.zeros(80, np.float64)
    for good in (s64, None, s64.ctypes.data, C.c_void_p(s64.ctypes.data), s64.ctypes.data_as(C.POINTER(C.c_double)), (C.c_double * 80)()):
        assert _sizes_call(hip_lib, good) == ok
    for bad in (np.zeros(80, np.float32), np.zeros(80, np.int64), np.zeros(160)[::2], [0.0] * 80, 1.5, "s"):
        with pytest.raises((C.ArgumentError, TypeError)) as e:
            _sizes_call(hip_lib, bad)
        assert "pqp_path_sizes: s " in str(e.value), str(e.value)
    with pytest.raises((C.ArgumentError, TypeError)) as e:                # a second function and pointee: int32_t* rows
        hip_lib.pqp_path_pattern(None, 80, 80, np.zeros(8, np.int64), None, None)
    assert "pqp_path_pattern: rows " in str(e.value) and "int32" in str(e.value)
    assert hip_lib.pqp_path_pattern(None, 80, 80, np.zeros(8, np.int32), None, None) == capi.ERR_INVALID      # refused by the library


def test_typed_data_pointers_check_a_tensors_element_type(hip_lib):
    import torch
    s_arg = hip_lib.pqp_path_sizes.argtypes[2]
    t64 = torch.zeros(80, dtype=torch.float64)
    assert s_arg.from_param(t64).value == t64.data_ptr()
    for dt in (torch.float32, torch.int32, torch.int64):
        with pytest.raises(TypeError, match="pqp_path_sizes: s "):
            s_arg.from_param(torch.zeros(80, dtype=dt))
    rows_arg = hip_lib.pqp_path_pattern.argtypes[3]
    assert rows_arg.from_param(torch.zeros(8, dtype=torch.int32)).value
    with pytest.raises(TypeError, match="pqp_path_pattern: rows "):
        rows_arg.from_param(t64)


def test_every_function_has_its_prototype(hip_lib):
    """argtypes and restype of all declared functions, the three included that a call-by-call binding had left to ctypes' defaults"""
    for f in HEADER.functions.values():
        fn = getattr(hip_lib, f.name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(f.params), f.name
    assert hip_lib.pqp_version.argtypes == () or list(hip_lib.pqp_version.argtypes) == []
    assert hip_lib.pqp_last_error.restype is C.c_char_p and hip_lib.pqp_default_params.restype is None
    assert list(hip_lib.pqp_stream_batch_default.argtypes) == [C.c_int] and hip_lib.pqp_multi_handle.restype is C.c_void_p
    assert hip_lib.pqp_create.argtypes[1] is C.POINTER(capi.PqpParams) and hip_lib.pqp_create.argtypes[0] is C.POINTER(C.c_void_p)


def test_a_library_short_of_a_function_is_refused(tmp_path):
    (tmp_path / "short.c").write_text("void pqp_default_params(void* p) { (void)p; }\n")
    r = _gcc(["-shared", "-fPIC", "short.c", "-o", "libshort.so"], tmp_path)
    assert r.returncode == 0, r.stderr
    with pytest.raises(OSError, match="pqp_production_params"):
        capi.load_library(str(tmp_path / "libshort.so"), with_torch=False)
