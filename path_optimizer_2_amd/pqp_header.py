"""Reader of include/pqp.h: the constants, structs and prototypes of the C ABI, as data.

capi.py builds its ctypes classes, constants and argtypes from what read() returns, so the header is the one place the ABI is written
down.  The header's vocabulary is small (see _statement); whatever falls outside it is refused with a HeaderError, never skipped: a
declaration this reader does not understand must not become a binding that is silently short of it.  A header that pqp.h includes by
`#include "pqp_x.h"` (pqp_search_params.h) is read too: it may hold struct typedefs and nothing else, and they arrive in Header.included.
"""
import functools
import os
import re
from collections import namedtuple

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pqp.h")

# Struct.fields: (name, type) with type "double", "int32_t" or an earlier struct's name, in declaration order.
# Function.ret / Param.type: C spellings normalised to "const T*", "T**", "T* const*" (one space after const, none before a star).
Struct = namedtuple("Struct", "name fields")
Param = namedtuple("Param", "name type")
Function = namedtuple("Function", "name ret params")
# constants: {name: int}, #defines and enumerators alike; included: the structs of the headers pqp.h includes (pqp_search_params.h), as structs
Header = namedtuple("Header", "constants structs opaque functions included")

SCALARS = ("int", "double")
DATA = ("double", "float", "int32_t", "int", "uint8_t")                 # pointees of the data pointers
RETURNS = ("int", "void", "const char*", "pqp_handle*")

_INT = r"-?\d+"
_NAME = r"[A-Za-z_]\w*"
_GUARD = "PQP_H_"


class HeaderError(ValueError):
    pass


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@functools.lru_cache(maxsize=None)
def _norm_type(t):
    t = re.sub(r"\s+", " ", t).strip()
    return re.sub(r"\s*\*\s*", "*", t).replace("*const", "* const")


@functools.lru_cache(maxsize=None)
def pointee(ctype):
    """"const double*" -> ("double", 1); "pqp_handle**" and "double* const*" -> (.., 2); "int" -> ("int", 0)"""
    m = re.fullmatch(rf"(?:const )?({_NAME})(\*\*|\* const\*|\*|)", ctype)
    if not m:
        raise HeaderError(f"type not understood: {ctype!r}")
    return m.group(1), {"": 0, "*": 1}.get(m.group(2), 2)


def _preprocessor(text, constants, includes):
    """takes the # lines out; every one must be the include guard, <stdint.h>, #include "pqp_x.h" (its name goes to `includes`), the
    extern "C" bracket or #define PQP_X <int>"""
    text, n = re.subn(r'#ifdef __cplusplus\s*(?:extern "C" \{|\})\s*#endif', "", text)
    if n != 2:
        raise HeaderError('expected one opening and one closing extern "C" bracket')
    out = []
    for line in text.split("\n"):
        s = line.strip()
        if not s.startswith("#"):
            out.append(line)
            continue
        m = re.fullmatch(rf"#define (PQP_[A-Z_0-9]+)\s+({_INT})", s)
        inc = re.fullmatch(r'#include "(pqp_[a-z_0-9]+\.h)"', s)
        if m and m.group(1) not in constants:
            constants[m.group(1)] = int(m.group(2))
        elif inc and inc.group(1) not in includes:
            includes.append(inc.group(1))
        elif s not in (f"#ifndef {_GUARD}", f"#define {_GUARD}", "#include <stdint.h>", "#endif"):
            raise HeaderError(f"preprocessor line not understood: {s!r}")
    return "\n".join(out)


def _statements(text):
    """the text cut at every ';' outside braces, whitespace collapsed"""
    depth, start = 0, 0
    for m in re.finditer(r"[{};]", text):
        i, ch = m.start(), m.group()
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
        elif ch == ";" and depth == 0:
            yield re.sub(r"\s+", " ", text[start:i]).strip()
            start = i + 1
    if depth != 0 or text[start:].strip():
        raise HeaderError(f"text behind the last statement: {text[start:].strip()[:80]!r}")


def _enum(body, constants):
    for item in body.split(","):
        m = re.fullmatch(rf"\s*(PQP_[A-Z_0-9]+)\s*=\s*({_INT})\s*", item)
        if not m or m.group(1) in constants:
            raise HeaderError(f"enumerator not understood (explicit integer values only): {item.strip()!r}")
        constants[m.group(1)] = int(m.group(2))


def _struct(name, body, structs):
    fields = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        m = re.fullmatch(rf"\s*({_NAME})\s+({_NAME}(?:\s*,\s*{_NAME})*)\s*", decl)
        if not m or not (m.group(1) in ("double", "int32_t") or m.group(1) in structs):
            raise HeaderError(f"{name}: field not understood: {decl.strip()!r}")
        fields += [(f.strip(), m.group(1)) for f in m.group(2).split(",")]
    if not fields or name in structs:
        raise HeaderError(f"{name}: empty or declared twice")
    structs[name] = Struct(name, tuple(fields))


def _included(name, include_dir, h):
    """a header pqp.h includes: its own guard, <stdint.h> and struct typedefs, nothing else; the structs go to h.included"""
    if include_dir is None:
        raise HeaderError(f'#include "{name}": no directory to read it from')
    with open(os.path.join(include_dir, name)) as f:
        text = strip_comments(f.read())
    guard = name[:-2].upper() + "_H_"
    body = []
    for line in text.split("\n"):
        s = line.strip()
        if not s.startswith("#"):
            body.append(line)
        elif s not in (f"#ifndef {guard}", f"#define {guard}", "#include <stdint.h>", "#endif"):
            raise HeaderError(f"{name}: preprocessor line not understood: {s!r}")
    known = dict(h.structs)
    for s in _statements("\n".join(body)):
        m = re.fullmatch(rf"typedef struct ({_NAME}) \{{(.*)\}} \1", s)
        if not m or m.group(1) in h.included or m.group(1) in h.opaque:
            raise HeaderError(f"{name}: declaration not understood (struct typedefs only): {s[:120]!r}")
        _struct(m.group(1), m.group(2), known)
        h.included[m.group(1)] = known[m.group(1)]


def _param(fn, text, h):
    m = re.fullmatch(rf"(.*\W)({_NAME})", text.strip())
    if not m:
        raise HeaderError(f"{fn}: parameter not understood: {text.strip()!r}")
    ctype, name = _norm_type(m.group(1)), m.group(2)
    base, stars = pointee(ctype)
    ok = (stars == 0 and ctype in SCALARS
          or stars == 1 and (base in DATA or base in h.structs or base in h.included or base in h.opaque or ctype == "void*")
          or ctype in ("void**", "double* const*") or (stars == 2 and ctype == base + "**" and base in h.opaque))
    if not ok:
        raise HeaderError(f"{fn}: type of parameter {name} not understood: {ctype!r}")
    return Param(name, ctype)


def _statement(s, h):
    """one of: [typedef] enum [name] { A = 1, ... } [name];  typedef struct name { fields } name;  typedef struct name name;
    ret name(params)"""
    m = re.fullmatch(rf"(?:typedef enum ({_NAME}) \{{(.*)\}} \1|enum \{{(.*)\}})", s)
    if m:
        return _enum(m.group(2) if m.group(2) is not None else m.group(3), h.constants)
    m = re.fullmatch(rf"typedef struct ({_NAME}) \{{(.*)\}} \1", s)
    if m:
        return _struct(m.group(1), m.group(2), h.structs)
    m = re.fullmatch(rf"typedef struct ({_NAME}) \1", s)
    if m:
        return h.opaque.append(m.group(1))
    m = re.fullmatch(r"(.*?)(pqp_[a-z_0-9]+) ?\((.*)\)", s)
    if m and "(" not in m.group(3):
        ret, name, params = _norm_type(m.group(1)), m.group(2), m.group(3).strip()
        if ret not in RETURNS or name in h.functions:
            raise HeaderError(f"{name}: return type {ret!r} not understood, or declared twice")
        h.functions[name] = Function(name, ret, tuple(_param(name, p, h) for p in params.split(",")) if params != "void" else ())
        return None
    raise HeaderError(f"declaration not understood: {s[:120]!r}")


def parse(text, include_dir=None):
    """Header of a header text; include_dir: where the headers it includes lie.  Raises HeaderError on anything outside the vocabulary."""
    h = Header({}, {}, [], {}, {})
    text = strip_comments(text)
    includes = []
    body = _preprocessor(text, h.constants, includes)
    for name in includes:
        _included(name, include_dir, h)
    for s in _statements(body):
        _statement(s, h)
    # the tripwire: every name the text calls like a function was read as one (the count tests/test_capi_symbols.py uses)
    called = set(re.findall(r"\b(pqp_[a-z_0-9]+)\s*\(", text))
    if called != set(h.functions):
        raise HeaderError(f"functions read and names followed by '(' differ: {sorted(called ^ set(h.functions))}")
    return h


def read(path=HEADER_PATH):
    with open(path) as f:
        return parse(f.read(), os.path.dirname(path))


def class_name(struct):
    """pqp_grid_geometry -> PqpGridGeometry"""
    return "".join(w.capitalize() for w in struct.split("_"))
