"""ctypes binding of libmickey_hip.so (the C ABI declared in include/mickey_hip.h).

The product path calls the HIP kernels ONLY through this module; there is no CPU or ATen fallback:
if the shared library is missing or a call fails, an exception is raised.

The binding is DERIVED from the two headers at import (parse_header below): an entry point is declared in the header and
defined in csrc/*.hip, nowhere else.  The parser is strict -- a declaration it cannot read in full raises at import.
"""
import collections
import ctypes
import os
import re

import torch

from . import build as _build


class MickeyHipError(RuntimeError):
    pass


# every type the headers may use; widening this set is a deliberate edit here
_SCALARS = {"int": "i", "long long": "l", "float": "f", "unsigned long long": "u"}   # any pointer and mk_stream_t: "p"
_FIELDS = {"long long": "q", "double": "d"}                                          # struct fields; any pointer: "q"
_CODES = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_longlong, "f": ctypes.c_float, "u": ctypes.c_ulonglong,
          "s": ctypes.c_char_p}
_TYPE_WORDS = {"void", "char", "short", "int", "long", "float", "double", "signed", "unsigned", "const", "mk_stream_t"}

Header = collections.namedtuple("Header", "signatures params constants structs")


def _bad(what, stmt):
    return MickeyHipError("mickey_hip headers: %s in `%s`" % (what, " ".join(stmt.split())))


def _ctype(text, stmt):
    """a C type as written -> (its words without const, whether it is a pointer)"""
    m = re.fullmatch(r"\s*((?:\w+\s+)*\w+)\s*((?:\*\s*)*)", text)
    if not m:
        raise _bad("unreadable type `%s`" % text.strip(), stmt)
    return " ".join(w for w in m.group(1).split() if w != "const"), bool(m.group(2))


def _code(text, stmt, table):
    base, pointer = _ctype(text, stmt)
    if pointer:
        return "q" if table is _FIELDS else "p"
    if base == "mk_stream_t" and table is _SCALARS:
        return "p"
    if base not in table:
        raise _bad("type `%s` outside the binding's set" % text.strip(), stmt)
    return table[base]


def _declarator(text, stmt):
    """`const float* x` -> (`const float*`, `x`); a declaration without a name raises"""
    m = re.fullmatch(r"\s*(.*[\s*])(\w+)\s*", text, re.S)
    if not m or m.group(2) in _TYPE_WORDS:
        raise _bad("parameter `%s` without a name" % text.strip(), stmt)
    return m.group(1), m.group(2)


def parse_header(text):
    """The declarations of a mickey_hip header -> Header(signatures {name: (result code, argument codes)}, params {name:
    parameter names}, constants {MK_*: int} (enumerators and #defines), structs {name: [(field, struct-module code)]}).
    Anything but enum blocks, `typedef struct`s, the mk_stream_t typedef and `ret mk_name(params);` prototypes raises."""
    signatures, params, constants, structs = {}, {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    for line, name, value in re.findall(r"^([ \t]*#[ \t]*define[ \t]+(MK_\w+)\b(.*))$", text, re.M):
        if not re.fullmatch(r"\s+-?\d+\s*", value) or name in constants:
            raise _bad("not a new #define MK_NAME n", line)
        constants[name] = int(value)
    text = re.sub(r"^[ \t]*#[^\n]*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}\s*$', r"\1", text, flags=re.S)

    def enum(m):
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            e = re.fullmatch(r"(MK_\w+)\s*=\s*(-?\d+)", item)
            if not e or e.group(1) in constants:
                raise _bad("enumerator `%s` is not a new MK_NAME = n" % item, m.group(0))
            constants[e.group(1)] = int(e.group(2))
        return ""

    def struct(m):
        fields = []
        for stmt in filter(None, (s.strip() for s in m.group(2).split(";"))):
            first, *more = stmt.split(",")
            base, name = _declarator(first, stmt)
            fields.append((name, _code(base, stmt, _FIELDS)))
            base = base.rstrip("* \t\n")   # `float *p, *g`: the stars belong to each name
            for decl in more:
                d = re.fullmatch(r"\s*(\**)\s*(\w+)\s*", decl)
                if not d:
                    raise _bad("unreadable field `%s`" % decl.strip(), stmt)
                fields.append((d.group(2), _code(base + d.group(1), stmt, _FIELDS)))
        if m.group(1) in structs or len({f for f, _ in fields}) != len(fields):
            raise _bad("duplicate declaration", m.group(0))
        structs[m.group(1)] = fields
        return ""

    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", struct, text)
    text = re.sub(r"\btypedef\s+void\s*\*\s*mk_stream_t\s*;", "", text)
    *stmts, rest = text.split(";")
    if rest.strip():
        raise _bad("unterminated statement", rest)
    for stmt in stmts:
        m = re.fullmatch(r"\s*([\w\s*]+?[\s*])(mk_\w+)\s*\(([^()]*)\)\s*", stmt, re.S)
        if not m:
            raise _bad("not a prototype `ret mk_name(params)`", stmt)
        ret, name, plist = m.groups()
        if name in signatures:
            raise _bad("duplicate declaration", stmt)
        res = "s" if _ctype(ret, stmt) == ("char", True) and "const" in ret.split() else _code(ret, stmt, _SCALARS)
        decls = [] if plist.strip() in ("", "void") else [_declarator(p, stmt) for p in plist.split(",")]
        signatures[name] = (res, "".join(_code(t, stmt, _SCALARS) for t, _ in decls))
        params[name] = tuple(n for _, n in decls)
    return Header(signatures, params, constants, structs)


def _parse_file(name):
    with open(os.path.join(_build.INCLUDE, name)) as f:
        return parse_header(f.read())


_ABI, _DEV = _parse_file("mickey_hip.h"), _parse_file("mickey_hip_dev.h")
for _kind in ("signatures", "constants", "structs"):
    _twice = set(getattr(_ABI, _kind)) & set(getattr(_DEV, _kind))
    if _twice:
        raise MickeyHipError("mickey_hip headers: %s declared in both headers" % sorted(_twice))

# name -> (restype code, argument codes); order and meaning exactly as in include/mickey_hip.h
SIGNATURES = _ABI.signatures
# development knobs (include/mickey_hip_dev.h): process-wide schedule selectors for benchmarks / tests, never called by
# the product path
DEV_SIGNATURES = _DEV.signatures
PARAM_NAMES = {**_ABI.params, **_DEV.params}
CONSTANTS = {**_ABI.constants, **_DEV.constants}   # every MK_* enumerator and #define, also a module attribute of its C name
STRUCTS = {**_ABI.structs, **_DEV.structs}
globals().update(CONSTANTS)

MK_BF16, MK_F16, MK_F32 = (CONSTANTS[k] for k in ("MK_BF16", "MK_F16", "MK_F32"))   # (spelled out: dtype_code names them)
ACT_NONE, ACT_RELU, ACT_GELU = (CONSTANTS[k] for k in ("MK_ACT_NONE", "MK_ACT_RELU", "MK_ACT_GELU"))

_lib = None
_missing = set()


def lib_path():
    return os.environ.get("MICKEY_HIP_LIB", _build.lib_path())


def load():
    """Load libmickey_hip.so; raises MickeyHipError if it is absent (never falls back)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise MickeyHipError("libmickey_hip.so not found at %s -- build it with `python -m mickey_amd.build` "
                             "(mickey_amd has no CPU/ATen fallback)" % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in list(SIGNATURES.items()) + list(DEV_SIGNATURES.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError:
            _missing.add(name)  # reported by missing_symbols(); calling it raises
            continue
        fn.restype = _CODES[res]
        fn.argtypes = [_CODES[c] for c in args]
    _lib = lib
    return lib


def exported_symbols():
    return list(SIGNATURES)


def missing_symbols():
    load()
    return sorted(_missing)


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise MickeyHipError("expected a device tensor")
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dtype_code(dt):
    if dt == torch.bfloat16:
        return MK_BF16
    if dt == torch.float16:
        return MK_F16
    if dt == torch.float32:
        return MK_F32   # the exact parity mode: "lp" buffers hold fp32, contractions on the fp32-input MFMA
    raise MickeyHipError("unsupported low-precision dtype %s" % dt)


def _exported(lib, name):
    if name in _missing:
        raise MickeyHipError("libmickey_hip.so does not export %s (stale build?)" % name)
    return getattr(lib, name)


def call(name, *args):
    """Call an ABI function that returns a status code; raise on failure."""
    lib = load()
    try:
        rc = _exported(lib, name)(*args)
    except ctypes.ArgumentError as e:   # ctypes says "argument 13: TypeError: ...": name the C parameter
        m = re.match(r"argument (\d+)(.*)", str(e), re.S)
        names = PARAM_NAMES.get(name, ())
        if not m or not 0 < int(m.group(1)) <= len(names):
            raise
        raise MickeyHipError("%s: argument %s '%s'%s" % (name, m.group(1), names[int(m.group(1)) - 1], m.group(2))) from None
    if rc != 0:
        raise MickeyHipError("%s failed (%d): %s" % (name, rc, lib.mk_last_error().decode()))


def query(name, *args):
    return _exported(load(), name)(*args)
