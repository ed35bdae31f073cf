"""Reads include/instag_hip.h: the header is the only statement of the C ABI, the ctypes structs, prototypes and
constants are derived from its text.

``parse(text)`` -> (structs, protos, constants): struct typedef name -> ``ctypes.Structure`` subclass, function name ->
``(restype, [argtypes])``, ``#define INSTAG_*`` name -> int, each in the header's order.  It takes the C subset the header
is written in and raises ValueError, naming the declaration, on anything else.  The reader does
not follow ``#include``: a header whose prototypes take a struct of another header is read with ``declared``, the
structs that header gave (they are not returned again).
"""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "instag_hip.h")

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "size_t": C.c_size_t,
            "float": C.c_float, "double": C.c_double, "uint8_t": C.c_uint8, "uint64_t": C.c_uint64, "int16_t": C.c_int16,
            "uint16_t": C.c_uint16}
_SPACE = re.compile(r"\s*")
_STRUCT = re.compile(r"typedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_FUNCTION = re.compile(r"([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)")
_FIRST = re.compile(r"(\w+)\b((?:\s*\*)*)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?")    # base type, stars, name, array length
_NEXT = re.compile(r"()((?:\*\s*)*)(\w+)\s*(?:\[\s*(\d+)\s*\])?")             # ", *name": the base type is the first's


def class_name(name):
    """instag_raster_args -> RasterArgs."""
    if not name.startswith("instag_"):
        raise ValueError(f"{name}: an ABI name starts with instag_")
    return "".join(p.capitalize() for p in name[len("instag_"):].split("_"))


def _ctype(base, stars, structs, what, ret=False):
    if base == "instag_stream_t" and stars == 0:
        return C.c_void_p
    if base in structs:
        if stars != 1:
            raise ValueError(f"{what}: struct {base} goes by one pointer, not by value or through two")
        return C.POINTER(structs[base])
    if base == "char" and stars == 1 and ret:
        return C.c_char_p
    if base in _SCALARS and stars == 0:
        return _SCALARS[base]
    if (base in _SCALARS or base == "void") and stars > 0:          # T* and the host arrays of device pointers, T* const*
        return C.c_void_p
    raise ValueError(f"{what}: cannot bind type {base + '*' * stars!r}")


def _declarators(text, structs, what):
    """'float *bg, *viewmatrix' or 'void* w[32]' -> [(name, ctype)]."""
    out, base = [], None
    for part in text.split(","):
        m = (_NEXT if base else _FIRST).fullmatch(part.strip())
        if not m:
            raise ValueError(f"{what}: cannot read {' '.join(text.split())!r}")
        base = base or m.group(1)
        t = _ctype(base, m.group(2).count("*"), structs, f"{what}: {m.group(3)}")
        out.append((m.group(3), t * int(m.group(4)) if m.group(4) else t))
    return out


def parse(text, declared=None):
    structs, protos, constants = {}, {}, {}
    seen = dict(declared or {})                                      # what a declaration may point to: theirs and ours
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for line in re.findall(r"^[ \t]*#.*$", text, flags=re.M):
        m = re.match(r"\s*#\s*define\s+(INSTAG_\w+)(.*)", line)
        if line.rstrip().endswith("\\") or (m and m.group(2)[:1] == "("):
            raise ValueError(f"{line.strip()}: a preprocessor line is one line, a constant has no parameters")
        if m and m.group(2).strip():                                 # (the include guard has no value)
            try:
                constants[m.group(1)] = int(m.group(2), 0)
            except ValueError:
                raise ValueError(f"{m.group(1)}: not an integer constant: {m.group(2).strip()!r}") from None
    text = re.sub(r"^[ \t]*#.*$|\bconst\b", " ", text, flags=re.M)
    text, braces = re.subn(r'extern\s+"C"\s*\{', " ", text.rstrip(), count=1)
    if braces:
        if not text.endswith("}"):
            raise ValueError('extern "C": the brace is not closed at the end of the header')
        text = text[:-1]
    pos = _SPACE.match(text).end()
    while pos < len(text):
        m = _STRUCT.match(text, pos)
        if m:
            tag, body, name = m.groups()
            if tag not in ("", name) or name in seen:
                raise ValueError(f"{name}: struct tag {tag!r} differs from the typedef, or the struct is declared twice")
            fields = [f for stmt in body.split(";") if stmt.strip() for f in _declarators(stmt, seen, name)]
            seen[name] = structs[name] = type(class_name(name), (C.Structure,),
                                 {"_fields_": fields, "__doc__": f"struct {name} (include/instag_hip.h)."})
            end = m.end()
        else:
            end = text.find(";", pos) + 1
            stmt = " ".join(text[pos:end - 1 if end else len(text)].split())
            m = _FUNCTION.fullmatch(stmt)
            if not end or (not m and stmt != "typedef void* instag_stream_t"):
                called = re.search(r"(\w+)\s*\(", stmt)
                raise ValueError(f"{called.group(1) if called else stmt[:60]}: not a declaration this reader takes: {stmt[:120]!r}")
            if m:
                ret, name, params = m.groups()
                ret = ret.replace("*", " * ").split()
                if name in protos or not ret or any(s != "*" for s in ret[1:]):
                    raise ValueError(f"{name}: declared twice, or cannot read the return type {m.group(1).strip()!r}")
                res = _ctype(ret[0], len(ret) - 1, seen, f"{name}: return type", ret=True)
                args = []
                if params.strip() != "void":
                    args = [t for p in params.split(",") for _, t in _declarators(p, seen, name)]
                    if any(issubclass(t, C.Array) for t in args):
                        raise ValueError(f"{name}: an array parameter is a pointer in C: declare it as one")
                class_name(name)                                     # (the instag_ prefix)
                protos[name] = (res, args)
        pos = _SPACE.match(text, end).end()
    return structs, protos, constants


def read(path=HEADER, declared=None):
    with open(path) as f:
        return parse(f.read(), declared)
