"""Reader of the C ABI headers (include/gcm_hip.h, include/gcm_hip_debug.h): the ctypes prototypes, the integer
constants and the struct layout of a binding come from the header text itself, so nothing mirrors it by hand.
Plain `re` over the declarations; a declaration this reader cannot map raises at import, naming it."""
import ctypes
import functools
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "include")

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "int32_t": ctypes.c_int32,
            "int64_t": ctypes.c_int64, "long": ctypes.c_long, "gcm_stream_t": ctypes.c_void_p}


def header(name):
    """Text of include/<name> without its comments."""
    with open(os.path.join(INCLUDE, name)) as f:
        return strip_comments(f.read())


def strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


@functools.lru_cache(maxsize=None)      # ("int B", "gcm_stream_t stream", ... recur in every declaration)
def _ctype(decl):
    """ctypes class of `type` or `type name` (comment-free text); every pointer is a c_void_p."""
    if "*" in decl:
        return ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if not 1 <= len(words) <= 2 or words[0] not in _SCALARS:
        raise TypeError(f"no ctypes mapping for '{' '.join(words)}'")
    return _SCALARS[words[0]]


def prototypes(text):
    """name -> (restype, [argtypes]) of every function declared in the comment-free header `text`."""
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    text = re.sub(r"typedef\b[^;{]*(\{[^}]*\})?[^;]*;", "", text)              # typedefs, struct bodies included
    text = text.replace('extern "C" {', "").replace("}", "")
    out = {}
    for decl in filter(None, map(str.strip, text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(\w+)\s*\((.*)\)", decl, flags=re.S)
        if not m:
            raise TypeError(f"not a function declaration: '{' '.join(decl.split())}'")
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        try:
            res = ctypes.c_char_p if ret.replace(" ", "") == "constchar*" else _ctype(ret)
            out[name] = (res, [] if params == "void" else [_ctype(p) for p in params.split(",")])
        except TypeError as e:
            raise TypeError(f"{name}: {e}") from None
    return out


def constants(text):
    """NAME -> int of every `#define GCM_NAME <decimal literal>`; (-2) and 4u count, expressions are skipped."""
    out = {}
    for line in text.splitlines():
        words = line.split(None, 2) if line.startswith("#define GCM_") else ()
        m = len(words) == 3 and re.fullmatch(r"\(?\s*(-?\d+)[uU]?\s*\)?", words[2].strip())
        if m:
            out[words[1]] = int(m.group(1))
    return out


def struct_fields(text, struct):
    """ctypes `_fields_` of `typedef struct <struct> { ... }`: scalar, `type a, b;`, `type a[n];` and pointer members."""
    body = text[text.index("typedef struct %s {" % struct):]
    fields = []
    for member in filter(None, map(str.strip, body[body.index("{") + 1:body.index("}")].split(";"))):
        kind, names = member.rsplit("*", 1) if "*" in member else member.replace("const ", "").split(None, 1)
        base = _ctype(member if "*" in member else kind)
        for name in names.split(","):
            name, _, dim = name.strip().rstrip("]").partition("[")
            fields.append((name, base * int(dim) if dim else base))
    return fields
