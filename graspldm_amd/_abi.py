"""include/gldm.h as ctypes: the prototypes, descriptor structs and integer constants of the C ABI, parsed from the header
itself so that the Python side cannot drift from it.  The header is plain, regular C and this reads exactly that much: it
raises on anything it does not understand, never skips it.  No torch import.
"""
import ctypes
import os
import re


class GldmError(RuntimeError):
    pass


HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gldm.h")

_ARGS = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong,
         "unsigned long long": ctypes.c_ulonglong, "gldm_stream_t": ctypes.c_void_p}
_RETURNS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char *": ctypes.c_char_p}
_POINTEES = {"void", "char", "float", "double", "int32_t", "uint8_t", *_ARGS}   # what a pointer parameter may point to
_PROTO = re.compile(r"([A-Za-z_][\w\s*]*?)\b(gldm_\w+)\s*\(([^()]*)\)\s*;")
_ITEM = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(GLDM_\w+)[ \t]+(\S[^\n]*)$"                 # 1, 2: name, expression
                   r"|\benum\s+\w+\s*\{(.*?)\}"                                            # 3: enumerators
                   r"|\btypedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", re.M | re.S)      # 4, 5: fields, name


def _int(expr, consts):
    """A constant expression over integers and earlier constants."""
    try:
        if not re.fullmatch(r"[\w\s()+*-]+", expr):
            raise ValueError(expr)
        return int(eval(expr, {"__builtins__": {}}, dict(consts)))   # names, integers, + - * ( ) only: checked above
    except Exception as e:
        raise GldmError(f"gldm.h: '{expr.strip()}' is not an integer constant expression") from e


def _struct(name, body, structs, consts):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(\w+)\s+(.+)", decl, re.S)
        base = {"int32_t": ctypes.c_int32, **structs}.get(m.group(1)) if m else None
        if base is None:
            raise GldmError(f"gldm.h: struct {name}: field '{decl}' is neither int32_t nor an earlier struct")
        for item in m.group(2).split(","):
            f = re.fullmatch(r"\s*(\w+)\s*(?:\[(.+)\])?\s*", item)
            if not f:
                raise GldmError(f"gldm.h: struct {name}: cannot read the declarator '{item.strip()}'")
            fields.append((f.group(1), base * _int(f.group(2), consts) if f.group(2) else base))
    return type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"`{name}` of include/gldm.h."})


def _arg(param, fn, structs):
    words = [w for w in param.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        kind, known = " ".join(words[:words.index("*")]), _POINTEES | set(structs)
    else:
        kind, known = " ".join(words[:-1]), _ARGS
    if kind in structs and "*" not in words:
        raise GldmError(f"gldm.h: {fn}: parameter '{param}' passes a struct by value")
    if kind not in known:
        raise GldmError(f"gldm.h: {fn}: unknown type in parameter '{param}'")
    return ctypes.c_void_p if "*" in words else _ARGS[kind]


def parse(text):
    """Header text -> (prototypes {name: (restype, argtypes)}, structs {name: ctypes.Structure class}, constants
    {name: int}), each in declaration order."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    protos, structs, consts = {}, {}, {}
    for m in _ITEM.finditer(text):
        if m.group(1):
            consts[m.group(1)] = _int(m.group(2), consts)
        elif m.group(3) is not None:
            value = -1
            for item in filter(None, (e.strip() for e in m.group(3).split(","))):
                name, _, expr = item.partition("=")
                consts[name.strip()] = value = _int(expr, consts) if expr else value + 1
        else:
            structs[m.group(5)] = _struct(m.group(5), m.group(4), structs, consts)
    code = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    for ret, fn, params in _PROTO.findall(code):
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in _RETURNS:
            raise GldmError(f"gldm.h: {fn}: unknown return type '{ret}'")
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        protos[fn] = (_RETURNS[ret], [_arg(p, fn, structs) for p in params])
    missed = set(re.findall(r"\b(gldm_\w+)\s*\(", code)) - set(protos)
    if missed:
        raise GldmError(f"gldm.h: declared but not understood as prototypes: {sorted(missed)}")
    return protos, structs, consts


def _load():
    try:
        with open(HEADER) as f:
            return parse(f.read())
    except OSError as e:
        raise GldmError(f"{HEADER} is missing: the binding is derived from it ({e})") from e


PROTOTYPES, STRUCTS, CONSTANTS = _load()
