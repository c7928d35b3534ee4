"""include/vs_amd.h read as data: every prototype's return kind, parameter names and parameter kinds, and the same kinds of a ctypes type.
test_capi_symbols.py holds the binding's SIGNATURES table against it; test_capi_calls_cpu.py takes the parameter names from it."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a C type without `*` or `[]` -> its kind; anything with either is a "pointer"
_SCALAR_KINDS = {"void": "void", "int": "int", "int32_t": "int", "int64_t": "int64", "size_t": "size", "double": "double", "float": "float",
                 "vs_transform": "transform", "vs_point": "point"}


def _c_kind(decl):
    """the kind of `decl`, a return type or a parameter with its name taken off"""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    assert len(words) == 1 and words[0] in _SCALAR_KINDS, "no kind for the C type %r" % decl
    return _SCALAR_KINDS[words[0]]


def prototypes():
    """{name: (return kind, [(parameter name, kind), ...])} of every `type name(args);` in the header, comments stripped"""
    text = open(os.path.join(ROOT, "include", "vs_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(vs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in out, name
        params = []
        args = " ".join(args.split())
        if args != "void":
            for a in args.split(","):
                m = re.fullmatch(r"\s*(.*?)\b(\w+)\s*((?:\[\d*\])?)\s*", a)
                assert m, (name, a)
                params.append((m.group(2), _c_kind(m.group(1) + m.group(3))))
        out[name] = (_c_kind(ret), params)
    return out


def ctypes_kind(t, capi):
    """the kind of a SIGNATURES entry (a ctypes type, or None for void)"""
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    for ct, kind in ((C.c_int, "int"), (C.c_int32, "int"), (C.c_int64, "int64"), (C.c_size_t, "size"), (C.c_double, "double"), (C.c_float, "float"),
                     (capi.Transform, "transform"), (capi.Point, "point")):
        if t is ct:
            return kind
    raise AssertionError("no kind for the ctypes type %r" % (t,))
