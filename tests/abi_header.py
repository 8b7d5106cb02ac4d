"""The header side of the ABI tests, stated once: what a test reads out of include/*.h to hold a ctypes mirror, a Python constant or a
table of rows against it.  The parser knows the C the headers use and no more: `typedef struct X { ... } X;` with int32_t, float,
double and earlier structs as field types, scalar and one-dimensional array fields, extents written as digits or as object-like
`#define NAME <digits>` macros.  tests/abi_derive.py is the call side."""
import ctypes as C
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = {"int32_t": C.c_int32, "float": C.c_float, "double": C.c_double}


def header(name):
    """the text of include/<name>"""
    with open(os.path.join(INCLUDE, name)) as f:
        return f.read()


def defines(*texts):
    """{macro: int} of every `#define NAME <digits>` of the texts"""
    return {k: int(v) for text in texts for k, v in re.findall(r"^[ \t]*#define (\w+) (\d+)\b", text, flags=re.M)}


def statements(name, *texts):
    """the member declarations of `typedef struct name { ... } name;`, comments stripped, as the header words them"""
    pat = r"typedef struct %s \{(.*?)\} %s;" % (name, name)
    body = next(m.group(1) for m in (re.search(pat, text, flags=re.S) for text in texts) if m)
    body = re.sub(r"/\*.*?\*/|//[^\n]*", "", body, flags=re.S)
    return [s.strip() for s in body.split(";") if s.strip()]


def struct_of(name, *texts, known=None):
    """the ctypes class of `typedef struct name { ... } name;`, found in the texts given; a symbolic extent is a #define of these same
    texts; known = {struct name: class} for fields of an earlier struct"""
    types = dict(SCALARS, **(known or {}))
    macros = defines(*texts)
    fields = []
    for stmt in statements(name, *texts):
        ty, decl = stmt.split(None, 1)
        for d in decl.split(","):
            field, extent = re.fullmatch(r"(\w+)\s*(?:\[\s*(\w+)\s*\])?", d.strip()).groups()
            n = None if extent is None else int(extent) if extent.isdigit() else macros[extent]
            fields.append((field, types[ty] if n is None else types[ty] * n))
    return type(name, (C.Structure,), {"_fields_": fields})


def layout(cls):
    """[(field, offset, size)]"""
    return [(n, getattr(cls, n).offset, getattr(cls, n).size) for n, _ in cls._fields_]


def same_layout(got, want):
    return C.sizeof(got) == C.sizeof(want) and layout(got) == layout(want)


def aot_symbols(text):
    """the `int NAME(MD_AOT_ARGS);` declarations of a header, in order (the expression of _lib.exported_symbols)"""
    return re.findall(r"^\s*int\s+(\w+)\s*\(MD_AOT_ARGS\)\s*;", text, flags=re.M)
