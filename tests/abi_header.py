"""The one reader of include/m3ae_hip.h for the tests: prototypes, descriptor layouts, constants and the ABI number, from the header
text alone.  tests/test_host_logic.py holds the ctypes binding (m3ae_amd/_lib.py) to all of it; the per-feature host tests state
their own relations between entry points on top of `prototypes()`.  A declaration this reader cannot classify raises ValueError
with the declaration's name -- nothing is skipped."""
import collections
import ctypes as C
import functools
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "m3ae_hip.h")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
RESTYPES = {"int": C.c_int, "int64_t": C.c_int64, "void": None, "const char*": C.c_char_p}
DESCRIPTORS = ("m3ae_gemm_desc", "m3ae_attn_desc", "m3ae_xattn_desc")
# what a pointer may point at: a typed ctypes POINTER in the binding must name this type (void: only a plain c_void_p)
POINTEES = dict(SCALARS, void=None, uint8_t=C.c_uint8, **{d: d for d in DESCRIPTORS})

Pointer = collections.namedtuple("Pointer", "pointee")   # a pointer or array parameter; pointee = the C type word


@functools.lru_cache(None)
def text():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER_PATH).read(), flags=re.S)


@functools.lru_cache(None)
def prototypes():
    """{name: (restype text, [normalised parameter text, ...])} of every declared function, whitespace collapsed."""
    found = {}
    for res, name, params in re.findall(r"^([A-Za-z_][\w \t*]*?)\s*\b(m3ae_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text(), flags=re.M):
        res = " ".join(res.split())
        if res not in RESTYPES:
            raise ValueError(f"{name}: return type {res!r} is not one of {sorted(RESTYPES)}")
        params = [" ".join(p.split()) for p in params.split(",")]
        found[name] = (res, [] if params == ["void"] else params)
    calls = re.findall(r"\b(m3ae_[a-z0-9_]+)\s*\(", text())
    if sorted(calls) != sorted(found):
        raise ValueError(f"declarations the prototype pattern did not take: {sorted(set(calls) ^ set(found))}")
    return found


def _parameter(decl, param):
    m = re.fullmatch(r"(?:const )?(\w+) ?(\*?) ?\w+ ?(\[\d*\])?", param)
    if not m or m.group(1) not in POINTEES:
        raise ValueError(f"{decl}: cannot read the parameter {param!r}")
    word, star, array = m.groups()
    if star or array:
        return Pointer(word)
    if word not in SCALARS:
        raise ValueError(f"{decl}: {word!r} is no scalar parameter type ({param!r})")
    return SCALARS[word]


def ctypes_signature(name):
    """(restype, [argtype, ...]) as the header implies them: a ctypes type per scalar, a Pointer(pointee) per pointer or array."""
    res, params = prototypes()[name]
    return RESTYPES[res], [_parameter(name, p) for p in params]


def binding_agrees(want, bound):
    """Does the binding's argtype `bound` carry the header's parameter `want` (an element of ctypes_signature's list)?  Scalars by
    the exact ctypes type; a pointer as c_void_p, or as a POINTER to the header's pointee (a descriptor: a Structure with the
    header's field list)."""
    if not isinstance(want, Pointer):
        return bound is want
    if bound is C.c_void_p:
        return True
    if not (isinstance(bound, type) and issubclass(bound, C._Pointer)):
        return False
    pointee = POINTEES[want.pointee]
    if want.pointee in DESCRIPTORS:
        return issubclass(bound._type_, C.Structure) and list(bound._type_._fields_) == struct_fields(pointee)
    return pointee is not None and bound._type_ is pointee


@functools.lru_cache(None)
def _struct_fields(name):
    m = re.search(r"typedef struct \{([^{}]*)\}\s*" + name + r"\s*;", text())
    if not m:
        raise ValueError(f"{name}: no `typedef struct {{ ... }} {name};` in the header")
    fields = []
    for decl in filter(None, (" ".join(d.split()) for d in m.group(1).split(";"))):
        base = re.fullmatch(r"(?:const )?(\w+) ?(.*)", decl)
        if base.group(1) not in POINTEES or base.group(1) in DESCRIPTORS:
            raise ValueError(f"{name}: cannot read the field declaration {decl!r}")
        for part in base.group(2).split(","):
            field = re.fullmatch(r"(\*?) ?(\w+)", part.strip())
            if not field or not (field.group(1) or base.group(1) in SCALARS):
                raise ValueError(f"{name}: cannot read the declarator {part!r} of {decl!r}")
            fields.append((field.group(2), C.c_void_p if field.group(1) else SCALARS[base.group(1)]))
    return tuple(fields)


def struct_fields(name):
    """[(field, ctype)] of `typedef struct { ... } name;`, multi-declarator lines expanded; every pointer is a c_void_p."""
    return list(_struct_fields(name))


def struct_sizeof(name):
    return C.sizeof(type(name, (C.Structure,), {"_fields_": struct_fields(name)}))


@functools.lru_cache(None)
def constants():
    """{M3AE_X: n} of every enumerator of every `enum { ... }` and of every numeric `#define M3AE_X n`."""
    found = {}
    for body in re.findall(r"\benum\s*\{([^{}]*)\}", text()):
        for item in filter(None, (" ".join(i.split()) for i in body.split(","))):
            m = re.fullmatch(r"(M3AE_[A-Z0-9_]+) = (-?\d+)", item)
            if not m:
                raise ValueError(f"cannot read the enumerator {item!r}")
            found[m.group(1)] = int(m.group(2))
    for name, value in re.findall(r"^#define[ \t]+(M3AE_[A-Z0-9_]+)[ \t]+(-?\d+)[ \t]*$", text(), flags=re.M):
        found[name] = int(value)
    return found


def abi_version():
    return int(re.search(r"^#define\s+M3AE_ABI_VERSION\s+(\d+)\s*$", text(), flags=re.M).group(1))
