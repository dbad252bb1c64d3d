"""
The ctypes binding (pyxu_amd/_lib.py EXPORTS) and the integer constants of pyxu_amd/_dev.py against the one place
that states them, include/pyxu_amd.h: every prototype's arity, return type and argument types, and every constant
that mirrors a PXA_* #define.  Host only: the header is parsed as text, nothing is loaded or launched.
"""
import ctypes as ct
import os
import re

from pyxu_amd import _dev
from pyxu_amd._lib import EXPORTS

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pyxu_amd.h")

# C scalar -> the one ctypes type that passes it
SCALARS = {
    "int": ct.c_int,
    "int32_t": ct.c_int32,
    "int64_t": ct.c_int64,
    "uint32_t": ct.c_uint32,
    "uint64_t": ct.c_uint64,
    "size_t": ct.c_size_t,
    "double": ct.c_double,
}
RETURNS = {**SCALARS, "const char*": ct.c_char_p}


def _header_text():
    with open(HEADER) as f:
        txt = f.read()
    return txt, re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.M)


def _prototypes():
    """[(name, return type, [argument types])] of every pxa_* prototype, types normalised to `const T*` spelling."""
    _, code = _header_text()
    out = []
    for ret, name, args in re.findall(r"([\w\s\*]+?)\b(pxa_\w+)\s*\(([^)]*)\)\s*;", code):
        types = []
        for a in (s.strip() for s in args.split(",")):
            if a in ("", "void"):
                continue
            m = re.fullmatch(r"(.*?)(\w+)", a, flags=re.S)  # the trailing word is the parameter's name
            types.append(re.sub(r"\s*\*", "*", " ".join(m.group(1).split())))
        out.append((name, re.sub(r"\s*\*", "*", " ".join(ret.split())), types))
    return out


def _arg_matches(ctype, py):
    """None when the ctypes type `py` passes the C type `ctype`, otherwise the reason."""
    if ctype in SCALARS:
        return None if py is SCALARS[ctype] else f"{ctype} needs {SCALARS[ctype].__name__}"
    if ctype in ("void*", "const void*"):
        return None if py is ct.c_void_p else f"{ctype} needs c_void_p"
    if ctype == "void**":
        return None if py is ct.POINTER(ct.c_void_p) else "void** needs POINTER(c_void_p)"
    m = re.fullmatch(r"(?:const )?(\w+)\*", ctype)
    if m and m.group(1) in SCALARS:  # a typed pointer: untyped, or a pointer to a type of the same width
        if py is ct.c_void_p:
            return None
        if isinstance(py, type) and issubclass(py, ct._Pointer) and ct.sizeof(py._type_) == ct.sizeof(SCALARS[m.group(1)]):
            return None
        return f"{ctype} needs c_void_p or a POINTER of {ct.sizeof(SCALARS[m.group(1)])}-byte elements"
    return f"unknown C type {ctype!r}"


def test_every_prototype_matches_the_binding():
    protos = _prototypes()
    assert len(protos) >= 120 and len({p[0] for p in protos}) == len(protos)
    assert {p[0] for p in protos} == set(EXPORTS), {p[0] for p in protos} ^ set(EXPORTS)
    bad = []
    for name, ret, types in protos:
        res, args = EXPORTS[name]
        if ret not in RETURNS:
            bad.append(f"{name}: unknown return type {ret!r}")
        elif res is not RETURNS[ret]:
            bad.append(f"{name}: returns {ret}, bound as {res.__name__}")
        if len(args) != len(types):
            bad.append(f"{name}: {len(types)} parameters, bound with {len(args)}")
            continue
        for i, (c, py) in enumerate(zip(types, args)):
            why = _arg_matches(c, py)
            if why:
                bad.append(f"{name}, argument {i}: {why}, bound as {getattr(py, '__name__', py)}")
    assert not bad, "\n".join(bad)


def test_parser_rejects_what_it_does_not_know():
    assert _arg_matches("float", ct.c_float) is not None
    assert _arg_matches("struct plan*", ct.c_void_p) is not None
    assert _arg_matches("int64_t", ct.c_int) is not None
    assert _arg_matches("const int64_t*", ct.POINTER(ct.c_int32)) is not None
    assert _arg_matches("const int64_t*", ct.POINTER(ct.c_int64)) is None
    assert _arg_matches("const int*", ct.POINTER(ct.c_int32)) is None  # same width


# _dev names whose PXA_ counterpart is not PXA_<NAME>; dictionaries map key k to PXA_<PREFIX>_<K>
RENAMED = {"_CG_BLOCKS": "PXA_CG_BLOCKS", "_PDS_W": "PXA_PDS_TAP_SLOTS", "_MAX_TAPS": "PXA_MAX_TAPS",
           "_PROXADAM_PLANES": "PXA_PROXADAM_PLANES"}
DICTS = {"MODES": "PXA_MODE", "PROXADAM_VARIANTS": "PXA_PROXADAM"}
FAMILIES = ("RED", "UN", "BIN", "SHRINK", "TUNE", "PROX", "NLCG")


def test_dev_constants_equal_the_header_defines():
    txt, _ = _header_text()
    defines = {k: int(v) for k, v in re.findall(r"^#define (PXA_\w+) \(?(-?\d+)\)?", txt, flags=re.M)}
    mirrored = {}
    for name, v in vars(_dev).items():
        if isinstance(v, int) and not isinstance(v, bool) and "PXA_" + name in defines:
            mirrored[name] = ("PXA_" + name, v)  # the rule: _dev.NAME mirrors PXA_NAME
    for name, cname in RENAMED.items():
        mirrored[name] = (cname, getattr(_dev, name))
    for name, prefix in DICTS.items():
        for k, v in getattr(_dev, name).items():
            mirrored[f"{name}[{k!r}]"] = (f"{prefix}_{k.upper()}", v)
    for name, (cname, v) in mirrored.items():
        assert cname in defines, f"_dev.{name}: the header has no {cname}"
        assert defines[cname] == v, f"_dev.{name} = {v}, {cname} = {defines[cname]}"
    # both directions: every constant of these families is defined on both sides
    for fam in FAMILIES:
        here = {n for n in vars(_dev) if n.startswith(fam + "_") and isinstance(getattr(_dev, n), int)}
        there = {k[4:] for k in defines if k.startswith(f"PXA_{fam}_") and k != "PXA_TUNE_COUNT"}
        assert here and here == there, (fam, here ^ there)
    for name, prefix in DICTS.items():
        there = {k[len(prefix) + 1:].lower() for k in defines
                 if k.startswith(prefix + "_") and k != "PXA_PROXADAM_PLANES"}
        assert set(getattr(_dev, name)) == there, (name, set(getattr(_dev, name)) ^ there)
