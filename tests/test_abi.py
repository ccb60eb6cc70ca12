"""The ctypes binding against ``include/alphadia_hip.h``: the header is parsed once, and ``_abi.PROTOTYPES`` - the one
table ``_abi.declare`` applies to the loaded library - must name its exports in its order, with the restype and every
argtype the header's text gives.  No GPU needed, and the library is not loaded: only ``_abi`` is imported."""

from __future__ import annotations

import ctypes as C
import glob
import os
import re

from alphadia_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "include", "alphadia_hip.h")) as _f:
    HEADER = _f.read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)  # the header without its comments

# (return type, name, [parameter declarations]) of every export, in the header's order
DECLS = [(ret, name, [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")])
         for ret, name, params in re.findall(r"\b(const char \*|int)\s*(adh_\w+)\s*\(([^)]*)\)\s*;", CODE)]

SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
           "double": C.c_double, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32}
BY_VALUE = ("int", "int32_t", "int64_t", "uint32_t", "uint64_t", "float", "double")
HANDLES = ("adh_handle_t", "adh_mlp_t", "adh_quant_t", "adh_pg_t", "adh_pfdr_t", "adh_tl_t", "adh_mbr_t")


def c_type_of(param: str) -> str:
    """The type of a parameter declaration, without the parameter's name and with the stars closed up."""
    return re.sub(r"\s*\*\s*", "*", re.sub(r"\w+$", "", param).strip())


def expected_ctype(c_type: str):
    """The ctypes type the rule gives for a C type of the header; a spelling the rule does not know is an error."""
    if c_type in BY_VALUE:
        return SCALARS[c_type]
    if c_type in ("const float*const*", "float*const*"):
        return C.POINTER(C.POINTER(C.c_float))
    if c_type in ("void*", "const void*"):
        return C.c_void_p
    if c_type in ("void**", "void*const*"):
        return C.POINTER(C.c_void_p)
    m = re.fullmatch(r"(?:const )?(\w+)(\*{1,2})", c_type)
    if not m:
        raise AssertionError(f"C type not covered by the binding's rule: {c_type!r}")
    base, stars = m.groups()
    if base in HANDLES:
        return C.c_void_p if stars == "*" else C.POINTER(C.c_void_p)
    if stars == "*" and base in SCALARS:
        return C.POINTER(SCALARS[base])
    if stars == "*" and base in _abi.STRUCTS:
        return C.POINTER(_abi.STRUCTS[base])
    raise AssertionError(f"C type not covered by the binding's rule: {c_type!r}")


def test_header_declares_what_the_table_lists_in_its_order():
    names = [name for _, name, _ in DECLS]
    assert len(names) == len(set(names)) == 126
    assert set(names) == set(_abi.PROTOTYPES)
    assert names == list(_abi.PROTOTYPES)
    assert set(re.findall(r"\badh_\w+(?=\s*\()", CODE)) == set(names)  # no declaration the parse above missed


def test_every_prototype_has_the_header_types():
    wrong = []
    for ret, name, params in DECLS:
        restype, argtypes = _abi.PROTOTYPES[name]
        want = [expected_ctype(c_type_of(p)) for p in params]
        if restype != (C.c_char_p if ret.startswith("const char") else C.c_int32):
            wrong.append(f"{name}: restype {restype.__name__}")
        if len(want) != len(argtypes):
            wrong.append(f"{name}: {len(argtypes)} argtypes for {len(want)} parameters")
            continue
        wrong += [f"{name}: parameter {i} `{p}` is {got.__name__}, the header gives {exp.__name__}"
                  for i, (p, got, exp) in enumerate(zip(params, argtypes, want)) if got != exp]
    assert not wrong, "\n".join(wrong)
    assert [name for name, (restype, _) in _abi.PROTOTYPES.items() if restype == C.c_char_p] == ["adh_last_error"]


def _struct_fields(name: str) -> list[str]:
    tag = name[: -len("_t")]
    body = re.search(rf"typedef struct {tag} \{{(.*?)\}} {name};", CODE, re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        for declarator in decl.split(","):
            fields.append(re.search(r"(\w+)\s*(?:\[[^\]]*\])?$", declarator.strip()).group(1))
    return fields


def test_every_struct_taken_by_pointer_has_its_class():
    taken = set()
    for _, _, params in DECLS:
        for p in params:
            m = re.fullmatch(r"(?:const )?(adh_\w+_t)\*", c_type_of(p))
            if m and m.group(1) not in HANDLES:
                taken.add(m.group(1))
    assert taken and taken <= set(_abi.STRUCTS)
    for name, cls in _abi.STRUCTS.items():
        assert issubclass(cls, C.Structure)
        assert _struct_fields(name) == [f[0] for f in cls._fields_], name


def test_declare_sets_every_export_from_the_table():
    class Export:
        restype, argtypes = C.c_int, None

    class Library:
        def __getattr__(self, name):
            if name not in _abi.PROTOTYPES:
                raise AttributeError(name)
            self.__dict__[name] = Export()
            return self.__dict__[name]

    lib = Library()
    _abi.declare(lib)
    assert list(vars(lib)) == list(_abi.PROTOTYPES)
    for name, (restype, argtypes) in _abi.PROTOTYPES.items():
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes, name


def test_call_sites_name_declared_exports_and_reach_all_of_them():
    called = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "alphadia_amd", "*.py"))):
        with open(path) as f:
            called[os.path.basename(path)] = set(re.findall(r"\b(?:lib|_pylib)\.(adh_\w+)", f.read()))
    for module, names in called.items():
        assert names <= set(_abi.PROTOTYPES), (module, sorted(names - set(_abi.PROTOTYPES)))
    assert set(_abi.PROTOTYPES) - called["runtime.py"] - {"adh_last_error"} == set()


def test_argtypes_are_assigned_in_declare_only():
    for path in sorted(glob.glob(os.path.join(ROOT, "alphadia_amd", "*.py"))):
        with open(path) as f:
            src = f.read()
        assert len(re.findall(r"\.argtypes\s*=", src)) == (1 if path.endswith("_abi.py") else 0), path
        assert set(re.findall(r"\b\w*_PROTOTYPES\b", src)) == set(), path


def test_limits_equal_the_header_defines():
    defines = dict(re.findall(r"^#define (ADH_\w+) \(?(-?\d+)u?\)?\s*$", CODE, re.M))
    for define, value in (("ADH_NUM_FEATURES", _abi.NUM_FEATURES), ("ADH_FLAG_SKIP", _abi.FLAG_SKIP),
                          ("ADH_MLP_MAX_LINEAR", _abi.MLP_MAX_LINEAR), ("ADH_LOESS_MAX_KERNELS", _abi.LOESS_MAX_KERNELS),
                          ("ADH_LOESS_MAX_DEGREE", _abi.LOESS_MAX_DEGREE), ("ADH_QUANT_MAX_COLUMNS", _abi.QUANT_MAX_COLUMNS),
                          ("ADH_TL_MAX_MATRICES", _abi.TL_MAX_MATRICES), ("ADH_TL_QC_SLICE", _abi.TL_QC_SLICE),
                          ("ADH_CANDIDATE_LIBRARY_MAX_SERIES", _abi.CANDIDATE_LIBRARY_MAX_SERIES),
                          ("ADH_GENERIC_LAUNCH_STATS", 2 * _abi.N_GENERIC_GROUPS),
                          ("ADH_IM_LAUNCH_STATS", 2 * _abi.N_IM_GROUPS)):
        assert int(defines[define]) == value, define
    assert "#define ADH_CALIBRATION_CHUNK_ROWS (1 << 20)" in CODE and _abi.CALIBRATION_CHUNK_ROWS == 1 << 20


def test_export_families_have_their_counts():
    count = lambda prefix: sum(name.startswith(prefix) for name in _abi.PROTOTYPES)  # noqa: E731
    assert (count("adh_quant_"), count("adh_pg_"), count("adh_pfdr_"), count("adh_tl_"), count("adh_mbr_")) == (10, 6, 9, 9, 11)
