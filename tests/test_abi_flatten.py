"""The ctypes binding against ``include/alphadia_hip_flatten.h``, by the rules tests/test_abi.py applies to the main
header: ``_abi.FLATTEN_EXPORTS`` - the third table ``_abi.declare`` applies to the loaded library - must name that
header's exports in its order, with the restype and every argtype the header's text gives.  No GPU needed."""

from __future__ import annotations

import ctypes as C
import os
import re

from alphadia_amd import _abi
from test_abi import ROOT, c_type_of, expected_ctype

with open(os.path.join(ROOT, "include", "alphadia_hip_flatten.h")) as _f:
    HEADER = _f.read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)

DECLS = [(ret, name, [" ".join(p.split()) for p in params.split(",")])
         for ret, name, params in re.findall(r"\b(const char \*|int)\s*(\w+)\s*\(([^)]*)\)\s*;", CODE)]


def test_header_declares_what_the_table_lists_in_its_order():
    names = [name for _, name, _ in DECLS]
    assert names == list(_abi.FLATTEN_EXPORTS) and len(names) == len(set(names)) == 1
    assert all(n.startswith("adfl_") for n in names)
    assert set(re.findall(r"\b\w+(?=\s*\()", CODE)) == set(names)  # no declaration the parse above missed
    assert not re.findall(r"\badh_\w+\s*\(", HEADER)  # the main header's family stays in the main header
    assert '#include "alphadia_hip.h"' in CODE
    assert not set(_abi.FLATTEN_EXPORTS) & (set(_abi.PROTOTYPES) | set(_abi.LFQ_EXPORTS))
    assert "struct" not in CODE  # scalar and pointer parameters only


def test_every_export_has_the_header_types():
    for ret, name, params in DECLS:
        restype, argtypes = _abi.FLATTEN_EXPORTS[name]
        assert ret == "int" and restype is C.c_int32, name
        assert argtypes == [expected_ctype(c_type_of(p)) for p in params], name
        assert c_type_of(params[0]) == "adh_handle_t*", name


def test_the_limits_are_those_of_the_python_side():
    from alphadia_amd import flatten

    defines = {k: int(v) for k, v in re.findall(r"#define (ADFL_\w+) (\d+)", CODE)}
    assert set(defines) == {"ADFL_MAX_COLUMNS", "ADFL_MAX_ROWS", "ADFL_MAX_GROUP", "ADFL_CARD_WAVE_MAX_MEMBERS",
                            "ADFL_CARD_WAVE_DEBUG_MEMBERS", "ADFL_SELECT_WAVE_MAX_CELLS"}
    assert (defines["ADFL_MAX_COLUMNS"], defines["ADFL_MAX_ROWS"], defines["ADFL_MAX_GROUP"]) == (
        flatten.MAX_COLUMNS, flatten.MAX_ROWS, flatten.MAX_GROUP) == (32, 255, 255)
    assert 1 <= defines["ADFL_CARD_WAVE_MAX_MEMBERS"] <= defines["ADFL_CARD_WAVE_DEBUG_MEMBERS"] <= 64
    assert 64 <= defines["ADFL_SELECT_WAVE_MAX_CELLS"] < 255 * 32


def test_declare_takes_the_table():
    class Export:
        restype, argtypes = C.c_int, None

    class Library:
        def __getattr__(self, name):
            if name not in _abi.FLATTEN_EXPORTS:
                raise AttributeError(name)
            self.__dict__[name] = Export()
            return self.__dict__[name]

    lib = Library()
    _abi.declare(lib, _abi.FLATTEN_EXPORTS)
    assert list(vars(lib)) == list(_abi.FLATTEN_EXPORTS)
    for name, (restype, argtypes) in _abi.FLATTEN_EXPORTS.items():
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes, name


def test_the_runtime_calls_every_export_through_the_context():
    with open(os.path.join(ROOT, "alphadia_amd", "runtime.py")) as f:
        src = f.read()
    assert set(re.findall(r"\blib\.(adfl_\w+)", src)) == set(_abi.FLATTEN_EXPORTS)
    assert "_abi.declare(lib, _abi.FLATTEN_EXPORTS)" in src


def test_the_library_exports_them():
    import subprocess

    from alphadia_amd import runtime

    nm = subprocess.run(["nm", "-D", "--defined-only", runtime.LIB_PATH], capture_output=True, text=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if line.strip()}
    assert set(_abi.FLATTEN_EXPORTS) <= exported
    for name in _abi.FLATTEN_EXPORTS:
        assert getattr(runtime.lib, name).argtypes == _abi.FLATTEN_EXPORTS[name][1]
