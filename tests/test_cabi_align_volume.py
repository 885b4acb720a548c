"""The C ABI of the volume align calls (include/msiren.h; no GPU needed): msiren_align_volume(_dev) and msiren_align_volume_solve(_dev) are
exported by the built library, declared in the header and bound in mri_inr_amd/_lib.py with matching argument kinds, the options struct has
the header's size -- pure additions under ABI 9."""
import ctypes as C
import os
import re

import pytest

from mri_inr_amd import _lib

COST = ["p", "p", "i64", "i32", "i32", "p", "i64", "i32", "i32", "p", "p", "p", "p"]
SOLVE = ["p", "p", "i64", "i32", "i32", "p", "i64", "i32", "i32", "opts", "p", "p", "p", "p", "p", "p", "p"]
SYMBOLS = {"msiren_align_volume": COST, "msiren_align_volume_dev": COST, "msiren_align_volume_solve": SOLVE, "msiren_align_volume_solve_dev": SOLVE}
TAILS = {"msiren_align_volume": ["const float", "double", "float", "float"],
         "msiren_align_volume_solve": ["const float", "const double", "const double", "float", "double", "double", "double"]}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_abi_version_is_still_9_and_the_history_names_the_calls(lib):
    assert lib.msiren_abi_version() == 9 and _lib.ABI_VERSION == 9
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+MSIREN_ABI_VERSION\s+9\b", header)
    history = header[header.index("/* 9:"):header.index(" * 8:")]
    assert "msiren_align_volume(_dev)" in history and "msiren_align_volume_solve(_dev)" in history and "msiren_align_volume_solve_opts" in history


def test_options_struct_is_the_headers():
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*msiren_align_volume_solve_opts;", header)
    assert m, "msiren_align_volume_solve_opts is not declared in include/msiren.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), typ) for n in names.split(",")]
    want = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double}
    assert [(n, want[t]) for n, t in fields] == list(_lib.AlignVolumeSolveOpts._fields_)
    size = sum(C.sizeof(want[t]) for _, t in fields)  # (no padding: four 4-byte fields, then doubles)
    assert C.sizeof(_lib.AlignVolumeSolveOpts) == size == 64
    # msiren_align_solve_opts' fields, with the spacing in the place of its centre
    assert [n for n, _ in _lib.AlignVolumeSolveOpts._fields_] == [n for n, _ in _lib.AlignSolveOpts._fields_][:-2] + ["spacing"]


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(lib, name):
    assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"MSIREN_API\s+int\s+" + name + r"\s*\(([^;]*)\);", header)
    assert m, f"{name} is not declared in include/msiren.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    kinds = ["opts" if "msiren_align_volume_solve_opts*" in a else "p" if "*" in a or a.startswith("msiren_handle") else "i64" if a.startswith("int64_t") else "i32" for a in args]
    assert kinds == SYMBOLS[name], args
    tail = TAILS[name[:-4] if name.endswith("_dev") else name]
    assert [a.split("*")[0].strip() for a in args[-len(tail):]] == tail, args
    restype, argtypes = _lib.PROTOTYPES[name]
    want = {"p": C.c_void_p, "i64": C.c_int64, "i32": C.c_int32, "opts": C.POINTER(_lib.AlignVolumeSolveOpts)}
    assert restype is C.c_int and argtypes == [want[k] for k in kinds]
    assert getattr(lib, name).argtypes == argtypes


def test_null_handle_is_refused(lib):
    o = _lib.AlignVolumeSolveOpts(C.sizeof(_lib.AlignVolumeSolveOpts), 0, 4, 0, 1e-3, 0.1, 10.0, 1e-9, 1e9, 4.0)
    for name, kinds in SYMBOLS.items():
        args = [C.byref(o) if k == "opts" else None if k == "p" else 4 for k in kinds]
        assert getattr(lib, name)(*args) == _lib.E_INVALID
        assert "null handle" in _lib.last_error()
