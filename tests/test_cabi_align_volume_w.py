"""The C ABI of the weighted volume align calls (include/msiren.h; no GPU needed): msiren_align_volume_w(_dev) and msiren_align_volume_solve_w(_dev)
are exported by the built library, declared in the header and bound in mri_inr_amd/_lib.py with matching argument kinds, the options struct has
the header's size -- pure additions under ABI 9."""
import ctypes as C
import os
import re

import pytest

from mri_inr_amd import _lib

COST = ["p", "p", "i64", "i32", "i32", "p", "i64", "i32", "i32", "p", "p", "p", "p", "p", "p"]
SOLVE = ["p", "p", "i64", "i32", "i32", "p", "i64", "i32", "i32", "opts", "p", "p", "p", "p", "p", "p", "p", "p", "p", "p"]
SYMBOLS = {"msiren_align_volume_w": COST, "msiren_align_volume_w_dev": COST, "msiren_align_volume_solve_w": SOLVE, "msiren_align_volume_solve_w_dev": SOLVE}
TAILS = {"msiren_align_volume_w": ["const float", "const float", "const float", "double", "float", "float"],
         "msiren_align_volume_solve_w": ["const float", "const double", "const double", "const float", "const float", "float", "float", "double", "double", "double"]}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_abi_version_is_still_9_and_the_history_names_the_calls(lib):
    assert lib.msiren_abi_version() == 9 and _lib.ABI_VERSION == 9
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+MSIREN_ABI_VERSION\s+9\b", header)
    history = header[header.index("/* 9: msiren_resample_volume"):header.index(" * 8:")]
    assert "msiren_align_volume_w(_dev)" in history and "msiren_align_volume_solve_w(_dev)" in history and "msiren_align_volume_solve_w_opts" in history
    assert "msiren_align_volume(_dev)" in history and "msiren_align_solve_w_opts" in history  # the earlier additions under 9 are still named


def test_options_struct_is_the_headers():
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*msiren_align_volume_solve_w_opts;", header)
    assert m, "msiren_align_volume_solve_w_opts is not declared in include/msiren.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), typ) for n in names.split(",")]
    want = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double}
    assert [(n, want[t]) for n, t in fields] == list(_lib.AlignVolumeSolveWOpts._fields_)
    size = sum(C.sizeof(want[t]) for _, t in fields)  # (no padding: four 4-byte fields, then doubles)
    assert C.sizeof(_lib.AlignVolumeSolveWOpts) == size == 64 == C.sizeof(_lib.AlignVolumeSolveOpts)
    # msiren_align_volume_solve_opts' fields, with intensity_mode in the place of reserved
    old = [(n, t) for n, t in _lib.AlignVolumeSolveOpts._fields_]
    assert list(_lib.AlignVolumeSolveWOpts._fields_) == [("intensity_mode", t) if n == "reserved" else (n, t) for n, t in old]
    assert [getattr(_lib.AlignVolumeSolveWOpts, n).offset for n, _ in old if n != "reserved"] == [getattr(_lib.AlignVolumeSolveOpts, n).offset for n, _ in old if n != "reserved"]


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(lib, name):
    assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"MSIREN_API\s+int\s+" + name + r"\s*\(([^;]*)\);", header)
    assert m, f"{name} is not declared in include/msiren.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    kinds = ["opts" if "msiren_align_volume_solve_w_opts*" in a else "p" if "*" in a or a.startswith("msiren_handle") else "i64" if a.startswith("int64_t") else "i32" for a in args]
    assert kinds == SYMBOLS[name], args
    tail = TAILS[name[:-4] if name.endswith("_dev") else name]
    assert [a.split("*")[0].strip() for a in args[-len(tail):]] == tail, args
    restype, argtypes = _lib.PROTOTYPES[name]
    want = {"p": C.c_void_p, "i64": C.c_int64, "i32": C.c_int32, "opts": C.POINTER(_lib.AlignVolumeSolveWOpts)}
    assert restype is C.c_int and argtypes == [want[k] for k in kinds]
    assert getattr(lib, name).argtypes == argtypes


def test_null_handle_is_refused(lib):
    o = _lib.AlignVolumeSolveWOpts(C.sizeof(_lib.AlignVolumeSolveWOpts), 0, 4, 1, 1e-3, 0.1, 10.0, 1e-9, 1e9, 4.0)
    for name, kinds in SYMBOLS.items():
        args = [C.byref(o) if k == "opts" else None if k == "p" else 4 for k in kinds]
        assert getattr(lib, name)(*args) == _lib.E_INVALID
        assert "null handle" in _lib.last_error()


def test_the_python_interface_has_the_three_methods_and_the_helpers():
    from mri_inr_amd import ModulatedSiren, align_volume as av

    for name in ("align_volume_cost_w", "align_volume_solve_w", "align_volume_solve_rigid_w"):
        assert callable(getattr(ModulatedSiren, name))
    assert av.SUMS_VW == 80 and av.SolveOptionsVW()._fields[-1] == "intensity_mode" and av.SolveOptionsVW().intensity_mode == av.ESTIMATE
    for name in ("AlignResultVW", "SolveResultVW", "unpack_vw", "gauss_newton_step_vw", "lm_init_vw", "lm_step_vw", "solve_on_host_vw"):
        assert hasattr(av, name), name
