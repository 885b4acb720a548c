"""The C ABI of the grouped volume solve (include/msiren.h; no GPU needed): msiren_align_volume_solve_group(_dev) are exported by the built library,
declared in the header and bound in mri_inr_amd/_lib.py with matching argument kinds, the options struct has the header's size and refuses another
struct_size, null arguments are refused -- pure additions under ABI 9."""
import ctypes as C
import os
import re

import pytest

from mri_inr_amd import _lib

SOLVE = ["p", "p", "i64", "i32", "i32", "p", "i64", "i32", "i32", "opts", "p", "i64", "p", "p", "p", "p", "p", "p", "p", "p", "p", "p"]
SYMBOLS = {"msiren_align_volume_solve_group": SOLVE, "msiren_align_volume_solve_group_dev": SOLVE}
TAIL = ["const int32_t", "int64_t n_groups", "const double", "const double", "const float", "const float", "float", "float", "double", "double", "double", "double"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def opts(struct_size=None, iterations=4, est=1):
    return _lib.AlignVolumeSolveGroupOpts(C.sizeof(_lib.AlignVolumeSolveGroupOpts) if struct_size is None else struct_size, iterations, est, 0, 1e-3, 0.1, 10.0, 1e-9, 1e9, 4.0)


def test_abi_version_is_still_9_and_the_history_names_the_calls(lib):
    assert lib.msiren_abi_version() == 9 and _lib.ABI_VERSION == 9
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+MSIREN_ABI_VERSION\s+9\b", header)
    history = header[header.index("/* 9: msiren_resample_volume"):header.index(" * 8:")]
    assert "msiren_align_volume_solve_group(_dev)" in history and "msiren_align_volume_solve_group_opts" in history
    assert "msiren_align_volume_solve_w(_dev)" in history and "msiren_align_volume(_dev)" in history  # the earlier additions under 9 are still named


def test_options_struct_is_the_headers():
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*msiren_align_volume_solve_group_opts;", header)
    assert m, "msiren_align_volume_solve_group_opts is not declared in include/msiren.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), typ) for n in names.split(",")]
    want = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double}
    assert [(n, want[t]) for n, t in fields] == list(_lib.AlignVolumeSolveGroupOpts._fields_)
    assert [n for n, _ in fields] == ["struct_size", "iterations", "intensity_mode", "reserved", "damping", "down", "up", "lam_min", "lam_max", "spacing"]
    assert C.sizeof(_lib.AlignVolumeSolveGroupOpts) == sum(C.sizeof(want[t]) for _, t in fields) == 64  # (no padding: four 4-byte fields, then doubles)


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(lib, name):
    assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"MSIREN_API\s+int\s+" + name + r"\s*\(([^;]*)\);", header)
    assert m, f"{name} is not declared in include/msiren.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    kinds = ["opts" if "msiren_align_volume_solve_group_opts*" in a else "p" if "*" in a or a.startswith("msiren_handle") else "i64" if a.startswith("int64_t") else "i32" for a in args]
    assert kinds == SYMBOLS[name], args
    assert [a if a.startswith("int64_t") else a.split("*")[0].strip() for a in args[-len(TAIL):]] == TAIL, args
    restype, argtypes = _lib.PROTOTYPES[name]
    want = {"p": C.c_void_p, "i64": C.c_int64, "i32": C.c_int32, "opts": C.POINTER(_lib.AlignVolumeSolveGroupOpts)}
    assert restype is C.c_int and argtypes == [want[k] for k in kinds]
    assert getattr(lib, name).argtypes == argtypes


def test_null_handle_is_refused(lib):
    o = opts()
    for name, kinds in SYMBOLS.items():
        args = [C.byref(o) if k == "opts" else None if k == "p" else 4 for k in kinds]
        assert getattr(lib, name)(*args) == _lib.E_INVALID
        assert "null handle" in _lib.last_error()


def test_the_python_interface_has_the_method_and_the_helpers():
    from mri_inr_amd import ModulatedSiren, align_group as ag, align_volume as av

    assert callable(getattr(ModulatedSiren, "align_volume_solve_group"))
    assert ag.SolveOptionsG()._fields[-1] == "intensity_mode" and ag.SolveOptionsG().intensity_mode == av.ESTIMATE and ag.SolveOptionsG().iterations == 12
    assert ag.SolveResultG._fields == ("maps", "intensity", "count", "wsum", "cost", "rotation", "shift", "accepted", "mean_first", "mean_best", "damping", "flags", "trace")
    for name in ("lm_init_g", "lm_step_g", "solve_on_host_g", "group_offsets", "report_g", "solve_result_g"):
        assert hasattr(ag, name), name
    assert ag.group_offsets([3, 1, 2], 6) == [0, 3, 4, 6] == ag.group_offsets([0, 3, 4, 6], 6)
