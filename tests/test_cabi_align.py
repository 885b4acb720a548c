"""The C ABI of the align call (include/msiren.h; no GPU needed): msiren_align_slices(_dev) are exported by the built library, declared in
the header and bound in mri_inr_amd/_lib.py with the issue's argument list -- pure additions under ABI 9."""
import ctypes as C
import os
import re

import pytest

from mri_inr_amd import _lib

SYMBOLS = ["msiren_align_slices", "msiren_align_slices_dev"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_abi_version_is_still_9(lib):
    assert lib.msiren_abi_version() == 9 and _lib.ABI_VERSION == 9
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+MSIREN_ABI_VERSION\s+9\b", header) and re.search(r"/\* 9: msiren_resample_volume", header)
    history = header[header.index("/* 9:"):header.index(" * 8:")]
    assert "msiren_align_slices" in history


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported_declared_and_bound(lib, name):
    assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"MSIREN_API\s+int\s+" + name + r"\s*\(([^;]*)\);", header)
    assert m, f"{name} is not declared in include/msiren.h"
    args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    kinds = ["p" if "*" in a or a.startswith("msiren_handle") else "i64" if a.startswith("int64_t") else "i32" for a in args]
    assert kinds == ["p", "p", "i64", "i32", "i32", "p", "i32", "i32", "p", "p", "p", "p"], args
    assert re.search(r"double\*\s+sums_", m.group(1))
    restype, argtypes = _lib.PROTOTYPES[name]
    want = {"p": C.c_void_p, "i64": C.c_int64, "i32": C.c_int32}
    assert restype is C.c_int and argtypes == [want[k] for k in kinds]
    assert getattr(lib, name).argtypes == argtypes


def test_null_handle_is_refused(lib):
    for name in SYMBOLS:
        assert getattr(lib, name)(None, None, 1, 40, 40, None, 4, 4, None, None, None, None) == _lib.E_INVALID
