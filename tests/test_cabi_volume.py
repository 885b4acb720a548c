"""The C ABI of the volume calls (include/msiren.h, ABI 9; no GPU needed): msiren_resample_volume* are exported by the built library,
declared in the header and bound in mri_inr_amd/_lib.py with the argument lists of their msiren_resample_slices* counterparts."""
import os
import re

import pytest

from mri_inr_amd import _lib

SYMBOLS = ["msiren_resample_volume" + s for s in ("", "_dev", "_native", "_native_dev", "_grad", "_grad_dev")]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_abi_version_is_9(lib):
    assert lib.msiren_abi_version() == 9 and _lib.ABI_VERSION == 9
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+MSIREN_ABI_VERSION\s+9\b", header) and re.search(r"/\* 9: msiren_resample_volume", header)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported_declared_and_bound(lib, name):
    assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"MSIREN_API\s+int\s+" + name + r"\s*\(", header), f"{name} is not declared in include/msiren.h"
    restype, argtypes = _lib.PROTOTYPES[name]
    twin = _lib.PROTOTYPES[name.replace("resample_volume", "resample_slices")]
    assert (restype, argtypes) == twin and len(argtypes) == (9 if "grad" in name else 8)
    assert getattr(lib, name).argtypes == argtypes
