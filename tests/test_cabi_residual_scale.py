"""The C ABI of the robust-scale call (include/msiren.h; no GPU needed): msiren_residual_scale(_dev) are exported by the built library, declared in the
header and bound in mri_inr_amd/_lib.py with matching argument kinds; msiren_scale_opts has 32 bytes with the documented fields on both sides; null
handles are refused; a C program that includes the header sees the symbols with the documented prototypes, links against the library and is refused in
the same way -- pure additions under ABI 9."""
import ctypes as C
import os
import re
import shutil
import subprocess
import textwrap

import pytest

from mri_inr_amd import _lib

ARGS = ["p", "p", "p", "p", "p", "i64", "i32", "i32", "opts", "p", "i64", "p", "p"]
SYMBOLS = {"msiren_residual_scale": ARGS, "msiren_residual_scale_dev": ARGS}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def declared(name):
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"MSIREN_API\s+int\s+" + name + r"\s*\(([^;]*)\);", header)
    assert m, f"{name} is not declared in include/msiren.h"
    return [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_abi_version_is_still_9_and_the_history_names_the_calls(lib):
    assert lib.msiren_abi_version() == 9 and _lib.ABI_VERSION == 9
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+MSIREN_ABI_VERSION\s+9\b", header)
    history = header[header.index("/* 9: msiren_resample_volume"):header.index(" * 8:")]
    assert "msiren_residual_scale(_dev)" in history and "msiren_scale_opts" in history
    assert "msiren_align_stack_r(_dev)" in history and "msiren_solve_volume_r(_dev)" in history  # the earlier additions under 9 are still named


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(lib, name):
    assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    args = declared(name)
    kinds = ["opts" if "msiren_scale_opts*" in a else "p" if "*" in a or a.startswith("msiren_handle") else "i64" if a.startswith("int64_t") else "i32" for a in args]
    assert kinds == SYMBOLS[name], args
    restype, argtypes = _lib.PROTOTYPES[name]
    want = {"p": C.c_void_p, "i64": C.c_int64, "i32": C.c_int32, "opts": C.POINTER(_lib.ScaleOpts)}
    assert restype is C.c_int and argtypes == [want[k] for k in kinds]
    assert getattr(lib, name).argtypes == argtypes


def test_the_two_forms_take_the_same_arguments():
    host, dev = declared("msiren_residual_scale"), declared("msiren_residual_scale_dev")
    types = lambda args: [a if a.startswith("int") else a.split("*")[0].strip() + "*" for a in args]  # noqa: E731
    assert types(host) == types(dev)
    assert [a.split()[-1].replace("_host", "") for a in host] == [a.split()[-1].replace("_dev", "") for a in dev]
    assert host[9].endswith("group_start") and dev[9].endswith("group_start")  # a host array in both forms


def test_the_options_have_32_bytes_and_the_documented_fields():
    assert C.sizeof(_lib.ScaleOpts) == 32
    assert [(n, t) for n, t in _lib.ScaleOpts._fields_] == [("struct_size", C.c_int32), ("centre", C.c_int32), ("quantile", C.c_double), ("tune", C.c_double),
                                                            ("floor", C.c_double)]
    header = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct \{([^}]*)\} msiren_scale_opts;", header).group(1)
    fields = re.findall(r"\b(int32_t|double)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [("int32_t", "struct_size"), ("int32_t", "centre"), ("double", "quantile"), ("double", "tune"), ("double", "floor")]
    o = _lib.ScaleOpts(32, 1, 0.5, 8.9, 0.25)
    assert bytes(o)[:8] == (32).to_bytes(4, "little") + (1).to_bytes(4, "little")


def test_null_handle_is_refused(lib):
    o = _lib.ScaleOpts(32, 1, 0.5, 8.9, 0.0)
    for name, kinds in SYMBOLS.items():
        args = [C.byref(o) if k == "opts" else None if k == "p" else 4 for k in kinds]
        assert getattr(lib, name)(*args) == _lib.E_INVALID
        assert "null handle" in _lib.last_error()


PROG = textwrap.dedent(r"""
    #include <stdio.h>
    #include <string.h>
    #include "msiren.h"

    /* the prototype a consumer writes from the documentation: an assignment of another type does not compile with -Werror */
    typedef int (*scale_fn)(msiren_handle, const float*, const float*, const float*, const float*, int64_t, int32_t, int32_t, const msiren_scale_opts*, const int32_t*,
                            int64_t, double*, double*);

    int main(void) {
        scale_fn fn[2] = {msiren_residual_scale, msiren_residual_scale_dev};
        msiren_scale_opts o;
        int32_t groups[2] = {0, 2};
        double scale[2];
        int k;
        memset(&o, 0, sizeof o);
        o.struct_size = (int32_t)sizeof o, o.centre = 1, o.quantile = 0.5, o.tune = 8.9, o.floor = 0.0;
        if (sizeof o != 32 || MSIREN_ABI_VERSION != 9 || msiren_abi_version() != 9) return 1;
        for (k = 0; k < 2; ++k) {
            if (fn[k](NULL, NULL, NULL, NULL, NULL, 2, 4, 4, &o, groups, 1, scale, NULL) != MSIREN_E_INVALID) return 2;
            if (!strstr(msiren_last_error(), "null handle")) return 3;
        }
        puts("ok");
        return 0;
    }
""")


def test_a_c_consumer_sees_links_and_calls_the_new_symbols(lib, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no C compiler"
    src, exe = tmp_path / "consumer.c", tmp_path / "consumer"
    src.write_text(PROG)
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(os.path.abspath(_lib.HEADER_PATH)), str(src), "-o", str(exe), "-L", libdir, "-lmsiren",
                    "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.returncode, res.stderr)


def test_the_python_interface_has_the_method_and_the_helpers():
    from mri_inr_amd import ModulatedSiren, residual_scale as rs

    assert callable(getattr(ModulatedSiren, "residual_scale")) and rs.MAD_TO_SIGMA == 1.482602218505602
    for name in ("residual_scale_on_host", "ResidualScaleResult", "sort_key", "rank", "pixel_residual", "pixel_counts", "deviation", "scale_of"):
        assert hasattr(rs, name), name
