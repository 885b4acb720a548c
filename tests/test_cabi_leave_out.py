"""The C ABI of the leave-one-out call (include/msiren.h; no GPU needed): msiren_leave_out_targets(_dev) are exported by the built library, declared in
the header and bound in mri_inr_amd/_lib.py with matching argument kinds; they reuse msiren_fuse_opts; MSIREN_LEAVE_OUT_FLOOR is 2^-20 on both sides;
null handles are refused; a C program that includes the header sees the symbols with the documented prototypes, links against the library and is
refused in the same way -- pure additions under ABI 9."""
import ctypes as C
import os
import re
import shutil
import subprocess
import textwrap

import pytest

from mri_inr_amd import _lib

ARGS = ["p", "p", "i64", "i32", "i32", "p", "p", "p", "opts", "p", "i64", "i64", "i32", "i32", "p", "p", "p", "p", "p", "p", "p"]
SYMBOLS = {"msiren_leave_out_targets": ARGS, "msiren_leave_out_targets_dev": ARGS}


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


def test_abi_version_is_still_9_and_the_history_names_the_call(lib):
    assert lib.msiren_abi_version() == 9 and _lib.ABI_VERSION == 9
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+MSIREN_ABI_VERSION\s+9\b", header)
    history = header[header.index("/* 9: msiren_resample_volume"):header.index(" * 8:")]
    assert "msiren_leave_out_targets(_dev)" in history
    assert "msiren_residual_scale(_dev)" in history and "msiren_fuse_targets(_dev)" in history  # the earlier additions under 9 are still named


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(lib, name):
    assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    args = declared(name)
    kinds = ["opts" if "msiren_fuse_opts*" in a else "p" if "*" in a or a.startswith("msiren_handle") else "i64" if a.startswith("int64_t") else "i32" for a in args]
    assert kinds == SYMBOLS[name], args
    restype, argtypes = _lib.PROTOTYPES[name]
    want = {"p": C.c_void_p, "i64": C.c_int64, "i32": C.c_int32, "opts": C.POINTER(_lib.FuseOpts)}
    assert restype is C.c_int and argtypes == [want[k] for k in kinds]
    assert getattr(lib, name).argtypes == argtypes


def test_the_two_forms_take_the_same_arguments():
    host, dev = declared("msiren_leave_out_targets"), declared("msiren_leave_out_targets_dev")
    types = lambda args: [a.split("*")[0].strip() + "*" if "*" in a else a for a in args]  # noqa: E731
    assert types(host) == types(dev)
    assert [a.split()[-1].replace("_host", "") for a in host] == [a.split()[-1].replace("_dev", "") for a in dev]
    assert host[9].endswith("group_start") and dev[9].endswith("group_start") and host[8].endswith("opts") and dev[8].endswith("opts")  # host arrays in both forms
    assert [a.split()[-1].replace("_host", "") for a in host[14:]] == ["simulated", "coverage", "residual", "stats", "flags", "volume", "volume_coverage"]


def test_the_floor_is_a_power_of_two_on_both_sides():
    from mri_inr_amd import leave_out as lo

    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"#define\s+MSIREN_LEAVE_OUT_FLOOR\s+\(1\.0 / (\d+)\.0\)", header)
    assert m and int(m.group(1)) == 1 << 20 and lo.LEAVE_OUT_FLOOR == 2.0 ** -20


def test_null_handle_is_refused(lib):
    o = _lib.FuseOpts(32, 0, 4.0, 4.0, 0.0)
    for name, kinds in SYMBOLS.items():
        args = [C.byref(o) if k == "opts" else None if k == "p" else 4 for k in kinds]
        assert getattr(lib, name)(*args) == _lib.E_INVALID
        assert "null handle" in _lib.last_error()


PROG = textwrap.dedent(r"""
    #include <stdio.h>
    #include <string.h>
    #include "msiren.h"

    /* the prototype a consumer writes from the documentation: an assignment of another type does not compile with -Werror */
    typedef int (*leave_out_fn)(msiren_handle, const float*, int64_t, int32_t, int32_t, const float*, const float*, const float*, const msiren_fuse_opts*, const int32_t*,
                                int64_t, int64_t, int32_t, int32_t, float*, float*, float*, double*, int32_t*, float*, float*);

    int main(void) {
        leave_out_fn fn[2] = {msiren_leave_out_targets, msiren_leave_out_targets_dev};
        msiren_fuse_opts o;
        int32_t groups[2] = {0, 2};
        float sim[32];
        int k;
        memset(&o, 0, sizeof o);
        o.struct_size = (int32_t)sizeof o, o.spacing = 4.0, o.thickness = 4.0, o.min_coverage = 0.0;
        if (sizeof o != 32 || MSIREN_ABI_VERSION != 9 || msiren_abi_version() != 9) return 1;
        if (MSIREN_LEAVE_OUT_FLOOR * 1048576.0 != 1.0) return 4;
        for (k = 0; k < 2; ++k) {
            if (fn[k](NULL, NULL, 2, 4, 4, NULL, NULL, NULL, &o, groups, 1, 3, 8, 8, sim, NULL, NULL, NULL, NULL, NULL, NULL) != MSIREN_E_INVALID) return 2;
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
    from mri_inr_amd import ModulatedSiren, leave_out as lo

    assert callable(getattr(ModulatedSiren, "leave_out_targets"))
    assert lo.LeaveOutResult._fields == ("simulated", "coverage", "residual", "stats", "flags", "volume", "volume_coverage")
    for name in ("leave_out_on_host", "own_terms", "left_out_sums", "voxel_takes", "left_out_value", "members_left_out", "LEAVE_OUT_FLOOR", "leave_out_chain_on_host"):
        assert hasattr(lo, name), name
