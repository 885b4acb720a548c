"""The C ABI of the stack alignment calls (include/msiren.h; no GPU needed): msiren_align_stack_r(_dev) and msiren_align_stack_solve_group_r(_dev) are
exported by the built library, declared in the header and bound in mri_inr_amd/_lib.py with matching argument kinds -- msiren_align_volume_r's and
msiren_align_volume_solve_group_r's lists with the stack in the place of the images, the same options struct; null handles are refused; a C program
that includes the header sees the symbols with the documented prototypes, links against the library and is refused in the same way -- pure additions
under ABI 9."""
import ctypes as C
import os
import re
import shutil
import subprocess
import textwrap

import pytest

from mri_inr_amd import _lib

COST = ["p", "p", "i64", "i32", "i32", "p", "i64", "i32", "i32", "p", "p", "p", "p", "p", "p", "p", "p"]
SOLVE = ["p", "p", "i64", "i32", "i32", "p", "i64", "i32", "i32", "opts", "p", "i64", "p", "p", "p", "p", "p", "p", "p", "p", "p", "p", "p"]
SYMBOLS = {"msiren_align_stack_r": COST, "msiren_align_stack_r_dev": COST, "msiren_align_stack_solve_group_r": SOLVE, "msiren_align_stack_solve_group_r_dev": SOLVE}
TWINS = {"msiren_align_stack_r": "msiren_align_volume_r", "msiren_align_stack_solve_group_r": "msiren_align_volume_solve_group_r"}


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
    assert "msiren_align_stack_r(_dev)" in history and "msiren_align_stack_solve_group_r(_dev)" in history
    assert "msiren_align_volume_r(_dev)" in history and "msiren_solve_volume_r(_dev)" in history  # the earlier additions under 9 are still named


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(lib, name):
    assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    args = declared(name)
    kinds = ["opts" if "msiren_align_volume_solve_group_opts*" in a else "p" if "*" in a or a.startswith("msiren_handle") else "i64" if a.startswith("int64_t") else "i32" for a in args]
    assert kinds == SYMBOLS[name], args
    restype, argtypes = _lib.PROTOTYPES[name]
    want = {"p": C.c_void_p, "i64": C.c_int64, "i32": C.c_int32, "opts": C.POINTER(_lib.AlignVolumeSolveGroupOpts)}
    assert restype is C.c_int and argtypes == [want[k] for k in kinds]
    assert getattr(lib, name).argtypes == argtypes


@pytest.mark.parametrize("name", sorted(TWINS))
@pytest.mark.parametrize("suffix", ["", "_dev"])
def test_the_argument_list_is_the_volume_calls_with_the_stack_for_the_images(name, suffix):
    mine, twin = declared(name + suffix), declared(TWINS[name] + suffix)
    types = lambda args: [a if a.startswith("int") else a.split("*")[0].strip() + "*" for a in args]  # noqa: E731
    assert types(mine) == types(twin)
    assert "stack" in mine[1] and "images" in twin[1] and [a.split()[-1] for a in mine[2:]] == [a.split()[-1] for a in twin[2:]]  # the same names behind the first array


def test_null_handle_is_refused(lib):
    o = _lib.AlignVolumeSolveGroupOpts(64, 4, 1, 0, 1e-3, 0.1, 10.0, 1e-9, 1e9, 4.0)
    for name, kinds in SYMBOLS.items():
        args = [C.byref(o) if k == "opts" else None if k == "p" else 4 for k in kinds]
        assert getattr(lib, name)(*args) == _lib.E_INVALID
        assert "null handle" in _lib.last_error()


PROG = textwrap.dedent(r"""
    #include <stdio.h>
    #include <string.h>
    #include "msiren.h"

    /* the prototypes a consumer writes from the documentation: an assignment of another type does not compile with -Werror */
    typedef int (*cost_fn)(msiren_handle, const float*, int64_t, int32_t, int32_t, const float*, int64_t, int32_t, int32_t, const float*, const float*, const float*,
                           const double*, double*, float*, float*, float*);
    typedef int (*solve_fn)(msiren_handle, const float*, int64_t, int32_t, int32_t, const float*, int64_t, int32_t, int32_t, const msiren_align_volume_solve_group_opts*,
                            const int32_t*, int64_t, const double*, const double*, const float*, const float*, const double*, float*, float*, double*, double*, double*,
                            double*);

    int main(void) {
        cost_fn cost[2] = {msiren_align_stack_r, msiren_align_stack_r_dev};
        solve_fn solve[2] = {msiren_align_stack_solve_group_r, msiren_align_stack_solve_group_r_dev};
        msiren_align_volume_solve_group_opts o;
        double scale[2] = {0.01, 0.01};
        int k;
        memset(&o, 0, sizeof o);
        o.struct_size = (uint32_t)sizeof o, o.iterations = 4, o.intensity_mode = 1, o.damping = 1e-3, o.down = 0.1, o.up = 10.0, o.lam_min = 1e-9, o.lam_max = 1e9, o.spacing = 4.0;
        if (sizeof o != 64 || MSIREN_ABI_VERSION != 9 || msiren_abi_version() != 9) return 1;
        for (k = 0; k < 2; ++k) {
            if (cost[k](NULL, NULL, 4, 21, 27, NULL, 2, 4, 4, NULL, NULL, NULL, scale, NULL, NULL, NULL, NULL) != MSIREN_E_INVALID) return 2;
            if (!strstr(msiren_last_error(), "null handle")) return 3;
            if (solve[k](NULL, NULL, 4, 21, 27, NULL, 2, 4, 4, &o, NULL, 1, NULL, NULL, NULL, NULL, scale, NULL, NULL, NULL, NULL, NULL, NULL) != MSIREN_E_INVALID) return 4;
            if (!strstr(msiren_last_error(), "null handle")) return 5;
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


def test_the_python_interface_has_the_methods_and_the_helpers():
    from mri_inr_amd import ModulatedSiren, align_stack as ast

    assert callable(getattr(ModulatedSiren, "align_stack_cost")) and callable(getattr(ModulatedSiren, "align_stack_solve"))
    for name in ("read_stack", "pixel_terms", "chunk_sums", "cost_on_host", "result_on_host", "solve_on_host_s"):
        assert hasattr(ast, name), name
