"""The C ABI of msiren_solve_volume(_dev) (include/msiren.h; no GPU needed): exported by the built library, declared in the header and bound in
mri_inr_amd/_lib.py with matching argument kinds; null handles are refused; a C program that includes the header sees the symbols with the documented
prototypes, links against the library and is refused in the same way -- pure additions under ABI 9, msiren_solve_opts of 40 bytes."""
import ctypes as C
import os
import re
import shutil
import subprocess
import textwrap

import pytest

from mri_inr_amd import _lib

KINDS = ["p", "p", "i64", "i32", "i32", "p", "p", "p", "opts", "i64", "i32", "i32", "p", "p", "p", "p", "p", "p"]
SYMBOLS = ("msiren_solve_volume", "msiren_solve_volume_dev")
TYPES = ["msiren_handle h", "const float", "int64_t m_targets", "int32_t th", "int32_t tw", "const float", "const float", "const float", "const msiren_solve_opts",
         "int64_t n_slices", "int32_t height", "int32_t width", "const float", "float", "float", "double", "int32_t", "int32_t"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_abi_version_is_still_9_and_the_history_names_the_call(lib):
    assert lib.msiren_abi_version() == 9 and _lib.ABI_VERSION == 9
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+MSIREN_ABI_VERSION\s+9\b", header)
    history = header[header.index("/* 9: msiren_resample_volume"):header.index(" * 8:")]
    assert "msiren_solve_volume(_dev)" in history and "msiren_solve_opts" in history
    assert "msiren_project_volume(_dev)" in history and "msiren_fuse_targets(_dev)" in history  # the earlier additions under 9 are still named


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported_declared_and_bound(lib, name):
    assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"MSIREN_API\s+int\s+" + name + r"\s*\(([^;]*)\);", header)
    assert m, f"{name} is not declared in include/msiren.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    kinds = ["opts" if "msiren_solve_opts*" in a else "p" if "*" in a or a.startswith("msiren_handle") else "i64" if a.startswith("int64_t") else "i32" for a in args]
    assert kinds == KINDS, args
    assert [a if "*" not in a else a.split("*")[0].strip() for a in args] == TYPES, args
    restype, argtypes = _lib.PROTOTYPES[name]
    want = {"p": C.c_void_p, "i64": C.c_int64, "i32": C.c_int32, "opts": C.POINTER(_lib.SolveOpts)}
    assert restype is C.c_int and argtypes == [want[k] for k in kinds]
    assert getattr(lib, name).argtypes == argtypes


def test_the_options_struct_has_40_bytes_and_the_fusions_is_unchanged():
    header = open(_lib.HEADER_PATH).read()
    (body,) = re.findall(r"typedef struct \{([^}]*)\}\s*msiren_solve_opts;", header)
    fields = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split()
    assert " ".join(fields) == "int32_t struct_size; int32_t iterations; double spacing, thickness, min_coverage, lambda;"
    assert C.sizeof(_lib.SolveOpts) == 40 and [f[0] for f in _lib.SolveOpts._fields_] == ["struct_size", "iterations", "spacing", "thickness", "min_coverage", "lam"]
    assert _lib.SolveOpts.lam.offset == 32
    assert len(re.findall(r"typedef struct \{([^}]*)\}\s*msiren_fuse_opts;", header)) == 1 and C.sizeof(_lib.FuseOpts) == 32


def test_null_handle_is_refused(lib):
    o = _lib.SolveOpts(40, 1, 4.0, 4.0, 0.0, 0.0)
    for name in SYMBOLS:
        args = [C.byref(o) if k == "opts" else None if k == "p" else 4 for k in KINDS]
        assert getattr(lib, name)(*args) == _lib.E_INVALID
        assert "null handle" in _lib.last_error()


PROG = textwrap.dedent(r"""
    #include <stddef.h>
    #include <stdio.h>
    #include <string.h>
    #include "msiren.h"

    /* the prototype a consumer writes from the documentation: an assignment of another type does not compile with -Werror */
    typedef int (*solve_fn)(msiren_handle, const float*, int64_t, int32_t, int32_t, const float*, const float*, const float*, const msiren_solve_opts*, int64_t, int32_t, int32_t,
                            const float*, float*, float*, double*, int32_t*, int32_t*);

    int main(void) {
        solve_fn solve[2] = {msiren_solve_volume, msiren_solve_volume_dev};
        msiren_solve_opts o;
        int k;
        memset(&o, 0, sizeof o);
        o.struct_size = (int32_t)sizeof o, o.iterations = 3, o.spacing = 4.0, o.thickness = 4.0, o.min_coverage = 0.0, o.lambda = 0.01;
        if (sizeof o != 40 || offsetof(msiren_solve_opts, lambda) != 32 || MSIREN_ABI_VERSION != 9 || msiren_abi_version() != 9) return 1;
        for (k = 0; k < 2; ++k) {
            if (solve[k](NULL, NULL, 2, 4, 4, NULL, NULL, NULL, &o, 4, 40, 40, NULL, NULL, NULL, NULL, NULL, NULL) != MSIREN_E_INVALID) return 3;
            if (!strstr(msiren_last_error(), "null handle")) return 4;
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
    import inspect

    from mri_inr_amd import ModulatedSiren
    from mri_inr_amd import solve_volume as sv

    sig = inspect.signature(ModulatedSiren.solve_volume)
    assert list(sig.parameters) == ["self", "targets", "maps", "shape", "spacing", "iterations", "lam", "thickness", "weights", "intensity", "min_coverage", "start", "coverage",
                                    "history"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[5:])
    assert sig.parameters["iterations"].default is inspect.Parameter.empty and sig.parameters["lam"].default == 0.0
    assert sv.SolveVolumeResult._fields == ("volume", "coverage", "history", "flags", "stopped_at")
    for name in ("solve_volume_on_host", "forward_on_host", "transpose_on_host", "laplacian_on_host", "ordered_dot", "objective_on_host"):
        assert callable(getattr(sv, name)), name
    assert list(inspect.signature(sv.solve_volume_on_host).parameters)[:4] == ["targets", "maps", "shape", "spacing"]
