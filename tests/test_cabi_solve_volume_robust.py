"""The C ABI of msiren_solve_volume_r(_dev) (include/msiren.h; no GPU needed): exported by the built library, declared in the header and bound in
mri_inr_amd/_lib.py with matching argument kinds; null handles are refused; a C program that includes the header sees the symbols with the documented
prototypes, links against the library and is refused in the same way -- pure additions under ABI 9, msiren_solve_r_opts of 56 bytes."""
import ctypes as C
import os
import re
import shutil
import subprocess
import textwrap

import pytest

from mri_inr_amd import _lib

HOST = ["p", "p", "i64", "i32", "i32", "p", "p", "p", "p", "opts", "i64", "i32", "i32", "p", "p", "p", "p", "p", "p", "p", "p"]
KINDS = {"msiren_solve_volume_r": HOST, "msiren_solve_volume_r_dev": HOST[:-1] + ["p", "p"]}   # (the _dev form has `residual` in front of `stats`)
HOST_TYPES = ["msiren_handle h", "const float", "int64_t m_targets", "int32_t th", "int32_t tw", "const float", "const float", "const float", "const double",
              "const msiren_solve_r_opts", "int64_t n_slices", "int32_t height", "int32_t width", "const float", "float", "float", "double", "int32_t", "int32_t", "float", "double"]
TYPES = {"msiren_solve_volume_r": HOST_TYPES, "msiren_solve_volume_r_dev": HOST_TYPES[:-1] + ["float", "double"]}


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
    assert "msiren_solve_volume_r(_dev)" in history and "msiren_solve_r_opts" in history
    assert "msiren_solve_volume(_dev)" in history and "msiren_project_volume(_dev)" in history and "msiren_fuse_targets(_dev)" in history  # the earlier additions are still named


@pytest.mark.parametrize("name", sorted(KINDS))
def test_symbol_is_exported_declared_and_bound(lib, name):
    assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"MSIREN_API\s+int\s+" + name + r"\s*\(([^;]*)\);", header)
    assert m, f"{name} is not declared in include/msiren.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    kinds = ["opts" if "msiren_solve_r_opts*" in a else "p" if "*" in a or a.startswith("msiren_handle") else "i64" if a.startswith("int64_t") else "i32" for a in args]
    assert kinds == KINDS[name], args
    assert [a if "*" not in a else a.split("*")[0].strip() for a in args] == TYPES[name], args
    restype, argtypes = _lib.PROTOTYPES[name]
    want = {"p": C.c_void_p, "i64": C.c_int64, "i32": C.c_int32, "opts": C.POINTER(_lib.SolveROpts)}
    assert restype is C.c_int and argtypes == [want[k] for k in kinds]
    assert getattr(lib, name).argtypes == argtypes


def test_the_options_struct_has_56_bytes_and_the_plain_solves_is_unchanged():
    header = open(_lib.HEADER_PATH).read()
    (body,) = re.findall(r"typedef struct \{([^}]*)\}\s*msiren_solve_r_opts;", header)
    fields = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split()
    assert " ".join(fields) == "int32_t struct_size; int32_t iterations; int32_t rounds; int32_t reserved; double spacing, thickness, min_coverage, lambda, anneal;"
    assert C.sizeof(_lib.SolveROpts) == 56
    assert [f[0] for f in _lib.SolveROpts._fields_] == ["struct_size", "iterations", "rounds", "reserved", "spacing", "thickness", "min_coverage", "lam", "anneal"]
    assert _lib.SolveROpts.spacing.offset == 16 and _lib.SolveROpts.anneal.offset == 48
    assert len(re.findall(r"typedef struct \{([^}]*)\}\s*msiren_solve_opts;", header)) == 1 and C.sizeof(_lib.SolveOpts) == 40 and C.sizeof(_lib.FuseOpts) == 32


def test_null_handle_is_refused(lib):
    o = _lib.SolveROpts(56, 1, 1, 0, 4.0, 4.0, 0.0, 0.0, 1.0)
    for name, kinds in KINDS.items():
        args = [C.byref(o) if k == "opts" else None if k == "p" else 4 for k in kinds]
        assert getattr(lib, name)(*args) == _lib.E_INVALID
        assert "null handle" in _lib.last_error()


PROG = textwrap.dedent(r"""
    #include <stddef.h>
    #include <stdio.h>
    #include <string.h>
    #include "msiren.h"

    /* the prototypes a consumer writes from the documentation: an assignment of another type does not compile with -Werror */
    typedef int (*solve_r_fn)(msiren_handle, const float*, int64_t, int32_t, int32_t, const float*, const float*, const float*, const double*, const msiren_solve_r_opts*,
                              int64_t, int32_t, int32_t, const float*, float*, float*, double*, int32_t*, int32_t*, float*, double*);
    typedef int (*solve_r_dev_fn)(msiren_handle, const float*, int64_t, int32_t, int32_t, const float*, const float*, const float*, const double*,
                                  const msiren_solve_r_opts*, int64_t, int32_t, int32_t, const float*, float*, float*, double*, int32_t*, int32_t*, float*, float*, double*);

    int main(void) {
        solve_r_fn host = msiren_solve_volume_r;
        solve_r_dev_fn dev = msiren_solve_volume_r_dev;
        msiren_solve_r_opts o;
        memset(&o, 0, sizeof o);
        o.struct_size = (int32_t)sizeof o, o.iterations = 3, o.rounds = 5, o.spacing = 4.0, o.thickness = 4.0, o.min_coverage = 0.0, o.lambda = 0.01, o.anneal = 4.0;
        if (sizeof o != 56 || offsetof(msiren_solve_r_opts, spacing) != 16 || offsetof(msiren_solve_r_opts, anneal) != 48) return 1;
        if (sizeof(msiren_solve_opts) != 40 || MSIREN_ABI_VERSION != 9 || msiren_abi_version() != 9) return 2;
        if (host(NULL, NULL, 2, 4, 4, NULL, NULL, NULL, NULL, &o, 4, 40, 40, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != MSIREN_E_INVALID) return 3;
        if (!strstr(msiren_last_error(), "null handle")) return 4;
        if (dev(NULL, NULL, 2, 4, 4, NULL, NULL, NULL, NULL, &o, 4, 40, 40, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != MSIREN_E_INVALID) return 5;
        if (!strstr(msiren_last_error(), "null handle")) return 6;
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
    from mri_inr_amd import solve_volume_robust as svr

    sig = inspect.signature(ModulatedSiren.solve_volume_robust)
    assert list(sig.parameters) == ["self", "targets", "maps", "shape", "spacing", "scale", "rounds", "iterations", "anneal", "lam", "thickness", "weights", "intensity",
                                    "min_coverage", "start", "coverage", "history", "rweight", "stats"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[6:])
    assert sig.parameters["rounds"].default is inspect.Parameter.empty and sig.parameters["iterations"].default is inspect.Parameter.empty
    assert sig.parameters["anneal"].default == 1.0 and sig.parameters["lam"].default == 0.0
    assert svr.SolveVolumeRobustResult._fields == ("volume", "coverage", "history", "flags", "stopped_at", "rweight", "stats")
    for name in ("solve_volume_robust_on_host", "schedule", "robust_weight", "reweight_on_host", "robust_stats_on_host", "robust_objective_on_host"):
        assert callable(getattr(svr, name)), name
    assert list(inspect.signature(svr.solve_volume_robust_on_host).parameters)[:5] == ["targets", "maps", "shape", "spacing", "scale"]
    assert "iterates" in inspect.signature(svr.solve_volume_robust_on_host).parameters
