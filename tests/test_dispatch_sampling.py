"""dispatch.h with a call that brings its own coordinate set (CallMode::coords: msiren_sample_*, the *_scaled pipeline): the unit count,
and with it the half-unit rule, follows the call's coordinates; coords = 0 is the handle's P (rows of tests/test_dispatch.py)."""
import os
import shutil
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = textwrap.dedent(r"""
    #include <cassert>
    #include <cstdio>
    #include <cstring>
    #include "dispatch.h"
    using namespace msiren;

    static bool is(int inst, const char* expect) {
        assert(inst >= 0 && inst < kNumInstances);
        if (std::strcmp(kInstances[inst].name, expect) == 0) return true;
        std::fprintf(stderr, "picked %s, expected %s\n", kInstances[inst].name, expect);
        return false;
    }
    static DispatchHandle f16x3(int L) {
        DispatchHandle d;
        d.precision = MSIREN_PREC_F16X3; d.H = d.HP = 256; d.L = L; d.Z = 256; d.P = 24 * 24; d.act = MSIREN_ACT_SINE; d.num_cus = 256;
        d.f16x3_ready = d.em_enc = d.em_mod = true;
        d.f16_ring3_fits = true; d.f16_ring4_fits = L <= 11; d.ws_depth_ok = L >= 3 && L <= 5;
        return d;
    }
    static CallMode dev(int nstreams, int coords = 0) { CallMode m; m.nstreams = nstreams; m.coords = coords; return m; }

    int main() {
        const DispatchHandle d = f16x3(5);
        // the x2 lattice of the default model: 2 304 coordinates = 72 units per patch; half-units while units <= 2 x 256 CUs
        TrunkPick t = pick_trunk(d, dev(2, 2304), 7);   // 504 units
        assert(is(t.inst, "siren_trunk_f16x3h_kernel<0,3,5>") && t.half && t.ring == 3);
        t = pick_trunk(d, dev(2, 2304), 8);             // 576 units
        assert(is(t.inst, "siren_trunk_f16x3n_kernel<0,3,5>") && !t.half && t.guard == Guard::f32_cond);
        // a single coordinate: one unit per patch
        assert(is(pick_trunk(d, dev(1, 1), 512).inst, "siren_trunk_f16x3h_kernel<0,4,5>"));
        assert(is(pick_trunk(d, dev(1, 1), 513).inst, "siren_trunk_f16x3w_kernel<0,4>"));
        // coords = 0: the handle's own P (18 units per patch) -- rows of tests/test_dispatch.py
        assert(dev(2).coords == 0);
        assert(is(pick_trunk(d, dev(2, 0), 400).inst, "siren_trunk_f16x3n_kernel<0,3,5>"));
        assert(is(pick_trunk(d, dev(1, 0), 28).inst, "siren_trunk_f16x3h_kernel<0,4,5>"));
        assert(is(pick_trunk(d, dev(1, 0), 29).inst, "siren_trunk_f16x3w_kernel<0,4>"));
        assert(is(pick_trunk(d, dev(2, 0), 28).inst, "siren_trunk_f16x3h_kernel<0,3,5>"));
        // ... and the call's own count equal to P is the same call
        assert(pick_trunk(d, dev(1, 576), 28).inst == pick_trunk(d, dev(1, 0), 28).inst);
        assert(pick_trunk(d, dev(1, 576), 29).inst == pick_trunk(d, dev(1, 0), 29).inst);
        std::puts("ok");
        return 0;
    }
""")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_dispatch_follows_the_calls_coordinates(tmp_path):
    src = tmp_path / "dispatch_sampling.cpp"
    src.write_text(PROG)
    exe = tmp_path / "dispatch_sampling"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mri_inr_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr
