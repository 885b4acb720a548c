"""dispatch.h: which handles run the *_native ragged / resample calls on the split-fp16 ragged trunk (ragged_native_pick), and which
instance by depth -- over precision x hidden width x depth x residual.  Everything that is not native runs the exact-fp32 ragged kernels
(fp32 handles, the 16-bit trunks at H = 512, MSIREN_PREC_F16 / BF16 at other widths, residual models, depths outside 2..11)."""
import os
import shutil
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = textwrap.dedent(r"""
    #include <cassert>
    #include <cstdio>
    #include "dispatch.h"
    using namespace msiren;

    // a handle as msiren_commit_weights describes it: pack_trunk_f16x3 packs H = 256, L = 2..11 (the ring of 3 fits the LDS up to 11, the
    // ring of 4 up to 5) on MSIREN_PREC_F16X3; pack_trunk_x1 packs H = 512 on the single-product 16-bit precisions
    static DispatchHandle handle(int prec, int H, int L, int res) {
        DispatchHandle d;
        d.precision = prec; d.H = H; d.HP = (H + 127) / 128 * 128; d.L = L; d.Z = 256; d.P = 24 * 24; d.res = res;
        d.f16_ring3_fits = L <= 11; d.f16_ring4_fits = L <= 5; d.ws_depth_ok = L >= 3 && L <= 5;
        d.f16x3_ready = prec == MSIREN_PREC_F16X3 && H == 256 && L >= 2 && d.f16_ring3_fits;
        d.x1_ready = (prec == MSIREN_PREC_BF16 || prec == MSIREN_PREC_F16) && H == 512 && L >= 2 && L <= 11;
        return d;
    }

    int main() {
        int native = 0, total = 0;
        const int precs[] = {MSIREN_PREC_F32, MSIREN_PREC_BF16, MSIREN_PREC_F16X3, MSIREN_PREC_F16};
        const int widths[] = {128, 200, 256, 384, 512};
        for (int prec : precs)
            for (int H : widths)
                for (int L = 1; L <= 13; ++L)
                    for (int res = 0; res < 2; ++res) {
                        const DispatchHandle d = handle(prec, H, L, res);
                        const RaggedNativePick r = ragged_native_pick(d);
                        const bool want = prec == MSIREN_PREC_F16X3 && H == 256 && !res && L >= 2 && L <= 11;
                        ++total;
                        if (r.native != want) {
                            std::fprintf(stderr, "prec %d H %d L %d res %d: native %d, expected %d\n", prec, H, L, res, (int)r.native, (int)want);
                            return 1;
                        }
                        if (!want) {
                            assert(r.ring == 0 && r.lfix == 0);
                            continue;
                        }
                        ++native;
                        // the instance: <ACT,3,5> at L = 5, <ACT,4,0> at L = 2..4, <ACT,3,0> at L = 6..11
                        const int ring = L == 5 ? 3 : L < 5 ? 4 : 3, lfix = L == 5 ? 5 : 0;
                        if (r.ring != ring || r.lfix != lfix) {
                            std::fprintf(stderr, "L %d: <ACT,%d,%d>, expected <ACT,%d,%d>\n", L, r.ring, r.lfix, ring, lfix);
                            return 1;
                        }
                        // a native handle is one whose forward calls run a split-fp16 trunk with the conditional fp32 launch behind it
                        CallMode m; m.nstreams = 2;
                        const TrunkPick t = pick_trunk(d, m, 1000);
                        assert(t.guard == Guard::f32_cond && kInstances[t.inst].family == Kernel::f16x3n);
                    }
        assert(total == 4 * 5 * 13 * 2 && native == 10);
        // packed weights are what counts, not the precision alone: a split-fp16 handle whose trunk was not packed is not native
        DispatchHandle d = handle(MSIREN_PREC_F16X3, 256, 5, 0);
        d.f16x3_ready = false;
        assert(!ragged_native_pick(d).native);
        // ... and the activation does not matter to the rule (the launcher picks ACT)
        d = handle(MSIREN_PREC_F16X3, 256, 7, 0);
        d.act = MSIREN_ACT_MORLET;
        assert(ragged_native_pick(d).native && ragged_native_pick(d).ring == 3 && ragged_native_pick(d).lfix == 0);
        std::puts("ok");
        return 0;
    }
""")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_native_eligibility_over_precision_width_depth_residual(tmp_path):
    src = tmp_path / "dispatch_ragged_native.cpp"
    src.write_text(PROG)
    exe = tmp_path / "dispatch_ragged_native"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mri_inr_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr
