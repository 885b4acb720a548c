"""Which kernel runs for which model and call (mri_inr_amd/csrc/dispatch.h, plain C++ compiled with g++): every row of DESIGN.md
section 4, with the exact instance names msiren_last_trunk_kernel reports and bench.py's roofline.kernel compares."""
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
    #include <set>
    #include <string>
    #include <tuple>
    #include "dispatch.h"
    using namespace msiren;

    static const char* name(int inst) { assert(inst >= 0 && inst < kNumInstances); return kInstances[inst].name; }
    static bool is(int inst, const char* expect) {
        if (std::strcmp(name(inst), expect) == 0) return true;
        std::fprintf(stderr, "picked %s, expected %s\n", name(inst), expect);
        return false;
    }

    // a committed handle as msiren_commit_weights describes it (LDS facts, pinned by static_assert in
    // launch_dispatch.hip: F16Lds<4> fits up to L = 5, F16Lds<3> up to L = 11; WS_MIN_L = 3, WS_MAX_L = 5)
    static DispatchHandle f16x3(int L, int act = MSIREN_ACT_SINE) {
        DispatchHandle d;
        d.precision = MSIREN_PREC_F16X3; d.H = d.HP = 256; d.L = L; d.Z = 256; d.P = 24 * 24; d.act = act; d.num_cus = 256;
        d.f16x3_ready = d.em_enc = d.em_mod = true;
        d.f16_ring3_fits = L <= 11; d.f16_ring4_fits = L <= 5; d.ws_depth_ok = L >= 3 && L <= 5;
        return d;
    }
    static DispatchHandle fp32(int H, int act, int res) {
        DispatchHandle d;
        d.precision = MSIREN_PREC_F32; d.H = H; d.HP = (H + 127) / 128 * 128; d.L = 5; d.Z = 256; d.P = 576; d.act = act; d.res = res;
        return d;
    }
    static DispatchHandle x1(int prec, int L, int act = 0, int res = 0) {
        DispatchHandle d;
        d.precision = prec; d.H = d.HP = 512; d.L = L; d.Z = 128; d.P = 576; d.act = act; d.res = res; d.x1_ready = true;
        d.em_enc = d.em_mod = true;
        return d;
    }
    static CallMode dev(int nstreams) { CallMode m; m.nstreams = nstreams; return m; }
    static CallMode sync(int nstreams) { CallMode m = dev(nstreams); m.sync = true; return m; }

    int main() {
        // ---- the instance table: one row per compiled instance, names as the template arguments read ----
        {
            std::set<std::string> names;
            std::set<std::tuple<int, int, int, int, int>> keys;
            for (int i = 0; i < kNumInstances; ++i) {
                const Instance& r = kInstances[i];
                assert(names.insert(r.name).second);
                assert(keys.insert({(int)r.family, r.arg[0], r.arg[1], r.arg[2], r.arg[3]}).second);
                assert(instance(r.family, r.arg[0], r.arg[1], r.arg[2], r.arg[3]) == i);
                assert(std::strchr(r.name, ' ') == nullptr);
            }
            assert(kNumInstances == 19 + 9 + 4 + 3 + 8 + 8 + 10);
            assert(is(instance(Kernel::f16x3w, 0, 4), "siren_trunk_f16x3w_kernel<0,4>"));
            assert(is(instance(Kernel::f16x3w, 0, 4, 1), "siren_trunk_f16x3w_kernel<0,4,1>"));
            assert(is(instance(Kernel::f16x3n, 0, 3, 5), "siren_trunk_f16x3n_kernel<0,3,5>"));
            assert(is(instance(Kernel::f16x3n, 0, 4, 5, 1), "siren_trunk_f16x3n_kernel<0,4,5,1>"));
            assert(is(instance(Kernel::f16x3h, 1, 4, 5), "siren_trunk_f16x3h_kernel<1,4,5>"));
            assert(is(instance(Kernel::x1n, 1, 0, 1, 3), "siren_trunk_x1n_kernel<1,0,1,3>"));
            assert(is(instance(Kernel::x1w, 0, 1, 1), "siren_trunk_x1w_kernel<0,1,1>"));
            assert(is(instance(Kernel::f32, 256, 0, 0), "siren_trunk_f32_kernel<256,0,0>"));
            assert(is(instance(Kernel::f32, 256, 0, 0, 1), "siren_trunk_f32_kernel<256,0,0,1>"));
            assert(is(instance(Kernel::f32_cond, 1), "siren_trunk_f32_cond_kernel<1>"));
            assert(is(instance(Kernel::latent_mods, 2, 2, 8, 3), "latent_mods_f16x3_kernel<2,2,8,3>"));
            assert(is(instance(Kernel::encoder_conv, 1), "encoder_conv_f16x3_kernel<1>"));
            assert(instance(Kernel::f16x3n, 0, 2, 5) < 0 && instance(Kernel::f32, 640, 0, 0) < 0);
        }

        for (int act : {0, 1}) {
            const int A = act ? MSIREN_ACT_MORLET : MSIREN_ACT_SINE;
            char n3[64], w4[64], h4[64], h3[64], n45[64], n40[64], n30[64];
            std::snprintf(n3, 64, "siren_trunk_f16x3n_kernel<%d,3,5>", act);
            std::snprintf(n45, 64, "siren_trunk_f16x3n_kernel<%d,4,5>", act);
            std::snprintf(n40, 64, "siren_trunk_f16x3n_kernel<%d,4,0>", act);
            std::snprintf(n30, 64, "siren_trunk_f16x3n_kernel<%d,3,0>", act);
            std::snprintf(w4, 64, "siren_trunk_f16x3w_kernel<%d,4>", act);
            std::snprintf(h4, 64, "siren_trunk_f16x3h_kernel<%d,4,5>", act);
            std::snprintf(h3, 64, "siren_trunk_f16x3h_kernel<%d,3,5>", act);
            const DispatchHandle d = f16x3(5, A);

            // f16x3, H = 256, L = 5, *_dev on a two-stream handle: register-resident, ring of 3, the conditional fp32 trunk behind it
            TrunkPick t = pick_trunk(d, dev(2), 400);
            assert(is(t.inst, n3) && t.ring == 3 && !t.half && t.guard == Guard::f32_cond);
            assert(is(pick_trunk(d, dev(3), 3200).inst, n3));
            // one-stream handle, or a synchronous host call (on any handle): weight-stationary
            for (int64_t B : {29, 400, 3200}) {
                assert(is(pick_trunk(d, dev(1), B).inst, w4));
                assert(is(pick_trunk(d, sync(2), B).inst, w4));
            }
            assert(pick_trunk(d, sync(2), 400).guard == Guard::f32_cond);
            // B * 18 units <= 2 x CUs (B <= 28), no plan: half-unit instance, its ring by the call
            t = pick_trunk(d, dev(1), 28);
            assert(is(t.inst, h4) && t.half && t.ring == 4);
            assert(is(pick_trunk(d, sync(2), 1).inst, h4));
            assert(is(pick_trunk(d, dev(2), 28).inst, h3));
            // the same with a plan, or with half_allowed = 0: not the half-unit instance
            CallMode planned = dev(1);
            planned.plan = true;
            assert(is(pick_trunk(d, planned, 28).inst, w4));
            planned.nstreams = 2;
            assert(is(pick_trunk(d, planned, 28).inst, n3));
            DispatchHandle nohalf = d;
            nohalf.half_allowed = 0;
            assert(is(pick_trunk(nohalf, dev(1), 28).inst, w4));
            assert(is(pick_trunk(nohalf, dev(2), 28).inst, n3));
            // f16_ws = 0: register-resident, ring of 4 where nothing runs beside it
            DispatchHandle nows = d;
            nows.f16_ws = 0;
            t = pick_trunk(nows, dev(1), 400);
            assert(is(t.inst, n45) && t.ring == 4);
            assert(is(pick_trunk(nows, sync(2), 400).inst, n45));
            assert(is(pick_trunk(nows, dev(2), 400).inst, n3));
            assert(!ws_capable(nows, 400) && ws_capable(d, 400));
            // L = 3 / 4: the ring of 3 becomes 4 (loop form); alone: weight-stationary
            for (int L : {3, 4}) {
                assert(is(pick_trunk(f16x3(L, A), dev(2), 400).inst, n40));
                assert(is(pick_trunk(f16x3(L, A), dev(1), 400).inst, w4));
                assert(is(pick_trunk(f16x3(L, A), dev(1), 28).inst, w4));  // (no half-unit instance below depth 5)
            }
            // L = 2: loop form with the ring of 4 in every mode; L = 6...11: the ring of 4 does not fit the LDS, loop form with the ring of 3
            for (CallMode m : {dev(1), dev(2), sync(2)}) {
                t = pick_trunk(f16x3(2, A), m, 400);
                assert(is(t.inst, n40) && t.ring == 4);
                for (int L : {6, 8, 11}) {
                    t = pick_trunk(f16x3(L, A), m, 400);
                    assert(is(t.inst, n30) && t.ring == 3 && !t.half);
                }
            }
            {   // (the flag alone decides: a depth whose ring of 4 did fit would run it)
                DispatchHandle fits = f16x3(6, A);
                fits.f16_ring4_fits = true;
                assert(is(pick_trunk(fits, dev(1), 400).inst, n40));
            }
            // a pipelined host call's chunks: trunk 1 -> register-resident with room beside it, trunk 2 -> weight-stationary
            CallMode chunk = sync(2);
            chunk.trunk = 1;
            assert(is(pick_trunk(d, chunk, 112).inst, n3) && is(pick_trunk(d, chunk, 400).inst, n3));
            chunk.trunk = 2;
            assert(is(pick_trunk(d, chunk, 288).inst, w4) && is(pick_trunk(nows, chunk, 288).inst, w4));
            // a synchronous one-chunk call reads the guard on the host: no conditional launch
            CallMode one = sync(2);
            one.host_check = true;
            for (int64_t B : {1, 400}) assert(pick_trunk(d, one, B).guard == Guard::host);
            assert(is(pick_trunk(d, one, 1).inst, h4) && is(pick_trunk(d, one, 400).inst, w4));
        }

        // fp32 at H = 128, 256, 384, 512 (and padded widths), each activation / residual: the exact-fp32 trunk, nothing behind it
        for (int H : {128, 200, 256, 384, 512})
            for (int act : {0, 1})
                for (int res : {0, 1}) {
                    char nm[64];
                    std::snprintf(nm, 64, "siren_trunk_f32_kernel<%d,%d,%d>", (H + 127) / 128 * 128, act, res);
                    for (CallMode m : {dev(1), dev(2), sync(2)}) {
                        const TrunkPick t = pick_trunk(fp32(H, act ? MSIREN_ACT_MORLET : MSIREN_ACT_SINE, res), m, 400);
                        assert(is(t.inst, nm) && t.guard == Guard::none);
                    }
                }
        {   // a split-fp16 handle with the residual skip, or whose weights were not packed: fp32 as well
            DispatchHandle r = f16x3(5);
            r.res = 1;
            assert(is(pick_trunk(r, dev(1), 400).inst, "siren_trunk_f32_kernel<256,0,1>"));
            DispatchHandle u = f16x3(5);
            u.f16x3_ready = false;
            assert(is(pick_trunk(u, dev(1), 400).inst, "siren_trunk_f32_kernel<256,0,0>"));
        }

        // bf16 / f16, H = 512: weight-stationary for L >= 3 (the balanced grid when nothing runs beside it), x1n<...,3> at L = 2;
        // both have the conditional f32<512> behind them (bf16 too: its modulation table in LDS is fp16)
        for (int prec : {MSIREN_PREC_BF16, MSIREN_PREC_F16})
            for (int act : {0, 1})
                for (int res : {0, 1}) {
                    const int bf = prec == MSIREN_PREC_BF16;
                    char w[64], n[64];
                    std::snprintf(w, 64, "siren_trunk_x1w_kernel<%d,%d,%d>", bf, act, res);
                    std::snprintf(n, 64, "siren_trunk_x1n_kernel<%d,%d,%d,3>", bf, act, res);
                    const Guard g = Guard::f32_512;
                    for (int L : {3, 5, 10}) {
                        const DispatchHandle d = x1(prec, L, act ? MSIREN_ACT_MORLET : MSIREN_ACT_SINE, res);
                        TrunkPick t = pick_trunk(d, dev(1), 400);
                        assert(is(t.inst, w) && t.balanced && t.guard == g);
                        t = pick_trunk(d, sync(2), 400);
                        assert(is(t.inst, w) && t.balanced);
                        t = pick_trunk(d, dev(2), 400);
                        assert(is(t.inst, w) && !t.balanced);
                        CallMode one = sync(1);
                        one.host_check = true;  // (its own guard: the host check is the split-fp16 trunk's)
                        assert(pick_trunk(d, one, 400).guard == g);
                    }
                    const TrunkPick t = pick_trunk(x1(prec, 2, act ? MSIREN_ACT_MORLET : MSIREN_ACT_SINE, res), dev(1), 400);
                    assert(is(t.inst, n) && !t.balanced && t.guard == g);
                }

        // ---- prologue: depth 8 / 4 / 2 by alone / row blocks / beside; MSIREN_EM_DEPTH; H = 512 never below 4; the halves MODE 1 / 2;
        //      L2 prefetch only for H = 256, alone, <= 64 row blocks, both halves ----
        {
            const DispatchHandle d = f16x3(5), c5 = x1(MSIREN_PREC_BF16, 10);
            CallMode beside = sync(2);
            beside.beside = true;
            struct Row { DispatchHandle d; CallMode m; int mode; int64_t nblk; const char* name; int pf; };
            const Row rows[] = {
                {d, dev(1), 3, 1, "latent_mods_f16x3_kernel<2,2,8,3>", 64},
                {d, dev(1), 3, 64, "latent_mods_f16x3_kernel<2,2,8,3>", 64},
                {d, dev(1), 3, 65, "latent_mods_f16x3_kernel<2,2,8,3>", 0},
                {d, dev(1), 3, 256, "latent_mods_f16x3_kernel<2,2,8,3>", 0},
                {d, dev(1), 3, 257, "latent_mods_f16x3_kernel<2,2,4,3>", 0},
                {d, sync(2), 3, 7, "latent_mods_f16x3_kernel<2,2,8,3>", 64},
                {d, sync(2), 3, 400, "latent_mods_f16x3_kernel<2,2,4,3>", 0},
                {d, dev(2), 3, 7, "latent_mods_f16x3_kernel<2,2,2,3>", 0},
                {d, dev(3), 3, 400, "latent_mods_f16x3_kernel<2,2,2,3>", 0},
                {d, beside, 3, 25, "latent_mods_f16x3_kernel<2,2,2,3>", 0},
                {d, dev(1), 1, 1, "latent_mods_f16x3_kernel<2,2,4,1>", 0},
                {d, dev(2), 1, 400, "latent_mods_f16x3_kernel<2,2,4,1>", 0},
                {d, dev(1), 2, 1, "latent_mods_f16x3_kernel<2,2,4,2>", 0},
                {d, sync(2), 2, 400, "latent_mods_f16x3_kernel<2,2,4,2>", 0},
                {c5, dev(1), 3, 25, "latent_mods_f16x3_kernel<4,1,8,3>", 0},
                {c5, dev(1), 3, 257, "latent_mods_f16x3_kernel<4,1,4,3>", 0},
                {c5, dev(2), 3, 25, "latent_mods_f16x3_kernel<4,1,4,3>", 0},
                {c5, dev(1), 1, 25, "latent_mods_f16x3_kernel<4,1,4,1>", 0},
                {c5, dev(2), 2, 25, "latent_mods_f16x3_kernel<4,1,4,2>", 0},
            };
            for (const Row& r : rows) {
                const ProloguePick p = pick_prologue(r.d, r.m, r.mode, r.nblk);
                assert(is(p.inst, r.name) && p.pf_blocks == r.pf);
            }
            // MSIREN_EM_DEPTH forces the depth of the combined instance (the prefetch still follows the call)
            for (int depth : {2, 4, 8}) {
                DispatchHandle f = d;
                f.em_depth = depth;
                char nm[64];
                std::snprintf(nm, 64, "latent_mods_f16x3_kernel<2,2,%d,3>", depth);
                for (CallMode m : {dev(1), dev(2), beside}) assert(is(pick_prologue(f, m, 3, 7).inst, nm));
                assert(pick_prologue(f, dev(1), 3, 7).pf_blocks == 64 && pick_prologue(f, dev(2), 3, 7).pf_blocks == 0);
                assert(is(pick_prologue(f, dev(1), 1, 7).inst, "latent_mods_f16x3_kernel<2,2,4,1>"));
                DispatchHandle g = c5;
                g.em_depth = depth;
                std::snprintf(nm, 64, "latent_mods_f16x3_kernel<4,1,%d,3>", depth < 4 ? 4 : depth);
                assert(is(pick_prologue(g, dev(2), 3, 7).inst, nm));
            }
        }

        // exact-fp32 Linear layers: the 32 x 32-tile kernel from 1024 rows (256 for >= 512 outputs), below 2^32 elements per operand
        assert(!linear_tiled(1023, 256, 256, 256) && linear_tiled(1024, 256, 256, 256) && linear_tiled(1024, 64, 2048, 0));
        assert(!linear_tiled(255, 512, 128, 512) && linear_tiled(256, 512, 128, 512));
        assert(!linear_tiled((1LL << 32) / 2048, 64, 2048, 0) && linear_tiled((1LL << 32) / 2048 - 1, 64, 2048, 0));

        // (the shapes tests/fp32_prologue_cases.py relies on: H < 512 from 1024 rows, 512-wide layers from 256 -- by the layer's own
        //  H, so conv3 (64 outputs) of a 512-latent encoder stays on 16 x 16 tiles at 273 rows while its Linear(64, 512) is tiled)
        assert(!linear_tiled(1023, 48, 48, 48) && linear_tiled(1024, 48, 48, 0) && linear_tiled(1041, 256, 128, 256));
        assert(!linear_tiled(273, 64, 2048, 0) && linear_tiled(273, 512, 64, 0) && linear_tiled(273, 512, 512, 512) && !linear_tiled(255, 512, 512, 512));

        // exact-fp32 per-layer launches: the MFMA Linear kernels take H and Z that are multiples of 16, the VALU Modulator everything
        // else; the fused per-tile encoder kernel where Linear(64, Z) does not fit them (Z alone decides)
        assert(modulator_mfma(256, 128) && modulator_mfma(48, 48) && modulator_mfma(64, 16) && modulator_mfma(512, 512) && modulator_mfma(256, 320));
        assert(!modulator_mfma(100, 24) && !modulator_mfma(250, 256) && !modulator_mfma(256, 24) && !modulator_mfma(20, 3) && !modulator_mfma(8, 16));
        assert(encoder_fused_valu(24) && encoder_fused_valu(3) && encoder_fused_valu(1300));
        assert(!encoder_fused_valu(16) && !encoder_fused_valu(256) && !encoder_fused_valu(128));
        assert(!modulator_mfma(250, 256) && !encoder_fused_valu(256));  // the MFMA encoder in front of the VALU Modulator
        // the VALU Modulator's LDS: 8 192 static + MOD_ROWS K 4 of input rows, K = (L > 1 ? H : 0) + Z; a plain launch carries 64 KB
        assert(modulator_valu_lds_bytes(100, 24, 3) == 8192 + 8 * 124 * 4 && modulator_valu_lds_bytes(100, 24, 1) == 8192 + 8 * 24 * 4);
        assert(modulator_valu_lds_bytes(500, 1292, 2) == 65536 && modulator_valu_fits(500, 1292, 2));
        assert(modulator_valu_lds_bytes(500, 1300, 2) == 65792 && !modulator_valu_fits(500, 1300, 2));
        assert(modulator_valu_fits(500, 1300, 1) && modulator_valu_fits(500, 1792, 1) && !modulator_valu_fits(500, 1793, 1));
        assert(modulator_valu_fits(512, 2048, 10) && modulator_valu_fits(496, 1312, 2));  // (the MFMA kernels keep nothing in LDS but partial sums)
        assert(!modulator_valu_fits(500, 0x7fffffff, 2));                                  // (no overflow at the largest latent_dim)

        // ---- call level ----
        {   // a host call pipelines itself from host_pipe_min tiles up: split-fp16 trunk, L = 5, both prologue halves, weight-stationary
            const DispatchHandle d = f16x3(5);
            assert(!host_call_pipelines(d, 2399) && host_call_pipelines(d, 2400) && host_call_pipelines(d, 25600));
            DispatchHandle e = d;
            e.host_pipe_min = 128;
            assert(!host_call_pipelines(e, 127) && host_call_pipelines(e, 128));
            for (int L : {3, 4, 6}) assert(!host_call_pipelines(f16x3(L), 3200));
            e = d; e.em_mod = false;    assert(!host_call_pipelines(e, 3200));
            e = d; e.em_enc = false;    assert(!host_call_pipelines(e, 3200));
            e = d; e.f16_ws = 0;        assert(!host_call_pipelines(e, 3200));
            e = d; e.res = 1;           assert(!host_call_pipelines(e, 3200));
            assert(!host_call_pipelines(fp32(256, 0, 0), 3200) && !host_call_pipelines(x1(MSIREN_PREC_BF16, 10), 3200));
            // the slice pipeline fuses tiling + flags + plan for synchronous calls that tile the images themselves
            assert(fused_slice_tiling(sync(1), true) && fused_slice_tiling(sync(2), true));
            assert(!fused_slice_tiling(sync(2), false) && !fused_slice_tiling(dev(1), true) && !fused_slice_tiling(dev(2), true));
        }
        std::puts("ok");
        return 0;
    }
""")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_dispatch_table(tmp_path):
    src = tmp_path / "dispatch.cpp"
    src.write_text(PROG)
    exe = tmp_path / "dispatch"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mri_inr_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr
