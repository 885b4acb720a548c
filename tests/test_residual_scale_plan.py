"""mri_inr_amd/csrc/residual_scale_plan.h (plain C++, no GPU): the block of the stream's scratch has its four parts in order without overlap, every word
the kernels index lies inside it; the chunking covers every pixel once; the launch count is what the call enqueues for each centre and number of
groups; the key is the rule's total order and turns back; the rank is the rule's (0.29 x 100 floors to 28); the scale takes the floor; and the check
refuses exactly what include/msiren.h lists, naming the argument, flipping at m th tw = 2^28 without overflow at the largest arguments the entry
points can be given.  The program is a stand-alone host program with its own main, built twice: plainly, and with the address and
undefined-behaviour sanitizers."""
import os
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = textwrap.dedent(r"""
    #include <cmath>
    #include <cstdio>
    #include <cstdlib>
    #include <cstdint>
    #include <cstring>
    #include <limits>
    #include <vector>
    #include "residual_scale_plan.h"
    using namespace msiren;
    typedef int64_t i64;
    #define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

    static msiren_scale_opts opts(int centre = 1, double quantile = 0.5, double tune = 8.9, double floor_ = 0.0) {
        msiren_scale_opts o;
        o.struct_size = (int32_t)sizeof o, o.centre = centre, o.quantile = quantile, o.tune = tune, o.floor = floor_;
        return o;
    }
    static char msg[256];
    static bool ok(const RscaleArgs& a) { return rscale_check(a, msg, sizeof msg); }
    static bool refused(const RscaleArgs& a, const char* word) { return !rscale_check(a, msg, sizeof msg) && std::strstr(msg, word); }
    static uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }

    int main() {
        const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
        CHECK(sizeof(msiren_scale_opts) == 32);
        // chunks, segments, uploads, launches
        CHECK(rscale_chunks(0) == 0 && rscale_chunks(1) == 1 && rscale_chunks(4096) == 1 && rscale_chunks(4097) == 2 && rscale_chunks(12707) == 4 && rscale_chunks(102400) == 25);
        CHECK(rscale_segments(6, 0) == 6 && rscale_segments(6, 3) == 3 && rscale_segments(6, 1) == 1);
        CHECK(rscale_uploads(0) == 0 && rscale_uploads(1) == 1 && rscale_uploads(511) == 1 && rscale_uploads(512) == 2 && rscale_uploads(1030) == 3);
        for (bool stats : {false, true}) {
            CHECK(rscale_launches(false, 1, 3, stats) == 0);
            CHECK(rscale_launches(true, 0, 0, stats) == 9 && rscale_launches(true, 1, 0, stats) == 17);
            CHECK(rscale_launches(true, 0, 3, stats) == 10 && rscale_launches(true, 1, 1030, stats) == 20);
        }
        // the block: keys, partials, state, group_start in order, and every word the kernels index inside it
        for (i64 m : {1, 6, 258, 1030})
            for (i64 P : {1, 6, 35, 437, 4096, 4097, 12707})
                for (i64 G : {(i64)0, (i64)1, m}) {
                    const RscaleLayout l = rscale_layout(m, P, G);
                    const i64 chunks = rscale_chunks(P), S = rscale_segments(m, G);
                    CHECK(l.keys == 0 && l.partials == (size_t)((4 * m * P + 15) / 16 * 16) && l.partials % 16 == 0 && l.state == l.partials + (size_t)(4 * m * chunks * 256));
                    CHECK(l.group_start == l.state + (size_t)(32 * S) && l.total == l.group_start + (size_t)(G ? 4 * (G + 1) : 0) && l.total % 4 == 0);
                    std::vector<unsigned char> block(l.total);
                    for (i64 q = 0; q < m; ++q)
                        for (i64 ch = 0; ch < chunks; ++ch) {
                            const i64 start = ch * kRscaleChunk, len = P - start < kRscaleChunk ? P - start : kRscaleChunk;
                            CHECK(len >= 1 && len <= kRscaleChunk);
                            for (i64 i = 0; i < len; ++i) block[l.keys + 4 * (size_t)(q * P + start + i)] += 1;   // every pixel once
                            block[l.partials + 4 * ((size_t)(q * chunks + ch) * 256 + 255) + 3] = 1;
                        }
                    for (i64 i = 0; i < m * P; ++i) CHECK(block[l.keys + 4 * (size_t)i] == 1);
                    block[l.state + 4 * ((size_t)(S - 1) * kRscaleState + kRscaleState - 1) + 3] = 1;   // (RSCALE_CENTRE < kRscaleState)
                    if (G) block[l.group_start + 4 * (size_t)G + 3] = 1;
                    CHECK(block[l.total - 1] == 1 && RSCALE_CENTRE < kRscaleState);
                }
        CHECK(rscale_layout(0, 35, 0).total == 0 && rscale_layout(3, 0, 0).total == 3 * 32);
        // the key: the total order of the bit patterns, and back
        const float order[] = {-std::numeric_limits<float>::infinity(), -3e38f, -1.5f, -1e-45f, -0.0f, 0.0f, 1e-45f, 1.17549435e-38f, 0.75f, 3e38f,
                               std::numeric_limits<float>::infinity()};
        for (size_t i = 0; i + 1 < sizeof order / sizeof order[0]; ++i) CHECK(rscale_key(bits(order[i])) < rscale_key(bits(order[i + 1])));
        for (float x : order) CHECK(rscale_unkey(rscale_key(bits(x))) == bits(x) && rscale_key(bits(x)) != kRscaleNoKey);
        CHECK(rscale_key(bits(-0.0f)) == 0x7fffffffu && rscale_key(bits(0.0f)) == 0x80000000u && rscale_key(0x7fffffffu) == kRscaleNoKey);   // (a NaN's bits)
        // the rank
        CHECK(rscale_rank(0.29, 101) == 28 && rscale_rank(0.5, 101) == 50 && rscale_rank(0.5, 100) == 49 && rscale_rank(0.0, 7) == 0 && rscale_rank(1.0, 7) == 6);
        CHECK(rscale_rank(1.0, ((i64)1 << 28) - 1) == ((i64)1 << 28) - 2 && rscale_rank(0.5, 1) == 0 && rscale_rank(1.0, 1) == 0);
        // the scale
        CHECK(rscale_scale(2.0, 3.0f, 0.0) == 36.0 && rscale_scale(2.0, 3.0f, 36.0) == 36.0 && rscale_scale(2.0, 3.0f, 37.0) == 37.0 && rscale_scale(2.0, 0.0f, 0.0) == 0.0);
        CHECK(rscale_scale(2.0, std::numeric_limits<float>::infinity(), 5.0) == inf && rscale_scale(0.5, 0.5f, 0.0) == 0.0625);
        // the check
        float t[8];
        double sc[4];
        msiren_scale_opts o = opts();
        const RscaleArgs good{t, nullptr, nullptr, nullptr, 2, 2, 2, &o, nullptr, 0, sc, nullptr, false};
        CHECK(ok(good));
        { RscaleArgs a = good; a.m = 0, a.targets = nullptr, a.opts = nullptr, a.scale = nullptr; CHECK(ok(a)); }
        { RscaleArgs a = good; a.th = 0; CHECK(ok(a)); }
        { RscaleArgs a = good; a.simulated = t, a.intensity = t, a.weights = t, a.stats = sc; CHECK(ok(a)); }
        { RscaleArgs a = good; a.m = -1; CHECK(refused(a, "m_targets")); }
        { RscaleArgs a = good; a.th = -1; CHECK(refused(a, "th")); }
        { RscaleArgs a = good; a.tw = -1; CHECK(refused(a, "tw")); }
        { RscaleArgs a = good; a.opts = nullptr; CHECK(refused(a, "opts")); }
        { RscaleArgs a = good; a.targets = nullptr; CHECK(refused(a, "targets")); }
        { RscaleArgs a = good; a.scale = nullptr; CHECK(refused(a, "scale")); }
        { RscaleArgs a = good; a.intensity = t; CHECK(refused(a, "intensity")); }
        for (int size : {0, 24, 40}) { msiren_scale_opts b = opts(); b.struct_size = size; RscaleArgs a = good; a.opts = &b; CHECK(refused(a, "struct_size")); }
        for (int centre : {-1, 2}) { msiren_scale_opts b = opts(centre); RscaleArgs a = good; a.opts = &b; CHECK(refused(a, "centre")); }
        for (double q : {-1e-9, 1.0000001, nan, inf}) { msiren_scale_opts b = opts(1, q); RscaleArgs a = good; a.opts = &b; CHECK(refused(a, "quantile")); }
        for (double q : {0.0, 1.0, 0.29}) { msiren_scale_opts b = opts(1, q); RscaleArgs a = good; a.opts = &b; CHECK(ok(a)); }
        for (double tn : {0.0, -1.0, nan, inf}) { msiren_scale_opts b = opts(1, 0.5, tn); RscaleArgs a = good; a.opts = &b; CHECK(refused(a, "tune")); }
        for (double f : {-1e-300, nan, inf, -inf}) { msiren_scale_opts b = opts(1, 0.5, 1.0, f); RscaleArgs a = good; a.opts = &b; CHECK(refused(a, "floor")); }
        { msiren_scale_opts b = opts(0, 0.5, 1.0, 1e300); RscaleArgs a = good; a.opts = &b; CHECK(ok(a)); }
        // m th tw below 2^28, without overflow
        const int32_t I32 = 0x7fffffff;
        { RscaleArgs a = good; a.m = 1 << 12, a.th = 1 << 8, a.tw = (1 << 8) - 1; CHECK(ok(a)); a.tw = 1 << 8; CHECK(refused(a, "m_targets th tw")); }
        { RscaleArgs a = good; a.m = ((i64)1 << 28) - 1, a.th = 1, a.tw = 1; CHECK(ok(a)); a.m = (i64)1 << 28; CHECK(refused(a, "2^28")); }
        { RscaleArgs a = good; a.m = 1, a.th = I32, a.tw = I32; CHECK(refused(a, "2^28")); a.m = INT64_MAX; CHECK(refused(a, "2^28")); a.th = 0; CHECK(refused(a, "2^28")); }
        { RscaleArgs a = good; a.m = 1, a.th = 1 << 14, a.tw = (1 << 14) - 1; CHECK(ok(a)); a.tw = 1 << 14; CHECK(refused(a, "2^28")); }
        // the groups: both given or both absent, and align_plan.h's rule
        const int32_t g2[] = {0, 1, 2}, bad_first[] = {1, 2}, bad_order[] = {0, 2, 2}, bad_last[] = {0, 1, 3};
        { RscaleArgs a = good; a.group_start = g2, a.n_groups = 2; CHECK(ok(a)); a.n_groups = 0; CHECK(refused(a, "n_groups")); a.n_groups = -1; CHECK(refused(a, "n_groups")); }
        { RscaleArgs a = good; a.n_groups = 2; CHECK(refused(a, "group_start")); }
        { RscaleArgs a = good; a.group_start = bad_first, a.n_groups = 1; CHECK(refused(a, "group_start[0]")); }
        { RscaleArgs a = good; a.group_start = bad_order, a.n_groups = 2; CHECK(refused(a, "group_start[2]")); }
        { RscaleArgs a = good; a.group_start = bad_last, a.n_groups = 2; CHECK(refused(a, "last offset")); }
        // device pointers: 4 bytes for the floats, 8 for scale and stats; host pointers are not looked at
        const char* p = (const char*)sc;
        { RscaleArgs a = good; a.targets = p + 2; CHECK(ok(a)); a.device = true; CHECK(refused(a, "targets")); }
        { RscaleArgs a = good; a.device = true, a.simulated = p + 1; CHECK(refused(a, "simulated")); }
        { RscaleArgs a = good; a.device = true, a.weights = p + 2; CHECK(refused(a, "weights")); }
        { RscaleArgs a = good; a.device = true, a.simulated = p, a.intensity = p + 3; CHECK(refused(a, "intensity")); }
        { RscaleArgs a = good; a.device = true, a.scale = p + 4; CHECK(refused(a, "scale")); a.scale = p + 8; CHECK(ok(a)); }
        { RscaleArgs a = good; a.device = true, a.stats = p + 4; CHECK(refused(a, "stats")); a.stats = p + 16; CHECK(ok(a)); }
        std::puts("ok");
        return 0;
    }
""")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan-ubsan"])
def test_the_residual_scale_plan(tmp_path, flags):
    src, exe = tmp_path / "rscale_plan.cpp", tmp_path / "rscale_plan"
    src.write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mri_inr_amd", "csrc"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
