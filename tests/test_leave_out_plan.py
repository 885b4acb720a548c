"""mri_inr_amd/csrc/leave_out_plan.h (plain C++, no GPU): the block of the stream's scratch has its four parts in order without overlap, the sums on a
16-byte boundary, and every word the kernels index lies inside it; the launch count is what the call enqueues for each number of groups and set of
outputs; and the check refuses exactly what include/msiren.h lists, naming the argument, without overflow at the largest arguments the entry points can
be given.  The program is a stand-alone host program with its own main, built twice: plainly, and with the address and undefined-behaviour
sanitizers."""
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
    #include "leave_out_plan.h"
    using namespace msiren;
    typedef int64_t i64;
    #define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

    static msiren_fuse_opts opts(double spacing = 4.0, double thickness = 4.0, double min_coverage = 0.0) {
        msiren_fuse_opts o;
        std::memset(&o, 0, sizeof o);
        o.struct_size = (int32_t)sizeof o, o.spacing = spacing, o.thickness = thickness, o.min_coverage = min_coverage;
        return o;
    }
    static char msg[256];
    static bool ok(const LeaveOutArgs& a) { return leave_out_check(a, msg, sizeof msg); }
    static bool refused(const LeaveOutArgs& a, const char* word) { return !leave_out_check(a, msg, sizeof msg) && std::strstr(msg, word); }

    int main() {
        const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
        CHECK(sizeof(msiren_fuse_opts) == 32 && MSIREN_LEAVE_OUT_FLOOR == std::ldexp(1.0, -20));
        // uploads and launches
        CHECK(leave_out_uploads(0) == 0 && leave_out_uploads(1) == 1 && leave_out_uploads(511) == 1 && leave_out_uploads(512) == 2 && leave_out_uploads(600) == 2 &&
              leave_out_uploads(1023) == 2 && leave_out_uploads(1024) == 3);
        for (bool volume : {false, true}) {
            CHECK(leave_out_launches(true, 0, false, volume) == 3 && leave_out_launches(true, 0, true, volume) == 4);
            CHECK(leave_out_launches(true, 4, false, volume) == 4 && leave_out_launches(true, 600, true, volume) == 6);
            for (bool rs : {false, true}) CHECK(leave_out_launches(false, 0, rs, volume) == (volume ? 1 : 0));
        }
        // the block: records, group_start, sums, columns in order, and every word the kernels index inside it
        for (i64 m : {0, 1, 8, 600})
            for (i64 G : {(i64)0, (i64)1, m})
                for (int32_t tw : {2, 23})
                    for (bool stats : {false, true}) {
                        const i64 n = 3, H = 5, W = 7;
                        const LeaveOutLayout l = leave_out_layout(m, tw, G, n, (int32_t)H, (int32_t)W, stats);
                        const bool groups = G > 0 && m > 0;
                        CHECK(l.records == 0 && l.group_start == (size_t)(160 * m) && l.sums % 16 == 0 && l.sums >= l.group_start + (groups ? 4 * (size_t)(G + 1) : 0));
                        CHECK(l.sums < l.group_start + (groups ? 4 * (size_t)(G + 1) : 0) + 16 && l.columns == l.sums + (size_t)(16 * n * H * W));
                        CHECK(l.total == l.columns + (stats ? (size_t)(32 * m * tw) : 0));
                        std::vector<unsigned char> block(l.total);
                        for (i64 q = 0; q < m; ++q) block[l.records + 8 * (size_t)(q * kFuseRecord + FUSE_FLAGS)] += 1;       // the last field of every record
                        if (groups) for (i64 g = 0; g <= G; ++g) block[l.group_start + 4 * (size_t)g] += 1;
                        for (i64 v = 0; v < n * H * W; ++v) block[l.sums + 16 * (size_t)v] += 1, block[l.sums + 16 * (size_t)v + 8] += 1;
                        if (stats) for (i64 c = 0; c < m * tw * kProjectSums; ++c) block[l.columns + 8 * (size_t)c] += 1;
                        for (unsigned char b : block) CHECK(b <= 1);                                                           // no two parts share a word
                    }
        // the check
        float t[64];
        double st[8];
        msiren_fuse_opts o = opts();
        const LeaveOutArgs good{t, 2, 2, 2, t, nullptr, nullptr, &o, nullptr, 0, 3, 4, 5, t, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false};
        CHECK(ok(good));
        { LeaveOutArgs a = good; a.m = 0, a.targets = a.maps = a.simulated = nullptr, a.opts = nullptr; CHECK(ok(a)); a.volume = t; CHECK(ok(a)); }
        { LeaveOutArgs a = good; a.weights = a.intensity = a.coverage = a.residual = a.flags = a.volume = a.volume_coverage = t, a.stats = st; CHECK(ok(a)); }
        { LeaveOutArgs a = good; a.m = -1; CHECK(refused(a, "m_targets")); }
        { LeaveOutArgs a = good; a.th = 1; CHECK(refused(a, "th and tw")); a.th = 2, a.tw = 1; CHECK(refused(a, "th and tw")); }
        { LeaveOutArgs a = good; a.opts = nullptr; CHECK(refused(a, "opts")); }
        { LeaveOutArgs a = good; a.targets = nullptr; CHECK(refused(a, "(targets)")); }
        { LeaveOutArgs a = good; a.maps = nullptr; CHECK(refused(a, "(maps)")); }
        { LeaveOutArgs a = good; a.simulated = nullptr; CHECK(refused(a, "(simulated)")); }
        { LeaveOutArgs a = good; a.n = 0; CHECK(refused(a, "n_slices")); a.n = 3, a.H = 0; CHECK(refused(a, "height")); a.H = 4, a.W = 0; CHECK(refused(a, "width")); }
        for (int size : {0, 24, 40}) { msiren_fuse_opts b = opts(); b.struct_size = size; LeaveOutArgs a = good; a.opts = &b; CHECK(refused(a, "struct_size")); }
        for (double x : {0.0, -1.0, nan, inf}) {
            msiren_fuse_opts b = opts(x); LeaveOutArgs a = good; a.opts = &b; CHECK(refused(a, "spacing"));
            msiren_fuse_opts c = opts(4.0, x); a.opts = &c; CHECK(refused(a, "thickness"));
        }
        for (double x : {-1e-300, nan}) { msiren_fuse_opts b = opts(4.0, 4.0, x); LeaveOutArgs a = good; a.opts = &b; CHECK(refused(a, "min_coverage")); }
        { msiren_fuse_opts b = opts(4.0, 1.0, inf); LeaveOutArgs a = good; a.opts = &b; CHECK(ok(a)); }
        // the limits, without overflow
        const int32_t I32 = 0x7fffffff;
        { LeaveOutArgs a = good; a.n = 1 << 10, a.H = 1 << 10, a.W = (1 << 10) - 1; CHECK(ok(a)); a.W = 1 << 10; CHECK(refused(a, "n_slices height width")); }
        { LeaveOutArgs a = good; a.n = INT64_MAX, a.H = I32, a.W = I32; CHECK(refused(a, "2^30")); }
        { LeaveOutArgs a = good; a.m = 1 << 10, a.th = 1 << 10, a.tw = (1 << 10) - 1; CHECK(ok(a)); a.tw = 1 << 10; CHECK(refused(a, "m_targets th tw")); }
        { LeaveOutArgs a = good; a.m = INT64_MAX, a.th = I32, a.tw = I32; CHECK(refused(a, "2^30")); }
        // the groups: both given or both absent, first 0, strictly ascending, last m
        const int32_t g2[] = {0, 1, 2}, g1[] = {0, 2}, bad_first[] = {1, 2}, bad_order[] = {0, 2, 2}, bad_last[] = {0, 1, 3};
        { LeaveOutArgs a = good; a.group_start = g2, a.n_groups = 2; CHECK(ok(a)); a.n_groups = 0; CHECK(refused(a, "n_groups")); a.n_groups = -1; CHECK(refused(a, "n_groups")); }
        { LeaveOutArgs a = good; a.group_start = g1, a.n_groups = 1; CHECK(ok(a)); }
        { LeaveOutArgs a = good; a.n_groups = 2; CHECK(refused(a, "group_start")); }
        { LeaveOutArgs a = good; a.group_start = bad_first, a.n_groups = 1; CHECK(refused(a, "group_start[0]")); }
        { LeaveOutArgs a = good; a.group_start = bad_order, a.n_groups = 2; CHECK(refused(a, "group_start[2]") && std::strstr(msg, "ascending")); }
        { LeaveOutArgs a = good; a.group_start = bad_last, a.n_groups = 2; CHECK(refused(a, "last offset")); }
        // device pointers: 4 bytes for the floats and the flags, 8 for stats; host pointers are not looked at
        const char* p = (const char*)st;
        const void* LeaveOutArgs::*ptrs[] = {&LeaveOutArgs::targets, &LeaveOutArgs::maps, &LeaveOutArgs::weights, &LeaveOutArgs::intensity, &LeaveOutArgs::simulated,
                                             &LeaveOutArgs::coverage, &LeaveOutArgs::residual, &LeaveOutArgs::flags, &LeaveOutArgs::volume, &LeaveOutArgs::volume_coverage};
        const char* names[] = {"targets", "maps", "weights", "intensity", "simulated", "coverage", "residual", "flags", "device volume ", "volume_coverage"};
        for (int e = 0; e < 10; ++e) {
            LeaveOutArgs a = good;
            a.*ptrs[e] = p + 2;
            CHECK(ok(a));
            a.device = true;
            CHECK(refused(a, names[e]));
            a.*ptrs[e] = p + 4;
            CHECK(ok(a));
        }
        { LeaveOutArgs a = good; a.device = true, a.stats = p + 4; CHECK(refused(a, "stats")); a.stats = p + 8; CHECK(ok(a)); }
        std::puts("ok");
        return 0;
    }
""")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan-ubsan"])
def test_the_leave_out_plan(tmp_path, flags):
    src, exe = tmp_path / "leave_out_plan.cpp", tmp_path / "leave_out_plan"
    src.write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mri_inr_amd", "csrc"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
