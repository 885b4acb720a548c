"""The stack family's share of mri_inr_amd/csrc/align_plan.h (plain C++, no GPU): stack_layout puts the partial records at offset 0 and the grouped
solve's state behind them on an 8-byte boundary with nothing overlapping; stack_voxels_fit and stack_pixels_fit flip exactly at n H W = 2^30, an
extent of 2^24 and m th tw = 2^28, without overflow at the largest arguments the entry points can be given.  The program is a stand-alone host program
with its own main, built twice: plainly, and with the address and undefined-behaviour sanitizers."""
import os
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = textwrap.dedent(r"""
    #include <cstdio>
    #include <cstdlib>
    #include <cstdint>
    #include <vector>
    #include "align_plan.h"
    using namespace msiren;
    typedef int64_t i64;
    #define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

    int main() {
        const i64 I32 = 0x7fffffffLL;
        for (i64 m : {1, 6, 11, 1000})
            for (i64 Mt : {1, 437, 1024, 1025, 1221, 102400}) {
                const GeomLayout l = stack_layout(m, Mt, 80);
                const i64 chunks = (Mt + 1023) / 1024;
                CHECK(align_chunks(Mt) == chunks);
                CHECK(l.partials == 0 && l.total == (size_t)(m * chunks * 640) && l.total % 8 == 0 && l.zero_bytes == 0);
                CHECK(l.counts == 0 && l.ent == 0 && l.coords == 0 && l.pair == 0);   // nothing else is carved
                for (i64 G : {(i64)1, m}) {
                    const GroupSolveLayout s = group_solve_layout(l.total, m, G, 80, 70, 4, 2), z = group_solve_layout(0, m, G, 80, 70, 4, 2);
                    CHECK(s.sums == l.total && s.sums % 8 == 0 && s.total - l.total == z.total);
                    CHECK(s.sums < s.sums_best && s.sums_best < s.rec && s.rec < s.rigid_trial && s.rigid_trial < s.rigid_best && s.rigid_best < s.scal && s.scal < s.trial);
                    CHECK(s.trial < s.best && s.best < s.gb_trial && s.gb_trial < s.gb_best && s.gb_best < s.group_of && s.group_of < s.group_start && s.group_start < s.cnt);
                    // the block as the kernels index it: every record of the partials and every word of the state lies inside it
                    std::vector<unsigned char> block(s.total);
                    for (i64 r = 0; r < m * chunks; ++r) block[(size_t)r * 640 + 639] = 1;
                    block[s.cnt + 4 * (size_t)G * 2 - 1] = 1;
                    CHECK(block[s.total - 1] == 1);
                }
            }
        // the voxels: every extent below 2^24, n H W below 2^30
        CHECK(stack_voxels_fit(2, 2, 2) && stack_voxels_fit(4, 21, 27) && stack_voxels_fit(16, 320, 320));
        CHECK(stack_voxels_fit(1 << 10, 1 << 10, (1 << 10) - 1) && !stack_voxels_fit(1 << 10, 1 << 10, 1 << 10));
        CHECK(stack_voxels_fit(0x00ffffffLL, 2, 2) && !stack_voxels_fit(0x01000000LL, 2, 2) && !stack_voxels_fit(2, 0x01000000LL, 2) && !stack_voxels_fit(2, 2, 0x01000000LL));
        CHECK(stack_voxels_fit(2, 2, 0x00ffffffLL) && !stack_voxels_fit(0x00ffffffLL, 0x00ffffffLL, 2) && !stack_voxels_fit(2, I32, I32) && !stack_voxels_fit(I32, I32, I32));
        CHECK(!stack_voxels_fit(INT64_MAX, I32, I32) && !stack_voxels_fit(1 << 15, 1 << 15, 2) && stack_voxels_fit((1 << 15) - 1, 1 << 14, 2));
        // the pixels: m th tw below 2^28
        CHECK(stack_pixels_fit(16, 320, 320) && stack_pixels_fit(0, I32, I32) == false);
        CHECK(stack_pixels_fit(1 << 12, 1 << 8, (1 << 8) - 1) && !stack_pixels_fit(1 << 12, 1 << 8, 1 << 8));
        CHECK(stack_pixels_fit(0x0fffffffLL, 1, 1) && !stack_pixels_fit(0x10000000LL, 1, 1) && !stack_pixels_fit(1, I32, I32) && !stack_pixels_fit(INT64_MAX, I32, I32));
        CHECK(stack_pixels_fit(0x0fffffffLL, 0, I32) && stack_pixels_fit(1, 1 << 14, (1 << 14) - 1) && !stack_pixels_fit(1, 1 << 14, 1 << 14));
        std::puts("ok");
        return 0;
    }
""")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan-ubsan"])
def test_the_stack_plans(tmp_path, flags):
    src, exe = tmp_path / "stack_plan.cpp", tmp_path / "stack_plan"
    src.write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mri_inr_amd", "csrc"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
