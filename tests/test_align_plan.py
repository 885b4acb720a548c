"""Scratch layouts and size limits of the geometry calls (mri_inr_amd/csrc/align_plan.h, plain C++ compiled with g++): the five pipelines
(resample, resample-volume, align, align-w, align-volume) and the three solve states.  The reference is the arithmetic those calls carried
inline before the header existed, restated literally: every section offset and total, the documented order without overlap, 8-byte
alignment of coords, partials and every double section, and each limit flipping exactly where that arithmetic's expression does."""
import os
import shutil
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = textwrap.dedent(r"""
    #include <cstdio>
    #include <cstdlib>
    #include <initializer_list>
    #include "align_plan.h"
    using namespace msiren;
    typedef int64_t i64;

    #define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
    static const i64 CHUNK = 1024;

    // ---- the reference: the inline arithmetic, literally ----------------------------------------------------------------------------
    struct Ref { size_t counts, cursors, offsets, items, ent, tile, pair, coords, w, f, partials, total, zero, ints_end, flts_end; bool has_partials; };
    static Ref ref_ints(i64 B, i64 T) {   // [counts B][cursors B][offsets B + 1][items B + 1][ent T]...
        Ref r{};
        r.counts = 0, r.cursors = 4 * (size_t)B, r.offsets = 4 * (size_t)(2 * B), r.items = r.offsets + 4 * (size_t)(B + 1), r.ent = r.items + 4 * (size_t)(B + 1);
        r.tile = r.ent + 4 * (size_t)T;
        r.zero = (size_t)2 * B * sizeof(int);
        return r;
    }
    static Ref ref_resample(i64 NPt, i64 M, int K) {
        const i64 T = M * K;
        const size_t nint = (size_t)(4 * NPt + 2 + 2 * T + 1) & ~(size_t)1;
        Ref r = ref_ints(NPt, T);
        r.coords = 4 * nint, r.w = r.coords + 4 * (size_t)(2 * T);
        r.total = (nint + 3 * (size_t)T) * 4;
        r.pair = r.tile + 4 * (size_t)T, r.f = r.w + 4 * (size_t)T;   // (empty sections: where they would start)
        r.ints_end = r.pair, r.flts_end = r.f;
        return r;
    }
    static Ref ref_volume(i64 NP, i64 M, int K) {
        const i64 MK = M * K, T = 2 * MK;
        const size_t nint = (size_t)(4 * NP + 2 + T + MK + M + 1) & ~(size_t)1;
        Ref r = ref_ints(NP, T);
        r.pair = r.tile + 4 * (size_t)MK, r.coords = 4 * nint, r.w = r.coords + 4 * (size_t)(2 * T), r.f = r.w + 4 * (size_t)MK;
        r.total = (nint + 2 * (size_t)T + MK + M) * 4;
        r.ints_end = r.pair + 4 * (size_t)M, r.flts_end = r.f + 4 * (size_t)M;
        return r;
    }
    static Ref ref_align(i64 NP, i64 n, i64 M, int K, int nsums) {
        const i64 T = n * M * K, chunks = (M + CHUNK - 1) / CHUNK;
        const size_t nint = (size_t)(4 * NP + 2 + 2 * T + 1) & ~(size_t)1, nflt = (size_t)(3 * T + 1) & ~(size_t)1;
        Ref r = ref_ints(NP, T);
        r.coords = 4 * nint, r.w = r.coords + 4 * (size_t)(2 * T), r.partials = r.coords + 4 * nflt;
        r.total = (nint + nflt) * 4 + (size_t)n * chunks * nsums * sizeof(double);
        r.pair = r.tile + 4 * (size_t)T, r.f = r.w + 4 * (size_t)T;
        r.ints_end = r.pair, r.flts_end = r.f;
        r.has_partials = true;
        return r;
    }
    static Ref ref_align_volume(i64 NP, i64 m, i64 Mt, int K, int nsums) {
        const i64 M = m * Mt, MK = M * K, T = 2 * MK, chunks = (Mt + CHUNK - 1) / CHUNK;
        const size_t nint = (size_t)(4 * NP + 2 + T + MK + M + 1) & ~(size_t)1, nflt = (size_t)(2 * T + MK + M + 1) & ~(size_t)1;
        Ref r = ref_ints(NP, T);
        r.pair = r.tile + 4 * (size_t)MK, r.coords = 4 * nint, r.w = r.coords + 4 * (size_t)(2 * T), r.f = r.w + 4 * (size_t)MK, r.partials = r.coords + 4 * nflt;
        r.total = (nint + nflt) * 4 + (size_t)m * chunks * nsums * sizeof(double);
        r.ints_end = r.pair + 4 * (size_t)M, r.flts_end = r.f + 4 * (size_t)M;
        r.has_partials = true;
        return r;
    }
    static void same(const GeomLayout& l, const Ref& r) {
        CHECK(l.counts == r.counts && l.cursors == r.cursors && l.offsets == r.offsets && l.items == r.items && l.ent == r.ent && l.tile == r.tile);
        CHECK(l.pair == r.pair && l.coords == r.coords && l.w == r.w && l.f == r.f && l.total == r.total && l.zero_bytes == r.zero);
        if (r.has_partials) CHECK(l.partials == r.partials && l.partials % 8 == 0 && l.total % 8 == 0 && l.partials <= l.total);
        // the documented order, nothing overlapping: each section ends where the next begins or before it
        CHECK(l.counts < l.cursors && l.cursors < l.offsets && l.offsets < l.items && l.items < l.ent && l.ent <= l.tile && l.tile <= l.pair && l.pair <= l.coords);
        CHECK(l.coords <= l.w && l.w <= l.f && l.f <= r.flts_end && r.flts_end <= l.partials && r.flts_end <= l.total);
        CHECK(l.cursors + l.cursors == l.offsets && l.zero_bytes == l.offsets);                 // the memset is counts and cursors, no more
        CHECK(l.items - l.offsets == l.cursors + 4 && l.ent - l.items == l.cursors + 4);         // B + 1 words each
        CHECK(l.coords % 8 == 0 && l.coords >= r.ints_end && l.coords - r.ints_end < 8);       // float2 entries: one pad word at the most in front
        CHECK(l.partials - r.flts_end < 8 && (r.has_partials || l.total == r.flts_end));        // and in front of the doubles
        CHECK(l.w - l.coords == 2 * (l.tile - l.ent));                                           // 8 bytes of coordinates per entry
    }

    // the solve states: [sums u S][sums_best u S][rigid_trial u R][rigid_best u R][scal u 3] doubles, then [trial u P][best u P][gb_trial u 2][gb_best u 2][cnt u 2]
    static void check_solve(size_t bytes, i64 u, int S, int R, int P, bool gb) {
        const size_t nd = (size_t)u * (2 * S + R + R + 3), extra = nd * sizeof(double) + (size_t)u * (P + P + (gb ? 2 + 2 : 0) + 2) * 4;
        const size_t d0 = bytes, f0 = d0 + 8 * nd;
        const SolveLayout s = solve_layout(bytes, u, S, R, P, gb);
        CHECK(s.sums == d0 && s.sums_best == d0 + 8 * (size_t)(u * S) && s.rigid_trial == s.sums_best + 8 * (size_t)(u * S) && s.rigid_best == s.rigid_trial + 8 * (size_t)(u * R));
        CHECK(s.scal == s.rigid_best + 8 * (size_t)(u * R) && s.trial == f0 && s.best == f0 + 4 * (size_t)(u * P));
        if (gb) CHECK(s.gb_trial == s.best + 4 * (size_t)(u * P) && s.gb_best == s.gb_trial + 4 * (size_t)(u * 2) && s.cnt == s.gb_best + 4 * (size_t)(u * 2));
        else CHECK(s.cnt == s.best + 4 * (size_t)(u * P) && s.gb_trial == s.cnt && s.gb_best == s.cnt);
        CHECK(s.total == bytes + extra && solve_layout(0, u, S, R, P, gb).total == extra);
        CHECK(s.sums % 8 == 0 && s.sums_best % 8 == 0 && s.rigid_trial % 8 == 0 && s.rigid_best % 8 == 0 && s.scal % 8 == 0 && s.trial % 4 == 0 && s.cnt % 4 == 0);
        CHECK(s.sums < s.sums_best && s.sums_best < s.rigid_trial && s.rigid_trial < s.rigid_best && s.rigid_best < s.scal && s.scal < s.trial && s.trial < s.best && s.best < s.cnt && s.cnt < s.total);
    }

    // ---- the limits: `refuse` is the inline expression, `fits` the header's; both monotone in x -------------------------------------------
    template <class R, class F>
    static void flips(R refuse, F fits, i64 hi) {
        if (refuse(0)) { CHECK(!fits(0) && !fits(1)); return; }   // refused whatever x is
        i64 lo = 0;                                                // largest accepted x in [0, hi]
        CHECK(refuse(hi));
        while (hi - lo > 1) { const i64 mid = lo + (hi - lo) / 2; (refuse(mid) ? hi : lo) = mid; }
        CHECK(!refuse(lo) && refuse(lo + 1));
        CHECK(fits(lo) && !fits(lo + 1));                          // at the largest accepted value and at one more
        if (lo > 0) CHECK(fits(lo - 1));
        CHECK(fits(0) && !fits(lo + 2));
    }
    static void check_limits(i64 n, i64 m, i64 Mt, int K, i64 NPt) {
        const i64 big = (i64)1 << 40;
        // resample: M points shared by n slices
        flips([&](i64 M) { return M > 0x0fffffffLL || n > 0x0fffffffLL || M * K * 8 > 0x7fffffffLL || n * M * K * 12 > 0x7fffffffLL || n * NPt > 0x3fffffffLL; },
              [&](i64 M) { return resample_fits(n, M, K, NPt); }, big);
        flips([&](i64 nn) { return Mt > 0x0fffffffLL || nn > 0x0fffffffLL || Mt * K * 8 > 0x7fffffffLL || nn * Mt * K * 12 > 0x7fffffffLL || nn * NPt > 0x3fffffffLL; },
              [&](i64 nn) { return resample_fits(nn, Mt, K, NPt); }, big);
        // resample-volume: points, then slices
        flips([&](i64 M) { return M > 0x0fffffffLL || 32 * M * K + 8 * M > 0x3fffffffLL; }, [&](i64 M) { return volume_points_fit(M, K); }, big);
        flips([&](i64 nn) { return nn > 0x00ffffffLL || 16 * nn * NPt > 0x3fffffffLL; }, [&](i64 nn) { return volume_slices_fit(nn, NPt); }, big);
        // align, align-w: pixels (in n and in th tw), then slices
        for (int S : {29, 47}) {
            flips([&](i64 nn) { return nn > 0x00ffffffLL || Mt > 0x0fffffffLL || nn * Mt > 0x0fffffffLL || 20 * nn * Mt * K + 8 * S * nn * ((Mt + CHUNK - 1) / CHUNK) > 0x3fffffffLL; },
                  [&](i64 nn) { return align_pixels_fit(nn, Mt, K, S); }, big);
            flips([&](i64 M) { return n > 0x00ffffffLL || M > 0x0fffffffLL || n * M > 0x0fffffffLL || 20 * n * M * K + 8 * S * n * ((M + CHUNK - 1) / CHUNK) > 0x3fffffffLL; },
                  [&](i64 M) { return align_pixels_fit(n, M, K, S); }, big);
        }
        CHECK(8 * 29 == 232 && 8 * 47 == 376 && 8 * 56 == 448);   // the bytes per partial record the messages and comments name
        flips([&](i64 nn) { return 16 * nn * NPt > 0x3fffffffLL; }, [&](i64 nn) { return bins_fit(nn, NPt); }, big);
        // align-volume: pixels (in m and in th tw); its slices are resample-volume's
        flips([&](i64 mm) { const i64 chunks = (Mt + CHUNK - 1) / CHUNK;
                            return Mt > 0x0fffffffLL || mm > 0x0fffffffLL || mm * Mt > 0x0fffffffLL || 32 * mm * Mt * K + 8 * mm * Mt + 8 * 56 * mm * chunks > 0x3fffffffLL; },
              [&](i64 mm) { return align_volume_pixels_fit(mm, Mt, K, 56); }, big);
        flips([&](i64 M) { const i64 chunks = (M + CHUNK - 1) / CHUNK;
                           return M > 0x0fffffffLL || m > 0x0fffffffLL || m * M > 0x0fffffffLL || 32 * m * M * K + 8 * m * M + 8 * 56 * m * chunks > 0x3fffffffLL; },
              [&](i64 M) { return align_volume_pixels_fit(m, M, K, 56); }, big);
    }

    int main() {
        CHECK(kAlignChunk == CHUNK && align_chunks(1) == 1 && align_chunks(1024) == 1 && align_chunks(1025) == 2);
        for (i64 n : {1, 2, 3, 257})
            for (i64 m : {1, 2, 3, 257})
                for (i64 Mt : {1, 5, 1023, 1024, 1025})
                    for (int K : {1, 4, 9})
                        for (i64 NPt : {1, 6}) {
                            const i64 NP = n * NPt;
                            same(resample_layout(NPt, m * Mt, K), ref_resample(NPt, m * Mt, K));        // (M = m th tw points)
                            same(resample_volume_layout(NP, m * Mt, K), ref_volume(NP, m * Mt, K));
                            same(align_layout(NP, n, Mt, K, 29), ref_align(NP, n, Mt, K, 29));
                            same(align_layout(NP, n, Mt, K, 47), ref_align(NP, n, Mt, K, 47));
                            same(align_volume_layout(NP, m, Mt, K, 56), ref_align_volume(NP, m, Mt, K, 56));
                            check_solve(align_layout(NP, n, Mt, K, 29).total, n, 29, 4, 6, false);
                            check_solve(align_layout(NP, n, Mt, K, 47).total, n, 47, 4, 6, true);
                            check_solve(align_volume_layout(NP, m, Mt, K, 56).total, m, 56, 12, 9, false);
                            check_limits(n, m, Mt, K, NPt);
                        }
        // hand-picked rows at the boundaries: 2^28 points or pixels, 2^24 slices, 2^30 bytes of bins, of entries, of entries and records
        CHECK(resample_fits(0, 0x0fffffffLL, 1, 1) && !resample_fits(0, 0x10000000LL, 1, 1));              // M below 2^28 (no slice: 12 n M K does not bind)
        CHECK(resample_fits(0x0fffffffLL, 0, 1, 1) && !resample_fits(0x10000000LL, 0, 1, 1));               // n below 2^28
        CHECK(resample_fits(0, 0x7fffffffLL / 72, 9, 1) && !resample_fits(0, 0x7fffffffLL / 72 + 1, 9, 1));  // 8 M K below 2^31
        CHECK(resample_fits(2, 0x7fffffffLL / 96, 4, 1) && !resample_fits(2, 0x7fffffffLL / 96 + 1, 4, 1));  // 12 n M K below 2^31
        CHECK(resample_fits(0x3fffffffLL / 6, 1, 1, 6) && !resample_fits(0x3fffffffLL / 6 + 1, 1, 1, 6));    // n nV nH below 2^30
        CHECK(volume_points_fit(0x3fffffffLL / 40, 1) && !volume_points_fit(0x3fffffffLL / 40 + 1, 1));      // 32 M K + 8 M below 2^30
        CHECK(volume_points_fit(0x3fffffffLL / 296, 9) && !volume_points_fit(0x3fffffffLL / 296 + 1, 9));
        CHECK(volume_slices_fit(0x00ffffffLL, 1) && !volume_slices_fit(0x01000000LL, 1));                    // n an fp32 integer (16 n = 2^28)
        CHECK(volume_slices_fit(0x3fffffffLL / 96, 6) && !volume_slices_fit(0x3fffffffLL / 96 + 1, 6));      // 16 n nV nH below 2^30
        CHECK(bins_fit(0x3fffffffLL / 16, 1) && !bins_fit(0x3fffffffLL / 16 + 1, 1));
        CHECK(align_pixels_fit(0x3fffffffLL / 252, 1, 1, 29) && !align_pixels_fit(0x3fffffffLL / 252 + 1, 1, 1, 29));   // one pixel each: (20 + 232) n below 2^30
        CHECK(!align_pixels_fit(0x01000000LL, 0, 1, 29) && align_pixels_fit(0x00ffffffLL, 0, 1, 29));       // n below 2^24, whatever the pixels
        CHECK(!align_pixels_fit(1, 0x10000000LL, 1, 29) && !align_pixels_fit(2, 0x08000000LL, 1, 29));      // th tw, n th tw below 2^28
        {   // one slice: 20 M K + 232 ceil(M / 1024) below 2^30, a chunk boundary inside the search
            i64 lo = 0, hi = 0x0fffffffLL;   // (20 * 2^28 is refused)
            CHECK(!align_pixels_fit(1, hi, 1, 29));
            while (hi - lo > 1) { const i64 mid = (lo + hi) / 2; (20 * mid + 232 * ((mid + 1023) / 1024) > 0x3fffffffLL ? hi : lo) = mid; }
            CHECK(align_pixels_fit(1, lo, 1, 29) && !align_pixels_fit(1, lo + 1, 1, 29));
            CHECK(align_pixels_fit(1, lo, 1, 47) == !(20 * lo + 376 * ((lo + 1023) / 1024) > 0x3fffffffLL));  // the larger record refuses sooner or at the same size
        }
        CHECK(!align_volume_pixels_fit(1, 0x10000000LL, 1, 56) && !align_volume_pixels_fit(0x10000000LL, 1, 1, 56) && !align_volume_pixels_fit(0x4000, 0x4000, 1, 56));
        {
            i64 lo = 0, hi = 0x0fffffffLL;   // one target, K = 4: 136 Mt + 448 ceil(Mt / 1024) below 2^30
            while (hi - lo > 1) { const i64 mid = (lo + hi) / 2; (32 * mid * 4 + 8 * mid + 448 * ((mid + 1023) / 1024) > 0x3fffffffLL ? hi : lo) = mid; }
            CHECK(align_volume_pixels_fit(1, lo, 4, 56) && !align_volume_pixels_fit(1, lo + 1, 4, 56));
        }
        // a call at its limits stays below 2^30 bytes in each half of the bins, and below 2^31 in all
        {
            const i64 M = 0x3fffffffLL / 296;
            const GeomLayout l = resample_volume_layout(0x3fffffffLL / 16, M, 9);
            CHECK(l.total < ((size_t)1 << 31) && l.coords % 8 == 0);
        }
        std::puts("ok");
        return 0;
    }
""")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_align_plans(tmp_path):
    src = tmp_path / "align_plan.cpp"
    src.write_text(PROG)
    exe = tmp_path / "align_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mri_inr_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
