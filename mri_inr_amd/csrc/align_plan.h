// Scratch layouts and size limits of the geometry calls (plain C++, no HIP: unit-tested on the CPU by tests/test_align_plan.py): the five
// pipelines of resample.hip -- resample, resample-volume, align, align-w, align-volume (and its weighted form) -- the state of the solves, and
// the groups of the grouped volume solve.  Every call carves one block of its stream's scratch, in this order, offsets in bytes:
//     [counts B][cursors B][offsets B + 1][items B + 1][ent E][tile S][pair P]  ints, padded to an even count
//     [coords 2 E][w S][f P]                                                    floats; coords are float2: 8-byte aligned
//     [partials R records of `nsums` doubles]                                   behind the floats padded to an even count (align forms)
//     [solve state]                                                             behind the partials (solve_layout, group_solve_layout)
// B bins, E entries (what the ragged trunk evaluates), S slots (tile and fold weight), P points (pair of slices and fraction):
//     resample          B = nV nH      E = S = M K             P = 0          (M points, K = KA KA covering tiles at most)
//     resample-volume   B = n nV nH    E = 2 M K, S = M K      P = M
//     align, align-w    B = n nV nH    E = S = n th tw K       P = 0          R = n chunks, chunks = ceil(th tw / 1024), 29 / 47 sums
//     align-volume      B = n nV nH    E = 2 M K, S = M K      P = M = m th tw, R = m chunks, 56 sums
//     align-volume-w    align-volume's, with 80 sums (640 bytes per partial record)
//     align-stack       no bins, entries, slots or points: the block starts with the partials, R = m chunks, 80 sums (stack_layout)
// The memset in front of the count kernel covers counts and cursors: zero_bytes.  The limits keep every buffer of a call below 2^31 bytes and
// every index in 32 bits; the bin scratch over the points and over the bins stays below 2^30 each.
#pragma once
#include <cstddef>
#include <cstdint>

namespace msiren {

constexpr int64_t kAlignChunk = 1024;  // pixels per partial record (align.hip.h: ALIGN_CHUNK)
inline int64_t align_chunks(int64_t Mt) { return (Mt + kAlignChunk - 1) / kAlignChunk; }

struct GeomLayout {
    size_t counts, cursors, offsets, items, ent, tile, pair, coords, w, f, partials;  // partials: where they would start, also without any
    size_t zero_bytes;  // counts and cursors
    size_t total;       // bins + partials: what follows is the solve's
};

inline GeomLayout geom_layout(int64_t bins, int64_t entries, int64_t slots, int64_t points, int64_t records = 0, int nsums = 0) {
    const size_t B = (size_t)bins, E = (size_t)entries, S = (size_t)slots, P = (size_t)points;
    const size_t nint = (4 * B + 2 + E + S + P + 1) & ~(size_t)1, nflt = 2 * E + S + P;
    GeomLayout l{};
    l.counts = 0, l.cursors = 4 * B, l.offsets = 4 * (2 * B), l.items = 4 * (3 * B + 1), l.ent = 4 * (4 * B + 2);
    l.tile = l.ent + 4 * E, l.pair = l.tile + 4 * S;
    l.coords = 4 * nint, l.w = l.coords + 4 * (2 * E), l.f = l.w + 4 * S;
    l.partials = 4 * (nint + ((nflt + 1) & ~(size_t)1));
    l.zero_bytes = 2 * B * sizeof(int);
    l.total = records ? l.partials + (size_t)records * nsums * sizeof(double) : 4 * (nint + nflt);
    return l;
}
inline GeomLayout resample_layout(int64_t NPt, int64_t M, int K) { return geom_layout(NPt, M * K, M * K, 0); }
inline GeomLayout resample_volume_layout(int64_t NP, int64_t M, int K) { return geom_layout(NP, 2 * M * K, M * K, M); }
inline GeomLayout align_layout(int64_t NP, int64_t n, int64_t Mt, int K, int nsums) {
    return geom_layout(NP, n * Mt * K, n * Mt * K, 0, n * align_chunks(Mt), nsums);
}
inline GeomLayout align_volume_layout(int64_t NP, int64_t m, int64_t Mt, int K, int nsums) {
    return geom_layout(NP, 2 * m * Mt * K, m * Mt * K, m * Mt, m * align_chunks(Mt), nsums);
}

// align-stack: a plain voxel stack is read, so there are no bins, entries, slots or points -- the block is the partial
// records of `nsums` doubles at offset 0, and what follows them is the solve's (group_solve_layout).  Every other offset of the layout is 0 and unused.
inline GeomLayout stack_layout(int64_t m, int64_t Mt, int nsums) {
    GeomLayout l{};
    l.total = (size_t)m * (size_t)align_chunks(Mt) * nsums * sizeof(double);
    return l;
}

// A solve's state per unit (slice or target) behind `base` = GeomLayout::total, a multiple of 8: the doubles, then the 4-byte words.
//     [sums u nsums][sums_best u nsums][rigid_trial u nrigid][rigid_best u nrigid][scal u 3] [trial u nmap][best u nmap][gb_trial u 2][gb_best u 2][cnt u 2]
// align: (29, 4, 6), align-w: (47, 4, 6) with the (gain, bias) pair, align-volume: (56, 12, 9), align-volume-w: (80, 12, 9) with the pair
struct SolveLayout {
    size_t sums, sums_best, rigid_trial, rigid_best, scal, trial, best, gb_trial, gb_best, cnt;  // gb_*: = cnt without the pair
    size_t total;  // from the start of the scratch
};
inline SolveLayout solve_layout(size_t base, int64_t units, int nsums, int nrigid, int nmap, bool gb) {
    const size_t u = (size_t)units;
    SolveLayout s{};
    s.sums = base, s.sums_best = s.sums + 8 * u * nsums, s.rigid_trial = s.sums_best + 8 * u * nsums, s.rigid_best = s.rigid_trial + 8 * u * nrigid;
    s.scal = s.rigid_best + 8 * u * nrigid;
    s.trial = s.scal + 8 * u * 3, s.best = s.trial + 4 * u * nmap, s.gb_trial = s.best + 4 * u * nmap, s.gb_best = s.gb_trial + (gb ? 4 * u * 2 : 0);
    s.cnt = s.gb_best + (gb ? 4 * u * 2 : 0);
    s.total = s.cnt + 4 * u * 2;
    return s;
}

// The grouped volume solve (align_group.hip.h) behind `base`, a multiple of 8: per target the 80 sums at the trial and at
// the best state and one record of `nrec` doubles, per group the rigid states and `nscal` doubles; then the 4-byte words.
//     [sums m 80][sums_best m 80][rec m nrec][rigid_trial G 12][rigid_best G 12][scal G nscal]
//     [trial m 9][best m 9][gb_trial m 2][gb_best m 2][group_of m][group_start G + 1][cnt G ncnt]
struct GroupSolveLayout {
    size_t sums, sums_best, rec, rigid_trial, rigid_best, scal, trial, best, gb_trial, gb_best, group_of, group_start, cnt;
    size_t total;  // from the start of the scratch
};
inline GroupSolveLayout group_solve_layout(size_t base, int64_t m, int64_t G, int nsums, int nrec, int nscal, int ncnt) {
    const size_t u = (size_t)m, g = (size_t)G;
    GroupSolveLayout s{};
    s.sums = base, s.sums_best = s.sums + 8 * u * nsums, s.rec = s.sums_best + 8 * u * nsums, s.rigid_trial = s.rec + 8 * u * nrec;
    s.rigid_best = s.rigid_trial + 8 * g * 12, s.scal = s.rigid_best + 8 * g * 12;
    s.trial = s.scal + 8 * g * nscal, s.best = s.trial + 4 * u * 9, s.gb_trial = s.best + 4 * u * 9, s.gb_best = s.gb_trial + 4 * u * 2;
    s.group_of = s.gb_best + 4 * u * 2, s.group_start = s.group_of + 4 * u, s.cnt = s.group_start + 4 * (g + 1);
    s.total = s.cnt + 4 * g * ncnt;
    return s;
}

// group_start (G + 1) of the grouped solve: G >= 1 groups of consecutive targets, the first offset 0, the last m, strictly ascending (no empty
// group).  GROUPS_OK, or what is wrong and in *index the offending offset's index (GROUPS_ORDER: the first i with group_start[i] <=
// group_start[i - 1]; an offset outside 0 .. m shows as GROUPS_FIRST, GROUPS_ORDER or GROUPS_LAST).
enum GroupStartError { GROUPS_OK = 0, GROUPS_NONE, GROUPS_NULL, GROUPS_FIRST, GROUPS_ORDER, GROUPS_LAST };
inline GroupStartError group_start_check(const int32_t* group_start, int64_t G, int64_t m, int64_t* index) {
    *index = 0;
    if (G < 1) return GROUPS_NONE;
    if (!group_start) return GROUPS_NULL;
    if (group_start[0] != 0) return GROUPS_FIRST;
    for (int64_t i = 1; i <= G; ++i)
        if (group_start[i] <= group_start[i - 1]) return *index = i, GROUPS_ORDER;
    if (group_start[G] != m) return *index = G, GROUPS_LAST;
    return GROUPS_OK;
}

// The limits: true = the call fits.  NPt = nV nH tiles per slice.
inline bool resample_fits(int64_t n, int64_t M, int K, int64_t NPt) {  // the entries' coordinates (8 bytes each), the trunk's three planes
    return !(M > 0x0fffffffLL || n > 0x0fffffffLL || M * K * 8 > 0x7fffffffLL || n * M * K * 12 > 0x7fffffffLL || n * NPt > 0x3fffffffLL);
}
// 2 M K entries (slot and 8 bytes of coordinates), tile and weight per M K, pair and fraction per M: 32 M K + 8 M bytes
inline bool volume_points_fit(int64_t M, int K) { return !(M > 0x0fffffffLL || 32 * M * K + 8 * M > 0x3fffffffLL); }
inline bool bins_fit(int64_t n, int64_t NPt) { return !(16 * n * NPt > 0x3fffffffLL); }                       // 16 bytes per bin
inline bool volume_slices_fit(int64_t n, int64_t NPt) { return !(n > 0x00ffffffLL) && bins_fit(n, NPt); }  // n is compared as an fp32 integer
// 20 bytes per entry (slot, tile, weight, 8 bytes of coordinates) and one record per chunk; the trunk's three planes are 12 T bytes
inline bool align_pixels_fit(int64_t n, int64_t Mt, int K, int nsums) {
    return !(n > 0x00ffffffLL || Mt > 0x0fffffffLL || n * Mt > 0x0fffffffLL || 20 * n * Mt * K + 8 * nsums * n * align_chunks(Mt) > 0x3fffffffLL);
}
// resample-volume's bytes over M = m th tw pixels and one record per chunk; the trunk's three planes are 24 M K bytes
inline bool align_volume_pixels_fit(int64_t m, int64_t Mt, int K, int nsums) {
    return !(Mt > 0x0fffffffLL || m > 0x0fffffffLL || m * Mt > 0x0fffffffLL || 32 * m * Mt * K + 8 * m * Mt + 8 * nsums * m * align_chunks(Mt) > 0x3fffffffLL);
}
// align-stack: every extent is compared as an fp32 integer (below 2^24), a voxel's index stays below 2^30 and a pixel's below 2^28.  The arguments
// are not negative.
inline bool stack_voxels_fit(int64_t n, int64_t H, int64_t W) {
    return !(n > 0x00ffffffLL || H > 0x00ffffffLL || W > 0x00ffffffLL || n * H > 0x3fffffffLL || n * H * W > 0x3fffffffLL);
}
inline bool stack_pixels_fit(int64_t m, int64_t th, int64_t tw) {
    return !(m > 0x0fffffffLL || th * tw > 0x0fffffffLL || m * (th * tw) > 0x0fffffffLL);
}

}  // namespace msiren
