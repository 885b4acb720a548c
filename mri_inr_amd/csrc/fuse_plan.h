// msiren_fuse_targets(_dev) on the host side, plain C++ without HIP (unit-tested on the CPU by tests/test_fuse_reference.py):
// what the call refuses before any launch, its tiling and its block of the stream's scratch:
//     [records m x 20 doubles]   one per target, written by fuse_setup_kernel, read by fuse_gather_kernel with a wave-uniform index
// A record (FuseRecordField: the kernels of fuse.hip.h, project.hip.h and solve_volume.hip.h read it by these names):
//     [a 3][b 3][t 3][G11][G12][G22][det][dt][c 3][g][bias][flags]        flags as a double: 0, 1, 2 or 3
// One workgroup gathers a 16 x 16 (y, x) tile of one slice: ceil(H / 16) ceil(W / 16) n workgroups in a flat grid.  n H W < 2^30 keeps every
// voxel index and the tile count in 32 bits, m th tw < 2^30 every target index.  The tile, the record, its size and the tile counts below are the
// family's: project_plan.h and solve_volume_plan.h take them from here.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/msiren.h"

namespace msiren {

constexpr int kFuseTile = 16;      // voxels, or target pixels, per tile edge
constexpr int kFuseRecord = 20;    // doubles per target record
constexpr int64_t kFuseLimit = (int64_t)1 << 30;
enum FuseRecordField { FUSE_A = 0, FUSE_B = 3, FUSE_T = 6, FUSE_G11 = 9, FUSE_G12 = 10, FUSE_G22 = 11, FUSE_DET = 12, FUSE_DT = 13, FUSE_C = 14, FUSE_GAIN = 17,
                       FUSE_BIAS = 18, FUSE_FLAGS = 19 };

struct FuseLayout {
    size_t records;  // offset of the records
    size_t total;    // bytes of the call's block
};
inline size_t fuse_records_bytes(int64_t m) { return (size_t)(m > 0 ? m : 0) * kFuseRecord * sizeof(double); }
inline FuseLayout fuse_layout(int64_t m) { return FuseLayout{0, fuse_records_bytes(m)}; }

inline int64_t fuse_tiles_y(int32_t H) { return ((int64_t)H + kFuseTile - 1) / kFuseTile; }
inline int64_t fuse_tiles_x(int32_t W) { return ((int64_t)W + kFuseTile - 1) / kFuseTile; }
inline int64_t fuse_tiles(int64_t n, int32_t H, int32_t W) { return n * fuse_tiles_y(H) * fuse_tiles_x(W); }

// a b c < 2^30, without overflow for any int64 a and positive int32 b, c
inline bool fuse_product_fits(int64_t a, int32_t b, int32_t c) { return a < kFuseLimit && a * b < kFuseLimit && a * b * c < kFuseLimit; }

// What one call is given.  `device`: the pointers are device pointers, whose alignment is checked.
struct FuseArgs {
    const void* targets;
    int64_t m;
    int32_t th, tw;
    const void *maps, *weights, *intensity;
    const msiren_fuse_opts* opts;
    int64_t n;
    int32_t H, W;
    const void *volume, *coverage, *flags;
    bool device;
};

// What every call of the family refuses of the options and the sizes, in msiren_fuse_targets' words.  true: accepted.  false: `msg` names the argument.
inline bool fuse_check_sizes(int64_t m, int32_t th, int32_t tw, const msiren_fuse_opts* opts, int64_t n, int32_t H, int32_t W, char* msg, size_t cap) {
#define MSIREN_FUSE_REFUSE(...) return std::snprintf(msg, cap, __VA_ARGS__), false
    if (m < 0) MSIREN_FUSE_REFUSE("m_targets must be >= 0, got %lld", (long long)m);
    if (m > 0 && !opts) MSIREN_FUSE_REFUSE("null argument (opts)");
    if (opts) {
        const msiren_fuse_opts& o = *opts;
        if (o.struct_size != (int32_t)sizeof(msiren_fuse_opts))
            MSIREN_FUSE_REFUSE("opts->struct_size is %d, this library's msiren_fuse_opts has %d bytes", o.struct_size, (int)sizeof(msiren_fuse_opts));
        if (!std::isfinite(o.spacing) || !(o.spacing > 0)) MSIREN_FUSE_REFUSE("opts->spacing must be finite and > 0, got %g", o.spacing);
        if (!std::isfinite(o.thickness) || !(o.thickness > 0)) MSIREN_FUSE_REFUSE("opts->thickness must be finite and > 0, got %g", o.thickness);
        if (!(o.min_coverage >= 0)) MSIREN_FUSE_REFUSE("opts->min_coverage must be >= 0 and not NaN, got %g", o.min_coverage);
    }
    if (m > 0 && (th < 2 || tw < 2)) MSIREN_FUSE_REFUSE("th and tw must be >= 2 (a bilinear read needs two rows and two columns), got th=%d, tw=%d", th, tw);
    if (n < 1) MSIREN_FUSE_REFUSE("n_slices must be >= 1, got %lld", (long long)n);
    if (H < 1) MSIREN_FUSE_REFUSE("height must be >= 1, got %d", H);
    if (W < 1) MSIREN_FUSE_REFUSE("width must be >= 1, got %d", W);
    if (!fuse_product_fits(n, H, W)) MSIREN_FUSE_REFUSE("too many voxels for one call: n_slices height width = %lld x %d x %d must stay below 2^30", (long long)n, H, W);
    if (m > 0 && !fuse_product_fits(m, th, tw))
        MSIREN_FUSE_REFUSE("too many target pixels for one call: m_targets th tw = %lld x %d x %d must stay below 2^30", (long long)m, th, tw);
    return true;
}

// msiren_fuse_targets' own pointers, after fuse_check_sizes
inline bool fuse_check_pointers(const FuseArgs& a, char* msg, size_t cap) {
    if (a.m > 0 && !a.targets) MSIREN_FUSE_REFUSE("null argument (targets)");
    if (a.m > 0 && !a.maps) MSIREN_FUSE_REFUSE("null argument (maps)");
    if (a.m > 0 && !a.volume) MSIREN_FUSE_REFUSE("null argument (volume)");
    if (a.device) {
        const struct { const void* p; const char* name; } ptrs[] = {{a.targets, "targets"}, {a.maps, "maps"}, {a.weights, "weights"}, {a.intensity, "intensity"},
                                                                    {a.volume, "volume"}, {a.coverage, "coverage"}, {a.flags, "flags"}};
        for (const auto& e : ptrs)
            if ((uintptr_t)e.p % 4) MSIREN_FUSE_REFUSE("device %s must be 4-byte aligned", e.name);
    }
#undef MSIREN_FUSE_REFUSE
    return true;
}

// true: the call is accepted.  false: `msg` names the argument that is refused.
inline bool fuse_check(const FuseArgs& a, char* msg, size_t cap) {
    return fuse_check_sizes(a.m, a.th, a.tw, a.opts, a.n, a.H, a.W, msg, cap) && fuse_check_pointers(a, msg, cap);
}

}  // namespace msiren
