// msiren_residual_scale(_dev) on the host side, plain C++ without HIP (unit-tested on the CPU by tests/test_residual_scale_plan.py):
// what the call refuses before any launch, its chunking, its launch count and its block of the stream's scratch
//     [keys m th tw]                 uint32, one per pixel: the order-preserving key of the residual (then of the deviation), 0xFFFFFFFF = does not count
//     [partials m chunks x 256]      uint32 on a 16-byte boundary, one histogram of the current digit per workgroup, written in full by every pass (never zeroed, never added to)
//     [state S x 8]                  uint32 per segment: RscaleStateField
//     [group_start G + 1]            int32, only when the caller gives groups (rscale_upload_kernel)
// A target of th tw pixels is cut into chunks of kRscaleChunk pixels, one workgroup each, so a workgroup never straddles two segments; a segment is the
// targets group_start[g] .. group_start[g + 1] - 1 (without groups: target g).  m th tw < 2^28 keeps every pixel index, every count and every rank in
// 32 bits.  The launch sequence depends on the arguments alone: rscale_launches counts it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/msiren.h"
#include "align_plan.h"

namespace msiren {

constexpr int kRscaleChunk = 4096;     // pixels per workgroup: 16 per thread
constexpr int kRscaleBins = 256;       // an 8-bit digit: four passes per selection
constexpr int kRscalePasses = 4;
constexpr int kRscaleState = 8;        // uint32 words per segment
constexpr int kRscaleOffsets = 512;    // offsets of group_start per upload launch
constexpr int64_t kRscaleLimit = (int64_t)1 << 28;
constexpr uint32_t kRscaleNoKey = 0xFFFFFFFFu;
// prefix: the digits chosen so far (after the last pass: the key of rank k); rank: k among the keys that share the prefix; count: the pixels that count;
// k: the rank asked for; centre: the key of c (centre = 1)
enum RscaleStateField { RSCALE_PREFIX = 0, RSCALE_RANK = 1, RSCALE_COUNT = 2, RSCALE_K = 3, RSCALE_CENTRE = 4 };

inline int64_t rscale_chunks(int64_t pixels) { return (pixels + kRscaleChunk - 1) / kRscaleChunk; }                   // per target
inline int64_t rscale_segments(int64_t m, int64_t n_groups) { return n_groups > 0 ? n_groups : m; }
inline int64_t rscale_uploads(int64_t n_groups) { return n_groups > 0 ? (n_groups + 1 + kRscaleOffsets - 1) / kRscaleOffsets : 0; }

// Launches of one call that has work (m > 0 and th tw > 0; none otherwise): the uploads of group_start; per selection the keys with the first digit's
// histogram, three more histograms and a choice behind each of the four; the scales.  centre = 1 selects twice.  stats are written by the last kernel:
// no launch of their own.
inline int64_t rscale_launches(bool work, int centre, int64_t n_groups, bool /*stats*/) {
    return work ? rscale_uploads(n_groups) + (int64_t)(centre ? 2 : 1) * 2 * kRscalePasses + 1 : 0;
}

struct RscaleLayout {
    size_t keys, partials, state, group_start;  // offsets in bytes, each a multiple of 4; partials: of 16 (rscale_choose_kernel loads four bins at once)
    size_t total;                               // bytes of the call's block
};
inline RscaleLayout rscale_layout(int64_t m, int64_t pixels, int64_t n_groups) {
    RscaleLayout l{};
    const size_t M = (size_t)(m > 0 ? m : 0), P = (size_t)(pixels > 0 ? pixels : 0);
    l.keys = 0;
    l.partials = (l.keys + 4 * M * P + 15) & ~(size_t)15;
    l.state = l.partials + 4 * M * (size_t)rscale_chunks((int64_t)P) * kRscaleBins;
    l.group_start = l.state + 4 * (size_t)rscale_segments((int64_t)M, n_groups) * kRscaleState;
    l.total = l.group_start + (n_groups > 0 ? 4 * ((size_t)n_groups + 1) : 0);
    return l;
}

// The rule's order of float32 values as an order of uint32 keys: -0 before +0, every bit pattern distinct.  0xFFFFFFFF is the key of no finite value.
inline uint32_t rscale_key(uint32_t bits) { return bits & 0x80000000u ? ~bits : bits ^ 0x80000000u; }
inline uint32_t rscale_unkey(uint32_t key) { return key & 0x80000000u ? key ^ 0x80000000u : ~key; }
// k = (int64)floor(quantile (count - 1)), one fp64 multiply; count >= 1, 0 <= quantile <= 1: 0 <= k <= count - 1
inline int64_t rscale_rank(double quantile, int64_t count) { return (int64_t)std::floor(quantile * (double)(count - 1)); }
// s = (tune d)^2, at least floor
inline double rscale_scale(double tune, float d, double floor_) {
    const double t = tune * (double)d, s = t * t;
    return s > floor_ ? s : floor_;
}

// What one call is given.  `device`: the pointers are device pointers, whose alignment is checked.  group_start is a host array in both forms.
struct RscaleArgs {
    const void *targets, *simulated, *weights, *intensity;
    int64_t m;
    int32_t th, tw;
    const msiren_scale_opts* opts;
    const int32_t* group_start;
    int64_t n_groups;
    const void *scale, *stats;
    bool device;
};

// true: the call is accepted.  false: `msg` names the argument that is refused.
inline bool rscale_check(const RscaleArgs& a, char* msg, size_t cap) {
#define MSIREN_RSCALE_REFUSE(...) return std::snprintf(msg, cap, __VA_ARGS__), false
    if (a.m < 0) MSIREN_RSCALE_REFUSE("m_targets must be >= 0, got %lld", (long long)a.m);
    if (a.th < 0 || a.tw < 0) MSIREN_RSCALE_REFUSE("th and tw must be >= 0, got th=%d, tw=%d", a.th, a.tw);
    if (a.m > 0 && !a.opts) MSIREN_RSCALE_REFUSE("null argument (opts)");
    if (a.opts) {
        const msiren_scale_opts& o = *a.opts;
        if (o.struct_size != (int32_t)sizeof(msiren_scale_opts))
            MSIREN_RSCALE_REFUSE("opts->struct_size is %d, this library's msiren_scale_opts has %d bytes", o.struct_size, (int)sizeof(msiren_scale_opts));
        if (o.centre != 0 && o.centre != 1) MSIREN_RSCALE_REFUSE("opts->centre must be 0 or 1, got %d", o.centre);
        if (!(o.quantile >= 0 && o.quantile <= 1)) MSIREN_RSCALE_REFUSE("opts->quantile must be in [0, 1] and not NaN, got %g", o.quantile);
        if (!std::isfinite(o.tune) || !(o.tune > 0)) MSIREN_RSCALE_REFUSE("opts->tune must be finite and > 0, got %g", o.tune);
        if (!(o.floor >= 0) || std::isinf(o.floor)) MSIREN_RSCALE_REFUSE("opts->floor must be finite, >= 0 and not NaN, got %g", o.floor);
    }
    const int64_t pixels = (int64_t)a.th * a.tw;  // < 2^62
    if (a.m >= kRscaleLimit || pixels >= kRscaleLimit || a.m * pixels >= kRscaleLimit)
        MSIREN_RSCALE_REFUSE("too many target pixels for one call: m_targets th tw = %lld x %d x %d must stay below 2^28", (long long)a.m, a.th, a.tw);
    if (a.m > 0 && !a.targets) MSIREN_RSCALE_REFUSE("null argument (targets)");
    if (a.m > 0 && !a.scale) MSIREN_RSCALE_REFUSE("null argument (scale)");
    if (a.intensity && !a.simulated) MSIREN_RSCALE_REFUSE("intensity given without simulated");
    if (a.group_start || a.n_groups != 0) {
        int64_t at = 0;
        switch (group_start_check(a.group_start, a.n_groups, a.m, &at)) {
            case GROUPS_OK: break;
            case GROUPS_NONE: MSIREN_RSCALE_REFUSE("n_groups must be >= 1 where group_start is given (and 0 where it is not), got %lld", (long long)a.n_groups);
            case GROUPS_NULL: MSIREN_RSCALE_REFUSE("null argument (group_start) with n_groups = %lld", (long long)a.n_groups);
            case GROUPS_FIRST: MSIREN_RSCALE_REFUSE("group_start[0] = %d: the first offset must be 0", a.group_start[0]);
            case GROUPS_ORDER:
                MSIREN_RSCALE_REFUSE("group_start[%lld] = %d is not above group_start[%lld] = %d: offsets must be strictly ascending", (long long)at, a.group_start[at],
                                     (long long)at - 1, a.group_start[at - 1]);
            default: MSIREN_RSCALE_REFUSE("group_start[%lld] = %d: the last offset must be m = %lld", (long long)at, a.group_start[at], (long long)a.m);
        }
    }
    if (a.device) {
        const struct { const void* p; const char* name; } ptrs[] = {{a.targets, "targets"}, {a.simulated, "simulated"}, {a.weights, "weights"}, {a.intensity, "intensity"}};
        for (const auto& e : ptrs)
            if ((uintptr_t)e.p % 4) MSIREN_RSCALE_REFUSE("device %s must be 4-byte aligned", e.name);
        if ((uintptr_t)a.scale % 8) MSIREN_RSCALE_REFUSE("device scale must be 8-byte aligned");
        if ((uintptr_t)a.stats % 8) MSIREN_RSCALE_REFUSE("device stats must be 8-byte aligned");
    }
#undef MSIREN_RSCALE_REFUSE
    return true;
}

}  // namespace msiren
