// msiren_leave_out_targets(_dev) on the host side, plain C++ without HIP (unit-tested on the CPU by tests/test_leave_out_plan.py):
// what the call refuses before any launch, its launch count and its block of the stream's scratch
//     [records m x 20 doubles]     fuse_plan.h's, written by fuse_setup_kernel
//     [group_start G + 1]          int32, only when the caller gives groups (loo_upload_kernel), padded to a multiple of 16 bytes
//     [sums n H W x 2]             doubles (num_v, den_v) per voxel on a 16-byte boundary: loo_sums_kernel stores them, loo_gather_kernel loads a pair at once
//     [column sums m x tw x 4]     doubles, only when stats are asked for: project_plan.h's, parked by project_stats_kernel
// The tiling is the family's: one workgroup per 16 x 16 tile of voxels (the sums) or of one target's pixels (the gather).  The launch sequence depends
// on the arguments alone: leave_out_launches counts it.
#pragma once
#include "project_plan.h"

namespace msiren {

constexpr int kLooOffsets = 512;  // offsets of group_start per upload launch

inline int64_t leave_out_uploads(int64_t n_groups) { return n_groups > 0 ? (n_groups + 1 + kLooOffsets - 1) / kLooOffsets : 0; }

// Launches of one call.  With targets: the set-up, the uploads of group_start, the sums, the gather and, for residual or stats, project_stats_kernel.
// Without: the sums alone where the plain fusion is asked for (its voxels are NaN with coverage 0), else nothing.
inline int64_t leave_out_launches(bool targets, int64_t n_groups, bool residual_or_stats, bool volume) {
    return targets ? 1 + leave_out_uploads(n_groups) + 2 + (residual_or_stats ? 1 : 0) : volume ? 1 : 0;
}

struct LeaveOutLayout {
    size_t records, group_start, sums, columns;  // offsets in bytes; sums: a multiple of 16
    size_t total;                                // bytes of the call's block
};
inline LeaveOutLayout leave_out_layout(int64_t m, int32_t tw, int64_t n_groups, int64_t n, int32_t H, int32_t W, bool stats) {
    LeaveOutLayout l{};
    l.records = 0;
    l.group_start = fuse_records_bytes(m);  // (a multiple of 160)
    l.sums = l.group_start + (((n_groups > 0 && m > 0 ? 4 * ((size_t)n_groups + 1) : 0) + 15) & ~(size_t)15);
    l.columns = l.sums + (size_t)n * (size_t)H * (size_t)W * 2 * sizeof(double);
    l.total = l.columns + (stats && m > 0 ? (size_t)m * (size_t)tw * kProjectSums * sizeof(double) : 0);
    return l;
}

// What one call is given.  `device`: the pointers are device pointers, whose alignment is checked.  opts and group_start are host memory in both forms.
struct LeaveOutArgs {
    const void* targets;
    int64_t m;
    int32_t th, tw;
    const void *maps, *weights, *intensity;
    const msiren_fuse_opts* opts;
    const int32_t* group_start;
    int64_t n_groups;
    int64_t n;
    int32_t H, W;
    const void *simulated, *coverage, *residual, *stats, *flags, *volume, *volume_coverage;
    bool device;
};

// true: the call is accepted.  false: `msg` names the argument that is refused.
inline bool leave_out_check(const LeaveOutArgs& a, char* msg, size_t cap) {
#define MSIREN_LOO_REFUSE(...) return std::snprintf(msg, cap, __VA_ARGS__), false
    if (!fuse_check_sizes(a.m, a.th, a.tw, a.opts, a.n, a.H, a.W, msg, cap)) return false;
    if (a.m > 0 && !a.targets) MSIREN_LOO_REFUSE("null argument (targets)");
    if (a.m > 0 && !a.maps) MSIREN_LOO_REFUSE("null argument (maps)");
    if (a.m > 0 && !a.simulated) MSIREN_LOO_REFUSE("null argument (simulated)");
    if (a.group_start || a.n_groups != 0) {  // msiren_residual_scale's conventions, in its words (align_plan.h's group_start_check cannot be included here:
                                             // its SolveLayout is another than solve_volume_plan.h's, which shares this unit)
        const int32_t* g = a.group_start;
        const int64_t G = a.n_groups;
        if (G < 1) MSIREN_LOO_REFUSE("n_groups must be >= 1 where group_start is given (and 0 where it is not), got %lld", (long long)G);
        if (!g) MSIREN_LOO_REFUSE("null argument (group_start) with n_groups = %lld", (long long)G);
        if (g[0] != 0) MSIREN_LOO_REFUSE("group_start[0] = %d: the first offset must be 0", g[0]);
        for (int64_t i = 1; i <= G; ++i)
            if (g[i] <= g[i - 1])
                MSIREN_LOO_REFUSE("group_start[%lld] = %d is not above group_start[%lld] = %d: offsets must be strictly ascending", (long long)i, g[i], (long long)i - 1,
                                  g[i - 1]);
        if (g[G] != a.m) MSIREN_LOO_REFUSE("group_start[%lld] = %d: the last offset must be m = %lld", (long long)G, g[G], (long long)a.m);
    }
    if (a.device) {
        const struct { const void* p; const char* name; } ptrs[] = {{a.targets, "targets"}, {a.maps, "maps"}, {a.weights, "weights"}, {a.intensity, "intensity"},
                                                                    {a.simulated, "simulated"}, {a.coverage, "coverage"}, {a.residual, "residual"}, {a.flags, "flags"},
                                                                    {a.volume_coverage, "volume_coverage"}, {a.volume, "volume"}};
        for (const auto& e : ptrs)
            if ((uintptr_t)e.p % 4) MSIREN_LOO_REFUSE("device %s must be 4-byte aligned", e.name);
        if ((uintptr_t)a.stats % 8) MSIREN_LOO_REFUSE("device stats must be 8-byte aligned");
    }
#undef MSIREN_LOO_REFUSE
    return true;
}

}  // namespace msiren
