// msiren_solve_volume_r(_dev) on the host side, plain C++ without HIP (unit-tested on the CPU by
// tests/test_solve_volume_robust_reference.py): what the call refuses before any launch, its block of the stream's scratch
//     [solve_volume_plan.h's block]   records, x r p q, D Wt z, column sums, slice sums, state: Wt holds the round's reweighted (w g) g omega
//     [Wt0][z']                       two more pixel vectors of m th tw doubles: the weight (w g) g that solve_coverage_kernel writes once, and A x's pixel
//                                     vector (Wt u) / D of the reweighting pass (the transpose reads it in place of z)
//     [stats columns m x tw x 4]      irls_stats_kernel parks (count, sum w, sum w omega, sum ((w om) e) e) per column
// the schedule of the scales, and the launch plan: how many kernels one call enqueues.  The sequence depends on m > 0, start, coverage, rounds,
// iterations and whether a final pass is asked for, never on the data.  In the final pass the reweighting kernel no longer needs Wt, z and z': it
// parks there what irls_stats_kernel reads -- whether the pixel counts (1.0 or 0.0), e and om.
#pragma once
#include <cmath>

#include "solve_volume_plan.h"

namespace msiren {

constexpr int kSolveRMaxRounds = 64;
constexpr int kSolveRSums = 4;  // doubles per column: count, sum w, sum w omega, sum ((w om) e) e

struct SolveRLayout {
    SolveLayout base;                 // section 5.19's block, unchanged
    size_t Wt0, zp, stat_columns;     // offsets
    size_t total;                     // bytes of the call's block
};
inline SolveRLayout solve_r_layout(int64_t m, int32_t th, int32_t tw, int64_t n, int32_t H, int32_t W) {
    SolveRLayout l;
    l.base = solve_layout(m, th, tw, n, H, W);
    const size_t pix = m > 0 ? (size_t)m * (size_t)th * (size_t)tw * sizeof(double) : 0;
    const size_t col = m > 0 ? (size_t)m * (size_t)tw * kSolveRSums * sizeof(double) : 0;
    l.Wt0 = l.base.total, l.zp = l.Wt0 + pix, l.stat_columns = l.zp + pix;
    l.total = l.stat_columns + col;
    return l;
}

// c[t], t = 0 .. rounds - 1: the factor of every target's scale in round t.  c[rounds - 1] = 1.0, c[t] = c[t + 1] anneal, in fp64
inline void solve_r_schedule(int32_t rounds, double anneal, double* c) {
    for (int t = rounds - 1; t >= 0; --t) c[t] = t == rounds - 1 ? 1.0 : c[t + 1] * anneal;
}

// the kernels one call enqueues (tests, and the cost notes of section 5.20)
inline int64_t solve_r_launches(int64_t m, bool start, bool coverage, int32_t rounds, int32_t iterations, bool final_pass) {
    const int64_t gathers = m > 0 ? 1 : 0;                          // a forward gather exists only with targets
    int64_t k = (m > 0 ? 1 : 0) + (!start || coverage ? 1 : 0);     // set-up; the fusion (start and / or coverage)
    k += 1 + gathers;                                               // start, coverage
    const int64_t boundary = gathers + 1 + 1 + 1 + 2 + 1;           // reweight, Pt z, Pt z' + lambda L x, residual, <r, r>, stopped_at[t]
    const int64_t step = gathers + 1 + 2 + 1 + 2 + 1;               // P p, A p, <p, q>, x and r, <r, r>, p
    k += (int64_t)rounds * (boundary + (int64_t)iterations * step);
    if (final_pass) k += 2 * gathers;                               // reweight, stats
    return k + 1;                                                   // store
}

// What one call is given.  `device`: the pointers are device pointers, whose alignment is checked.
struct SolveRArgs {
    const void* targets;
    int64_t m;
    int32_t th, tw;
    const void *maps, *weights, *intensity, *scale;
    const msiren_solve_r_opts* opts;
    int64_t n;
    int32_t H, W;
    const void *start, *volume, *coverage, *history, *flags, *stopped_at, *rweight, *residual, *stats;
    bool device;
};

// the options as msiren_solve_volume takes them
inline msiren_solve_opts solve_r_solve_opts(const msiren_solve_r_opts& o) {
    return msiren_solve_opts{(int32_t)sizeof(msiren_solve_opts), o.iterations, o.spacing, o.thickness, o.min_coverage, o.lambda};
}

// true: the call is accepted.  false: `msg` names the argument that is refused.
inline bool solve_r_check(const SolveRArgs& a, char* msg, size_t cap) {
#define MSIREN_SOLVE_R_REFUSE(...) return std::snprintf(msg, cap, __VA_ARGS__), false
    if (!a.opts) MSIREN_SOLVE_R_REFUSE("null argument (opts)");
    const msiren_solve_r_opts& o = *a.opts;
    if (o.struct_size != (int32_t)sizeof(msiren_solve_r_opts))
        MSIREN_SOLVE_R_REFUSE("opts->struct_size is %d, this library's msiren_solve_r_opts has %d bytes", o.struct_size, (int)sizeof(msiren_solve_r_opts));
    // what msiren_solve_volume refuses, in its words
    const msiren_solve_opts so = solve_r_solve_opts(o);
    const SolveArgs s{a.targets, a.m, a.th, a.tw, a.maps, a.weights, a.intensity, &so, a.n, a.H, a.W, a.start, a.volume, a.coverage, a.history, a.flags, a.stopped_at, a.device};
    if (!solve_check(s, msg, cap)) return false;
    if (o.rounds < 0 || o.rounds > kSolveRMaxRounds) MSIREN_SOLVE_R_REFUSE("opts->rounds must be in [0, %d], got %d", kSolveRMaxRounds, o.rounds);
    if ((int64_t)o.rounds * o.iterations > kSolveMaxIterations)
        MSIREN_SOLVE_R_REFUSE("opts->rounds x opts->iterations must be at most %d, got %d x %d", kSolveMaxIterations, o.rounds, o.iterations);
    if (!std::isfinite(o.anneal) || !(o.anneal >= 1)) MSIREN_SOLVE_R_REFUSE("opts->anneal must be finite and >= 1, got %g", o.anneal);
    if (a.m > 0 && !a.scale) MSIREN_SOLVE_R_REFUSE("null argument (scale)");
    if (a.device) {
        if ((uintptr_t)a.scale % 8) MSIREN_SOLVE_R_REFUSE("device scale must be 8-byte aligned");
        if ((uintptr_t)a.stats % 8) MSIREN_SOLVE_R_REFUSE("device stats must be 8-byte aligned");
        if ((uintptr_t)a.rweight % 4) MSIREN_SOLVE_R_REFUSE("device rweight must be 4-byte aligned");
        if ((uintptr_t)a.residual % 4) MSIREN_SOLVE_R_REFUSE("device residual must be 4-byte aligned");
    }
#undef MSIREN_SOLVE_R_REFUSE
    return true;
}

}  // namespace msiren
