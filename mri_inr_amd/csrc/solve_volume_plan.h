// msiren_solve_volume(_dev) on the host side, plain C++ without HIP (unit-tested on the CPU by
// tests/test_solve_volume_reference.py): what the call refuses before any launch, its block of the stream's scratch
//     [records m x 20 doubles]        fuse_plan.h's, written by fuse_setup_kernel
//     [x][r][p][q]                    four voxel vectors of n H W doubles: the iterate, the residual, the search direction, A p
//     [D][Wt][z]                      three pixel vectors of m th tw doubles: the row sum of P over the support (0.0 on a pixel that is not active), the
//                                     pixel weight (w g) g, and what the transpose reads, (Wt u) / D
//     [column sums n x W][slice sums n][state 8]     the ordered inner product's partial sums and the solve's scalars (SolveState)
// and the launch plan: how many kernels one call enqueues.  The sequence depends on m > 0, start, coverage and iterations alone, never on the data:
// a solve that has stopped still launches every kernel of the remaining iterations, which then leave x, r and p as they are.
#pragma once
#include <cmath>

#include "fuse_plan.h"

namespace msiren {

constexpr int kSolveMaxIterations = 1024;
constexpr int kSolveState = 8;  // doubles
enum SolveStateField { SOLVE_RHO = 0, SOLVE_ALPHA = 1, SOLVE_BETA = 2, SOLVE_STOPPED = 3, SOLVE_STOPPED_AT = 4 };
enum SolveReduceMode { SOLVE_REDUCE_FIRST = 0, SOLVE_REDUCE_GAMMA = 1, SOLVE_REDUCE_RHO = 2 };

struct SolveLayout {
    size_t records, x, r, p, q, D, Wt, z, columns, slices, state;  // offsets
    size_t total;                                                  // bytes of the call's block
};
inline SolveLayout solve_layout(int64_t m, int32_t th, int32_t tw, int64_t n, int32_t H, int32_t W) {
    const size_t rec = fuse_records_bytes(m);
    const size_t vox = (size_t)n * (size_t)H * (size_t)W * sizeof(double), pix = m > 0 ? (size_t)m * (size_t)th * (size_t)tw * sizeof(double) : 0;
    const size_t col = (size_t)n * (size_t)W * sizeof(double), sl = (size_t)n * sizeof(double);
    SolveLayout l;
    l.records = 0;
    l.x = rec, l.r = l.x + vox, l.p = l.r + vox, l.q = l.p + vox;
    l.D = l.q + vox, l.Wt = l.D + pix, l.z = l.Wt + pix;
    l.columns = l.z + pix, l.slices = l.columns + col, l.state = l.slices + sl;
    l.total = l.state + kSolveState * sizeof(double);
    return l;
}

// the kernels one call enqueues (tests, and the cost notes of section 5.19)
inline int64_t solve_launches(int64_t m, bool start, bool coverage, int32_t iterations) {
    const int64_t gathers = m > 0 ? 1 : 0;                          // a forward gather exists only with targets
    int64_t k = (m > 0 ? 1 : 0) + (!start || coverage ? 1 : 0);     // set-up; the fusion (start and / or coverage)
    k += 1 + gathers + 1 + gathers + 1 + 1 + 2;                     // start, coverage, rhs, P x, A x, residual, <r, r>
    k += (int64_t)iterations * (gathers + 1 + 2 + 1 + 2 + 1);       // P p, A p, <p, q>, x and r, <r, r>, p
    return k + 1;                                                   // store
}

inline int64_t solve_dot_blocks(int64_t n, int32_t W) { return (n * W + 255) / 256; }
inline int64_t solve_pointwise_blocks(int64_t n, int32_t H, int32_t W) { return (n * H * W + 255) / 256; }

// What one call is given.  `device`: the pointers are device pointers, whose alignment is checked.
struct SolveArgs {
    const void* targets;
    int64_t m;
    int32_t th, tw;
    const void *maps, *weights, *intensity;
    const msiren_solve_opts* opts;
    int64_t n;
    int32_t H, W;
    const void *start, *volume, *coverage, *history, *flags, *stopped_at;
    bool device;
};

// the options as msiren_fuse_targets takes them
inline msiren_fuse_opts solve_fuse_opts(const msiren_solve_opts& o) { return msiren_fuse_opts{(int32_t)sizeof(msiren_fuse_opts), 0, o.spacing, o.thickness, o.min_coverage}; }

// true: the call is accepted.  false: `msg` names the argument that is refused.
inline bool solve_check(const SolveArgs& a, char* msg, size_t cap) {
#define MSIREN_SOLVE_REFUSE(...) return std::snprintf(msg, cap, __VA_ARGS__), false
    if (!a.opts) MSIREN_SOLVE_REFUSE("null argument (opts)");
    const msiren_solve_opts& o = *a.opts;
    if (o.struct_size != (int32_t)sizeof(msiren_solve_opts))
        MSIREN_SOLVE_REFUSE("opts->struct_size is %d, this library's msiren_solve_opts has %d bytes", o.struct_size, (int)sizeof(msiren_solve_opts));
    if (!a.volume) MSIREN_SOLVE_REFUSE("null argument (volume)");
    // what msiren_fuse_targets refuses, in its words
    const msiren_fuse_opts fo = solve_fuse_opts(o);
    const FuseArgs f{a.targets, a.m, a.th, a.tw, a.maps, a.weights, a.intensity, &fo, a.n, a.H, a.W, a.volume, a.coverage, a.flags, a.device};
    if (!fuse_check(f, msg, cap)) return false;
    if (o.iterations < 0 || o.iterations > kSolveMaxIterations) MSIREN_SOLVE_REFUSE("opts->iterations must be in [0, %d], got %d", kSolveMaxIterations, o.iterations);
    if (!std::isfinite(o.lambda) || !(o.lambda >= 0)) MSIREN_SOLVE_REFUSE("opts->lambda must be finite and >= 0, got %g", o.lambda);
    if (a.device) {
        if ((uintptr_t)a.start % 4) MSIREN_SOLVE_REFUSE("device start must be 4-byte aligned");
        if ((uintptr_t)a.history % 8) MSIREN_SOLVE_REFUSE("device history must be 8-byte aligned");
        if ((uintptr_t)a.stopped_at % 4) MSIREN_SOLVE_REFUSE("device stopped_at must be 4-byte aligned");
    }
#undef MSIREN_SOLVE_REFUSE
    return true;
}

}  // namespace msiren
