// Robust reconstruction (msiren_solve_volume_r*): rounds of section 5.19's conjugate gradients, each on the normal equations
// reweighted by the Geman-McClure weight of every pixel's residual against the current iterate, warm-started from x in fp64.  The rule is
// include/msiren.h's, restated in numpy by mri_inr_amd/solve_volume_robust.py (solve_volume_robust_on_host): fp64 + - * /, contraction off, one
// rounding per operation -- the two agree bit for bit.  Everything but the reweighting is solve_volume.hip.h's, launched as it is.
//
//   irls_reweight_kernel   one thread per target pixel over project_visit_voxels' box, the record in SGPRs, no LDS, no atomics, no barrier: the forward
//                          gather of x (num), then on an active pixel u = num / D, e = T - ((g u) + b), om = 1 / (1 + (e e) / s), omega = om om and, in
//                          one pass, Wt = Wt0 omega, z = (Wt tau) / D (the right-hand side's pixel vector) and z' = (Wt u) / D (A x's): a round boundary
//                          costs one gather and two launches of solve_transpose_kernel.  All three are +0.0 on a pixel that is not active.
//                          The final pass (after the last round, scale factor 1.0) stores [rweight], [residual] and parks in the three vectors,
//                          which nothing reads any more, what irls_stats_kernel needs: whether the pixel counts (1.0 / 0.0), e and om
//   irls_stats_kernel      one workgroup per target, project_stats_kernel's layout: thread tid sums the columns tid, tid + 256, ... down the rows, parks
//                          the four sums per column in the stream's scratch, and after a barrier threads 0 .. 3 add one quantity each over the columns
//   irls_stop_kernel       stopped_at[t] of the round that has just ended, from the solve's scalars
#pragma once
#include <hip/hip_runtime.h>

#include "solve_volume.hip.h"
#include "solve_volume_r_plan.h"

namespace msiren {

// x (n, H, W) fp64, +0.0 outside the support; targets (m, th, tw); rec, D, Wt0 (m, th, tw); scale (m); c: the round's factor of the scale.
// final_pass == 0 -> Wt, zz, zp (m, th, tw).  final_pass != 0 -> Wt = counts, zz = e, zp = om; rweight, residual (m, th, tw) or null.
// grid: tiles_y tiles_x m workgroups (fuse_tile_lane)
__global__ __launch_bounds__(256) void irls_reweight_kernel(const double* __restrict__ x, const float* __restrict__ targets, const double* __restrict__ rec,
                                                            const double* __restrict__ D, const double* __restrict__ Wt0, const double* __restrict__ scale, double c,
                                                            int final_pass, int th, int tw, int n, int H, int W, int tiles_x, int tiles_y, double spacing,
                                                            double thickness, double* __restrict__ Wt, double* __restrict__ zz, double* __restrict__ zp,
                                                            float* __restrict__ rweight, float* __restrict__ residual) {
#pragma clang fp contract(off)
    const FuseTileLane l = fuse_tile_lane(tiles_x, tiles_y);
    const int q = l.outer, pi = l.row, pj = l.col;
    const bool inside = pi < th && pj < tw;
    const size_t at = ((size_t)q * th + (inside ? pi : 0)) * tw + (inside ? pj : 0);
    const double* r = rec + (size_t)q * kFuseRecord;  // wave-uniform: scalar loads
    const float nanf = __builtin_nanf("");
    if (r[FUSE_FLAGS] != 0.0) {                       // a flagged target: no pixel is active
        if (inside) {
            Wt[at] = 0.0, zz[at] = 0.0, zp[at] = 0.0;
            if (final_pass) {
                if (rweight) rweight[at] = nanf;
                if (residual) residual[at] = nanf;
            }
        }
        return;
    }
    double num = 0.0;  // section 5.19's forward gather of x: every voxel takes part (shortcut 1 of solve_volume.hip.h)
    project_visit_voxels(
        r, pi, pj, th, tw, n, H, W, spacing, thickness, [](size_t) { return true; }, [&](size_t u, double kb) { num += kb * x[u]; });
    if (!inside) return;
    const double d = D[at];
    if (!(d > 0.0)) {  // not active
        Wt[at] = 0.0, zz[at] = 0.0, zp[at] = 0.0;
        if (final_pass) {
            if (rweight) rweight[at] = nanf;
            if (residual) residual[at] = nanf;
        }
        return;
    }
    const double s = scale[q] * c;  // (wave-uniform)
    const double g = r[FUSE_GAIN], bias = r[FUSE_BIAS];
    const double T = (double)targets[at];
    const double u = num / d;
    const double sim = (g * u) + bias, e = T - sim;
    const double a = (e * e) / s, v = 1.0 + a, om = 1.0 / v;
    const bool positive = s > 0.0;  // (a NaN fails)
    const double omega = positive ? om * om : 0.0;
    if (final_pass) {
        Wt[at] = positive ? 1.0 : 0.0, zz[at] = e, zp[at] = om;
        if (rweight) rweight[at] = positive ? (float)omega : nanf;
        if (residual) residual[at] = (float)e;
        return;
    }
    const double wt = Wt0[at] * omega, tau = (T - bias) / g;
    Wt[at] = wt;
    zz[at] = (wt * tau) / d;
    zp[at] = (wt * u) / d;
}

// weights (m, th, tw) or null; counts, e, om (m, th, tw): the final pass of irls_reweight_kernel; columns (m, tw, 4): scratch -> stats (m, 4) or null
__global__ __launch_bounds__(256) void irls_stats_kernel(const float* __restrict__ weights, const double* __restrict__ counts, const double* __restrict__ ee,
                                                         const double* __restrict__ oms, int th, int tw, double* columns, double* stats) {
#pragma clang fp contract(off)
    if (!stats) return;  // (the same in every thread)
    const int q = blockIdx.x, tid = threadIdx.x;
    double* col = columns + (size_t)q * tw * kSolveRSums;
    for (int j = tid; j < tw; j += 256) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int i = 0; i < th; ++i) {
            const size_t at = ((size_t)q * th + i) * tw + j;
            if (counts[at] != 0.0) {
                const double wd = weights ? (double)weights[at] : 1.0, om = oms[at], e = ee[at];
                s0 += 1.0;
                s1 += wd;
                s2 += wd * (om * om);
                s3 += ((wd * om) * e) * e;
            }
        }
        col[4 * j] = s0, col[4 * j + 1] = s1, col[4 * j + 2] = s2, col[4 * j + 3] = s3;
    }
    __syncthreads();
    if (tid < 4) {
        double s = 0.0;
        for (int j = 0; j < tw; ++j) s += col[4 * j + tid];
        stats[4 * (size_t)q + tid] = s;
    }
}

// stopped_at (rounds) or null
__global__ __launch_bounds__(256) void irls_stop_kernel(const double* __restrict__ state, int t, int* __restrict__ stopped_at) {
    if (threadIdx.x == 0 && stopped_at) stopped_at[t] = (int)state[SOLVE_STOPPED_AT];
}

}  // namespace msiren
