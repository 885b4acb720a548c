// The stack that best explains all aligned targets at once (msiren_solve_volume*): a fixed number of conjugate-gradient
// iterations on (Pt Omega P + lambda L) x = Pt Omega tau over the support, P the row-normalised projection of project.hip.h.  The rule is
// include/msiren.h's, restated in numpy by mri_inr_amd/solve_volume.py (solve_volume_on_host): fp64 + - * /, contraction off, one rounding per
// operation -- the two agree bit for bit.  The per-target record is fuse_setup_kernel's; p, pa, pb, cp, i, j, k, the contribution test, i0, j0, fi,
// fj and the four beta are written once per side: fuse_visit_targets (fuse.hip.h, with the cull and its proof) for the transpose, project_visit_voxels
// (project.hip.h, with the box and the early window test) for the two forward gathers.
//
//   solve_start_kernel       x = (double)start on the support (the finite voxels of `sup`), 0.0 elsewhere
//   solve_coverage_kernel    once, one thread per target pixel over project_visit_voxels' box: D = section 5.18's den over the support; the pixel is
//                            ACTIVE iff its target is unflagged, T and w are a valid tap and D > min_coverage.  Writes D (0.0 where not active),
//                            Wt = (w g) g and z = (Wt tau) / D, the right-hand side's pixel vector
//   solve_forward_kernel     the same gather with the fp64 entry of v: num, then z = (Wt (num / D)) / D on the active pixels, 0.0 elsewhere.  The record in
//                            SGPRs, no LDS, no atomics, no barrier
//   solve_transpose_kernel   fuse_gather_kernel's tiling and loop (fuse_visit_targets), one workgroup per 16 x 16 tile: per voxel acc += k sn with sn
//                            the sum over the four taps of beta z_p, then out = acc + (lambda (L v)) with the six-neighbour Laplacian of v: A v in one
//                            pass over the voxels
//   solve_residual_kernel    r = r - q, p = r (the start of the loop)
//   solve_dot_kernel         one thread per (slice, column) goes down the rows, coalesced across the lanes, and parks the column's sum
//   solve_reduce_kernel      one workgroup: thread z adds the columns of slice z ascending, thread 0 the slices ascending, then updates the solve's
//                            scalars (solve_volume_plan.h: SolveState) and the history with plain stores
//   solve_update_xr_kernel   x += alpha p, r -= alpha q;   solve_update_p_kernel   p = r + beta p;   both leave everything as it is once the solve stopped
//   solve_store_kernel       volume = (float)x on the support, NaN elsewhere; [stopped_at]
// Two shortcuts that change no bit.  (1) The vectors x, r, p, q are +0.0 outside the support (every kernel that writes them sees to that), so the
// forward gather does not test the support: such a voxel adds kb (+0.0) = +0.0 (kb = k beta >= 0), and num, which starts at +0.0 and is a sum, is
// never -0.0, so num + 0.0 = num.  (2) z is +0.0 on a pixel that is not active, and z = y / D is one division per pixel instead of one per tap: the
// transpose adds beta (+0.0) = +0.0 to sn for such a tap, which changes no bit for the same reason, and beta (y_p / D_p) has the operands of the rule.
#pragma once
#include <hip/hip_runtime.h>

#include "project.hip.h"
#include "solve_volume_plan.h"

namespace msiren {

__global__ __launch_bounds__(256) void solve_start_kernel(const float* __restrict__ sup, int voxels, double* __restrict__ x) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= voxels) return;
    const float s = sup[e];
    x[e] = __builtin_isfinite(s) ? (double)s : 0.0;
}

// sup (n, H, W), targets, weights or null (m, th, tw), rec -> D, Wt, z (m, th, tw).  grid: tiles_y tiles_x m workgroups (fuse_tile_lane)
__global__ __launch_bounds__(256) void solve_coverage_kernel(const float* __restrict__ sup, const float* __restrict__ targets, const float* __restrict__ weights,
                                                             const double* __restrict__ rec, int th, int tw, int n, int H, int W, int tiles_x, int tiles_y, double spacing,
                                                             double thickness, double min_coverage, double* __restrict__ D, double* __restrict__ Wt, double* __restrict__ zz) {
#pragma clang fp contract(off)
    const FuseTileLane l = fuse_tile_lane(tiles_x, tiles_y);
    const int q = l.outer, pi = l.row, pj = l.col;
    const bool inside = pi < th && pj < tw;
    const size_t at = ((size_t)q * th + (inside ? pi : 0)) * tw + (inside ? pj : 0);
    const double* r = rec + (size_t)q * kFuseRecord;  // wave-uniform: scalar loads
    if (r[FUSE_FLAGS] != 0.0) {                       // a flagged target: no pixel is active
        if (inside) D[at] = 0.0, Wt[at] = 0.0, zz[at] = 0.0;
        return;
    }
    double den = 0.0;  // the window x bilinear weights of the voxels of the support
    project_visit_voxels(
        r, pi, pj, th, tw, n, H, W, spacing, thickness, [&](size_t v) { return __builtin_isfinite(sup[v]); }, [&](size_t, double kb) { den += kb; });
    if (inside) {
        const float T = targets[at], w = weights ? weights[at] : 1.f;
        const bool active = __builtin_isfinite(T) && __builtin_isfinite(w) && w > 0.f && den > min_coverage;
        const double g = r[FUSE_GAIN], bias = r[FUSE_BIAS];
        const double wt = ((double)w * g) * g, tau = ((double)T - bias) / g;
        D[at] = active ? den : 0.0;
        Wt[at] = active ? wt : 0.0;
        zz[at] = active ? (wt * tau) / den : 0.0;
    }
}

// v (n, H, W) fp64, +0.0 outside the support; rec, D, Wt (m, th, tw) -> z (m, th, tw).  A flagged target's z stays the 0.0 of solve_coverage_kernel
__global__ __launch_bounds__(256) void solve_forward_kernel(const double* __restrict__ v, const double* __restrict__ rec, const double* __restrict__ D,
                                                            const double* __restrict__ Wt, int th, int tw, int n, int H, int W, int tiles_x, int tiles_y, double spacing,
                                                            double thickness, double* __restrict__ zz) {
#pragma clang fp contract(off)
    const FuseTileLane l = fuse_tile_lane(tiles_x, tiles_y);
    const int q = l.outer, pi = l.row, pj = l.col;
    const bool inside = pi < th && pj < tw;
    const size_t at = ((size_t)q * th + (inside ? pi : 0)) * tw + (inside ? pj : 0);
    const double* r = rec + (size_t)q * kFuseRecord;  // wave-uniform: scalar loads
    if (r[FUSE_FLAGS] != 0.0) return;
    double num = 0.0;  // those weights times v: every voxel takes part (shortcut 1 of the header comment)
    project_visit_voxels(
        r, pi, pj, th, tw, n, H, W, spacing, thickness, [](size_t) { return true; }, [&](size_t u, double kb) { num += kb * v[u]; });
    if (inside) {
        const double d = D[at];
        zz[at] = d > 0.0 ? (Wt[at] * (num / d)) / d : 0.0;
    }
}

// zz (m, th, tw), rec, sup (n, H, W); v (n, H, W) or null: with it out = Pt z + (lambda (L v)), without it out = Pt z; 0.0 outside the support.
// grid: tiles_y tiles_x n workgroups (fuse_tile_lane).  The loop over the targets and its cull are fuse.hip.h's fuse_visit_targets
__global__ __launch_bounds__(256) void solve_transpose_kernel(const double* __restrict__ zz, const double* __restrict__ rec, const float* __restrict__ sup,
                                                              const double* __restrict__ v, int m, int th, int tw, int n, int H, int W, int tiles_x, int tiles_y,
                                                              double spacing, double lambda, double cz, double* __restrict__ out) {
#pragma clang fp contract(off)
    const FuseTileLane l = fuse_tile_lane(tiles_x, tiles_y);
    const int z = l.outer, y = l.row, x = l.col;
    double acc = 0.0;
    fuse_visit_targets(rec, m, th, tw, l, spacing, [&](const double*, double k, int at, double gi, double gj, double fi, double fj) {
        double sn = 0.0;
        sn += (gi * gj) * zz[at];
        sn += (gi * fj) * zz[at + 1];
        sn += (fi * gj) * zz[at + tw];
        sn += (fi * fj) * zz[at + tw + 1];
        acc += k * sn;
    });
    if (y < H && x < W) {
        const int HW = H * W;
        const int at = (z * H + y) * W + x;  // n H W < 2^30
        double res = 0.0;
        if (__builtin_isfinite(sup[at])) {
            res = acc;
            if (v) {
                const double vu = v[at];
                double s = 0.0;
                if (z > 0 && __builtin_isfinite(sup[at - HW])) s += cz * (vu - v[at - HW]);
                if (z < n - 1 && __builtin_isfinite(sup[at + HW])) s += cz * (vu - v[at + HW]);
                if (y > 0 && __builtin_isfinite(sup[at - W])) s += vu - v[at - W];
                if (y < H - 1 && __builtin_isfinite(sup[at + W])) s += vu - v[at + W];
                if (x > 0 && __builtin_isfinite(sup[at - 1])) s += vu - v[at - 1];
                if (x < W - 1 && __builtin_isfinite(sup[at + 1])) s += vu - v[at + 1];
                res = acc + (lambda * s);
            }
        }
        out[at] = res;
    }
}

// r = r - q, p = r (both vectors are +0.0 outside the support already)
__global__ __launch_bounds__(256) void solve_residual_kernel(const double* __restrict__ q, int voxels, double* __restrict__ r, double* __restrict__ p) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= voxels) return;
    const double d = r[e] - q[e];
    r[e] = d, p[e] = d;
}

// columns[z W + x] = the sum from 0.0 down the rows y of a b on the support, +0.0 elsewhere.  One thread per (slice, column)
__global__ __launch_bounds__(256) void solve_dot_kernel(const double* __restrict__ a, const double* __restrict__ b, const float* __restrict__ sup, int n, int H, int W,
                                                        double* __restrict__ columns) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n * W) return;
    const int z = e / W, x = e - z * W;
    const size_t base = (size_t)z * H * W + x;
    double s = 0.0;
    int y = 0;
    for (; y + 4 <= H; y += 4) {  // four rows' loads in flight; the additions stay in the rows' order
        double t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t at = base + (size_t)(y + u) * W;
            t[u] = __builtin_isfinite(sup[at]) ? a[at] * b[at] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) s += t[u];
    }
    for (; y < H; ++y) {
        const size_t at = base + (size_t)y * W;
        s += __builtin_isfinite(sup[at]) ? a[at] * b[at] : 0.0;
    }
    columns[e] = s;
}

// One workgroup.  columns (n, W) -> slices (n) -> the inner product; then the scalars of the solve.  mode: SolveReduceMode; `it` the iteration.
// history (iterations + 1, 2) or null
__global__ __launch_bounds__(256) void solve_reduce_kernel(const double* columns, int n, int W, int mode, int it, double* slices, double* state, double* history) {
#pragma clang fp contract(off)
    for (int z = threadIdx.x; z < n; z += 256) {
        double s = 0.0;
        for (int x = 0; x < W; ++x) s += columns[(size_t)z * W + x];
        slices[z] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int z = 0; z < n; ++z) total += slices[z];
    const double nan = __builtin_nan("");
    if (mode == SOLVE_REDUCE_FIRST) {
        state[SOLVE_RHO] = total, state[SOLVE_ALPHA] = 0.0, state[SOLVE_BETA] = 0.0, state[SOLVE_STOPPED] = 0.0, state[SOLVE_STOPPED_AT] = -1.0;
        if (history) history[0] = total, history[1] = nan;
    } else if (mode == SOLVE_REDUCE_GAMMA) {
        const double rho = state[SOLVE_RHO];
        const bool was = state[SOLVE_STOPPED] != 0.0;
        const bool stop = was || rho == 0.0 || !__builtin_isfinite(total) || !(total > 0.0);
        if (stop) {
            if (!was) state[SOLVE_STOPPED] = 1.0, state[SOLVE_STOPPED_AT] = (double)it;
        } else {
            state[SOLVE_ALPHA] = rho / total;
        }
        if (history) history[2 * it + 1] = stop ? nan : total;
    } else {
        double rho = state[SOLVE_RHO];
        if (state[SOLVE_STOPPED] == 0.0) {
            state[SOLVE_BETA] = total / rho;
            state[SOLVE_RHO] = rho = total;
        }
        if (history) history[2 * (it + 1)] = rho, history[2 * (it + 1) + 1] = nan;
    }
}

__global__ __launch_bounds__(256) void solve_update_xr_kernel(const double* __restrict__ state, const float* __restrict__ sup, const double* __restrict__ p,
                                                              const double* __restrict__ q, int voxels, double* __restrict__ x, double* __restrict__ r) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= voxels || state[SOLVE_STOPPED] != 0.0 || !__builtin_isfinite(sup[e])) return;
    const double alpha = state[SOLVE_ALPHA];
    x[e] = x[e] + (alpha * p[e]);
    r[e] = r[e] - (alpha * q[e]);
}

__global__ __launch_bounds__(256) void solve_update_p_kernel(const double* __restrict__ state, const float* __restrict__ sup, const double* __restrict__ r, int voxels,
                                                             double* __restrict__ p) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= voxels || state[SOLVE_STOPPED] != 0.0 || !__builtin_isfinite(sup[e])) return;
    p[e] = r[e] + (state[SOLVE_BETA] * p[e]);
}

// sup and volume may be the same buffer (start == NULL: the fusion was written there): each thread reads its voxel before it writes it
__global__ __launch_bounds__(256) void solve_store_kernel(const double* __restrict__ x, const double* __restrict__ state, const float* sup, int voxels, float* volume,
                                                          int* __restrict__ stopped_at) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e == 0 && stopped_at) *stopped_at = (int)state[SOLVE_STOPPED_AT];
    if (e >= voxels) return;
    volume[e] = __builtin_isfinite(sup[e]) ? (float)x[e] : __builtin_nanf("");
}

}  // namespace msiren
