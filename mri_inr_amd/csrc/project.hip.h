// A stack gathered onto the lattices of target slices (msiren_project_volume*): the forward operator next to fuse.hip.h's
// gather -- per target pixel the normalised sum of window x bilinear weight x voxel over the voxels that have the pixel among their four taps, with
// exactly the weights of msiren_fuse_targets.  The rule is include/msiren.h's, restated in numpy by mri_inr_amd/fuse.py (project_on_host,
// project_stats_on_host): fp64 + - * /, contraction off, one rounding per operation -- the two agree bit for bit.  The per-target record is
// fuse_setup_kernel's (fuse.hip.h), and p, pa, pb, cp, i, j, k, i0, j0, fi, fj and the four beta are fuse_visit_targets' expressions.
//
//   gather   project_gather_kernel   one workgroup of 256 per 16 x 16 tile of one target's pixels, one thread per pixel (fuse_tile_lane); the record of q is
//                                    read with a wave-uniform index (scalar loads).  Each thread visits the voxels around its own point through
//                                    project_visit_voxels, shared with solve_volume.hip.h's two forward gathers.  num and den stay in registers; no
//                                    LDS, no atomics, no barrier; pixels of a ragged tile outside (th, tw) store nothing
//   stats    project_stats_kernel    one workgroup per target: thread tid sums the columns tid, tid + 256, ... down the rows (coalesced across the
//                                    lanes), parks the four sums per column in the stream's scratch, and after a barrier threads 0 .. 3 add one
//                                    quantity each over the columns ascending; [residual] is written on the way
#pragma once
#include <hip/hip_runtime.h>

#include "fuse.hip.h"
#include "project_plan.h"

namespace msiren {

// The voxels that can add a term to pixel (pi, pj) of the target with record r, for project_gather_kernel, solve_coverage_kernel and
// solve_forward_kernel: the box of voxels around the pixel's own point x = t + a pi + b pj (project_plan.h: project_box, with the proof), z, then y, then x
// ascending: the rule's order.  The trip counts are the target's, the same in every lane; the first index is the lane's, clipped to the grid.
// takes(at) says whether the voxel at flat index `at` takes part (asked behind the window test, so it may load); term(at, kb) receives every (voxel,
// tap) pair of the rule, kb = k beta: the window times the bilinear weight the pixel has among the voxel's four taps.
// Why the box is invisible in what the callers sum: a voxel outside it does not have the pixel among its taps or fails the window (project_plan.h), so
// the rule has no term for it; a sum that starts at +0.0 sees exactly the terms of the rule in the rule's order.  Inside the loop the window is tested
// as cp cp < dt in front of the divisions: for dt > 0, fl(x / dt) < 1 iff x < dt (below dt the quotient is at most 1 - 2^-53, which is a double), so
// that is k > 0 bit for bit (a NaN fails both).
template <class Takes, class Term>
__device__ __forceinline__ void project_visit_voxels(const double* r, int pi, int pj, int th, int tw, int n, int H, int W, double spacing, double thickness, Takes takes,
                                                     Term term) {
#pragma clang fp contract(off)
    const double a0 = r[FUSE_A], a1 = r[FUSE_A + 1], a2 = r[FUSE_A + 2], b0 = r[FUSE_B], b1 = r[FUSE_B + 1], b2 = r[FUSE_B + 2];
    const double t0 = r[FUSE_T], t1 = r[FUSE_T + 1], t2 = r[FUSE_T + 2];
    const double G11 = r[FUSE_G11], G12 = r[FUSE_G12], G22 = r[FUSE_G22], det = r[FUSE_DET], dt = r[FUSE_DT], c0 = r[FUSE_C], c1 = r[FUSE_C + 1], c2 = r[FUSE_C + 2];
    // ---- the box: radii and trip counts are the target's, the first index is the lane's ----
    double R[3];
    const bool boxed = project_box(r, thickness, spacing, n, H, W, R);
    const int nz = project_count(boxed, R[0], n), ny = project_count(boxed, R[1], H), nx = project_count(boxed, R[2], W);
    const double dpi = (double)pi, dpj = (double)pj;
    const int z0 = project_base(((t0 + a0 * dpi) + b0 * dpj) / spacing, R[0], n, nz);
    const int y0 = project_base((t1 + a1 * dpi) + b1 * dpj, R[1], H, ny);
    const int x0 = project_base((t2 + a2 * dpi) + b2 * dpj, R[2], W, nx);
    const double th1 = (double)(th - 1), tw1 = (double)(tw - 1), th2 = (double)(th - 2), tw2 = (double)(tw - 2);
    for (int dz = 0; dz < nz; ++dz) {
        const int z = z0 + dz;  // 0 <= z0 and z0 + nz <= n (project_base): every index is inside the grid
        const double p0 = ((double)z * spacing) - t0;
        const double ea = a0 * p0, eb = b0 * p0, ec = c0 * p0;
        for (int dy = 0; dy < ny; ++dy) {
            const int y = y0 + dy;
            const double p1 = (double)y - t1;
            const double fa = ea + (a1 * p1), fb = eb + (b1 * p1), fc = ec + (c1 * p1);
            const size_t row = ((size_t)z * H + y) * W;
            for (int dx = 0; dx < nx; ++dx) {
                const int x = x0 + dx;
                const double p2 = (double)x - t2;
                const double cp = fc + (c2 * p2), cc = cp * cp;
                if (!(cc < dt)) continue;  // k <= 0 (above)
                if (!takes(row + x)) continue;
                const double pa = fa + (a2 * p2), pb = fb + (b2 * p2);
                const double i = ((G22 * pa) - (G12 * pb)) / det, j = ((G11 * pb) - (G12 * pa)) / det;
                const double k = 1.0 - (cc / dt);
                if (k > 0.0 && i >= 0.0 && i <= th1 && j >= 0.0 && j <= tw1) {
                    const double fi0 = fmin(floor(i), th2), fj0 = fmin(floor(j), tw2);
                    const double di = dpi - fi0, dj = dpj - fj0;  // exact: small integers
                    if ((di == 0.0 || di == 1.0) && (dj == 0.0 || dj == 1.0)) {
                        const double fi = i - fi0, fj = j - fj0, gi = 1.0 - fi, gj = 1.0 - fj;
                        const double beta = (di == 0.0 ? gi : fi) * (dj == 0.0 ? gj : fj);
                        term(row + x, k * beta);
                    }
                }
            }
        }
    }
}

// volume (n, H, W), rec (m, kFuseRecord) -> simulated (m, th, tw), coverage (m, th, tw) or null.  grid: tiles_y tiles_x m workgroups (fuse_tile_lane)
__global__ __launch_bounds__(256) void project_gather_kernel(const float* __restrict__ volume, const double* __restrict__ rec, int th, int tw, int n, int H, int W,
                                                             int tiles_x, int tiles_y, double spacing, double thickness, double min_coverage,
                                                             float* __restrict__ simulated, float* __restrict__ coverage) {
#pragma clang fp contract(off)
    const FuseTileLane l = fuse_tile_lane(tiles_x, tiles_y);
    const int q = l.outer, pi = l.row, pj = l.col;
    const bool inside = pi < th && pj < tw;
    const size_t at = ((size_t)q * th + (inside ? pi : 0)) * tw + (inside ? pj : 0);
    const double* r = rec + (size_t)q * kFuseRecord;  // wave-uniform: scalar loads
    if (r[FUSE_FLAGS] != 0.0) {                       // a flagged target: NaN, coverage 0
        if (inside) {
            simulated[at] = __builtin_nanf("");
            if (coverage) coverage[at] = 0.f;
        }
        return;
    }
    double num = 0.0, den = 0.0;
    project_visit_voxels(
        r, pi, pj, th, tw, n, H, W, spacing, thickness, [&](size_t v) { return __builtin_isfinite(volume[v]); },
        [&](size_t v, double kb) {
            num += kb * (double)volume[v];
            den += kb;
        });
    if (inside) {
        const double g = r[FUSE_GAIN], bias = r[FUSE_BIAS];
        simulated[at] = den > min_coverage ? (float)((g * (num / den)) + bias) : __builtin_nanf("");
        if (coverage) coverage[at] = (float)den;
    }
}

// targets, weights or null, simulated (m, th, tw) -> residual (m, th, tw) or null, stats (m, 4) or null; columns (m, tw, 4): scratch, with stats
__global__ __launch_bounds__(256) void project_stats_kernel(const float* __restrict__ targets, const float* __restrict__ weights, const float* __restrict__ simulated,
                                                            int th, int tw, double* columns, float* __restrict__ residual, double* stats) {
#pragma clang fp contract(off)
    const int q = blockIdx.x, tid = threadIdx.x;
    double* col = columns ? columns + (size_t)q * tw * 4 : nullptr;
    for (int j = tid; j < tw; j += 256) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int i = 0; i < th; ++i) {
            const size_t at = ((size_t)q * th + i) * tw + j;
            const float T = targets[at], S = simulated[at];
            const float rf = __builtin_isfinite(T) && __builtin_isfinite(S) ? (float)((double)T - (double)S) : __builtin_nanf("");
            if (residual) residual[at] = rf;
            const float w = weights ? weights[at] : 1.f;
            if (__builtin_isfinite(rf) && __builtin_isfinite(w) && w > 0.f) {
                const double rd = (double)rf, wd = (double)w, wr = wd * rd;
                s0 += 1.0;
                s1 += wd;
                s2 += wr;
                s3 += wr * rd;
            }
        }
        if (col) col[4 * j] = s0, col[4 * j + 1] = s1, col[4 * j + 2] = s2, col[4 * j + 3] = s3;
    }
    if (!stats) return;  // (the same in every thread)
    __syncthreads();
    if (tid < 4) {
        double s = 0.0;
        for (int j = 0; j < tw; ++j) s += col[4 * j + tid];
        stats[4 * (size_t)q + tid] = s;
    }
}

}  // namespace msiren
