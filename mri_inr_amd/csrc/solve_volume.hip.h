// The stack that best explains all aligned targets at once (msiren_solve_volume*): a fixed number of conjugate-gradient
// iterations on (Pt Omega P + lambda L) x = Pt Omega tau over the support, P the row-normalised projection of project.hip.h.  The rule is
// include/msiren.h's, restated in numpy by mri_inr_amd/solve_volume.py (solve_volume_on_host): fp64 + - * /, contraction off, one rounding per
// operation -- the two agree bit for bit.  The per-target record is fuse_setup_kernel's; p, pa, pb, cp, i, j, k, the contribution test, i0, j0, fi,
// fj and the four beta are fuse_gather_kernel's expressions; the box is project_plan.h's.
//
//   solve_start_kernel       x = (double)start on the support (the finite voxels of `sup`), 0.0 elsewhere
//   solve_coverage_kernel    once, one thread per target pixel over project_gather_kernel's box: D = section 5.18's den over the support; the pixel is
//                            ACTIVE iff its target is unflagged, T and w are a valid tap and D > min_coverage.  Writes D (0.0 where not active),
//                            Wt = (w g) g and z = (Wt tau) / D, the right-hand side's pixel vector
//   solve_forward_kernel     the same gather with the fp64 entry of v: num, then z = (Wt (num / D)) / D on the active pixels, 0.0 elsewhere.  The record in
//                            SGPRs, no LDS, no atomics, no barrier
//   solve_transpose_kernel   fuse_gather_kernel's structure and cull, one workgroup per 16 x 16 tile: per voxel acc += k sn with sn the sum over the four
//                            taps of beta z_p, then out = acc + (lambda (L v)) with the six-neighbour Laplacian of v: A v in one pass over the voxels
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

#include "fuse.hip.h"
#include "project_plan.h"
#include "solve_volume_plan.h"

namespace msiren {

constexpr int SOLVE_TILE = 16;

__global__ __launch_bounds__(256) void solve_start_kernel(const float* __restrict__ sup, int voxels, double* __restrict__ x) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= voxels) return;
    const float s = sup[e];
    x[e] = __builtin_isfinite(s) ? (double)s : 0.0;
}

// the sum of one target pixel over its box: COVERAGE the window x bilinear weights of the voxels of the support, else those times v
template <bool COVERAGE>
__device__ __forceinline__ double solve_pixel_sum(const double* r, const float* __restrict__ sup, const double* __restrict__ v, int pi, int pj, int th, int tw, int n,
                                                  int H, int W, double spacing, double thickness) {
#pragma clang fp contract(off)
    const double a0 = r[0], a1 = r[1], a2 = r[2], b0 = r[3], b1 = r[4], b2 = r[5], t0 = r[6], t1 = r[7], t2 = r[8];
    const double G11 = r[9], G12 = r[10], G22 = r[11], det = r[12], dt = r[13], c0 = r[14], c1 = r[15], c2 = r[16];
    double R[3];
    const bool boxed = project_box(r, thickness, spacing, n, H, W, R);
    const int nz = project_count(boxed, R[0], n), ny = project_count(boxed, R[1], H), nx = project_count(boxed, R[2], W);
    const double dpi = (double)pi, dpj = (double)pj;
    const int z0 = project_base(((t0 + a0 * dpi) + b0 * dpj) / spacing, R[0], n, nz);
    const int y0 = project_base((t1 + a1 * dpi) + b1 * dpj, R[1], H, ny);
    const int x0 = project_base((t2 + a2 * dpi) + b2 * dpj, R[2], W, nx);
    const double th1 = (double)(th - 1), tw1 = (double)(tw - 1), th2 = (double)(th - 2), tw2 = (double)(tw - 2);
    double sum = 0.0;
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
                if (!(cc < dt)) continue;  // k <= 0 (project.hip.h)
                if (COVERAGE && !__builtin_isfinite(sup[row + x])) continue;
                const double pa = fa + (a2 * p2), pb = fb + (b2 * p2);
                const double i = ((G22 * pa) - (G12 * pb)) / det, j = ((G11 * pb) - (G12 * pa)) / det;
                const double k = 1.0 - (cc / dt);
                if (k > 0.0 && i >= 0.0 && i <= th1 && j >= 0.0 && j <= tw1) {
                    const double fi0 = fmin(floor(i), th2), fj0 = fmin(floor(j), tw2);
                    const double di = dpi - fi0, dj = dpj - fj0;  // exact: small integers
                    if ((di == 0.0 || di == 1.0) && (dj == 0.0 || dj == 1.0)) {
                        const double fi = i - fi0, fj = j - fj0, gi = 1.0 - fi, gj = 1.0 - fj;
                        const double beta = (di == 0.0 ? gi : fi) * (dj == 0.0 ? gj : fj);
                        const double kb = k * beta;
                        if (COVERAGE)
                            sum += kb;
                        else
                            sum += kb * v[row + x];
                    }
                }
            }
        }
    }
    return sum;
}

// sup (n, H, W), targets, weights or null (m, th, tw), rec -> D, Wt, z (m, th, tw).  grid: tiles_y tiles_x m workgroups, the tile's column fastest
__global__ __launch_bounds__(256) void solve_coverage_kernel(const float* __restrict__ sup, const float* __restrict__ targets, const float* __restrict__ weights,
                                                             const double* __restrict__ rec, int th, int tw, int n, int H, int W, int tiles_x, int tiles_y, double spacing,
                                                             double thickness, double min_coverage, double* __restrict__ D, double* __restrict__ Wt, double* __restrict__ zz) {
#pragma clang fp contract(off)
    const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, q = blockIdx.x / (tiles_x * tiles_y);
    const int pj = bx * SOLVE_TILE + (threadIdx.x & (SOLVE_TILE - 1)), pi = by * SOLVE_TILE + (threadIdx.x / SOLVE_TILE);
    const bool inside = pi < th && pj < tw;
    const size_t at = ((size_t)q * th + (inside ? pi : 0)) * tw + (inside ? pj : 0);
    const double* r = rec + (size_t)q * FUSE_RECORD;  // wave-uniform: scalar loads
    if (r[19] != 0.0) {                               // a flagged target: no pixel is active
        if (inside) D[at] = 0.0, Wt[at] = 0.0, zz[at] = 0.0;
        return;
    }
    const double den = solve_pixel_sum<true>(r, sup, nullptr, pi, pj, th, tw, n, H, W, spacing, thickness);
    if (inside) {
        const float T = targets[at], w = weights ? weights[at] : 1.f;
        const bool active = __builtin_isfinite(T) && __builtin_isfinite(w) && w > 0.f && den > min_coverage;
        const double g = r[17], bias = r[18];
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
    const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, q = blockIdx.x / (tiles_x * tiles_y);
    const int pj = bx * SOLVE_TILE + (threadIdx.x & (SOLVE_TILE - 1)), pi = by * SOLVE_TILE + (threadIdx.x / SOLVE_TILE);
    const bool inside = pi < th && pj < tw;
    const size_t at = ((size_t)q * th + (inside ? pi : 0)) * tw + (inside ? pj : 0);
    const double* r = rec + (size_t)q * FUSE_RECORD;  // wave-uniform: scalar loads
    if (r[19] != 0.0) return;
    const double num = solve_pixel_sum<false>(r, nullptr, v, pi, pj, th, tw, n, H, W, spacing, thickness);
    if (inside) {
        const double d = D[at];
        zz[at] = d > 0.0 ? (Wt[at] * (num / d)) / d : 0.0;
    }
}

// zz (m, th, tw), rec, sup (n, H, W); v (n, H, W) or null: with it out = Pt z + (lambda (L v)), without it out = Pt z; 0.0 outside the support.
// grid: tiles_y tiles_x n workgroups, the tile's column fastest.  The loop over the targets and its cull are fuse_gather_kernel's
__global__ __launch_bounds__(256) void solve_transpose_kernel(const double* __restrict__ zz, const double* __restrict__ rec, const float* __restrict__ sup,
                                                              const double* __restrict__ v, int m, int th, int tw, int n, int H, int W, int tiles_x, int tiles_y,
                                                              double spacing, double lambda, double cz, double* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr double MARGIN = 0x1p-40;
    const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, z = blockIdx.x / (tiles_x * tiles_y);
    const int x = bx * SOLVE_TILE + (threadIdx.x & (SOLVE_TILE - 1)), y = by * SOLVE_TILE + (threadIdx.x / SOLVE_TILE);
    const double v0 = (double)z * spacing, vy = (double)y, vx = (double)x;
    const double yl = (double)(by * SOLVE_TILE), yh = (double)(by * SOLVE_TILE + SOLVE_TILE - 1), xl = (double)(bx * SOLVE_TILE), xh = (double)(bx * SOLVE_TILE + SOLVE_TILE - 1);
    const double th1 = (double)(th - 1), tw1 = (double)(tw - 1), th2 = (double)(th - 2), tw2 = (double)(tw - 2);
    const int Mt = th * tw;
    double acc = 0.0;
    for (int q = 0; q < m; ++q) {
        const double* r = rec + (size_t)q * FUSE_RECORD;  // wave-uniform: scalar loads
        if (r[19] != 0.0) continue;
        const double t0 = r[6], t1 = r[7], t2 = r[8], c0 = r[14], c1 = r[15], c2 = r[16], dt = r[13];
        const double p0 = v0 - t0;
        // ---- the tile-level cull: the same values in every lane ----
        const double pyl = yl - t1, pyh = yh - t1, pxl = xl - t2, pxh = xh - t2;
        const double pym = fmax(fabs(pyl), fabs(pyh)), pxm = fmax(fabs(pxl), fabs(pxh));
        {
            const double e0 = c0 * p0, eyl = c1 * pyl, eyh = c1 * pyh, exl = c2 * pxl, exh = c2 * pxh;
            const double k00 = (e0 + eyl) + exl, k01 = (e0 + eyl) + exh, k10 = (e0 + eyh) + exl, k11 = (e0 + eyh) + exh;
            const double S = (fabs(e0) + fabs(c1) * pym) + fabs(c2) * pxm, margin = S * MARGIN;
            const double lo_pos = fuse_min4(k00, k01, k10, k11) - margin, lo_neg = -(fuse_max4(k00, k01, k10, k11) + margin);
            const double lo = fmax(lo_pos, lo_neg);  // > 0: every voxel's |cp| is at least this
            const bool finite = __builtin_isfinite(((k00 + k01) + (k10 + k11)) + S);
            if (finite && lo > 0.0 && (lo * lo) * (1.0 - MARGIN) > dt) continue;
        }
        const double a0 = r[0], a1 = r[1], a2 = r[2], b0 = r[3], b1 = r[4], b2 = r[5], G11 = r[9], G12 = r[10], G22 = r[11], det = r[12];
        {
            const double ea = a0 * p0, eb = b0 * p0;
            const double ayl = a1 * pyl, ayh = a1 * pyh, axl = a2 * pxl, axh = a2 * pxh, byl = b1 * pyl, byh = b1 * pyh, bxl = b2 * pxl, bxh = b2 * pxh;
            const double pa00 = (ea + ayl) + axl, pa01 = (ea + ayl) + axh, pa10 = (ea + ayh) + axl, pa11 = (ea + ayh) + axh;
            const double pb00 = (eb + byl) + bxl, pb01 = (eb + byl) + bxh, pb10 = (eb + byh) + bxl, pb11 = (eb + byh) + bxh;
            const double Sa = (fabs(ea) + fabs(a1) * pym) + fabs(a2) * pxm, Sb = (fabs(eb) + fabs(b1) * pym) + fabs(b2) * pxm;
            const double mi = ((fabs(G22) * Sa + fabs(G12) * Sb) / det) * MARGIN, mj = ((fabs(G11) * Sb + fabs(G12) * Sa) / det) * MARGIN;
            const double i00 = ((G22 * pa00) - (G12 * pb00)) / det, i01 = ((G22 * pa01) - (G12 * pb01)) / det;
            const double i10 = ((G22 * pa10) - (G12 * pb10)) / det, i11 = ((G22 * pa11) - (G12 * pb11)) / det;
            const double j00 = ((G11 * pb00) - (G12 * pa00)) / det, j01 = ((G11 * pb01) - (G12 * pa01)) / det;
            const double j10 = ((G11 * pb10) - (G12 * pa10)) / det, j11 = ((G11 * pb11) - (G12 * pa11)) / det;
            const bool finite = __builtin_isfinite((((i00 + i01) + (i10 + i11)) + ((j00 + j01) + (j10 + j11))) + (mi + mj));
            const bool out_i = fuse_max4(i00, i01, i10, i11) + mi < 0.0 || fuse_min4(i00, i01, i10, i11) - mi > th1;
            const bool out_j = fuse_max4(j00, j01, j10, j11) + mj < 0.0 || fuse_min4(j00, j01, j10, j11) - mj > tw1;
            if (finite && (out_i || out_j)) continue;
        }
        // ---- the voxel ----
        const double p1 = vy - t1, p2 = vx - t2;
        const double pa = ((a0 * p0) + (a1 * p1)) + (a2 * p2), pb = ((b0 * p0) + (b1 * p1)) + (b2 * p2), cp = ((c0 * p0) + (c1 * p1)) + (c2 * p2);
        const double i = ((G22 * pa) - (G12 * pb)) / det, j = ((G11 * pb) - (G12 * pa)) / det;
        const double k = 1.0 - ((cp * cp) / dt);
        if (k > 0.0 && i >= 0.0 && i <= th1 && j >= 0.0 && j <= tw1) {
            const double fi0 = fmin(floor(i), th2), fj0 = fmin(floor(j), tw2);
            const double fi = i - fi0, fj = j - fj0, gi = 1.0 - fi, gj = 1.0 - fj;
            const int at = q * Mt + (int)fi0 * tw + (int)fj0;  // i0 <= th - 2, j0 <= tw - 2: the four taps are inside the target
            double sn = 0.0;
            sn += (gi * gj) * zz[at];
            sn += (gi * fj) * zz[at + 1];
            sn += (fi * gj) * zz[at + tw];
            sn += (fi * fj) * zz[at + tw + 1];
            acc += k * sn;
        }
    }
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
