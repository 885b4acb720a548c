// Weighted, gain/bias-compensated alignment of target slices to a stack read as a volume (msiren_align_volume_w* and
// msiren_align_volume_solve_w*): the reduce and the step stages of align_volume.hip.h for a per-pixel weight w and a per-target intensity (g, b),
// as align_w.hip.h has them for align.hip.h.  Points, bins, the jet ragged trunk and the blend are align_volume.hip.h's, unchanged: R, gZ, gY, gX
// stay the bits of msiren_resample_volume_grad.
//
//   reduce   align_volume_partial_w_kernel   one workgroup per (target, chunk of ALIGN_CHUNK pixels): align_volume_partial_kernel's blend per pixel,
//                                            [warped], [wgrad] (before gain and bias), the 80 fp64 sums of the chunk -> one partial record
//            align_volume_combine_w_kernel   one workgroup per target: its partial records added in index order -> sums (m, 80)
// A pixel is VALID iff target, R, gZ, gY, gX are all finite and its weight is finite and > 0; per valid pixel, in fp64 from the fp32 numbers,
// contraction off, in exactly this association:
//     mm = (g R) + b,  r = mm - T,  gz = g gZ,  gy = g gY,  gx = g gX,  J = (gz i, gz j, gz, gy i, gy j, gy, gx i, gx j, gx, R, 1),  wr = w r
//     count += 1, wsum += w, cost += wr r, dcost[a] += (2 wr) J[a], jtj[a, b] += (w J[a]) J[b] (a <= b)
// record = [count, wsum, cost, dcost 11, jtj packed upper triangle row-major 66].  With g = 1, b = 0, w = 1 every term over the map's nine
// parameters is align_volume_partial_kernel's term; a weight that is a power of two scales wsum, cost, dcost and jtj exactly.  The order of every
// sum is align.hip.h's.
//
// Shared: the pixel, B and the Cayley update are align_volume.hip.h's functions.  The reduce is align_volume_partial_w_body<ROBUST> below, which
// align_volume_r.hip.h instantiates for the robust loss; align_volume_partial_w_kernel is its ROBUST = false instance and carries nothing of the
// other (no scale, no division, no rweight).  The projection t = B^T g, HQ = B^T (H B) on the packed sums stands twice, in the step kernel below
// and in align_group_project_kernel: as one function it took align_volume_step_w_kernel<RIGID, 1> over its recorded registers (LAB_NOTES.md
// section 30); mri_inr_amd/align_volume.py: project_rigid is the one statement of it.
#pragma once
#include <hip/hip_runtime.h>

#include "align_volume.hip.h"

namespace msiren {

constexpr int ALIGN_VOLUME_SUMS_W = 80;  // count, wsum, cost, dcost[11], jtj[66]

// the robust factors of a valid pixel (align_volume_r.hip.h): wl for the cost, wq for dcost and jtj, rw the outlier weight
__device__ __forceinline__ void align_robust_factors(double wd, double r, double s, double* wl, double* wq, float* rw);

// The reduce of the 80 sums under the square loss (ROBUST = false: align_volume_partial_w_kernel, wl = wq = w, neither scale nor rweight is touched)
// or the Geman-McClure loss (ROBUST = true: align_volume_partial_r_kernel, scale (m) doubles, rweight (m, Mt) or null).  Per valid pixel
//     count += 1, wsum += w, cost += (wl r) r, dcost[a] += (2 (wq r)) J[a], jtj[a, b] += (wq J[a]) J[b] (a <= b)
// Where the pixel comes from is the caller's: pixel(gp, px, &R, &gZ, &gY, &gX) gives pixel px of the workgroup's target (gp = q Mt + px) and does the
// optional warped / wgrad stores.  The two kernels of the volume families pass align_volume_pixel; align_stack_partial_r_kernel (align_stack.hip.h)
// passes the point and a trilinear read of a voxel stack.  Inlined, the callable costs the older kernels no register (LAB_NOTES.md section 37).
template <bool ROBUST, typename Pixel>
__device__ __forceinline__ void align_volume_partial_w_body(Pixel pixel, const float* __restrict__ targets, const float* __restrict__ weights,
                                                            const float* __restrict__ intensity, const double* __restrict__ scale,
                                                            float* __restrict__ rweight, double* __restrict__ partials, int Mt, int tw, int chunks) {
#pragma clang fp contract(off)
    __shared__ double red[ALIGN_VOLUME_SUMS_W][4];
    const int q = blockIdx.x / chunks, chunk = blockIdx.x - q * chunks;
    const int lo = chunk * ALIGN_CHUNK, hi = lo + ALIGN_CHUNK < Mt ? lo + ALIGN_CHUNK : Mt;
    const double g = intensity ? (double)intensity[(size_t)q * 2] : 1.0, b = intensity ? (double)intensity[(size_t)q * 2 + 1] : 0.0;
    double s = 0.0;
    if constexpr (ROBUST) s = scale[q];
    const bool scored = !ROBUST || s > 0.0;  // (false for a NaN)
    double acc[ALIGN_VOLUME_SUMS_W];
#pragma unroll
    for (int a = 0; a < ALIGN_VOLUME_SUMS_W; ++a) acc[a] = 0.0;
    for (int px = lo + threadIdx.x; px < hi; px += 256) {
        const size_t gp = (size_t)q * Mt + px;
        float R, gZ, gY, gX;
        pixel(gp, px, &R, &gZ, &gY, &gX);
        const float tv = targets[gp], wv = weights ? weights[gp] : 1.f;
        float rw = __builtin_nanf("");
        if (scored && align_finite(tv) && align_finite(R) && align_finite(gZ) && align_finite(gY) && align_finite(gX) && align_finite(wv) && wv > 0.f) {
            const int i = px / tw, j = px - i * tw;
            const double wd = (double)wv, gr = g * (double)R, mm = gr + b, di = (double)i, dj = (double)j;
            const double r = mm - (double)tv, gz = g * (double)gZ, gy = g * (double)gY, gx = g * (double)gX;
            double wl = wd, wq = wd;
            if constexpr (ROBUST) align_robust_factors(wd, r, s, &wl, &wq, &rw);
            const double wlr = wl * r, wqr = wq * r, wr2 = 2.0 * wqr;
            double J[11];
            J[0] = gz * di, J[1] = gz * dj, J[2] = gz;
            J[3] = gy * di, J[4] = gy * dj, J[5] = gy;
            J[6] = gx * di, J[7] = gx * dj, J[8] = gx;
            J[9] = (double)R, J[10] = 1.0;
            acc[0] += 1.0;
            acc[1] += wd;
            acc[2] += wlr * r;
            int t = 14;
#pragma unroll
            for (int a = 0; a < 11; ++a) {
                acc[3 + a] += wr2 * J[a];
                const double wj = wq * J[a];
#pragma unroll
                for (int c = a; c < 11; ++c, ++t) acc[t] += wj * J[c];
            }
        }
        if constexpr (ROBUST) {
            if (rweight) rweight[gp] = rw;
        }
    }
    align_block_reduce<ALIGN_VOLUME_SUMS_W>(acc, red, partials);
}

// weights (m, Mt) and intensity (m, 2) may be null: every weight 1, (g, b) = (1, 0).  partials (m chunks, ALIGN_VOLUME_SUMS_W).  The grid and every
// other argument: align_volume_partial_kernel's
__global__ __launch_bounds__(256) void align_volume_partial_w_kernel(const float* __restrict__ vals, const int* __restrict__ ent, const int* __restrict__ tile,
                                                                     const float* __restrict__ w, const int* __restrict__ black, const int* __restrict__ pair,
                                                                     const float* __restrict__ fz, const float* __restrict__ targets,
                                                                     const float* __restrict__ weights, const float* __restrict__ intensity,
                                                                     float* __restrict__ warped, float* __restrict__ wgrad, double* __restrict__ partials, int m,
                                                                     int Mt, int tw, int K, int NPt, int T, int chunks) {
    const size_t M = (size_t)m * Mt;
    align_volume_partial_w_body<false>(
        [&](size_t gp, int, float* R, float* gZ, float* gY, float* gX) { align_volume_pixel(vals, ent, tile, w, black, pair, fz, warped, wgrad, gp, M, K, NPt, T, R, gZ, gY, gX); },
        targets, weights, intensity, nullptr, nullptr, partials, Mt, tw, chunks);
}

// sums[q, a] = the target's partial records added in index order
__global__ __launch_bounds__(256) void align_volume_combine_w_kernel(const double* __restrict__ partials, double* __restrict__ sums, int chunks) {
    align_combine<ALIGN_VOLUME_SUMS_W>(partials, sums, chunks);
}

// ---- msiren_align_volume_solve_w* (DESIGN.md section 5.14): section 5.13's loop on the 80 sums ---------------------------------------------------
// One thread per target between two evaluations.  State per target: align_volume_step_kernel's, plus the trial and the best (g, b) as fp32
// (gb_trial, gb_best) and sums_best of 80.  The rule is restated by mri_inr_amd/align_volume.py: lm_step_vw -- fp64 + - * / one at a time, every
// sum in the order written there.  Solved parameters P: affine 9 (intensity fixed) or 11 (estimated), rigid 6 or 8; mean = cost / wsum if
// count >= P else +inf.  The step kernel is instantiated per (mode, intensity mode), so each instantiation carries one system, of 9, 11, 6 or 8
// unknowns; every loop has constant bounds and is unrolled, nothing is indexed at run time, and only the triangle the solve reads stays live.
struct AlignVolumeSolveWParams {
    const double* sums;                  // (m, 80) of the evaluation at `trial`, `gb_trial`
    const double* planes;                // (m, 12) = (e_i, e_j, o, c), rigid mode
    float *trial, *best;                 // (m, 9)
    float *gb_trial, *gb_best;           // (m, 2)
    double *rigid_trial, *rigid_best;    // (m, 12)
    double* sums_best;                   // (m, 80)
    double* scal;                        // (m, 3) mean_best, mean_first, lam
    int* cnt;                            // (m, 2) accepted, flags
    double* trace;                       // (iterations, m, 14) or null
    float* maps_out;                     // (m, 9)      written behind the last evaluation
    float* intensity_out;                // (m, 2)
    double* rigid_out;                   // (m, 12) or null
    double* report;                      // (m, 7)
    int m, k, last;                      // k: the evaluation just done; last: k == iterations - 1
    double down, up, lam_min, lam_max, spacing;
};

// where jtj[a][b], a <= b, of the 11 x 11 matrix lies in a record
__device__ __forceinline__ constexpr int align_vw_packed(int a, int b) { return 14 + a * 11 - (a * (a - 1)) / 2 + (b - a); }

// before the first evaluation: trial := best := the inputs (rigid: the map of the input state; intensity null: (1, 0)), lam := damping
template <int MODE>
__global__ __launch_bounds__(256) void align_volume_solve_init_w_kernel(AlignVolumeSolveWParams p, const float* __restrict__ maps_in,
                                                                        const double* __restrict__ rigid_in, const float* __restrict__ intensity_in,
                                                                        double damping) {
#pragma clang fp contract(off)
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= p.m) return;
    float mp[9];
    double st[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) st[a] = 0.0;
    if (MODE == ALIGN_VOLUME_RIGID) {
        double pl[12];
#pragma unroll
        for (int a = 0; a < 12; ++a) st[a] = rigid_in[(size_t)q * 12 + a], pl[a] = p.planes[(size_t)q * 12 + a];
        align_rigid_map3(st, pl, p.spacing, mp);
    } else {
#pragma unroll
        for (int a = 0; a < 9; ++a) mp[a] = maps_in[(size_t)q * 9 + a];
    }
    const float g = intensity_in ? intensity_in[(size_t)q * 2] : 1.f, b = intensity_in ? intensity_in[(size_t)q * 2 + 1] : 0.f;
#pragma unroll
    for (int a = 0; a < 9; ++a) p.trial[(size_t)q * 9 + a] = mp[a], p.best[(size_t)q * 9 + a] = mp[a];
    p.gb_trial[(size_t)q * 2] = g, p.gb_trial[(size_t)q * 2 + 1] = b, p.gb_best[(size_t)q * 2] = g, p.gb_best[(size_t)q * 2 + 1] = b;
#pragma unroll
    for (int a = 0; a < 12; ++a) p.rigid_trial[(size_t)q * 12 + a] = st[a], p.rigid_best[(size_t)q * 12 + a] = st[a];
#pragma unroll
    for (int a = 0; a < ALIGN_VOLUME_SUMS_W; ++a) p.sums_best[(size_t)q * ALIGN_VOLUME_SUMS_W + a] = 0.0;
    p.scal[(size_t)q * 3] = __builtin_inf(), p.scal[(size_t)q * 3 + 1] = __builtin_inf(), p.scal[(size_t)q * 3 + 2] = damping;
    p.cnt[(size_t)q * 2] = 0, p.cnt[(size_t)q * 2 + 1] = 0;
}

// behind evaluation k: accept or reject the trial, then propose the next one from the best state.  grid: ceil(m / 256) workgroups of 256.
// EST: (g, b) are solved for.  As align_volume_step_kernel, what the proposal does not need while the system is formed and solved is read again
// from the state behind a compiler barrier instead of being held in registers across it.
template <int MODE, int EST>
__global__ __launch_bounds__(256) void align_volume_step_w_kernel(AlignVolumeSolveWParams p) {
#pragma clang fp contract(off)
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= p.m) return;
    constexpr int N = EST ? 11 : 9;                                      // parameters of the sums the proposal reads: the leading block
    constexpr int P = (MODE == ALIGN_VOLUME_RIGID ? 6 : 9) + (EST ? 2 : 0);  // solved parameters
    constexpr int S = ALIGN_VOLUME_SUMS_W;
    const double inf = __builtin_inf();
    double mean_best = p.scal[(size_t)q * 3], mean_first = p.scal[(size_t)q * 3 + 1], lam = p.scal[(size_t)q * 3 + 2];
    int accepted = p.cnt[(size_t)q * 2];
    const double* ev = p.sums + (size_t)q * S;
    const double count = ev[0], wsum = ev[1], cost = ev[2];
    if (p.trace) {
        double* tr = p.trace + ((size_t)p.k * p.m + q) * 14;
#pragma unroll
        for (int a = 0; a < 9; ++a) tr[a] = (double)p.trial[(size_t)q * 9 + a];
        tr[9] = (double)p.gb_trial[(size_t)q * 2], tr[10] = (double)p.gb_trial[(size_t)q * 2 + 1];
        tr[11] = cost, tr[12] = count, tr[13] = wsum;
    }
    const double mean = count >= (double)P ? cost / wsum : inf;
    const bool accept = align_lm_decide(p.k, mean, &mean_best, &mean_first, &lam, &accepted, p.down, p.up, p.lam_min, p.lam_max);
    if (accept) {  // best := trial, in the state
#pragma unroll
        for (int a = 0; a < S; ++a) p.sums_best[(size_t)q * S + a] = ev[a];
#pragma unroll
        for (int a = 0; a < 9; ++a) p.best[(size_t)q * 9 + a] = p.trial[(size_t)q * 9 + a];
        p.gb_best[(size_t)q * 2] = p.gb_trial[(size_t)q * 2], p.gb_best[(size_t)q * 2 + 1] = p.gb_trial[(size_t)q * 2 + 1];
#pragma unroll
        for (int a = 0; a < 12; ++a) p.rigid_best[(size_t)q * 12 + a] = p.rigid_trial[(size_t)q * 12 + a];
    }
    __asm__ volatile("" ::: "memory");
    const double* bs = p.sums_best + (size_t)q * S;  // the sums at the best state
    bool ok;
    float trial[9];
    double dg, db;
    if (MODE == ALIGN_VOLUME_AFFINE) {
        // A = H damped on its diagonal, over the leading N x N block
        double A[N][N], rhs[N], d[N];
#pragma unroll
        for (int a = 0; a < N; ++a)
#pragma unroll
            for (int b = a; b < N; ++b) {
                const double h = bs[align_vw_packed(a, b)];
                A[b][a] = h, A[a][b] = h;
            }
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const double h = A[a][a], lh = lam * h;
            A[a][a] = h + lh;
            rhs[a] = -0.5 * bs[3 + a];
        }
        ok = align_ldl_solve<N>(A, rhs, d);
#pragma unroll
        for (int a = 0; a < 9; ++a) trial[a] = (float)((double)p.best[(size_t)q * 9 + a] + d[a]);
        dg = EST ? d[N - 2] : 0.0, db = EST ? d[N - 1] : 0.0;
    } else {
        // B (N x Q): the map's nine over the motion's six; estimating, (g, b) over themselves
        constexpr int Q = EST ? 8 : 6;
        double B[N][Q];
        {
            double rb[12], pl[12];
#pragma unroll
            for (int a = 0; a < 12; ++a) rb[a] = p.rigid_best[(size_t)q * 12 + a], pl[a] = p.planes[(size_t)q * 12 + a];
            align_rigid_jacobian3<N, Q>(rb, pl, p.spacing, B);
        }
        double A[Q][Q], rhs[Q], d[Q];
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) {
                const double bg = B[a][k] * bs[3 + a];
                t = t + bg;
            }
            rhs[k] = -0.5 * t;
        }
        // HQ = B^T (H B), column by column: T[., r] = H B[., r], then A[k][r] = sum_a B[a][k] T[a][r] for k >= r (the triangle the solve reads)
#pragma unroll
        for (int r = 0; r < Q; ++r) {
            __asm__ volatile("" ::: "memory");  // (the sums are read again per column instead of being held across all of them)
            double Tc[N];
#pragma unroll
            for (int a = 0; a < N; ++a) {
                double t = 0.0;
#pragma unroll
                for (int b = 0; b < N; ++b) {
                    const double hb = bs[a <= b ? align_vw_packed(a, b) : align_vw_packed(b, a)] * B[b][r];
                    t = t + hb;
                }
                Tc[a] = t;
            }
#pragma unroll
            for (int k = r; k < Q; ++k) {
                double t = 0.0;
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    const double bt = B[a][k] * Tc[a];
                    t = t + bt;
                }
                A[k][r] = t;
            }
        }
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const double lh = lam * A[k][k];
            A[k][k] = A[k][k] + lh;
        }
        ok = align_ldl_solve<Q>(A, rhs, d);
        __asm__ volatile("" ::: "memory");
        double rb[12], pl[12], rt[12];
#pragma unroll
        for (int a = 0; a < 12; ++a) rb[a] = p.rigid_best[(size_t)q * 12 + a], pl[a] = p.planes[(size_t)q * 12 + a];
        align_cayley_update(d, rb, rt);
        align_rigid_map3(rt, pl, p.spacing, trial);
#pragma unroll
        for (int a = 0; a < 12; ++a) p.rigid_trial[(size_t)q * 12 + a] = rt[a];
        dg = EST ? d[Q - 2] : 0.0, db = EST ? d[Q - 1] : 0.0;
    }
    const float gbest = p.gb_best[(size_t)q * 2], bbest = p.gb_best[(size_t)q * 2 + 1];
    const float gt = EST ? (float)((double)gbest + dg) : gbest, bt = EST ? (float)((double)bbest + db) : bbest;
    const int flags = (ok ? 0 : ALIGN_SINGULAR) | (mean_first == inf ? ALIGN_NO_OVERLAP : 0);
#pragma unroll
    for (int a = 0; a < 9; ++a) p.trial[(size_t)q * 9 + a] = trial[a];
    p.gb_trial[(size_t)q * 2] = gt, p.gb_trial[(size_t)q * 2 + 1] = bt;
    p.scal[(size_t)q * 3] = mean_best, p.scal[(size_t)q * 3 + 1] = mean_first, p.scal[(size_t)q * 3 + 2] = lam;
    p.cnt[(size_t)q * 2] = accepted, p.cnt[(size_t)q * 2 + 1] = flags;
    if (p.last) {
#pragma unroll
        for (int a = 0; a < 9; ++a) p.maps_out[(size_t)q * 9 + a] = p.best[(size_t)q * 9 + a];
        p.intensity_out[(size_t)q * 2] = gbest, p.intensity_out[(size_t)q * 2 + 1] = bbest;
        if (p.rigid_out) {
#pragma unroll
            for (int a = 0; a < 12; ++a) p.rigid_out[(size_t)q * 12 + a] = p.rigid_best[(size_t)q * 12 + a];
        }
        double* rp = p.report + (size_t)q * 7;
        rp[0] = (double)accepted, rp[1] = mean_first, rp[2] = mean_best, rp[3] = bs[0], rp[4] = bs[1], rp[5] = lam, rp[6] = (double)flags;
    }
}

}  // namespace msiren
