// Weighted, gain/bias-compensated slice alignment (msiren_align_slices_w* and msiren_align_solve_w*): the reduce and
// the step stages of align.hip.h for a per-pixel weight w and a per-slice intensity (g, b).  Points, bins, the jet ragged trunk and the blend
// are align.hip.h's, unchanged: R, gY, gX stay the bits of msiren_resample_slices_grad.
//
//   reduce   align_partial_w_kernel   one workgroup per (slice, chunk of ALIGN_CHUNK pixels): blend of the three planes per pixel, [warped],
//                                     [wgrad] (before gain and bias), the 47 fp64 sums of the chunk -> one partial record
//            align_combine_w_kernel   one workgroup per slice: its partial records added in index order -> sums (n, 47)
// A pixel is VALID iff target, R, gY, gX are all finite and its weight is finite and > 0; per valid pixel, in fp64 from the fp32 numbers,
// contraction off, in exactly this association:
//     m = (g R) + b,  r = m - T,  gy = g gY,  gx = g gX,  J = (gy i, gy j, gy, gx i, gx j, gx, R, 1),  wr = w r
//     count += 1, wsum += w, cost += wr r, dcost[a] += (2 wr) J[a], jtj[a, b] += (w J[a]) J[b] (a <= b)
// record = [count, wsum, cost, dcost 8, jtj packed upper triangle row-major 36].  With g = 1, b = 0, w = 1 every term is align_partial_kernel's
// term; a weight that is a power of two scales wsum, cost, dcost and jtj exactly.  The order of every sum is align.hip.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "align.hip.h"

namespace msiren {

constexpr int ALIGN_SUMS_W = 47;  // count, wsum, cost, dcost[8], jtj[36]

// weights (n, M) and intensity (n, 2) may be null: every weight 1, (g, b) = (1, 0).  partials (n chunks, ALIGN_SUMS_W).  The grid and every
// other argument: align_partial_kernel's
__global__ __launch_bounds__(256) void align_partial_w_kernel(const float* __restrict__ vals, const int* __restrict__ ent, const int* __restrict__ tile,
                                                              const float* __restrict__ w, const int* __restrict__ black, const float* __restrict__ targets,
                                                              const float* __restrict__ weights, const float* __restrict__ intensity, float* __restrict__ warped,
                                                              float* __restrict__ wgrad, double* __restrict__ partials, int n, int M, int tw, int K, int NPt, int T,
                                                              int chunks) {
#pragma clang fp contract(off)
    __shared__ double red[ALIGN_SUMS_W][4];
    const int s = blockIdx.x / chunks, chunk = blockIdx.x - s * chunks;
    const int lo = chunk * ALIGN_CHUNK, hi = lo + ALIGN_CHUNK < M ? lo + ALIGN_CHUNK : M;
    const int* bl = black + (size_t)s * NPt;
    const double g = intensity ? (double)intensity[(size_t)s * 2] : 1.0, b = intensity ? (double)intensity[(size_t)s * 2 + 1] : 0.0;
    double acc[ALIGN_SUMS_W];
#pragma unroll
    for (int a = 0; a < ALIGN_SUMS_W; ++a) acc[a] = 0.0;
    for (int px = lo + threadIdx.x; px < hi; px += 256) {
        const size_t gp = (size_t)s * M + px;
        const int* e = ent + gp * K;
        const int* tl = tile + gp * K;
        const float* ww = w + gp * K;
        const float R = volume_slice_blend(vals, e, tl, ww, bl, K);
        const float gY = volume_slice_blend(vals + (size_t)T, e, tl, ww, bl, K);
        const float gX = volume_slice_blend(vals + (size_t)2 * T, e, tl, ww, bl, K);
        if (warped) warped[gp] = R;
        if (wgrad) {
            wgrad[gp] = gY;
            wgrad[(size_t)n * M + gp] = gX;
        }
        const float tv = targets[gp], wv = weights ? weights[gp] : 1.f;
        if (align_finite(tv) && align_finite(R) && align_finite(gY) && align_finite(gX) && align_finite(wv) && wv > 0.f) {
            const int i = px / tw, j = px - i * tw;
            const double wd = (double)wv, gr = g * (double)R, m = gr + b;
            const double r = m - (double)tv, gy = g * (double)gY, gx = g * (double)gX;
            const double wr = wd * r, wr2 = 2.0 * wr;
            double J[8];
            J[0] = gy * (double)i, J[1] = gy * (double)j, J[2] = gy;
            J[3] = gx * (double)i, J[4] = gx * (double)j, J[5] = gx;
            J[6] = (double)R, J[7] = 1.0;
            acc[0] += 1.0;
            acc[1] += wd;
            acc[2] += wr * r;
            int q = 11;
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                acc[3 + a] += wr2 * J[a];
                const double wj = wd * J[a];
#pragma unroll
                for (int c = a; c < 8; ++c, ++q) acc[q] += wj * J[c];
            }
        }
    }
    align_block_reduce<ALIGN_SUMS_W>(acc, red, partials);
}

// sums[s, a] = the slice's partial records added in index order
__global__ __launch_bounds__(256) void align_combine_w_kernel(const double* __restrict__ partials, double* __restrict__ sums, int chunks) {
    align_combine<ALIGN_SUMS_W>(partials, sums, chunks);
}

// ---- msiren_align_solve_w* (DESIGN.md section 5.12): section 5.11's loop on the 47 sums ------------------------------------------------------
// One thread per slice between two evaluations.  State per slice: align_step_kernel's, plus the trial and the best (g, b) as fp32 (gb_trial,
// gb_best) and sums_best of 47.  The rule is restated by mri_inr_amd/align.py: lm_step_w -- fp64 + - * / one at a time, every sum in the order
// written there.  Solved parameters P: affine 6 (intensity fixed) or 8 (estimated), rigid 3 or 5; mean = cost / wsum if count >= P else +inf.
struct AlignSolveWParams {
    const double* sums;                  // (n, 47) of the evaluation at `trial`, `gb_trial`
    float *trial, *best;                 // (n, 6)
    float *gb_trial, *gb_best;           // (n, 2)
    double *rigid_trial, *rigid_best;    // (n, 4)
    double* sums_best;                   // (n, 47)
    double* scal;                        // (n, 3) mean_best, mean_first, lam
    int* cnt;                            // (n, 2) accepted, flags
    double* trace;                       // (iterations, n, 11) or null
    float* maps_out;                     // (n, 6)      written behind the last evaluation
    float* intensity_out;                // (n, 2)
    double* rigid_out;                   // (n, 4) or null
    double* report;                      // (n, 7)
    int n, mode, estimate, k, last;      // mode 0 affine, 1 rigid; estimate: (g, b) are solved for; k: the evaluation just done
    double down, up, lam_min, lam_max, cy, cx;
};

// before the first evaluation: trial := best := the inputs (rigid: the map of the input state; intensity null: (1, 0)), lam := damping
__global__ __launch_bounds__(256) void align_solve_init_w_kernel(AlignSolveWParams p, const float* __restrict__ maps_in, const double* __restrict__ rigid_in,
                                                                 const float* __restrict__ intensity_in, double damping) {
#pragma clang fp contract(off)
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= p.n) return;
    float m[6];
    double r[4] = {0.0, 0.0, 0.0, 0.0};
    if (p.mode == 1) {
#pragma unroll
        for (int a = 0; a < 4; ++a) r[a] = rigid_in[(size_t)s * 4 + a];
        align_rigid_map(r[0], r[1], r[2], r[3], p.cy, p.cx, m);
    } else {
#pragma unroll
        for (int a = 0; a < 6; ++a) m[a] = maps_in[(size_t)s * 6 + a];
    }
    const float g = intensity_in ? intensity_in[(size_t)s * 2] : 1.f, b = intensity_in ? intensity_in[(size_t)s * 2 + 1] : 0.f;
#pragma unroll
    for (int a = 0; a < 6; ++a) p.trial[(size_t)s * 6 + a] = m[a], p.best[(size_t)s * 6 + a] = m[a];
    p.gb_trial[(size_t)s * 2] = g, p.gb_trial[(size_t)s * 2 + 1] = b, p.gb_best[(size_t)s * 2] = g, p.gb_best[(size_t)s * 2 + 1] = b;
#pragma unroll
    for (int a = 0; a < 4; ++a) p.rigid_trial[(size_t)s * 4 + a] = r[a], p.rigid_best[(size_t)s * 4 + a] = r[a];
#pragma unroll
    for (int a = 0; a < ALIGN_SUMS_W; ++a) p.sums_best[(size_t)s * ALIGN_SUMS_W + a] = 0.0;
    p.scal[(size_t)s * 3] = __builtin_inf(), p.scal[(size_t)s * 3 + 1] = __builtin_inf(), p.scal[(size_t)s * 3 + 2] = damping;
    p.cnt[(size_t)s * 2] = 0, p.cnt[(size_t)s * 2 + 1] = 0;
}

// behind evaluation k: accept or reject the trial, then propose the next one from the best state.  grid: ceil(n / 256) workgroups of 256
__global__ __launch_bounds__(256) void align_step_w_kernel(AlignSolveWParams p) {
#pragma clang fp contract(off)
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= p.n) return;
    const double inf = __builtin_inf();
    float trial[6], best[6], gbt[2], gbb[2];
    double rt[4], rb[4], bs[ALIGN_SUMS_W];
#pragma unroll
    for (int a = 0; a < 6; ++a) trial[a] = p.trial[(size_t)s * 6 + a], best[a] = p.best[(size_t)s * 6 + a];
#pragma unroll
    for (int a = 0; a < 2; ++a) gbt[a] = p.gb_trial[(size_t)s * 2 + a], gbb[a] = p.gb_best[(size_t)s * 2 + a];
#pragma unroll
    for (int a = 0; a < 4; ++a) rt[a] = p.rigid_trial[(size_t)s * 4 + a], rb[a] = p.rigid_best[(size_t)s * 4 + a];
    double mean_best = p.scal[(size_t)s * 3], mean_first = p.scal[(size_t)s * 3 + 1], lam = p.scal[(size_t)s * 3 + 2];
    int accepted = p.cnt[(size_t)s * 2];
    const double* ev = p.sums + (size_t)s * ALIGN_SUMS_W;
    const double count = ev[0], wsum = ev[1], cost = ev[2];
    if (p.trace) {
        double* tr = p.trace + ((size_t)p.k * p.n + s) * 11;
#pragma unroll
        for (int a = 0; a < 6; ++a) tr[a] = (double)trial[a];
        tr[6] = (double)gbt[0], tr[7] = (double)gbt[1], tr[8] = cost, tr[9] = count, tr[10] = wsum;
    }
    const double solved = (double)((p.mode == 1 ? 3 : 6) + (p.estimate ? 2 : 0));
    const double mean = count >= solved ? cost / wsum : inf;
    const bool accept = align_lm_decide(p.k, mean, &mean_best, &mean_first, &lam, &accepted, p.down, p.up, p.lam_min, p.lam_max);
#pragma unroll
    for (int a = 0; a < ALIGN_SUMS_W; ++a) bs[a] = accept ? ev[a] : p.sums_best[(size_t)s * ALIGN_SUMS_W + a];
    if (accept) {
#pragma unroll
        for (int a = 0; a < 6; ++a) best[a] = trial[a];
        gbb[0] = gbt[0], gbb[1] = gbt[1];
#pragma unroll
        for (int a = 0; a < 4; ++a) rb[a] = rt[a];
#pragma unroll
        for (int a = 0; a < ALIGN_SUMS_W; ++a) p.sums_best[(size_t)s * ALIGN_SUMS_W + a] = bs[a];
#pragma unroll
        for (int a = 0; a < 6; ++a) p.best[(size_t)s * 6 + a] = best[a];
        p.gb_best[(size_t)s * 2] = gbb[0], p.gb_best[(size_t)s * 2 + 1] = gbb[1];
#pragma unroll
        for (int a = 0; a < 4; ++a) p.rigid_best[(size_t)s * 4 + a] = rb[a];
    }
    double H[8][8], gr[8];
    {
        int q = 11;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            gr[a] = bs[3 + a];
#pragma unroll
            for (int b = a; b < 8; ++b, ++q) H[a][b] = bs[q], H[b][a] = bs[q];
        }
    }
    bool ok;
    double dg = 0.0, db = 0.0;
    if (p.mode == 0) {
        double d[8];
        ok = p.estimate ? align_propose_affine<8>(H, gr, lam, d) : align_propose_affine<6>(H, gr, lam, d);
#pragma unroll
        for (int a = 0; a < 6; ++a) trial[a] = (float)((double)best[a] + d[a]);
        dg = d[6], db = d[7];
    } else {
        const double c = rb[0], sn = rb[1], uY = rb[2], uX = rb[3], cy = p.cy, cx = p.cx;
        double d[5];
        ok = p.estimate ? align_propose_rigid<8>(H, gr, lam, c, sn, cy, cx, d) : align_propose_rigid<6>(H, gr, lam, c, sn, cy, cx, d);
        const double u = d[0] / 2.0, uu = u * u, den = 1.0 + uu;
        const double cd = (1.0 - uu) / den, sd = (2.0 * u) / den;
        const double ccd = c * cd, ssd = sn * sd, scd = sn * cd, csd = c * sd;
        rt[0] = ccd - ssd, rt[1] = scd + csd, rt[2] = uY + d[1], rt[3] = uX + d[2];
        align_rigid_map(rt[0], rt[1], rt[2], rt[3], cy, cx, trial);
#pragma unroll
        for (int a = 0; a < 4; ++a) p.rigid_trial[(size_t)s * 4 + a] = rt[a];
        dg = d[3], db = d[4];
    }
    if (p.estimate) {
        gbt[0] = (float)((double)gbb[0] + dg), gbt[1] = (float)((double)gbb[1] + db);
    } else {
        gbt[0] = gbb[0], gbt[1] = gbb[1];
    }
    const int flags = (ok ? 0 : ALIGN_SINGULAR) | (mean_first == inf ? ALIGN_NO_OVERLAP : 0);
#pragma unroll
    for (int a = 0; a < 6; ++a) p.trial[(size_t)s * 6 + a] = trial[a];
    p.gb_trial[(size_t)s * 2] = gbt[0], p.gb_trial[(size_t)s * 2 + 1] = gbt[1];
    p.scal[(size_t)s * 3] = mean_best, p.scal[(size_t)s * 3 + 1] = mean_first, p.scal[(size_t)s * 3 + 2] = lam;
    p.cnt[(size_t)s * 2] = accepted, p.cnt[(size_t)s * 2 + 1] = flags;
    if (p.last) {
#pragma unroll
        for (int a = 0; a < 6; ++a) p.maps_out[(size_t)s * 6 + a] = best[a];
        p.intensity_out[(size_t)s * 2] = gbb[0], p.intensity_out[(size_t)s * 2 + 1] = gbb[1];
        if (p.rigid_out) {
#pragma unroll
            for (int a = 0; a < 4; ++a) p.rigid_out[(size_t)s * 4 + a] = rb[a];
        }
        double* rp = p.report + (size_t)s * 7;
        rp[0] = (double)accepted, rp[1] = mean_first, rp[2] = mean_best, rp[3] = bs[0], rp[4] = bs[1], rp[5] = lam, rp[6] = (double)flags;
    }
}

}  // namespace msiren
