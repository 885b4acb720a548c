// Robust alignment of target slices to a stack read as a volume (msiren_align_volume_r* and
// msiren_align_volume_solve_group_r*): align_volume_w.hip.h's reduce with a Geman-McClure loss rho(r) = r^2 / (1 + r^2 / s) in place of the square,
// s = scale[q] > 0 per target in squared intensity units.  Points, bins, the jet ragged trunk and the blend are align_volume.hip.h's, unchanged:
// R, gZ, gY, gX stay the bits of msiren_resample_volume_grad.  The record stays section 5.14's 80 sums, so the combine kernel is
// align_volume_combine_w_kernel and every step stage that reads the 80 sums runs on these unchanged.
//
//   reduce   align_volume_partial_r_kernel   one workgroup per (target, chunk of ALIGN_CHUNK pixels): align_volume_partial_w_kernel's blend, wd, r and
//                                            J per pixel, [warped], [wgrad], [rweight], the 80 fp64 sums of the chunk -> one partial record
// A pixel is VALID iff align_volume_partial_w_kernel's condition holds and s > 0 (a NaN, zero or negative s: no pixel of the target is valid;
// s = +inf is allowed).  Per valid pixel, in fp64, contraction off, one rounding per operation, in exactly this association:
//     u = (r r) / s,  v = 1.0 + u,  om = 1.0 / v,  wl = wd om,  wq = wl om
//     count += 1, wsum += wd, cost += (wl r) r, dcost[a] += (2.0 (wq r)) J[a], jtj[a, b] += (wq J[a]) J[b] (a <= b)
// cost is the weighted loss, dcost its exact gradient, jtj the majoriser's (IRLS) Gauss-Newton matrix, wsum the plain sum of the weights.  With
// s = +inf: u = 0, v = om = 1, wl = wq = wd, and every term is align_volume_partial_w_kernel's term -- the same bits.
// rweight (m, Mt) float32, optional: (float)(om om) at a valid pixel, NaN elsewhere (the outlier map).
#pragma once
#include <hip/hip_runtime.h>

#include "align_volume_w.hip.h"

namespace msiren {

// scale (m) doubles.  rweight (m, Mt) may be null.  Every other argument and the grid: align_volume_partial_w_kernel's
__global__ __launch_bounds__(256) void align_volume_partial_r_kernel(const float* __restrict__ vals, const int* __restrict__ ent, const int* __restrict__ tile,
                                                                     const float* __restrict__ w, const int* __restrict__ black, const int* __restrict__ pair,
                                                                     const float* __restrict__ fz, const float* __restrict__ targets,
                                                                     const float* __restrict__ weights, const float* __restrict__ intensity,
                                                                     const double* __restrict__ scale, float* __restrict__ warped, float* __restrict__ wgrad,
                                                                     float* __restrict__ rweight, double* __restrict__ partials, int m, int Mt, int tw, int K, int NPt,
                                                                     int T, int chunks) {
#pragma clang fp contract(off)
    __shared__ double red[ALIGN_VOLUME_SUMS_W][4];
    const int q = blockIdx.x / chunks, chunk = blockIdx.x - q * chunks;
    const int lo = chunk * ALIGN_CHUNK, hi = lo + ALIGN_CHUNK < Mt ? lo + ALIGN_CHUNK : Mt;
    const size_t M = (size_t)m * Mt;
    const double g = intensity ? (double)intensity[(size_t)q * 2] : 1.0, b = intensity ? (double)intensity[(size_t)q * 2 + 1] : 0.0;
    const double s = scale[q];
    const bool scored = s > 0.0;  // (false for a NaN)
    double acc[ALIGN_VOLUME_SUMS_W];
#pragma unroll
    for (int a = 0; a < ALIGN_VOLUME_SUMS_W; ++a) acc[a] = 0.0;
    for (int px = lo + threadIdx.x; px < hi; px += 256) {
        const size_t gp = (size_t)q * Mt + px;
        const int z0 = pair[gp];
        float pl[3], gZ;
        if (z0 < 0) {  // invalid Z: NaN in every plane, as resample_volume_blend_kernel writes it
            pl[0] = pl[1] = pl[2] = gZ = __builtin_nanf("");
        } else {
            const float f = fz[gp], a0 = 1.0f - f;
            const int* e0 = ent + 2 * gp * K;
            const int* tl = tile + gp * K;
            const float* ww = w + gp * K;
            const int *b0 = black + (size_t)z0 * NPt, *b1 = black + (size_t)(z0 + 1) * NPt;
            gZ = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* v = vals + (size_t)c * T;
                const float R0 = volume_slice_blend(v, e0, tl, ww, b0, K);
                const float R1 = volume_slice_blend(v, e0 + K, tl, ww, b1, K);
                pl[c] = f == 0.f ? R0 : f == 1.f ? R1 : __builtin_fmaf(f, R1, a0 * R0);
                if (c == 0) gZ = R1 - R0;
            }
        }
        const float R = pl[0], gY = pl[1], gX = pl[2];
        if (warped) warped[gp] = R;
        if (wgrad) {
            wgrad[gp] = gZ;
            wgrad[M + gp] = gY;
            wgrad[2 * M + gp] = gX;
        }
        const float tv = targets[gp], wv = weights ? weights[gp] : 1.f;
        float rw = __builtin_nanf("");
        if (scored && align_finite(tv) && align_finite(R) && align_finite(gZ) && align_finite(gY) && align_finite(gX) && align_finite(wv) && wv > 0.f) {
            const int i = px / tw, j = px - i * tw;
            const double wd = (double)wv, gr = g * (double)R, mm = gr + b, di = (double)i, dj = (double)j;
            const double r = mm - (double)tv, gz = g * (double)gZ, gy = g * (double)gY, gx = g * (double)gX;
            const double rr = r * r, u = rr / s, v = 1.0 + u, om = 1.0 / v;
            const double wl = wd * om, wq = wl * om;
            const double wlr = wl * r, wqr = wq * r, wr2 = 2.0 * wqr;
            rw = (float)(om * om);
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
        if (rweight) rweight[gp] = rw;
    }
    align_block_reduce<ALIGN_VOLUME_SUMS_W>(acc, red, partials);
}

}  // namespace msiren
