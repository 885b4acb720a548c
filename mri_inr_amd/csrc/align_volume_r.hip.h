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
// The kernel's body is align_volume_partial_w_body<true> (align_volume_w.hip.h), shared with the weighted reduce and, with another pixel source, with
// align_stack_partial_r_kernel (align_stack.hip.h); here are the robust factors it calls and the kernel as a wrapper.
#pragma once
#include <hip/hip_runtime.h>

#include "align_volume_w.hip.h"

namespace msiren {

// u = (r r) / s,  v = 1.0 + u,  om = 1.0 / v  ->  wl = wd om,  wq = wl om,  rw = (float)(om om)
__device__ __forceinline__ void align_robust_factors(double wd, double r, double s, double* wl, double* wq, float* rw) {
#pragma clang fp contract(off)
    const double rr = r * r, u = rr / s, v = 1.0 + u, om = 1.0 / v;
    *wl = wd * om, *wq = *wl * om;
    *rw = (float)(om * om);
}

// scale (m) doubles.  rweight (m, Mt) may be null.  Every other argument and the grid: align_volume_partial_w_kernel's
__global__ __launch_bounds__(256) void align_volume_partial_r_kernel(const float* __restrict__ vals, const int* __restrict__ ent, const int* __restrict__ tile,
                                                                     const float* __restrict__ w, const int* __restrict__ black, const int* __restrict__ pair,
                                                                     const float* __restrict__ fz, const float* __restrict__ targets,
                                                                     const float* __restrict__ weights, const float* __restrict__ intensity,
                                                                     const double* __restrict__ scale, float* __restrict__ warped, float* __restrict__ wgrad,
                                                                     float* __restrict__ rweight, double* __restrict__ partials, int m, int Mt, int tw, int K, int NPt,
                                                                     int T, int chunks) {
    const size_t M = (size_t)m * Mt;
    align_volume_partial_w_body<true>(
        [&](size_t gp, int, float* R, float* gZ, float* gY, float* gX) { align_volume_pixel(vals, ent, tile, w, black, pair, fz, warped, wgrad, gp, M, K, NPt, T, R, gZ, gY, gX); },
        targets, weights, intensity, scale, rweight, partials, Mt, tw, chunks);
}

}  // namespace msiren
