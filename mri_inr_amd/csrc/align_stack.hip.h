// Target slices scored against a plain voxel stack (msiren_align_stack_r* and msiren_align_stack_solve_group_r*): section
// 5.16's robust 80 sums with the pixel read trilinearly from a float32 stack (n, H, W) instead of from the network's reconstruction.  No prologue, no
// bins, no trunk, no weights of the model.  The point is align_point3's; everything behind the pixel is align_volume_partial_w_body<true>.
//
//   reduce   align_stack_partial_r_kernel   one workgroup per (target, chunk of ALIGN_CHUNK pixels): per pixel the point, eight loads, the read below,
//                                           [warped], [wgrad], [rweight], the 80 fp64 sums of the chunk -> one partial record
//            align_volume_combine_w_kernel  (align_volume_w.hip.h) the chunks of a target in index order -> sums (m, 80)
// The read at (Z, Y, X), fp32 from align_point3.  Inside iff 0 <= Z <= n - 1, 0 <= Y <= H - 1, 0 <= X <= W - 1, compared in fp32 (n, H, W below 2^24: the
// bounds are exact; a NaN fails).  Outside: NaN in all four values.  Inside, in fp64 from the fp32 numbers, + - * only, one rounding each, contraction off:
//     z0 = min((int)floorf(Z), n - 2),  fz = (double)Z - z0,  az = 1.0 - fz      (y0, fy, ay and x0, fx, ax likewise with H, W)
//     V[dz][dy][dx] = (double)stack[z0 + dz, y0 + dy, x0 + dx]
//     c[dz][dy] = (ax V[dz][dy][0]) + (fx V[dz][dy][1])          dx_[dz][dy] = V[dz][dy][1] - V[dz][dy][0]
//     e[dz] = (ay c[dz][0]) + (fy c[dz][1])      ex[dz] = (ay dx_[dz][0]) + (fy dx_[dz][1])      ey[dz] = c[dz][1] - c[dz][0]
//     R = (float)((az e[0]) + (fz e[1]))     gX = (float)((az ex[0]) + (fz ex[1]))     gY = (float)((az ey[0]) + (fz ey[1]))     gZ = (float)(e[1] - e[0])
// A corner that is not finite is not special-cased: it reaches the values through the arithmetic (0 NaN included), so a pixel needs all eight corners
// finite.  At the upper faces the last cell is read with f = 1.  The gradient is the derivative of the interpolant inside the cell that was read.
// Every index stays inside the stack (z0 in 0 .. n - 2, y0 in 0 .. H - 2, x0 in 0 .. W - 2; n H W < 2^30: checked by the host).
#pragma once
#include <hip/hip_runtime.h>

#include "align_volume_r.hip.h"

namespace msiren {

// the lower corner of the cell that holds v on an axis of `len` voxels (0 <= v <= len - 1), and the fraction inside it
__device__ __forceinline__ int align_stack_cell(float v, int len, double* f, double* a) {
#pragma clang fp contract(off)
    int c = (int)floorf(v);
    c = c < len - 2 ? c : len - 2;
    *f = (double)v - (double)c;
    *a = 1.0 - *f;
    return c;
}

// R, gZ, gY, gX of the stack at (Z, Y, X): the rule above
__device__ __forceinline__ void align_stack_read(const float* __restrict__ stack, int n, int H, int W, float Z, float Y, float X, float* R, float* gZ, float* gY,
                                                 float* gX) {
#pragma clang fp contract(off)
    const bool inside = Z >= 0.f && Z <= (float)(n - 1) && Y >= 0.f && Y <= (float)(H - 1) && X >= 0.f && X <= (float)(W - 1);  // (false for a NaN)
    if (!inside) {
        *R = *gZ = *gY = *gX = __builtin_nanf("");
        return;
    }
    double fz, az, fy, ay, fx, ax;
    const int z0 = align_stack_cell(Z, n, &fz, &az), y0 = align_stack_cell(Y, H, &fy, &ay), x0 = align_stack_cell(X, W, &fx, &ax);
    const float* p = stack + ((size_t)z0 * H + y0) * W + x0;
    const size_t sz = (size_t)H * W;
    double e[2], ex[2], ey[2];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        double c[2], d[2];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const double v0 = (double)p[dz * sz + (size_t)dy * W], v1 = (double)p[dz * sz + (size_t)dy * W + 1];
            const double t0 = ax * v0, t1 = fx * v1;
            c[dy] = t0 + t1;
            d[dy] = v1 - v0;
        }
        const double t0 = ay * c[0], t1 = fy * c[1], u0 = ay * d[0], u1 = fy * d[1];
        e[dz] = t0 + t1;
        ex[dz] = u0 + u1;
        ey[dz] = c[1] - c[0];
    }
    const double r0 = az * e[0], r1 = fz * e[1], x0_ = az * ex[0], x1_ = fz * ex[1], y0_ = az * ey[0], y1_ = fz * ey[1];
    *R = (float)(r0 + r1);
    *gX = (float)(x0_ + x1_);
    *gY = (float)(y0_ + y1_);
    *gZ = (float)(e[1] - e[0]);
}

// stack (n, H, W).  maps (m, 9).  targets (m, Mt), weights (m, Mt) or null, intensity (m, 2) or null, scale (m) doubles.  warped (m, Mt), wgrad (3, m, Mt) and
// rweight (m, Mt) may be null.  partials (m chunks, ALIGN_VOLUME_SUMS_W).  grid: m * chunks workgroups (target-major), chunks = ceil(Mt / ALIGN_CHUNK)
__global__ __launch_bounds__(256) void align_stack_partial_r_kernel(const float* __restrict__ stack, const float* __restrict__ maps, const float* __restrict__ targets,
                                                                    const float* __restrict__ weights, const float* __restrict__ intensity,
                                                                    const double* __restrict__ scale, float* __restrict__ warped, float* __restrict__ wgrad,
                                                                    float* __restrict__ rweight, double* __restrict__ partials, int n, int H, int W, int m, int Mt, int tw,
                                                                    int chunks) {
    const size_t M = (size_t)m * Mt;
    const float* const mp = maps + 9 * (size_t)(blockIdx.x / chunks);
    align_volume_partial_w_body<true>(
        [&](size_t gp, int px, float* R, float* gZ, float* gY, float* gX) {
            const int i = px / tw;
            float Z, Y, X;
            align_point3(mp, i, px - i * tw, &Z, &Y, &X);
            align_stack_read(stack, n, H, W, Z, Y, X, R, gZ, gY, gX);
            if (warped) warped[gp] = *R;
            if (wgrad) {
                wgrad[gp] = *gZ;
                wgrad[M + gp] = *gY;
                wgrad[2 * M + gp] = *gX;
            }
        },
        targets, weights, intensity, scale, rweight, partials, Mt, tw, chunks);
}

}  // namespace msiren
