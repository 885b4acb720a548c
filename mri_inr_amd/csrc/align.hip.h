// Slices scored under affine maps against targets (msiren_align_slices*): the steps either side of the ragged jet
// trunk.  Slice s of n is read on the th x tw lattice of its target under its own map (a00, a01, t0, a10, a11, t1): pixel (i, j) at
//     Y = ((a00 i) + (a01 j)) + t0        X = ((a10 i) + (a11 j)) + t1        fp32, every operation rounded on its own (no fma)
// in reconstruction pixel coordinates.  (Y, X) -> cover rule, slots, local coordinate and weight are resample.hip.h's, the bins (slice,
// tile) and their election resample_volume.hip.h's with one slice per point: R, gY, gX are the bits of msiren_resample_slices_grad.
//
//   bin      align_count_kernel     one thread per (slice, pixel): covers per bin b = s nV nH + t, integer atomics aggregated per wave
//                                   (wave_bin_add)
//            resample_scan_kernel   (resample.hip.h) exclusive scan over the n nV nH bins -> the ragged offsets
//            align_fill_kernel      the same election on the cursors; entry, tile and weight per slot (g K + k), g = s th tw + p
//   trunk    the exact-fp32 jet ragged trunk over T = n th tw K entries at most, one replica, on the plan's rows
//   reduce   align_partial_kernel   one workgroup per (slice, chunk of ALIGN_CHUNK pixels): blend of the three planes per pixel
//                                   (volume_slice_blend), [warped], [wgrad], the 29 fp64 sums of the chunk -> one partial record
//            align_combine_kernel   one workgroup per slice: its partial records added in index order -> sums (n, 29)
// A pixel is VALID iff target, R, gY, gX are all finite; per valid pixel, in fp64 from the fp32 numbers, contraction off:
//     r = R - T,  J = (gY i, gY j, gY, gX i, gX j, gX),  count += 1, cost += r r, dcost[a] += (2 r) J[a], jtj[a, b] += J[a] J[b] (a <= b)
// record = [count, cost, dcost 6, jtj packed upper triangle row-major 21].
// Every sum has ONE order: thread t of a chunk adds its pixels lo + t, lo + t + 256, ... in that order, the 256 totals are combined as
// score_block_sum does (butterfly inside each wave, then the four waves in order), the chunks of a slice in index order.  No
// floating-point atomics: the same bits run to run, alone or in any batch, with or without the optional outputs.
#pragma once
#include <hip/hip_runtime.h>

#include "resample_volume.hip.h"

namespace msiren {

constexpr int ALIGN_CHUNK = 1024;  // pixels per partial workgroup (4 per thread)
constexpr int ALIGN_SUMS = 29;     // count, cost, dcost[6], jtj[21]

struct AlignParams {
    const float* maps;    // (n, 6)
    int n, th, tw, M;     // M = th tw pixels per slice
    int nV, nH, S, I, pad, KA;
    int* counts;          // (NP) covers per bin, NP = n nV nH; zero before the count kernel
    int* cursors;         // (NP) zero before the fill kernel
    int* offsets;         // (NP + 1)
    float* coords;        // (T, 2) entries: local coordinates, bin by bin; T = n M K
    int* ent;             // (T) slot (g, k) -> entry, -1: none
    int* tile;            // (T) slot (g, k) -> tile of the slice
    float* w;             // (T) slot (g, k) -> fold weight
};

// where pixel (i, j) of the lattice is read under map a[0..5]: fp32, one rounding per operation
__device__ __forceinline__ void align_point(const float* __restrict__ a, int i, int j, float* Y, float* X) {
#pragma clang fp contract(off)
    const float fi = (float)i, fj = (float)j;  // (below 2^24: exact)
    const float y0 = a[0] * fi, y1 = a[1] * fj, x0 = a[3] * fi, x1 = a[4] * fj;
    const float ys = y0 + y1, xs = x0 + x1;
    *Y = ys + a[2];
    *X = xs + a[5];
}

// thread g of the grid -> (slice, pixel) and its point; false beyond the last pixel
__device__ __forceinline__ bool align_thread_point(const AlignParams& p, int g, int* s, float* Y, float* X) {
    *s = 0, *Y = 0.f, *X = 0.f;
    if (g >= p.n * p.M) return false;  // (n M < 2^31: checked by the host)
    *s = g / p.M;
    const int px = g - *s * p.M, i = px / p.tw;
    align_point(p.maps + 6 * (size_t)*s, i, px - i * p.tw, Y, X);
    return true;
}

__global__ __launch_bounds__(256) void align_count_kernel(AlignParams p) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    int s, v0 = 0, h0 = 0, nv = 0, nh = 0;
    float Y, X;
    if (align_thread_point(p, g, &s, &Y, &X)) nv = cover_axis(Y, p.nV, p.S, p.I, p.pad, &v0), nh = cover_axis(X, p.nH, p.S, p.I, p.pad, &h0);
    const int NPt = p.nV * p.nH;
    for (int a = 0; a < p.KA; ++a)
        for (int b = 0; b < p.KA; ++b) {
            const bool has = a < nv && b < nh;
            (void)wave_bin_add(p.counts, has ? s * NPt + (v0 + a) * p.nH + h0 + b : 0, has);
        }
}

__global__ __launch_bounds__(256) void align_fill_kernel(AlignParams p) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int K = p.KA * p.KA;
    int s, v0 = 0, h0 = 0, nv = 0, nh = 0;
    float Y, X;
    const bool in = align_thread_point(p, g, &s, &Y, &X);
    if (in) nv = cover_axis(Y, p.nV, p.S, p.I, p.pad, &v0), nh = cover_axis(X, p.nH, p.S, p.I, p.pad, &h0);
    const int NPt = p.nV * p.nH;
    const double c = 0.5 * (double)(p.S - 1), den = (double)(p.S - 1);
    for (int a = 0; a < p.KA; ++a)
        for (int b = 0; b < p.KA; ++b) {
            const bool has = a < nv && b < nh;
            const int t = (v0 + a) * p.nH + h0 + b, bin = has ? s * NPt + t : 0;
            const int place = wave_bin_add(p.cursors, bin, has);
            if (has) {  // (g < n M)
                const int k = a * nh + b;  // the point's covering tiles in (v, h) row-major order
                const double ty = (double)Y - (double)((v0 + a) * p.I - p.pad), tx = (double)X - (double)((h0 + b) * p.I - p.pad);
                const int e = p.offsets[bin] + place;
                reinterpret_cast<float2*>(p.coords)[e] = make_float2((float)(-1.0 + ty * 2.0 / den), (float)(-1.0 + tx * 2.0 / den));
                p.ent[(size_t)g * K + k] = e;
                p.tile[(size_t)g * K + k] = t;
                p.w[(size_t)g * K + k] = (float)exp(-0.1 * sqrt((ty - c) * (ty - c) + (tx - c) * (tx - c)));
            }
        }
    if (in)
        for (int k = nv * nh; k < K; ++k) p.ent[(size_t)g * K + k] = -1;
}

__device__ __forceinline__ bool align_finite(float x) { return fabsf(x) < __builtin_inff(); }  // (false for a NaN)

// vals (3, T): the jet ragged trunk's outputs by entry.  black (n NPt).  targets (n, M).  warped (n, M) and wgrad (2, n, M) may be null.
// partials (n chunks, ALIGN_SUMS).  grid: n * chunks workgroups (slice-major), chunks = ceil(M / ALIGN_CHUNK)
__global__ __launch_bounds__(256) void align_partial_kernel(const float* __restrict__ vals, const int* __restrict__ ent, const int* __restrict__ tile,
                                                            const float* __restrict__ w, const int* __restrict__ black, const float* __restrict__ targets,
                                                            float* __restrict__ warped, float* __restrict__ wgrad, double* __restrict__ partials, int n, int M,
                                                            int tw, int K, int NPt, int T, int chunks) {
#pragma clang fp contract(off)
    __shared__ double red[ALIGN_SUMS][4];
    const int s = blockIdx.x / chunks, chunk = blockIdx.x - s * chunks;
    const int lo = chunk * ALIGN_CHUNK, hi = lo + ALIGN_CHUNK < M ? lo + ALIGN_CHUNK : M;
    const int* bl = black + (size_t)s * NPt;
    double acc[ALIGN_SUMS];
#pragma unroll
    for (int a = 0; a < ALIGN_SUMS; ++a) acc[a] = 0.0;
    for (int px = lo + threadIdx.x; px < hi; px += 256) {
        const size_t g = (size_t)s * M + px;
        const int* e = ent + g * K;
        const int* tl = tile + g * K;
        const float* ww = w + g * K;
        const float R = volume_slice_blend(vals, e, tl, ww, bl, K);
        const float gY = volume_slice_blend(vals + (size_t)T, e, tl, ww, bl, K);
        const float gX = volume_slice_blend(vals + (size_t)2 * T, e, tl, ww, bl, K);
        if (warped) warped[g] = R;
        if (wgrad) {
            wgrad[g] = gY;
            wgrad[(size_t)n * M + g] = gX;
        }
        const float tv = targets[g];
        if (align_finite(tv) && align_finite(R) && align_finite(gY) && align_finite(gX)) {
            const int i = px / tw, j = px - i * tw;
            const double r = (double)R - (double)tv, r2 = 2.0 * r;
            double J[6];
            J[0] = (double)gY * (double)i, J[1] = (double)gY * (double)j, J[2] = (double)gY;
            J[3] = (double)gX * (double)i, J[4] = (double)gX * (double)j, J[5] = (double)gX;
            acc[0] += 1.0;
            acc[1] += r * r;
            int q = 8;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                acc[2 + a] += r2 * J[a];
#pragma unroll
                for (int b = a; b < 6; ++b, ++q) acc[q] += J[a] * J[b];
            }
        }
    }
    // score_block_sum's order for all 29 at once: butterfly inside each wave, then the four wave totals in wave order
#pragma unroll
    for (int a = 0; a < ALIGN_SUMS; ++a) {
        double v = acc[a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) red[a][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < ALIGN_SUMS) {
        const int a = threadIdx.x;
        partials[(size_t)blockIdx.x * ALIGN_SUMS + a] = ((red[a][0] + red[a][1]) + red[a][2]) + red[a][3];
    }
}

// sums[s, a] = the slice's partial records added in index order
__global__ __launch_bounds__(256) void align_combine_kernel(const double* __restrict__ partials, double* __restrict__ sums, int chunks) {
#pragma clang fp contract(off)
    const int s = blockIdx.x, a = threadIdx.x;
    if (a < ALIGN_SUMS) {
        const double* pr = partials + (size_t)s * chunks * ALIGN_SUMS + a;
        double t = pr[0];
        for (int c = 1; c < chunks; ++c) t += pr[(size_t)c * ALIGN_SUMS];
        sums[(size_t)s * ALIGN_SUMS + a] = t;
    }
}

}  // namespace msiren
