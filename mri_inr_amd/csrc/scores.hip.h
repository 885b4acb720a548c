// The evaluation harness's image-quality scores (src/util/error.py:23-84, as mri_inr_amd/metrics.py restates them) on the device:
// per pair (original o, predicted p) of (H, W) float32 images, PSNR, SSIM (7 x 7 uniform window, K1 = 0.01, K2 = 0.03, sample
// covariance, mean over the (H-6) x (W-6) windows inside the image) and NRMSE ('euclidean': sqrt(mean((o-p)^2)) / sqrt(mean(o^2))).
//
// Three launches on one stream, every sum in a fixed order and no atomics, so a pair's scores are the same bits run to run and
// whether it is scored alone or inside a batch of any size (the partition of a pair depends on H and W only):
//   1. score_stats_kernel    one workgroup per chunk of SCORE_CHUNK pixels of a pair: min / max of o and p, sum (o-p)^2, sum o^2
//   2. score_ssim_kernel     one workgroup per 32 x 16 windows of a pair: data range from pass 1 (min / max: exact in any order),
//                            the five window moments as direct 7-tap fp64 sums (horizontal, then vertical, through LDS), the sum of S
//   3. score_combine_kernel  one workgroup per pair: the partials of 1 and 2 summed in index order -> (PSNR, SSIM, NRMSE) in fp64
// SSIM depends nonlinearly on the data range (C1, C2), which needs the whole image: hence a statistics pass before the window pass.
// The arithmetic follows metrics.py's expressions term by term with fused multiply-adds off, so identical images give exactly 1.0.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace msiren {

constexpr int SCORE_THREADS = 256;
constexpr int SCORE_CHUNK = 8192;   // pixels per statistics workgroup (32 per thread)
constexpr int SCORE_WIN = 7;        // skimage's default win_size
constexpr int SCORE_TW = 32, SCORE_TH = 16;  // windows per SSIM workgroup: 32 wide, 16 tall (35 KB of LDS: four workgroups per CU)
constexpr int SCORE_HW = SCORE_TW + SCORE_WIN - 1, SCORE_HH = SCORE_TH + SCORE_WIN - 1;  // the pixels they cover
constexpr int SCORE_LOADS = (SCORE_HW * SCORE_HH + SCORE_THREADS - 1) / SCORE_THREADS;   // halo loads per thread (all issued at once)

struct ScoreStat {  // pass-1 partial of one chunk
    float mn_o, mx_o, mn_p, mx_p;
    double sdd, soo;  // sum (o-p)^2, sum o^2
};

// Block-wide reductions of 256 threads in a fixed order: butterfly inside each wave (both lanes of a pair add the same two values,
// so every lane ends with the same bits), then the four wave totals in wave order.  Every thread returns the total.
__device__ __forceinline__ double score_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return t;
}
__device__ __forceinline__ void score_block_minmax(float& mn, float& mx, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = mn;
        red[4 + (threadIdx.x >> 6)] = mx;
    }
    __syncthreads();
    mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    __syncthreads();
}

// min over o and p, max over o and p of one pair, from its pass-1 partials
__device__ __forceinline__ void score_pair_range(const ScoreStat* __restrict__ st, int chunks, float& mn, float& mx, float* red) {
    mn = __builtin_inff();
    mx = -__builtin_inff();
    for (int i = threadIdx.x; i < chunks; i += SCORE_THREADS) {
        const ScoreStat s = st[i];
        mn = fminf(mn, fminf(s.mn_o, s.mn_p));
        mx = fmaxf(mx, fmaxf(s.mx_o, s.mx_p));
    }
    score_block_minmax(mn, mx, red);
}

// grid: n * chunks workgroups (pair-major)
__global__ __launch_bounds__(SCORE_THREADS) void score_stats_kernel(const float* __restrict__ o, const float* __restrict__ p,
                                                                    ScoreStat* __restrict__ stats, int64_t hw, int chunks) {
#pragma clang fp contract(off)
    __shared__ double dred[4];
    __shared__ float fred[8];
    const int64_t pair = blockIdx.x / chunks;
    const int chunk = (int)(blockIdx.x - pair * chunks);
    const float* po = o + pair * hw;
    const float* pp = p + pair * hw;
    const int64_t lo = (int64_t)chunk * SCORE_CHUNK;
    const int64_t hi = lo + SCORE_CHUNK < hw ? lo + SCORE_CHUNK : hw;
    float mn_o = __builtin_inff(), mx_o = -__builtin_inff(), mn_p = __builtin_inff(), mx_p = -__builtin_inff();
    double sdd = 0.0, soo = 0.0;
#pragma unroll 8
    for (int64_t i = lo + threadIdx.x; i < hi; i += SCORE_THREADS) {
        const float a = po[i], b = pp[i];
        mn_o = fminf(mn_o, a);
        mx_o = fmaxf(mx_o, a);
        mn_p = fminf(mn_p, b);
        mx_p = fmaxf(mx_p, b);
        const double d = (double)a - (double)b;  // exact: both are fp32
        sdd += d * d;
        soo += (double)a * (double)a;
    }
    score_block_minmax(mn_o, mx_o, fred);
    score_block_minmax(mn_p, mx_p, fred);
    sdd = score_block_sum(sdd, dred);
    soo = score_block_sum(soo, dred);
    if (threadIdx.x == 0) stats[blockIdx.x] = ScoreStat{mn_o, mx_o, mn_p, mx_p, sdd, soo};
}

// grid: n * tiles workgroups (pair-major), tiles = ceil((W-6)/32) * ceil((H-6)/16)
__global__ __launch_bounds__(SCORE_THREADS) void score_ssim_kernel(const float* __restrict__ o, const float* __restrict__ p,
                                                                   const ScoreStat* __restrict__ stats, double* __restrict__ ssim_part,
                                                                   int H, int W, int chunks, int tiles_x, int tiles) {
#pragma clang fp contract(off)
    __shared__ float so[SCORE_HH][SCORE_HW + 1], sp[SCORE_HH][SCORE_HW + 1];
    __shared__ double hs[5][SCORE_HH][SCORE_TW];  // horizontal 7-tap sums of o, p, o^2, p^2, o p
    __shared__ double dred[4];
    __shared__ float fred[8];
    const int tid = threadIdx.x;
    const int64_t pair = blockIdx.x / tiles;
    const int t = (int)(blockIdx.x - pair * tiles), ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y0 = ty * SCORE_TH, x0 = tx * SCORE_TW;
    const float* po = o + pair * H * (int64_t)W;
    const float* pp = p + pair * H * (int64_t)W;
    float va[SCORE_LOADS], vb[SCORE_LOADS];
#pragma unroll
    for (int j = 0; j < SCORE_LOADS; ++j) {  // every load in flight before the first LDS store
        const int i = tid + j * SCORE_THREADS, r = i / SCORE_HW, c = i - r * SCORE_HW, gy = y0 + r, gx = x0 + c;
        const bool in = i < SCORE_HW * SCORE_HH && gy < H && gx < W;  // pixels past the edge feed only windows that are not counted
        const int64_t g = (int64_t)gy * W + gx;
        va[j] = in ? po[g] : 0.f;
        vb[j] = in ? pp[g] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < SCORE_LOADS; ++j) {
        const int i = tid + j * SCORE_THREADS, r = i / SCORE_HW, c = i - r * SCORE_HW;
        if (i < SCORE_HW * SCORE_HH) {
            so[r][c] = va[j];
            sp[r][c] = vb[j];
        }
    }
    float mn, mx;
    score_pair_range(stats + pair * chunks, chunks, mn, mx, fred);  // (its barriers also order the LDS stores above)
    const float drf = mx - mn;  // in fp32, as numpy subtracts two float32 scalars (metrics.calculate_data_range)
    const double dr = (double)drf;
    const double c1 = (0.01 * dr) * (0.01 * dr), c2 = (0.03 * dr) * (0.03 * dr);
    for (int i = tid; i < SCORE_HH * SCORE_TW; i += SCORE_THREADS) {
        const int r = i / SCORE_TW, c = i - r * SCORE_TW;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
        for (int k = 0; k < SCORE_WIN; ++k) {
            const double a = so[r][c + k], b = sp[r][c + k];
            s0 += a;
            s1 += b;
            s2 += a * a;  // products of fp32 values: exact in fp64
            s3 += b * b;
            s4 += a * b;
        }
        hs[0][r][c] = s0;
        hs[1][r][c] = s1;
        hs[2][r][c] = s2;
        hs[3][r][c] = s3;
        hs[4][r][c] = s4;
    }
    __syncthreads();
    const double n = SCORE_WIN * SCORE_WIN, cov_norm = n / (n - 1.0);
    double acc = 0.0;
    for (int i = tid; i < SCORE_TH * SCORE_TW; i += SCORE_THREADS) {
        const int r = i / SCORE_TW, c = i - r * SCORE_TW;
        if (y0 + r > H - SCORE_WIN || x0 + c > W - SCORE_WIN) continue;  // window not fully inside the image
        double m[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < SCORE_WIN; ++k) s += hs[q][r + k][c];
            m[q] = s / n;
        }
        const double ux = m[0], uy = m[1], uxx = m[2], uyy = m[3], uxy = m[4];
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
        acc += ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
    }
    acc = score_block_sum(acc, dred);
    if (tid == 0) ssim_part[blockIdx.x] = acc;
}

// grid: n workgroups; scores[pair] = (PSNR, SSIM, NRMSE)
__global__ __launch_bounds__(SCORE_THREADS) void score_combine_kernel(const ScoreStat* __restrict__ stats, const double* __restrict__ ssim_part,
                                                                      double* __restrict__ scores, int H, int W, int chunks, int tiles) {
#pragma clang fp contract(off)
    __shared__ double dred[4];
    __shared__ float fred[8];
    const int64_t pair = blockIdx.x;
    const ScoreStat* st = stats + pair * chunks;
    const double* sp = ssim_part + pair * tiles;
    float mn, mx;
    score_pair_range(st, chunks, mn, mx, fred);
    double sdd = 0.0, soo = 0.0, ss = 0.0;
    for (int i = threadIdx.x; i < chunks; i += SCORE_THREADS) {
        sdd += st[i].sdd;
        soo += st[i].soo;
    }
    for (int i = threadIdx.x; i < tiles; i += SCORE_THREADS) ss += sp[i];
    sdd = score_block_sum(sdd, dred);
    soo = score_block_sum(soo, dred);
    ss = score_block_sum(ss, dred);
    if (threadIdx.x == 0) {
        const float drf = mx - mn;
        const double dr = (double)drf;
        const double npix = (double)H * (double)W;
        const double mse = sdd / npix;
        double* out = scores + pair * 3;
        out[0] = 10.0 * log10(dr * dr / mse);
        out[1] = ss / ((double)(H - SCORE_WIN + 1) * (double)(W - SCORE_WIN + 1));
        out[2] = sqrt(mse) / sqrt(soo / npix);
    }
}

}  // namespace msiren
