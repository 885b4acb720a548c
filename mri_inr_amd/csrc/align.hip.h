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

// The one order of a chunk's N sums over its 256 threads, score_block_sum's for all N at once: butterfly inside each wave, then the four wave
// totals in wave order -> partials[block, 0..N).  red: the workgroup's N x 4 doubles of LDS.  Every partial kernel ends with this.
template <int N>
__device__ __forceinline__ void align_block_reduce(const double (&acc)[N], double (&red)[N][4], double* __restrict__ partials) {
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double v = acc[a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) red[a][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int a = threadIdx.x;
        partials[(size_t)blockIdx.x * N + a] = ((red[a][0] + red[a][1]) + red[a][2]) + red[a][3];
    }
}

// sums[unit, a] = the unit's `chunks` partial records added in index order: the body of every combine kernel (one workgroup per unit)
template <int N>
__device__ __forceinline__ void align_combine(const double* __restrict__ partials, double* __restrict__ sums, int chunks) {
#pragma clang fp contract(off)
    const int s = blockIdx.x, a = threadIdx.x;
    if (a < N) {
        const double* pr = partials + (size_t)s * chunks * N + a;
        double t = pr[0];
        for (int c = 1; c < chunks; ++c) t += pr[(size_t)c * N];
        sums[(size_t)s * N + a] = t;
    }
}

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
    align_block_reduce<ALIGN_SUMS>(acc, red, partials);
}

// sums[s, a] = the slice's partial records added in index order
__global__ __launch_bounds__(256) void align_combine_kernel(const double* __restrict__ partials, double* __restrict__ sums, int chunks) {
    align_combine<ALIGN_SUMS>(partials, sums, chunks);
}

// ---- msiren_align_solve* (DESIGN.md section 5.11): the damped Gauss-Newton loop around the pipeline above -----------------------------------
// One thread per slice between two evaluations.  State per slice, in the stream's scratch behind the partials:
//     trial, best (6 fp32 each)   the map the next evaluation reads / the best map so far
//     rigid_trial, rigid_best     (c, s, uY, uX) fp64 each (rigid mode)
//     sums_best (29 fp64)         the sums at the best map;  scal = (mean_best, mean_first, lam);  cnt = (accepted, flags)
// The rule is DESIGN.md section 5.11's, restated by mri_inr_amd/align.py: lm_step -- fp64 + - * / one at a time (contraction off), every sum
// in the order written there, so the two give the same bits.  Every loop below has constant bounds and is unrolled: the matrices live in
// registers, nothing is indexed at run time.  Plain stores, no atomics: a slice's trajectory depends on that slice only.
constexpr int ALIGN_SINGULAR = 1, ALIGN_NO_OVERLAP = 2;

struct AlignSolveParams {
    const double* sums;                  // (n, 29) of the evaluation at `trial`
    float *trial, *best;                 // (n, 6)
    double *rigid_trial, *rigid_best;    // (n, 4)
    double* sums_best;                   // (n, 29)
    double* scal;                        // (n, 3)
    int* cnt;                            // (n, 2)
    double* trace;                       // (iterations, n, 8) or null
    float* maps_out;                     // (n, 6)      written behind the last evaluation
    double* rigid_out;                   // (n, 4) or null
    double* report;                      // (n, 6)
    int n, mode, k, last;                // mode 0 affine, 1 rigid; k: the evaluation just done; last: k == iterations - 1
    double down, up, lam_min, lam_max, cy, cx;
};

// rigid_maps' formula (mri_inr_amd/align.py) for one state: fp64, rounded once per entry
__device__ __forceinline__ void align_rigid_map(double c, double s, double uY, double uX, double cy, double cx, float* m) {
#pragma clang fp contract(off)
    const double ccy = c * cy, scx = s * cx, scy = s * cy, ccx = c * cx;
    const double ry = ccy - scx, rx = scy + ccx;
    const double ty = (cy - ry) + uY, tx = (cx - rx) + uX;
    m[0] = (float)c, m[1] = (float)(-s), m[2] = (float)ty, m[3] = (float)s, m[4] = (float)c, m[5] = (float)tx;
}

// A = L D L^T without pivoting, in place: the lower triangle and the diagonal of A are read, L is left over the strict lower triangle and D
// over the diagonal; then the three substitutions.  A pivot that is not positive and finite: x = 0, false.  x may not alias b.
template <int M>
__device__ __forceinline__ bool align_ldl_solve(double (&A)[M][M], const double (&b)[M], double (&x)[M]) {
#pragma clang fp contract(off)
    bool ok = true;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double dj = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) {
            const double ll = A[j][k] * A[j][k];
            dj = dj - ll * A[k][k];
        }
        ok = ok && dj > 0.0 && dj < __builtin_inf();  // (false for a NaN)
        A[j][j] = dj;
#pragma unroll
        for (int i = j + 1; i < M; ++i) {
            double v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) {
                const double ll = A[i][k] * A[j][k];
                v = v - ll * A[k][k];
            }
            A[i][j] = v / dj;
        }
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
        x[i] = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) x[i] = x[i] - A[i][k] * x[k];
    }
#pragma unroll
    for (int i = 0; i < M; ++i) x[i] = x[i] / A[i][i];
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
#pragma unroll
        for (int k = i + 1; k < M; ++k) x[i] = x[i] - A[k][i] * x[k];
    }
#pragma unroll
    for (int i = 0; i < M; ++i) x[i] = ok ? x[i] : 0.0;
    return ok;
}

// The proposals of the step kernels over the leading P of the N parameters of (gradient gr, matrix H): N = 6, or 8 with the (gain, bias) pair
// of align_w.hip.h behind the map's six.
// the affine proposal: d = ldl_solve(H damped, -gr / 2), zero behind the leading P
template <int P, int N>
__device__ __forceinline__ bool align_propose_affine(const double (&H)[N][N], const double (&gr)[N], double lam, double (&d)[N]) {
#pragma clang fp contract(off)
    double A[P][P], rhs[P], x[P];
#pragma unroll
    for (int a = 0; a < P; ++a) {
#pragma unroll
        for (int b = 0; b < P; ++b) A[a][b] = H[a][b];
        const double lh = lam * H[a][a];
        A[a][a] = H[a][a] + lh;
        rhs[a] = -0.5 * gr[a];
    }
    const bool ok = align_ldl_solve<P>(A, rhs, x);
#pragma unroll
    for (int a = 0; a < N; ++a) d[a] = 0.0;
#pragma unroll
    for (int a = 0; a < P; ++a) d[a] = x[a];
    return ok;
}

// the rigid proposal: B (P x Q) = section 5.11's 6 x 3 block [then B[6][3] = B[7][4] = 1], Q = P - 3; g_Q = B^T gr, H_Q = B^T (H B), every sum
// ascending from 0.0, zero entries included; d = ldl_solve(H_Q damped, -g_Q / 2) = (angle, uY, uX[, g, b])
template <int P, int N>
__device__ __forceinline__ bool align_propose_rigid(const double (&H)[N][N], const double (&gr)[N], double lam, double c, double sn, double cy, double cx,
                                                    double (&d)[N - 3]) {
#pragma clang fp contract(off)
    constexpr int Q = P - 3;
    double B[P][Q];
#pragma unroll
    for (int a = 0; a < P; ++a)
#pragma unroll
        for (int q = 0; q < Q; ++q) B[a][q] = 0.0;
    {
        const double scy = sn * cy, ccx = c * cx, ccy = c * cy, scx = sn * cx;
        B[0][0] = -sn, B[1][0] = -c, B[2][0] = scy + ccx;
        B[3][0] = c, B[4][0] = -sn, B[5][0] = -(ccy - scx);
        B[2][1] = 1.0, B[5][2] = 1.0;
        if (P == 8) B[P - 2][Q - 2] = 1.0, B[P - 1][Q - 1] = 1.0;
    }
    double gq[Q], T[P][Q], A[Q][Q], rhs[Q], x[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < P; ++a) {
            const double bg = B[a][q] * gr[a];
            t = t + bg;
        }
        gq[q] = t;
    }
#pragma unroll
    for (int a = 0; a < P; ++a)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < P; ++b) {
                const double hb = H[a][b] * B[b][q];
                t = t + hb;
            }
            T[a][q] = t;
        }
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int r = 0; r < Q; ++r) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < P; ++a) {
                const double bt = B[a][q] * T[a][r];
                t = t + bt;
            }
            A[q][r] = t;
        }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const double lh = lam * A[q][q];
        A[q][q] = A[q][q] + lh;
        rhs[q] = -0.5 * gq[q];
    }
    const bool ok = align_ldl_solve<Q>(A, rhs, x);
#pragma unroll
    for (int q = 0; q < N - 3; ++q) d[q] = 0.0;
#pragma unroll
    for (int q = 0; q < Q; ++q) d[q] = x[q];
    return ok;
}

// DESIGN.md section 5.11's accept / reject / damping rule behind evaluation k, the device twin of mri_inr_amd/align.py: lm_decide, for all
// three step kernels.  The first evaluation is accepted and sets mean_first; a lower mean is accepted, counted, and lowers lam; everything
// else (a NaN included) is rejected and raises it.  An accepted mean becomes mean_best.
__device__ __forceinline__ bool align_lm_decide(int k, double mean, double* mean_best, double* mean_first, double* lam, int* accepted, double down, double up,
                                                double lam_min, double lam_max) {
#pragma clang fp contract(off)
    bool accept;
    if (k == 0) {
        accept = true;
        *mean_first = mean;
    } else if (mean < *mean_best) {  // (false for a NaN)
        accept = true;
        *accepted += 1;
        const double x = *lam * down;
        *lam = x > lam_min ? x : lam_min;
    } else {
        accept = false;
        const double x = *lam * up;
        *lam = x < lam_max ? x : lam_max;
    }
    if (accept) *mean_best = mean;
    return accept;
}

// before the first evaluation: trial := best := the input (rigid: the map of the input state), lam := damping, nothing accepted
__global__ __launch_bounds__(256) void align_solve_init_kernel(AlignSolveParams p, const float* __restrict__ maps_in, const double* __restrict__ rigid_in,
                                                               double damping) {
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
#pragma unroll
    for (int a = 0; a < 6; ++a) p.trial[(size_t)s * 6 + a] = m[a], p.best[(size_t)s * 6 + a] = m[a];
#pragma unroll
    for (int a = 0; a < 4; ++a) p.rigid_trial[(size_t)s * 4 + a] = r[a], p.rigid_best[(size_t)s * 4 + a] = r[a];
#pragma unroll
    for (int a = 0; a < ALIGN_SUMS; ++a) p.sums_best[(size_t)s * ALIGN_SUMS + a] = 0.0;
    p.scal[(size_t)s * 3] = __builtin_inf(), p.scal[(size_t)s * 3 + 1] = __builtin_inf(), p.scal[(size_t)s * 3 + 2] = damping;
    p.cnt[(size_t)s * 2] = 0, p.cnt[(size_t)s * 2 + 1] = 0;
}

// behind evaluation k: accept or reject the trial, then propose the next one from the best map.  grid: ceil(n / 256) workgroups of 256
__global__ __launch_bounds__(256) void align_step_kernel(AlignSolveParams p) {
#pragma clang fp contract(off)
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= p.n) return;
    const double inf = __builtin_inf();
    float trial[6], best[6];
    double rt[4], rb[4], bs[ALIGN_SUMS];
#pragma unroll
    for (int a = 0; a < 6; ++a) trial[a] = p.trial[(size_t)s * 6 + a], best[a] = p.best[(size_t)s * 6 + a];
#pragma unroll
    for (int a = 0; a < 4; ++a) rt[a] = p.rigid_trial[(size_t)s * 4 + a], rb[a] = p.rigid_best[(size_t)s * 4 + a];
    double mean_best = p.scal[(size_t)s * 3], mean_first = p.scal[(size_t)s * 3 + 1], lam = p.scal[(size_t)s * 3 + 2];
    int accepted = p.cnt[(size_t)s * 2];
    const double* ev = p.sums + (size_t)s * ALIGN_SUMS;
    const double count = ev[0], cost = ev[1];
    if (p.trace) {
        double* tr = p.trace + ((size_t)p.k * p.n + s) * 8;
#pragma unroll
        for (int a = 0; a < 6; ++a) tr[a] = (double)trial[a];
        tr[6] = cost, tr[7] = count;
    }
    const double mean = count >= 6.0 ? cost / count : inf;
    const bool accept = align_lm_decide(p.k, mean, &mean_best, &mean_first, &lam, &accepted, p.down, p.up, p.lam_min, p.lam_max);
#pragma unroll
    for (int a = 0; a < ALIGN_SUMS; ++a) bs[a] = accept ? ev[a] : p.sums_best[(size_t)s * ALIGN_SUMS + a];
    if (accept) {
#pragma unroll
        for (int a = 0; a < 6; ++a) best[a] = trial[a];
#pragma unroll
        for (int a = 0; a < 4; ++a) rb[a] = rt[a];
#pragma unroll
        for (int a = 0; a < ALIGN_SUMS; ++a) p.sums_best[(size_t)s * ALIGN_SUMS + a] = bs[a];
#pragma unroll
        for (int a = 0; a < 6; ++a) p.best[(size_t)s * 6 + a] = best[a];
#pragma unroll
        for (int a = 0; a < 4; ++a) p.rigid_best[(size_t)s * 4 + a] = rb[a];
    }
    double H[6][6];
    {
        int q = 8;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b, ++q) H[a][b] = bs[q], H[b][a] = bs[q];
    }
    double gr[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) gr[a] = bs[2 + a];
    bool ok;
    if (p.mode == 0) {
        double d[6];
        ok = align_propose_affine<6>(H, gr, lam, d);
#pragma unroll
        for (int a = 0; a < 6; ++a) trial[a] = (float)((double)best[a] + d[a]);
    } else {
        const double c = rb[0], sn = rb[1], uY = rb[2], uX = rb[3], cy = p.cy, cx = p.cx;
        double d[3];
        ok = align_propose_rigid<6>(H, gr, lam, c, sn, cy, cx, d);
        const double u = d[0] / 2.0, uu = u * u, den = 1.0 + uu;
        const double cd = (1.0 - uu) / den, sd = (2.0 * u) / den;
        const double ccd = c * cd, ssd = sn * sd, scd = sn * cd, csd = c * sd;
        rt[0] = ccd - ssd, rt[1] = scd + csd, rt[2] = uY + d[1], rt[3] = uX + d[2];
        align_rigid_map(rt[0], rt[1], rt[2], rt[3], cy, cx, trial);
#pragma unroll
        for (int a = 0; a < 4; ++a) p.rigid_trial[(size_t)s * 4 + a] = rt[a];
    }
    const int flags = (ok ? 0 : ALIGN_SINGULAR) | (mean_first == inf ? ALIGN_NO_OVERLAP : 0);
#pragma unroll
    for (int a = 0; a < 6; ++a) p.trial[(size_t)s * 6 + a] = trial[a];
    p.scal[(size_t)s * 3] = mean_best, p.scal[(size_t)s * 3 + 1] = mean_first, p.scal[(size_t)s * 3 + 2] = lam;
    p.cnt[(size_t)s * 2] = accepted, p.cnt[(size_t)s * 2 + 1] = flags;
    if (p.last) {
#pragma unroll
        for (int a = 0; a < 6; ++a) p.maps_out[(size_t)s * 6 + a] = best[a];
        if (p.rigid_out) {
#pragma unroll
            for (int a = 0; a < 4; ++a) p.rigid_out[(size_t)s * 4 + a] = rb[a];
        }
        double* rp = p.report + (size_t)s * 6;
        rp[0] = (double)accepted, rp[1] = mean_first, rp[2] = mean_best, rp[3] = bs[0], rp[4] = lam, rp[5] = (double)flags;
    }
}

}  // namespace msiren
