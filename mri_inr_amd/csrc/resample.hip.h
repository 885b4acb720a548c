// A slice's reconstruction at arbitrary points (msiren_resample_slices*): the steps either side of the ragged
// trunk.  points[m] = (Y, X) in reconstruction pixel coordinates; with pad = (S - I) / 2 tile (v, h) COVERS the point iff
//     v I - pad <= Y <= v I - pad + S - 1     and     h I - pad <= X <= h I - pad + S - 1
// (closed at both ends; the fp32 coordinate is compared with the exactly representable integers, no arithmetic on it, so that every
// implementation classifies every point identically).  At most KA = ceil(S / I) tiles cover a point per axis, K = KA^2 in all: the
// point's SLOTS m K + k, k counting its covering tiles in (v, h) row-major order.
//
//   bin    resample_count_kernel   covers per tile (integer atomics)
//          resample_scan_kernel    exclusive scan over the nV nH tiles -> the ragged offsets
//          resample_fill_kernel    per cover: an entry of its tile's set (cursor: integer atomic) = the local coordinate, and per slot the
//                                  entry's index, the tile and the fold weight.  Where an entry lands inside its tile's set is decided by
//                                  the atomics and influences no output bit: the trunk evaluates a coordinate the same wherever it stands,
//                                  and every entry is read back through its own slot.
//   trunk  siren_trunk_f32_ragged_kernel / siren_trunk_f32_jet_ragged_kernel, replicated over the slices
//   blend  resample_blend_kernel   one thread per (slice, point): slots in order, fp32 num / den; a black tile contributes 0 with its
//                                  weight; no cover (outside, or a non-finite point): 0 / 0 = NaN
// Local coordinate and weight are formed in fp64 and rounded once:  ty = Y - (v I - pad),  x = -1 + ty 2 / (S - 1),
// w = exp(-0.1 sqrt((ty - c)^2 + (tx - c)^2)),  c = (S - 1) / 2  (the fold's weight function, tiling.py:67-88, without its constant
// normalisation, which cancels in num / den).
#pragma once
#include <hip/hip_runtime.h>

namespace msiren {

constexpr int RESAMPLE_MAX_KA = 4;  // covering tiles per axis: ceil(S / I) <= 4

struct ResampleParams {
    const float* points;  // (M, 2)
    int M, nV, nH, S, I, pad, KA;
    int* counts;          // (NP) covers per tile; zero before the count kernel
    int* cursors;         // (NP) zero before the fill kernel
    int* offsets;         // (NP + 1)
    float* coords;        // (M K, 2) entries: local coordinates, tile by tile
    int* ent;             // (M K) slot -> entry, -1: no cover
    int* tile;            // (M K) slot -> tile
    float* w;             // (M K) slot -> fold weight
};

// the tiles of one axis that cover coordinate y: first one and their number (they are consecutive)
__device__ __forceinline__ int cover_axis(float y, int n, int S, int I, int pad, int* first) {
    int cnt = 0;
    *first = 0;
    for (int v = 0; v < n; ++v) {
        const float lo = (float)(v * I - pad), hi = (float)(v * I - pad + S - 1);  // integers far below 2^24: exact
        if (lo <= y && y <= hi) {  // (false for a NaN)
            if (cnt == 0) *first = v;
            ++cnt;
        }
    }
    return cnt;
}

__global__ __launch_bounds__(256) void resample_count_kernel(ResampleParams p) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= p.M) return;
    int v0, h0;
    const int nv = cover_axis(p.points[2 * m], p.nV, p.S, p.I, p.pad, &v0), nh = cover_axis(p.points[2 * m + 1], p.nH, p.S, p.I, p.pad, &h0);
    for (int a = 0; a < nv; ++a)
        for (int b = 0; b < nh; ++b) atomicAdd(&p.counts[(v0 + a) * p.nH + h0 + b], 1);
}

// offsets[t] = covers of the tiles before t; one workgroup (the scan of compact_flags_block)
__global__ __launch_bounds__(256) void resample_scan_kernel(const int* __restrict__ counts, int NP, int* __restrict__ offsets) {
    __shared__ int wsum[4];
    __shared__ int carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < NP; base += 256) {
        const int t = base + tid;
        const int c = t < NP ? counts[t] : 0;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (t < NP) offsets[t] = before + incl - c;
        __syncthreads();
        if (tid == 255) carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) offsets[NP] = carry;
}

__global__ __launch_bounds__(256) void resample_fill_kernel(ResampleParams p) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= p.M) return;
    const int K = p.KA * p.KA;
    const float Y = p.points[2 * m], X = p.points[2 * m + 1];
    int v0, h0;
    const int nv = cover_axis(Y, p.nV, p.S, p.I, p.pad, &v0), nh = cover_axis(X, p.nH, p.S, p.I, p.pad, &h0);
    const double c = 0.5 * (double)(p.S - 1), den = (double)(p.S - 1);
    int k = 0;
    for (int a = 0; a < nv; ++a)
        for (int b = 0; b < nh; ++b, ++k) {
            const int t = (v0 + a) * p.nH + h0 + b;
            const double ty = (double)Y - (double)((v0 + a) * p.I - p.pad), tx = (double)X - (double)((h0 + b) * p.I - p.pad);
            const int e = p.offsets[t] + atomicAdd(&p.cursors[t], 1);
            reinterpret_cast<float2*>(p.coords)[e] = make_float2((float)(-1.0 + ty * 2.0 / den), (float)(-1.0 + tx * 2.0 / den));
            const int slot = m * K + k;
            p.ent[slot] = e;
            p.tile[slot] = t;
            p.w[slot] = (float)exp(-0.1 * sqrt((ty - c) * (ty - c) + (tx - c) * (tx - c)));
        }
    for (; k < K; ++k) p.ent[m * K + k] = -1;
}

// out[s, m] = sum_k w_k val_k / sum_k w_k over the point's slots in order, and the same per gradient plane.  vals (planes, n, T): the
// ragged trunk's outputs, entry e of slice s at s T + e.  black (n NP): a black tile's entry was never evaluated and counts as 0.
__global__ __launch_bounds__(256) void resample_blend_kernel(const float* __restrict__ vals, const int* __restrict__ ent, const int* __restrict__ tile,
                                                             const float* __restrict__ w, const int* __restrict__ black, float* __restrict__ out,
                                                             int n, int M, int K, int NP, int T, int planes) {
    const int i = blockIdx.x * 256 + threadIdx.x;  // (n M < 2^31: checked by the host)
    if (i >= n * M) return;
    const int s = i / M, m = i - s * M;
    for (int pl = 0; pl < planes; ++pl) {
        const float* v = vals + ((size_t)pl * n + s) * T;
        float num = 0.f, den = 0.f;
        for (int k = 0; k < K; ++k) {
            const int e = ent[m * K + k];
            if (e < 0) break;
            const float ww = w[m * K + k];
            den += ww;
            if (black[s * NP + tile[m * K + k]] == 0) num = __builtin_fmaf(ww, v[e], num);
        }
        out[(size_t)pl * n * M + i] = num / den;
    }
}

}  // namespace msiren
