// A stack of slices read as a volume at points (Z, Y, X) (msiren_resample_volume*): the steps either side of the
// ragged trunk.  (Y, X), cover rule, slots, local coordinate and weight are resample.hip.h's; Z is in slice units.  A point is VALID iff
// 0 <= Z <= n - 1 (the fp32 Z against the exact integers; false for a NaN) and then reads a PAIR of slices:
//     value forms      z0 = floorf(Z), f = Z - z0 (exact in fp32); f == 0: slice z0 alone (J = 1), else z0 and z0 + 1 (J = 2)
//     gradient forms   z0' = min(z0, n - 2), f' = Z - z0' in [0, 1]; always both slices (n >= 2)
// Bins are (slice, tile): b = s nV nH + t -- the ragged trunk's patches, reps = 1, on the plan's rows.  A point owns up to J K slots,
// slot (m, j, k) at (2 m + j) K + k; tile and weight do not depend on j and are kept once per (m, k).
//
//   bin    resample_volume_count_kernel   covers per bin.  Integer atomics, AGGREGATED PER WAVE: for each slot index the lanes that hold the
//                                         same bin elect a leader (readfirstlane + ballot), which adds their number once
//          resample_scan_kernel           (resample.hip.h) exclusive scan over the n nV nH bins -> the ragged offsets
//          resample_volume_fill_kernel    the same election on the cursors: the leader's add is broadcast, each lane takes base + rank.  Where
//                                         an entry lands inside its bin influences no output bit (resample.hip.h)
//   trunk  the ragged trunks over T = 2 M K entries at most
//   blend  resample_volume_blend_kernel   one thread per point: per slice of the pair resample_blend_kernel's num / den, then
//              value    = R0 if f == 0, R1 if f == 1, else fmaf(f, R1, (1.0f - f) R0)
//              grad[0]  = R1 - R0 (per slice of Z), grad[1], grad[2] = the same selection over the in-plane gradient planes
//          NaN in every plane for an invalid Z, written explicitly; no cover: 0 / 0 = NaN as in resample_blend_kernel
#pragma once
#include <hip/hip_runtime.h>

#include "resample.hip.h"

namespace msiren {

struct ResampleVolumeParams {
    const float* points;  // (M, 3) = (Z, Y, X)
    int M, n, nV, nH, S, I, pad, KA;
    int both;             // gradient forms: always two slices, the pair clamped to n - 2
    int* counts;          // (NP) covers per bin, NP = n nV nH; zero before the count kernel
    int* cursors;         // (NP) zero before the fill kernel
    int* offsets;         // (NP + 1)
    float* coords;        // (2 M K, 2) entries: local coordinates, bin by bin
    int* ent;             // (2 M K) slot (m, j, k) -> entry, -1: none
    int* tile;            // (M K) slot (m, k) -> tile of the slice
    float* w;             // (M K) slot (m, k) -> fold weight
    int* pair;            // (M) first slice of the point's pair, -1: invalid Z
    float* f;             // (M) weight of the second slice
};

// the point's pair: returns the number of slices it reads (0: invalid Z), *z0 the first one, *f the second one's weight
__device__ __forceinline__ int volume_pair(float Z, int n, int both, int* z0, float* f) {
    *z0 = -1, *f = 0.f;
    if (!(0.f <= Z && Z <= (float)(n - 1))) return 0;  // (n < 2^24: exact; false for a NaN)
    const float fl = floorf(Z);
    int z = (int)fl;
    if (both && z > n - 2) z = n - 2;
    *z0 = z;
    *f = Z - (float)z;  // exact: the fractional part of an fp32 number, or 1
    return (both || *f != 0.f) ? 2 : 1;
}

// One slot index of the wave: the lanes with `pending` hold bin b and need `1` added to ctr[b].  Lanes of the same bin elect the lowest one,
// which issues one add of their number; returns the lane's place base + rank among the adds to its bin (the count kernel ignores it).
// Wave-uniform control flow: call with every lane of the wave.  Each round retires the first pending lane at least, so 64 rounds end it.
__device__ __forceinline__ int wave_bin_add(int* __restrict__ ctr, int b, bool pending) {
    int place = 0;
    const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1ull;
    for (int round = 0; round < 64 && __ballot(pending) != 0ull; ++round) {
        if (pending) {
            const int lb = __builtin_amdgcn_readfirstlane(b);
            const bool mine = b == lb;
            const unsigned long long same = __ballot(mine);  // (the pending lanes of bin lb)
            if (mine) {
                const int rank = __popcll(same & below);
                int base = 0;
                if (rank == 0) base = atomicAdd(&ctr[lb], (int)__popcll(same));
                place = __builtin_amdgcn_readfirstlane(base) + rank;  // (the first lane of `same` is the leader)
                pending = false;
            }
        }
    }
    return place;
}

__global__ __launch_bounds__(256) void resample_volume_count_kernel(ResampleVolumeParams p) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    const bool in = m < p.M;
    int z0 = -1, v0 = 0, h0 = 0, nv = 0, nh = 0, J = 0;
    float f;
    if (in) {
        J = volume_pair(p.points[3 * (size_t)m], p.n, p.both, &z0, &f);
        nv = cover_axis(p.points[3 * (size_t)m + 1], p.nV, p.S, p.I, p.pad, &v0), nh = cover_axis(p.points[3 * (size_t)m + 2], p.nH, p.S, p.I, p.pad, &h0);
    }
    const int NPt = p.nV * p.nH;
    for (int j = 0; j < 2; ++j)
        for (int a = 0; a < p.KA; ++a)
            for (int b = 0; b < p.KA; ++b) {
                const bool has = j < J && a < nv && b < nh;
                (void)wave_bin_add(p.counts, has ? (z0 + j) * NPt + (v0 + a) * p.nH + h0 + b : 0, has);
            }
}

// The fill kernels' fp64 expressions, shared with align_volume_fill_kernel (align_volume.hip.h): a point's offset inside a tile along one axis,
// its local coordinate there and its fold weight -- fp64 from the fp32 coordinate, rounded once
__device__ __forceinline__ double volume_tile_offset(float Y, int v, int I, int pad) { return (double)Y - (double)(v * I - pad); }
__device__ __forceinline__ float volume_local_coord(double t, double den) { return (float)(-1.0 + t * 2.0 / den); }
__device__ __forceinline__ float volume_fold_weight(double ty, double tx, double c) { return (float)exp(-0.1 * sqrt((ty - c) * (ty - c) + (tx - c) * (tx - c))); }

__global__ __launch_bounds__(256) void resample_volume_fill_kernel(ResampleVolumeParams p) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    const bool in = m < p.M;
    const int K = p.KA * p.KA;
    int z0 = -1, v0 = 0, h0 = 0, nv = 0, nh = 0, J = 0;
    float f = 0.f, Y = 0.f, X = 0.f;
    if (in) {
        J = volume_pair(p.points[3 * (size_t)m], p.n, p.both, &z0, &f);
        Y = p.points[3 * (size_t)m + 1], X = p.points[3 * (size_t)m + 2];
        nv = cover_axis(Y, p.nV, p.S, p.I, p.pad, &v0), nh = cover_axis(X, p.nH, p.S, p.I, p.pad, &h0);
        p.pair[m] = z0;
        p.f[m] = f;
    }
    const int NPt = p.nV * p.nH;
    const double c = 0.5 * (double)(p.S - 1), den = (double)(p.S - 1);
    for (int j = 0; j < 2; ++j)
        for (int a = 0; a < p.KA; ++a)
            for (int b = 0; b < p.KA; ++b) {
                const bool has = j < J && a < nv && b < nh;
                const int t = (v0 + a) * p.nH + h0 + b, bin = has ? (z0 + j) * NPt + t : 0;
                const int place = wave_bin_add(p.cursors, bin, has);
                if (has) {  // (m < M)
                    const int k = a * nh + b;  // the point's covering tiles in (v, h) row-major order
                    const double ty = volume_tile_offset(Y, v0 + a, p.I, p.pad), tx = volume_tile_offset(X, h0 + b, p.I, p.pad);
                    const int e = p.offsets[bin] + place;
                    reinterpret_cast<float2*>(p.coords)[e] = make_float2(volume_local_coord(ty, den), volume_local_coord(tx, den));
                    p.ent[((size_t)2 * m + j) * K + k] = e;
                    if (j == 0) {
                        p.tile[(size_t)m * K + k] = t;
                        p.w[(size_t)m * K + k] = volume_fold_weight(ty, tx, c);
                    }
                }
            }
    if (in) {
        const int used = nv * nh;
        for (int j = 0; j < 2; ++j)
            for (int k = j < J ? used : 0; k < K; ++k) p.ent[((size_t)2 * m + j) * K + k] = -1;
    }
}

// resample_blend_kernel's sum for slice j of point m's pair: slots in order, fp32 num / den, a black bin 0 with its weight
__device__ __forceinline__ float volume_slice_blend(const float* __restrict__ v, const int* __restrict__ ent, const int* __restrict__ tile, const float* __restrict__ w,
                                                    const int* __restrict__ black, int K) {
    float num = 0.f, den = 0.f;
    for (int k = 0; k < K; ++k) {
        const int e = ent[k];
        if (e < 0) break;
        const float ww = w[k];
        den += ww;
        if (black[tile[k]] == 0) num = __builtin_fmaf(ww, v[e], num);
    }
    return num / den;
}

// vals (planes, T): the ragged trunk's outputs by entry, plane 0 the value, 1 / 2 the in-plane gradient.  black (n NPt).  out (M) may be
// null; grad (3, M) may be null (then planes = 1).
__global__ __launch_bounds__(256) void resample_volume_blend_kernel(const float* __restrict__ vals, const int* __restrict__ ent, const int* __restrict__ tile,
                                                                    const float* __restrict__ w, const int* __restrict__ black, const int* __restrict__ pair,
                                                                    const float* __restrict__ fz, float* __restrict__ out, float* __restrict__ grad, int M, int K,
                                                                    int NPt, int T, int planes, int both) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int z0 = pair[m];
    if (z0 < 0) {  // invalid Z
        const float qnan = __builtin_nanf("");
        if (out) out[m] = qnan;
        if (grad)
            for (int pl = 0; pl < 3; ++pl) grad[(size_t)pl * M + m] = qnan;
        return;
    }
    const float f = fz[m], a0 = 1.0f - f;
    const bool two = both || f != 0.f;
    const int* e0 = ent + (size_t)2 * m * K;
    const int* tl = tile + (size_t)m * K;
    const float* ww = w + (size_t)m * K;
    for (int pl = 0; pl < planes; ++pl) {
        const float* v = vals + (size_t)pl * T;
        const float R0 = volume_slice_blend(v, e0, tl, ww, black + (size_t)z0 * NPt, K);
        const float R1 = two ? volume_slice_blend(v, e0 + K, tl, ww, black + (size_t)(z0 + 1) * NPt, K) : 0.f;
        const float sel = f == 0.f ? R0 : f == 1.f ? R1 : __builtin_fmaf(f, R1, a0 * R0);
        if (pl == 0) {
            if (out) out[m] = sel;
            if (grad) grad[m] = R1 - R0;
        } else {
            grad[(size_t)pl * M + m] = sel;
        }
    }
}

}  // namespace msiren
