// Kernels of msiren_residual_scale(_dev): per segment of targets an exact order statistic of the residuals, as a robust scale
// per target, with nothing read back.  The rule is include/msiren.h's, restated in numpy by mri_inr_amd/residual_scale.py (residual_scale_on_host): the
// two agree bit for bit.  The layout of the scratch, the chunking and the launch count: residual_scale_plan.h.
// An MSD radix select over 32-bit keys, 8 bits per pass.  A pass is one histogram of the current digit over the keys whose higher digits equal the
// segment's prefix, one workgroup per chunk of 4096 pixels of one target, and behind it one small workgroup per segment that adds the chunks'
// histograms, scans the 256 bins, finds the bin that holds the rank and narrows prefix and rank.
//   upload   rscale_upload_kernel   up to 512 offsets of group_start, carried by value in the kernel's arguments -> the scratch (no host sync)
//   keys     rscale_keys_kernel     e per pixel in fp64 -> its key (centre = 1: the total order of the bits; centre = 0: the bits of |e|), 0xFFFFFFFF
//                                   where the pixel does not count, stored once; the first digit's histogram on the way
//   hist     rscale_hist_kernel     the histogram of digit 1, 2 or 3 under the segment's prefix
//   choose   rscale_choose_kernel   per segment: bins summed over the chunks' rows, four rows at a time, scanned; [count and k from the first pass]; prefix, rank
//   rekey    rscale_rekey_kernel    centre = 1, between the two selections: key -> e, d = fabsf(e - c), the bits of d as the new key, in place; the first
//                                   digit's histogram on the way
//   finish   rscale_finish_kernel   one thread per target: s = (tune d)^2 or floor -> scale[q]; the first target of a segment writes stats
// Atomics: integer adds on LDS only (ds_add_u32), into a histogram private to each wave; the four are added after a barrier and STORED to the chunk's
// row of the partials, so no word of global memory is ever added to and nothing has to be zeroed.  Counts are integers: they do not depend on the
// order in which the adds arrive, so every result is the same bits run to run.  No count can overflow: all of them are at most m th tw < 2^28.
// Residuals cluster in two or three exponents, so in the first pass most lanes of a wave hold the same digit.  The add therefore peels up to two
// digits off the wave first -- the digit of the first lane that still has one, a ballot of the lanes that share it, one add of the population count
// by that lane -- and only what is left goes to the LDS as one add per lane.
#pragma once
#include <hip/hip_runtime.h>

#include "residual_scale_plan.h"

namespace msiren {

struct RscaleOffsets { int v[kRscaleOffsets]; };

// dst[base + i] = s.v[i] for i < count: group_start reaches the device in kernel arguments.  grid: 512 / 256 workgroups of 256.
__global__ __launch_bounds__(256) void rscale_upload_kernel(RscaleOffsets s, int* __restrict__ dst, int base, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) dst[base + i] = s.v[i];
}

// the segment of target q and its targets lo .. hi - 1: the last g with group_start[g] <= q; without groups the target itself.  The same in every lane.
__device__ __forceinline__ int rscale_segment(const int* __restrict__ group_start, int G, int q, int* first, int* last) {
    if (!group_start) return *first = q, *last = q + 1, q;
    int lo = 0, hi = G;  // group_start[lo] <= q < group_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (group_start[mid] <= q) lo = mid;
        else hi = mid;
    }
    return *first = group_start[lo], *last = group_start[lo + 1], lo;
}

// one digit per lane that has one (`has`) into the wave's histogram `hw`; every lane of the wave calls it
__device__ __forceinline__ void rscale_wave_add(unsigned* hw, bool has, unsigned digit) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        const unsigned long long todo = __ballot(has);
        if (!todo) return;  // (the same in every lane)
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned d0 = (unsigned)__shfl((int)digit, leader);
        const bool mine = has && digit == d0;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(&hw[d0], (unsigned)__popcll(same));
        has = has && !mine;
    }
    if (has) atomicAdd(&hw[digit], 1u);
}

// the histogram's frame shared by the three kernels that count: zero the four wave histograms, key(i) -> (counts, digit) for the pixels i of the chunk,
// add, store the sum of the four to the chunk's row.  The trip count is the chunk's: the same in every lane.
template <class Key>
__device__ __forceinline__ void rscale_count_chunk(int len, unsigned* __restrict__ row, Key key) {
    __shared__ unsigned h[4][kRscaleBins];
    const int tid = threadIdx.x;
#pragma unroll
    for (int w = 0; w < 4; ++w) h[w][tid] = 0u;
    __syncthreads();
    unsigned* const hw = h[tid >> 6];
    for (int i0 = 0; i0 < len; i0 += 256) {
        const int i = i0 + tid;
        unsigned digit = 0u;
        const bool has = i < len && key(i, &digit);
        rscale_wave_add(hw, has, digit);
    }
    __syncthreads();
    row[tid] = (h[0][tid] + h[1][tid]) + (h[2][tid] + h[3][tid]);
}

// grid: m chunks_per_target workgroups of 256; workgroup (q, ch) owns pixels ch 4096 .. of target q
__global__ __launch_bounds__(256) void rscale_keys_kernel(const float* __restrict__ targets, const float* __restrict__ simulated, const float* __restrict__ weights,
                                                          const float* __restrict__ intensity, int pixels, int chunks, int centre, unsigned* __restrict__ keys,
                                                          unsigned* __restrict__ partials) {
#pragma clang fp contract(off)
    const int q = blockIdx.x / chunks, ch = blockIdx.x - q * chunks;
    const int start = ch * kRscaleChunk, len = min(kRscaleChunk, pixels - start);
    const size_t base = (size_t)q * pixels + start;
    const double g = intensity ? (double)intensity[2 * (size_t)q] : 1.0, b = intensity ? (double)intensity[2 * (size_t)q + 1] : 0.0;
    rscale_count_chunk(len, partials + (size_t)blockIdx.x * kRscaleBins, [&](int i, unsigned* digit) {
        const size_t at = base + i;
        const float T = targets[at];
        float e = T;
        if (simulated) {
            const double S = (double)simulated[at];
            e = intensity ? (float)((double)T - ((g * S) + b)) : (float)((double)T - S);
        }
        const float w = weights ? weights[at] : 1.f;
        const bool counts = __builtin_isfinite(e) && __builtin_isfinite(w) && w > 0.f;
        const unsigned bits = __float_as_uint(e);
        const unsigned k = !counts ? kRscaleNoKey : centre ? (bits & 0x80000000u ? ~bits : bits ^ 0x80000000u) : bits & 0x7FFFFFFFu;
        keys[at] = k;
        *digit = k >> 24;
        return counts;
    });
}

// grid as above.  shift = 24 - 8 pass, pass = 1, 2, 3: the digit is (key >> shift) & 255 and the prefix the bits above it
__global__ __launch_bounds__(256) void rscale_hist_kernel(const unsigned* __restrict__ keys, const int* __restrict__ group_start, int G, const unsigned* __restrict__ state,
                                                          int pixels, int chunks, int shift, unsigned* __restrict__ partials) {
    const int q = blockIdx.x / chunks, ch = blockIdx.x - q * chunks;
    const int start = ch * kRscaleChunk, len = min(kRscaleChunk, pixels - start);
    const size_t base = (size_t)q * pixels + start;
    int first, last;
    const int seg = rscale_segment(group_start, G, q, &first, &last);
    const unsigned prefix = state[(size_t)seg * kRscaleState + RSCALE_PREFIX];
    rscale_count_chunk(len, partials + (size_t)blockIdx.x * kRscaleBins, [&](int i, unsigned* digit) {
        const unsigned k = keys[base + i];
        *digit = (k >> shift) & 255u;
        return k != kRscaleNoKey && (k >> (shift + 8)) == prefix;
    });
}

// grid as above, centre = 1 behind the first selection: the segment's prefix is the key of c
__global__ __launch_bounds__(256) void rscale_rekey_kernel(unsigned* __restrict__ keys, const int* __restrict__ group_start, int G, const unsigned* __restrict__ state,
                                                           int pixels, int chunks, unsigned* __restrict__ partials) {
    const int q = blockIdx.x / chunks, ch = blockIdx.x - q * chunks;
    const int start = ch * kRscaleChunk, len = min(kRscaleChunk, pixels - start);
    const size_t base = (size_t)q * pixels + start;
    int first, last;
    const int seg = rscale_segment(group_start, G, q, &first, &last);
    const unsigned ck = state[(size_t)seg * kRscaleState + RSCALE_PREFIX];
    const float c = __uint_as_float(ck & 0x80000000u ? ck ^ 0x80000000u : ~ck);  // (a segment without a pixel that counts has no key to turn)
    rscale_count_chunk(len, partials + (size_t)blockIdx.x * kRscaleBins, [&](int i, unsigned* digit) {
        const unsigned k = keys[base + i];
        if (k == kRscaleNoKey) return false;
        const float e = __uint_as_float(k & 0x80000000u ? k ^ 0x80000000u : ~k);
        const unsigned d = __float_as_uint(fabsf(e - c));  // not negative, at most +inf: orders as its bits, never 0xFFFFFFFF
        keys[base + i] = d;
        *digit = d >> 24;
        return true;
    });
}

// grid: one workgroup of 256 per segment.  The chunks' rows are added four at a time: wave w takes the rows w, w + 4, ... of the segment, lane l the bins
// 4 l .. 4 l + 3 of a row in one 16-byte load; the four waves' sums meet in LDS, and from there thread b owns bin b.  (Integer sums: the order does not
// show.)  begin: the pass is a selection's first -- count = the sum of all bins, k from the quantile, the prefix starts empty; with keep_centre the
// prefix the first selection left (the key of c) is put aside first.
__global__ __launch_bounds__(256) void rscale_choose_kernel(const unsigned* __restrict__ partials, const int* __restrict__ group_start, int G, int chunks, int begin,
                                                            int keep_centre, double quantile, unsigned* __restrict__ state) {
#pragma clang fp contract(off)
    __shared__ unsigned scan[kRscaleBins];
    __shared__ uint4 rows[4][kRscaleBins / 4];
    const int seg = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int first = group_start ? group_start[seg] : seg, last = group_start ? group_start[seg + 1] : seg + 1;
    unsigned* const st = state + (size_t)seg * kRscaleState;
    const unsigned old_prefix = st[RSCALE_PREFIX], old_rank = st[RSCALE_RANK];  // (read by every thread before any thread writes: the barriers below)
    uint4 acc = make_uint4(0u, 0u, 0u, 0u);
    const uint4* const row4 = (const uint4*)partials;  // (the partials start on a 16-byte boundary: rscale_layout)
#pragma unroll 4
    for (size_t r = (size_t)first * chunks + wave; r < (size_t)last * chunks; r += 4) {
        const uint4 v = row4[r * (kRscaleBins / 4) + lane];
        acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
    }
    rows[wave][lane] = acc;
    __syncthreads();
    const unsigned* const flat = (const unsigned*)rows;
    const unsigned mine = (flat[tid] + flat[kRscaleBins + tid]) + (flat[2 * kRscaleBins + tid] + flat[3 * kRscaleBins + tid]);
    scan[tid] = mine;
    __syncthreads();
    for (int step = 1; step < kRscaleBins; step <<= 1) {  // inclusive scan over the bins
        const unsigned below = tid >= step ? scan[tid - step] : 0u;
        __syncthreads();
        scan[tid] += below;
        __syncthreads();
    }
    const unsigned upto = scan[tid], before = upto - mine, count = scan[kRscaleBins - 1];
    unsigned rank = old_rank, prefix = old_prefix;
    if (begin) {
        rank = count ? (unsigned)(long long)floor(quantile * (double)((long long)count - 1)) : 0u;
        prefix = 0u;
        if (tid == 0) {
            st[RSCALE_COUNT] = count, st[RSCALE_K] = rank;
            if (keep_centre) st[RSCALE_CENTRE] = old_prefix;
            if (!count) st[RSCALE_PREFIX] = 0u, st[RSCALE_RANK] = 0u;
        }
    }
    if (mine && before <= rank && rank < upto) st[RSCALE_PREFIX] = (prefix << 8) | (unsigned)tid, st[RSCALE_RANK] = rank - before;  // exactly one bin where count > 0
}

// grid: ceil(m / 256) workgroups of 256, one thread per target
__global__ __launch_bounds__(256) void rscale_finish_kernel(const unsigned* __restrict__ state, const int* __restrict__ group_start, int G, int m, int centre, double tune,
                                                            double floor_, double* __restrict__ scale, double* __restrict__ stats) {
#pragma clang fp contract(off)
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    int first, last;
    const int seg = rscale_segment(group_start, G, q, &first, &last);
    const unsigned* const st = state + (size_t)seg * kRscaleState;
    const unsigned count = st[RSCALE_COUNT], ck = st[RSCALE_CENTRE];
    const float c = centre ? __uint_as_float(ck & 0x80000000u ? ck ^ 0x80000000u : ~ck) : 0.f;
    const float d = __uint_as_float(st[RSCALE_PREFIX]);
    double s = __builtin_inf();
    if (count) {
        const double t = tune * (double)d;
        s = t * t;
        s = s > floor_ ? s : floor_;
    }
    scale[q] = s;
    if (stats && q == first) {
        double* const out = stats + 4 * (size_t)seg;
        out[0] = (double)count, out[1] = count ? (double)st[RSCALE_K] : 0.0, out[2] = count ? (double)c : 0.0, out[3] = count ? (double)d : 0.0;
    }
}

}  // namespace msiren
