// The exact-fp32 trunks over one coordinate set PER PATCH ("ragged" sets): msiren_sample_ragged_*, and the
// trunk step of msiren_resample_slices*, where every tile of a slice evaluates the points that fall into its cover.
//
// Patch t owns coords[offsets[t] : offsets[t + 1]].  A work item is (patch, chunk of that patch's set): 64 coordinates for the value
// kernel, 32 for the jet, the chunk sizes and LDS budgets of siren_trunk_f32_kernel / siren_trunk_f32_jet_kernel -- whose layer bodies
// (siren_trunk_f32_body, siren_trunk_f32_jet_body) run here unchanged on an ItemSpan that points into the patch's set.  A coordinate's
// column of the MFMAs never sees its neighbours, so every output is THE BITS the shared-set kernels give for the same coordinate and
// modulation rows (tests/test_gpu_ragged.py: np.array_equal).
//
// The offsets live on the device, so the host does not know the item count: ragged_items_kernel (one workgroup) writes the per-patch
// first-item prefix, the trunk is launched over the upper bound ceil(T / chunk) + NP per replica, a workgroup finds its patch by a
// workgroup-uniform BINARY SEARCH in that prefix (no expanded item table: NP + 1 words instead of one per item, ~log2 NP scalar loads),
// and surplus workgroups leave on the device-side total before any barrier -- as plan[0] is honoured in the shared-set kernels.
//
// Replicas (the slice form): the grid is `reps` copies of the item range, replica s evaluating the same sets with the modulation rows of
// patch s * NP + t; `pos` (the slice pipeline's plan) maps that patch to its row among the kept ones, negative = black: leave.
//
// No atomics, no scratch; every output element is written by exactly one thread.
#pragma once
#include "siren_trunk_f32_jet.hip.h"

namespace msiren {

struct TrunkRaggedParams {
    TrunkParams t;       // t.grid = coords (T, 2); t.mods (L, t.B, mod_stride); t.out (reps, T), may be null in the jet form; P / chunks / plan unused
    const int* offsets;  // (NP + 1), non-decreasing, offsets[0] = 0, offsets[NP] = T
    const int* first;    // (NP + 1): first[t] = items of the patches before t, first[NP] = items per replica (ragged_items_kernel)
    const int* pos;      // optional (reps * NP): modulation row of patch s * NP + t, negative: the patch is not evaluated
    float* grad;         // jet form: (2, reps, T) planar
    float gscale;        // jet form: every gradient is multiplied by it
    int NP, T, reps;     // patches per replica; coordinates; replicas (grid = reps * bound)
    int bound;           // items launched per replica: ceil(T / chunk) + NP >= first[NP]
};

// first[t] = sum over t' < t of ceil(count(t') / CHUNK), t = 0..NP; one workgroup of 256 threads (the scan of compact_flags_block).
// Offsets are clamped into [0, T] and counts to >= 0, as ragged_span reads them: malformed device offsets cannot index outside the
// call's buffers.
__device__ __forceinline__ int ragged_count(const int* __restrict__ offsets, int t, int T) {
    const int o0 = min(max(offsets[t], 0), T), o1 = min(max(offsets[t + 1], o0), T);
    return o1 - o0;
}

template <int CHUNK>
__global__ __launch_bounds__(256) void ragged_items_kernel(const int* __restrict__ offsets, int NP, int T, int* __restrict__ first) {
    __shared__ int wsum[4];
    __shared__ int carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < NP; base += 256) {
        const int t = base + tid;
        const int items = t < NP ? (ragged_count(offsets, t, T) + CHUNK - 1) / CHUNK : 0;
        int incl = items;  // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (t < NP) first[t] = before + incl - items;
        __syncthreads();
        if (tid == 255) carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) first[NP] = carry;
}

// This workgroup's item -> its span; false: nothing to do (surplus workgroup, or a patch the plan dropped).  Workgroup-uniform.
template <int CHUNK>
__device__ __forceinline__ bool ragged_span(const TrunkRaggedParams& pr, ItemSpan& sp, size_t& o) {
    const int rep = (int)blockIdx.x / pr.bound;
    const int item = (int)blockIdx.x - rep * pr.bound;
    if (item >= pr.first[pr.NP]) return false;
    int lo = 0, hi = pr.NP;  // first[lo] <= item < first[hi]: the patch is the last one whose first item is <= item (an empty patch never is)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pr.first[mid] <= item) lo = mid;
        else hi = mid;
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    const int row = pr.pos ? pr.pos[(size_t)rep * pr.NP + lo] : lo;
    if (row < 0) return false;
    const int o0 = min(max(pr.offsets[lo], 0), pr.T);
    o = (size_t)rep * pr.T + o0;
    sp = ItemSpan{row, pr.t.grid + 2 * (size_t)o0, (item - pr.first[lo]) * CHUNK, ragged_count(pr.offsets, lo, pr.T), pr.t.out ? pr.t.out + o : nullptr};
    return true;
}

template <int HP, int ACT, int RES>
__global__ __launch_bounds__(256, (HP <= 256 ? 2 : 1)) void siren_trunk_f32_ragged_kernel(TrunkRaggedParams pr) {
    ItemSpan sp;
    size_t o;
    if (!ragged_span<64>(pr, sp, o)) return;  // before any barrier
    siren_trunk_f32_body<HP, ACT, RES, 0>(pr.t, sp, 0);
}

// The value kernel (H = 256, no residual) as the CONDITIONAL launch behind siren_trunk_f16x3n_ragged_kernel on the same stream: every
// workgroup leaves unless that launch wrote its number to *cond (a scaled modulation beyond fp16: siren_trunk_f32_kernel's rule), so a
// flagged call holds the exact path's bits.  pr.t.cond / cond_val / host_flag as launch_trunk_f32_cond sets them.
template <int ACT>
__global__ __launch_bounds__(256, 2) void siren_trunk_f32_ragged_cond_kernel(TrunkRaggedParams pr) {
    ItemSpan sp;
    size_t o;
    if (__builtin_amdgcn_readfirstlane(*pr.t.cond) != pr.t.cond_val) return;
    if (blockIdx.x == 0 && threadIdx.x == 0 && pr.t.host_flag) *pr.t.host_flag = 1;  // (before the span test: workgroup 0's item may be a dropped patch)
    if (!ragged_span<64>(pr, sp, o)) return;  // before any barrier
    siren_trunk_f32_body<256, ACT, 0, 0>(pr.t, sp, 0);
}

template <int HP, int ACT>
__global__ __launch_bounds__(256, 1) void siren_trunk_f32_jet_ragged_kernel(TrunkRaggedParams pr) {
    ItemSpan sp;
    size_t o;
    if (!ragged_span<32>(pr, sp, o)) return;  // before any barrier
    siren_trunk_f32_jet_body<HP, ACT>(pr.t, sp, pr.grad + o, pr.grad + (size_t)pr.reps * pr.T + o, pr.gscale);
}

}  // namespace msiren
