// The exact-fp32 trunk with its spatial gradient: value and d/dcoords of SirenNet.forward in one forward-mode ("jet") pass
// (msiren_sample_grad_*, msiren_reconstruct_slices_grad).
//
// The arithmetic is the five layers of siren_trunk_f32.hip.h applied to three columns per coordinate instead of one: the value h and its
// two tangents dh/d(row), dh/d(column).  With the weights pre-scaled by w0/2pi the accumulators are in revolutions:
//     layer 0        r = w_row x + w_col y + b                  dr = (w_row, w_col)                     (no bias in a tangent)
//     hidden layer   r = W' h + b'                              dr = W' dh                              (the same MFMAs, bias never added)
//     activation     h' = act(r) mod                            dh' = act'(r) mod dr                    (r from the value tile)
//     last layer     out = sin(2 pi s),  s = wout' . h + bout   dout = 2 pi cos(2 pi s) (wout' . dh)
//     sine           act'(r) = 2 pi cos(2 pi r): v_cos_f32, whose argument is in revolutions like v_sin_f32's -- not sin_rev(r + 1/4), which
//                    rounds the phase at |r| of tens of revolutions
//     Morlet         act'(r) = (2 pi cos(2 pi r) + sin(2 pi r) 2 ln2 cg r) exp2(cg r^2)
//
// Work decomposition
//   workgroup = 256 threads = 4 waves = one (patch b, chunk of 32 coordinates); grid = B * ceil(Q/32).
//   LDS holds X as [k/4][96 columns][k%4] fp32: column tile 0 the value, tile 1 d/d(row), tile 2 d/d(column) of the same 32 coordinates.
//   HP * 384 B (96 KB at HP = 256) beside the HP * 16 B of layer-0 rows: one workgroup per CU, the opt-in dynamic-LDS limit.  H = 512 would
//   need 192 KB: out of scope.
//   Each wave owns HP/4 output features for the 96 columns: acc[TT][3] x 16 registers.  The A fragments come from the fp32 trunk's packed
//   stream through the same 4-stage register ring; each is used by three column tiles.  The value and the two tangents of one
//   (feature, coordinate) sit in the same lane and register index of the three accumulators, so the tangent epilogue needs no shuffle.
//
// The value column produces THE BITS OF siren_trunk_f32_kernel<HP, ACT, 0>: the same v_mfma_f32_32x32x2_f32 on the same k pairs in the same
// order per accumulator, the same two fmaf in layer 0, the same epilogue expressions, dot4_acc and the same order of the last_layer sum
// (tests/test_gpu_grad.py: np.array_equal against the fp32 model's sample_mods).
//
// No atomics, no scratch; every output element is written by exactly one thread.
#pragma once
#include "siren_trunk_f32.hip.h"

namespace msiren {

struct TrunkJetParams {
    TrunkParams t;  // grid = the call's coordinates (Q = t.P of them); t.out (B, Q) may be null; t.chunks = ceil(Q / 32)
    float* grad;    // (2, B, Q): plane 0 d/d(row coordinate), plane 1 d/d(column coordinate)
    float gscale;   // every gradient is multiplied by it (1 for the sampling calls; the slice form: coordinate units per output pixel)
};

constexpr int jet_lds_bytes(int HP) { return HP * 384 + HP * 16; }  // X image + layer-0 rows

__device__ __forceinline__ float cos_rev(float r) { return __builtin_amdgcn_cosf(r); }

// d act / d r for r in revolutions (activate<ACT> of siren_trunk_f32.hip.h)
template <int ACT>
__device__ __forceinline__ float activate_d(float r, float cg) {
    constexpr float TWO_PI = 6.283185307179586f, TWO_LN2 = 1.3862943611198906f;
    if constexpr (ACT == 1) {
        return (TWO_PI * cos_rev(r) + sin_rev(r) * (TWO_LN2 * cg * r)) * __builtin_amdgcn_exp2f(cg * r * r);
    } else {
        return TWO_PI * cos_rev(r);
    }
}

// One work item = (modulation row, chunk of 32 coordinates) = `sp` (siren_trunk_f32.hip.h); grad0 / grad1: the two gradient planes'
// entries of the set's coordinate 0.
template <int HP, int ACT>
__device__ __forceinline__ void siren_trunk_f32_jet_body(const TrunkParams& p, const ItemSpan& sp, float* grad0, float* grad1, const float gscale) {
    constexpr int TT = HP / 128;  // 32-feature tiles per wave
    constexpr int QN = HP / 8;    // k-blocks of 8 per layer
    constexpr int KG = HP / 4;    // k-groups of 4 (rows of the X image)
    constexpr int XS = 96;        // columns of the X image: 3 tiles of 32
    static_assert(HP == 128 || HP == 256, "the three-tile image fits the LDS up to a hidden width of 256");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    f32x4* X = reinterpret_cast<f32x4*>(lds);  // X[kg * 96 + 32 * tile + coord]   HP*384 B
    f32x4* P0 = X + KG * XS;                   // layer-0 rows {wx, wy, b, mod}    HP*16 B

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int c32 = lane & 31;
    const int b = sp.b;
    const int L = p.L;

    // ---------------- weight stream: the ring of siren_trunk_f32_item ---------------------------
    const int nblk = (L - 1) * QN;
    const f32x4* wbase = reinterpret_cast<const f32x4*>(p.wp) + lane;
    auto loadA = [&](f32x4(&a)[TT], int s) {
        s = s < nblk ? s : nblk - 1;  // past the end: harmless re-load of the last block
        const int l1 = s / QN, q = s - l1 * QN;
        const f32x4* ptr = wbase + (((size_t)l1 * 4 + wave) * QN + q) * (TT * 64);
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) a[tt] = ptr[tt * 64];
    };
    f32x4 a0[TT], a1[TT], a2[TT], a3[TT];
    if (L > 1) {
        loadA(a0, 0);
        loadA(a1, 1);
        loadA(a2, 2);
    }

    // ---------------- layer 0: K = 2, value and tangents straight into the X image --------------
    {
        const float* mod0 = p.mods + (size_t)b * p.mod_stride;
        const f32x4* l0 = reinterpret_cast<const f32x4*>(p.l0);
        for (int f = tid; f < HP; f += 256) {
            f32x4 w = l0[f];
            w[3] = mod0[f];
            P0[f] = w;
        }
        int pc = sp.first + c32;
        pc = pc < sp.count ? pc : sp.count - 1;
        const float2 xy = reinterpret_cast<const float2*>(sp.coords)[pc];
        __syncthreads();
#pragma unroll 2
        for (int i = 0; i < KG / 8; ++i) {
            const int kg = wave * (KG / 4) + 2 * i + half;  // two rows (one per half-wave) at a time
            f32x4 v, dx, dy;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4 w = P0[4 * kg + e];
                const float r = __builtin_fmaf(xy.y, w.y, __builtin_fmaf(xy.x, w.x, w.z));
                v[e] = activate<ACT>(r, p.cg0) * w[3];
                const float d = activate_d<ACT>(r, p.cg0) * w[3];
                dx[e] = d * w.x;
                dy[e] = d * w.y;
            }
            X[kg * XS + c32] = v;
            X[kg * XS + 32 + c32] = dx;
            X[kg * XS + 64 + c32] = dy;
        }
    }
    __syncthreads();

    // ---------------- hidden layers 1..L-1 on the matrix cores ---------------------------------
    const int fwave = wave * (32 * TT);      // first feature owned by this wave
    float part[3] = {0.f, 0.f, 0.f};         // last_layer partial sums: value, d/d(row), d/d(column)

    for (int l = 1; l < L; ++l) {
        const float* bl = p.bias + (size_t)(l - 1) * HP;
        const float* ml = p.mods + ((size_t)l * p.B + b) * p.mod_stride;
        const bool last = (l == L - 1);

        // per-feature constants of this wave's rows: issued now, consumed in the epilogue (on the final hidden layer the modulation
        // is pre-multiplied by last_layer's weight, as in siren_trunk_f32_item)
        f32x4 bias_r[TT][4], mod_r[TT][4];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int fo = fwave + 32 * tt + 8 * g + 4 * half;
                bias_r[tt][g] = *reinterpret_cast<const f32x4*>(bl + fo);
                mod_r[tt][g] = *reinterpret_cast<const f32x4*>(ml + fo);
            }
        if (last) {
#pragma unroll
            for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    mod_r[tt][g] *= *reinterpret_cast<const f32x4*>(p.wout + fwave + 32 * tt + 8 * g + 4 * half);
        }

        f32x16 acc[TT][3];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int jc = 0; jc < 3; ++jc)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tt][jc][r] = 0.f;

        const f32x4* xB = X + half * XS + c32;  // + (2q)*96 + 32*jc
        auto loadB = [&](f32x4(&bb)[3], int q) {
            q = q < QN ? q : QN - 1;
            bb[0] = xB[(2 * q) * XS];
            bb[1] = xB[(2 * q) * XS + 32];
            bb[2] = xB[(2 * q) * XS + 64];
        };
        auto mma = [&](const f32x4(&a)[TT], const f32x4(&bb)[3]) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                    for (int jc = 0; jc < 3; ++jc)
                        acc[tt][jc] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tt][j], bb[jc][j], acc[tt][jc], 0, 0, 0);
        };

        f32x4 b0[3], b1[3];
        loadB(b0, 0);
        const int sb = (l - 1) * QN;
        // sched_barrier pins "issue the loads of later blocks, then this block's MFMAs" (siren_trunk_f32_item)
#pragma nounroll
        for (int q = 0; q < QN; q += 4) {
            loadA(a3, sb + q + 3);
            loadB(b1, q + 1);
            __builtin_amdgcn_sched_barrier(0);
            mma(a0, b0);
            __builtin_amdgcn_sched_barrier(0);
            loadA(a0, sb + q + 4);
            loadB(b0, q + 2);
            __builtin_amdgcn_sched_barrier(0);
            mma(a1, b1);
            __builtin_amdgcn_sched_barrier(0);
            loadA(a1, sb + q + 5);
            loadB(b1, q + 3);
            __builtin_amdgcn_sched_barrier(0);
            mma(a2, b0);
            __builtin_amdgcn_sched_barrier(0);
            loadA(a2, sb + q + 6);
            loadB(b0, q + 4);
            __builtin_amdgcn_sched_barrier(0);
            mma(a3, b1);
            __builtin_amdgcn_sched_barrier(0);
        }

        __syncthreads();  // every wave has finished reading X: rows may now be overwritten

        const int kgw = wave * (8 * TT);
        if (!last) {
            // epilogue: bias -> activation -> modulation (value); act'(r) * modulation * dr (tangents: the bias is never added)
#pragma unroll
            for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int xi = (kgw + 8 * tt + 2 * g + half) * XS + c32;
                    f32x4 v, dx, dy;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float r = acc[tt][0][4 * g + e] + bias_r[tt][g][e];
                        v[e] = activate<ACT>(r, p.cg) * mod_r[tt][g][e];
                        const float d = activate_d<ACT>(r, p.cg) * mod_r[tt][g][e];
                        dx[e] = d * acc[tt][1][4 * g + e];
                        dy[e] = d * acc[tt][2][4 * g + e];
                    }
                    X[xi] = v;
                    X[xi + 32] = dx;
                    X[xi + 64] = dy;
                }
            __syncthreads();
        } else {
            // final hidden layer: its output feeds last_layer's dot product straight from registers
#pragma unroll
            for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 av, ax, ay;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float r = acc[tt][0][4 * g + e] + bias_r[tt][g][e];
                        av[e] = activate<ACT>(r, p.cg);
                        const float d = activate_d<ACT>(r, p.cg);
                        ax[e] = d * acc[tt][1][4 * g + e];
                        ay[e] = d * acc[tt][2][4 * g + e];
                    }
                    part[0] = dot4_acc(part[0], av, mod_r[tt][g]);  // (mod_r holds modulation x last_layer.weight here)
                    part[1] = dot4_acc(part[1], ax, mod_r[tt][g]);
                    part[2] = dot4_acc(part[2], ay, mod_r[tt][g]);
                }
        }
    }

    // ---------------- last_layer: dot over H features, always sine -----------------------------
    float* red = lds;  // [3][4][32]; X is dead (or, for L == 1, read below before the barrier)
    if (L == 1) {
        // no hidden layer ran: the dot product from the X image, every wave its KG/4 rows in siren_trunk_f32_item's order (both half-waves
        // compute the same sums; one stores them)
        float s = 0.f, sx = 0.f, sy = 0.f;
        for (int i = 0; i < KG / 4; ++i) {
            const int kg = wave * (KG / 4) + i;
            const f32x4 v = X[kg * XS + c32];
            const f32x4 wo = *reinterpret_cast<const f32x4*>(p.wout + 4 * kg);
            s += v[0] * wo[0] + v[1] * wo[1] + v[2] * wo[2] + v[3] * wo[3];
            const f32x4 dx = X[kg * XS + 32 + c32], dy = X[kg * XS + 64 + c32];
            sx += dx[0] * wo[0] + dx[1] * wo[1] + dx[2] * wo[2] + dx[3] * wo[3];
            sy += dy[0] * wo[0] + dy[1] * wo[1] + dy[2] * wo[2] + dy[3] * wo[3];
        }
        part[0] = s, part[1] = sx, part[2] = sy;
        __syncthreads();
    } else {
#pragma unroll
        for (int jc = 0; jc < 3; ++jc) part[jc] += __shfl_xor(part[jc], 32);
        // (the barrier after the K loop already separates the last X reads from these writes)
    }
    if (half == 0) {
#pragma unroll
        for (int jc = 0; jc < 3; ++jc) red[(jc * 4 + wave) * 32 + c32] = part[jc];
    }
    __syncthreads();
    if (tid < 32) {
        constexpr float TWO_PI = 6.283185307179586f;
        const float s = red[tid] + red[32 + tid] + red[64 + tid] + red[96 + tid] + p.bout;
        const float sx = red[128 + tid] + red[160 + tid] + red[192 + tid] + red[224 + tid];
        const float sy = red[256 + tid] + red[288 + tid] + red[320 + tid] + red[352 + tid];
        const int pc = sp.first + tid;
        if (pc < sp.count) {
            const float dc = TWO_PI * cos_rev(s);
            if (sp.out) sp.out[pc] = sin_rev(s);
            grad0[pc] = (dc * sx) * gscale;
            grad1[pc] = (dc * sy) * gscale;
        }
    }
}

template <int HP, int ACT>
__global__ __launch_bounds__(256, 1) void siren_trunk_f32_jet_kernel(TrunkJetParams pj) {
    const TrunkParams& p = pj.t;
    const int item = (int)blockIdx.x;
    const int b = item / p.chunks;
    const int ch = item - b * p.chunks;
    if (p.plan && b >= p.plan[0]) return;  // workgroup-uniform, before any barrier
    const size_t o = (size_t)b * p.P;
    siren_trunk_f32_jet_body<HP, ACT>(p, ItemSpan{b, p.grid, ch * 32, p.P, p.out ? p.out + o : nullptr}, pj.grad + o, pj.grad + (size_t)p.B * p.P + o, pj.gscale);
}

}  // namespace msiren
