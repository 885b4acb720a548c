// Groups of target slices aligned to the stack read as a volume under one shared rigid motion per group (DESIGN.md section 5.15,
// msiren_align_volume_solve_group*): the step stage of section 5.14's loop for shared parameters.  Points, bins, the jet ragged trunk and the
// 80-sum reduce are align_volume_w.hip.h's, unchanged.  The m targets are G groups of consecutive targets, group y = targets group_start[y] ..
// group_start[y + 1] - 1; a group carries one rigid state (Rot, u), a target its own plane, weights and intensity (g, b).
//
//   upload   align_group_upload_kernel   up to 512 offsets of group_start, carried by value in the kernel's arguments -> the state (no host sync)
//   init     align_group_init_kernel     one thread per target: group_of, trial := best := the map of the group's input state, (g, b)
//   step     align_group_decide_kernel   one thread per group: E, C, W over its members, accept / reject, lam; on accept rigid_best := rigid_trial
//            align_group_project_kernel  one thread per target: commits best := trial where its group accepted; its record at the best state:
//                                        t = B^T g, the triangle of HQ = B^T (H B) and, estimating, X = D^-1 C, y = D^-1 c of its 2 x 2 block
//            align_group_step_kernel     one thread per group: M = sum HQ[0:6, 0:6], tm = sum t[0:6] over its members (run-time bounds), the
//                                        damping, minus every eliminating member's Schur term, the 6 x 6 solve, the Cayley update -> rigid_trial
//            align_group_apply_kernel    one thread per target: trial := the map of rigid_trial on its plane, (g, b)' = (g, b) + (y - X d);
//                                        behind the last evaluation the outputs
// The rule is restated by mri_inr_amd/align_group.py: lm_step_g -- fp64 + - * / one at a time, every sum in the order written there; a sum over
// the members of a group starts with the first member's term.  Within a system every loop has constant bounds and is unrolled and nothing is
// indexed at run time; plain stores, no atomics: a group's trajectory depends on that group only.
// Shared with the per-target solves (align_volume.hip.h): B is align_rigid_jacobian3, the proposal align_cayley_update.  The projection in the
// project kernel is its own copy of align_volume_step_w_kernel's (align_volume_w.hip.h says why).
#pragma once
#include <hip/hip_runtime.h>

#include "align_volume_w.hip.h"

namespace msiren {

constexpr int ALIGN_GROUP_OFFSETS = 512;  // offsets one upload launch carries
constexpr int ALIGN_GROUP_REC = 60;       // doubles per target record: t 8, HQ lower triangle row-major 36, X 2 x 6, y 2, eliminates, pad
constexpr int ALIGN_GROUP_REC_HQ = 8, ALIGN_GROUP_REC_X = 44, ALIGN_GROUP_REC_Y = 56, ALIGN_GROUP_REC_ELIM = 58;
constexpr int ALIGN_GROUP_SCAL = 9;       // doubles per group: mean_best, mean_first, lam, d[6]
constexpr int ALIGN_GROUP_CNT = 4;        // ints per group: accepted, flags, accept (of the evaluation just decided), pad

struct AlignGroupOffsets {
    int v[ALIGN_GROUP_OFFSETS];
};

struct AlignGroupParams {
    const double* sums;                  // (m, 80) of the evaluation at `trial`, `gb_trial`
    const double* planes;                // (m, 12) = (e_i, e_j, o, c)
    float *trial, *best;                 // (m, 9)
    float *gb_trial, *gb_best;           // (m, 2)
    double* sums_best;                   // (m, 80)
    double* rec;                         // (m, ALIGN_GROUP_REC)
    int* group_of;                       // (m)
    int* group_start;                    // (G + 1)
    double *rigid_trial, *rigid_best;    // (G, 12)
    double* scal;                        // (G, ALIGN_GROUP_SCAL)
    int* cnt;                            // (G, ALIGN_GROUP_CNT)
    double* trace;                       // (iterations, G, 15) or null
    float* maps_out;                     // (m, 9)      written behind the last evaluation
    float* intensity_out;                // (m, 2)
    double* rigid_out;                   // (G, 12) or null
    double* report;                      // (G, 7)
    double* target_report;               // (m, 3) or null
    int m, G, k, last, est;              // k: the evaluation just done; last: k == iterations - 1; est: (g, b) are solved for
    double down, up, lam_min, lam_max, spacing;
};

// where HQ[k][r], k >= r, lies in a record's triangle (the leading 6 x 6 block has the same places with the intensity fixed or estimated)
__device__ __forceinline__ constexpr int align_group_tri(int k, int r) { return ALIGN_GROUP_REC_HQ + (k * (k + 1)) / 2 + r; }

// dst[base + i] = s.v[i] for i < count: group_start reaches the device in kernel arguments.  grid: ceil(512 / 256) workgroups of 256.
__global__ __launch_bounds__(256) void align_group_upload_kernel(AlignGroupOffsets s, int* __restrict__ dst, int base, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) dst[base + i] = s.v[i];
}

// before the first evaluation, one thread per target: its group (the last y with group_start[y] <= q), trial := best := the map of the group's
// input state on its plane, (g, b) (intensity null: (1, 0)); the first member of a group also sets the group's state, lam := damping
__global__ __launch_bounds__(256) void align_group_init_kernel(AlignGroupParams p, const double* __restrict__ rigid_in, const float* __restrict__ intensity_in,
                                                               double damping) {
#pragma clang fp contract(off)
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= p.m) return;
    int lo = 0, hi = p.G;  // group_start[lo] <= q < group_start[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (p.group_start[mid] <= q) lo = mid;
        else hi = mid;
    }
    const int y = lo;
    p.group_of[q] = y;
    double st[12], pl[12];
    float mp[9];
#pragma unroll
    for (int a = 0; a < 12; ++a) st[a] = rigid_in[(size_t)y * 12 + a], pl[a] = p.planes[(size_t)q * 12 + a];
    align_rigid_map3(st, pl, p.spacing, mp);
    const float g = intensity_in ? intensity_in[(size_t)q * 2] : 1.f, b = intensity_in ? intensity_in[(size_t)q * 2 + 1] : 0.f;
#pragma unroll
    for (int a = 0; a < 9; ++a) p.trial[(size_t)q * 9 + a] = mp[a], p.best[(size_t)q * 9 + a] = mp[a];
    p.gb_trial[(size_t)q * 2] = g, p.gb_trial[(size_t)q * 2 + 1] = b, p.gb_best[(size_t)q * 2] = g, p.gb_best[(size_t)q * 2 + 1] = b;
#pragma unroll
    for (int a = 0; a < ALIGN_VOLUME_SUMS_W; ++a) p.sums_best[(size_t)q * ALIGN_VOLUME_SUMS_W + a] = 0.0;
#pragma unroll
    for (int a = 0; a < ALIGN_GROUP_REC; ++a) p.rec[(size_t)q * ALIGN_GROUP_REC + a] = 0.0;
    if (q == p.group_start[y]) {
#pragma unroll
        for (int a = 0; a < 12; ++a) p.rigid_trial[(size_t)y * 12 + a] = st[a], p.rigid_best[(size_t)y * 12 + a] = st[a];
        double* sc = p.scal + (size_t)y * ALIGN_GROUP_SCAL;
        sc[0] = __builtin_inf(), sc[1] = __builtin_inf(), sc[2] = damping;
#pragma unroll
        for (int a = 3; a < ALIGN_GROUP_SCAL; ++a) sc[a] = 0.0;
#pragma unroll
        for (int a = 0; a < ALIGN_GROUP_CNT; ++a) p.cnt[(size_t)y * ALIGN_GROUP_CNT + a] = 0;
    }
}

// behind evaluation k, one thread per group: E, C, W over the members' sums at the trial, mean = E / W if C >= P else +inf with P = 6, or
// 6 + 2 size where the intensity is estimated; align_lm_decide on it.  On accept rigid_best := rigid_trial; the members commit in the project kernel.
__global__ __launch_bounds__(256) void align_group_decide_kernel(AlignGroupParams p) {
#pragma clang fp contract(off)
    const int y = blockIdx.x * 256 + threadIdx.x;
    if (y >= p.G) return;
    constexpr int S = ALIGN_VOLUME_SUMS_W;
    const int lo = p.group_start[y], hi = p.group_start[y + 1];
    double C = p.sums[(size_t)lo * S], W = p.sums[(size_t)lo * S + 1], E = p.sums[(size_t)lo * S + 2];
    for (int q = lo + 1; q < hi; ++q) {
        C = C + p.sums[(size_t)q * S];
        W = W + p.sums[(size_t)q * S + 1];
        E = E + p.sums[(size_t)q * S + 2];
    }
    if (p.trace) {
        double* tr = p.trace + ((size_t)p.k * p.G + y) * 15;
#pragma unroll
        for (int a = 0; a < 12; ++a) tr[a] = p.rigid_trial[(size_t)y * 12 + a];
        tr[12] = E, tr[13] = C, tr[14] = W;
    }
    double* sc = p.scal + (size_t)y * ALIGN_GROUP_SCAL;
    int* cn = p.cnt + (size_t)y * ALIGN_GROUP_CNT;
    double mean_best = sc[0], mean_first = sc[1], lam = sc[2];
    int accepted = cn[0];
    const double P = (double)(6 + (p.est ? 2 * (hi - lo) : 0));
    const double mean = C >= P ? E / W : __builtin_inf();
    const bool accept = align_lm_decide(p.k, mean, &mean_best, &mean_first, &lam, &accepted, p.down, p.up, p.lam_min, p.lam_max);
    if (accept) {
#pragma unroll
        for (int a = 0; a < 12; ++a) p.rigid_best[(size_t)y * 12 + a] = p.rigid_trial[(size_t)y * 12 + a];
    }
    sc[0] = mean_best, sc[1] = mean_first, sc[2] = lam;
    cn[0] = accepted, cn[2] = accept ? 1 : 0;
}

// one thread per target: where its group accepted, best := trial in the state; then its record at the best state.  B, t and HQ are
// align_volume_step_w_kernel's expressions in rigid mode on the GROUP's best state and the target's plane, HQ undamped.  EST: the target's 2 x 2
// intensity block D = HQ[6:8, 6:8], damped on its diagonal by the group's lam, is factorised (L D L^T, ldl_solve's operations for two unknowns) and
// X = D^-1 HQ[6:8, 0:6], y = D^-1 (-0.5 t[6:8]) go into the record; a target with fewer than two valid pixels or a failed factorisation does not
// eliminate (X = y = 0, the flag 0).
template <int EST>
__global__ __launch_bounds__(256) void align_group_project_kernel(AlignGroupParams p) {
#pragma clang fp contract(off)
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= p.m) return;
    constexpr int N = EST ? 11 : 9, Q = EST ? 8 : 6, S = ALIGN_VOLUME_SUMS_W;
    const int y = p.group_of[q];
    if (p.cnt[(size_t)y * ALIGN_GROUP_CNT + 2]) {  // best := trial, in the state
        const double* ev = p.sums + (size_t)q * S;
#pragma unroll
        for (int a = 0; a < S; ++a) p.sums_best[(size_t)q * S + a] = ev[a];
#pragma unroll
        for (int a = 0; a < 9; ++a) p.best[(size_t)q * 9 + a] = p.trial[(size_t)q * 9 + a];
        p.gb_best[(size_t)q * 2] = p.gb_trial[(size_t)q * 2], p.gb_best[(size_t)q * 2 + 1] = p.gb_trial[(size_t)q * 2 + 1];
    }
    __asm__ volatile("" ::: "memory");
    const double* bs = p.sums_best + (size_t)q * S;  // the sums at the best state
    double* rec = p.rec + (size_t)q * ALIGN_GROUP_REC;
    double B[N][Q];
    {
        double rb[12], pl[12];
#pragma unroll
        for (int a = 0; a < 12; ++a) rb[a] = p.rigid_best[(size_t)y * 12 + a], pl[a] = p.planes[(size_t)q * 12 + a];
        align_rigid_jacobian3<N, Q>(rb, pl, p.spacing, B);
    }
    double t6 = 0.0, t7 = 0.0;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const double bg = B[a][k] * bs[3 + a];
            t = t + bg;
        }
        rec[k] = t;
        if (k == 6) t6 = t;
        if (k == 7) t7 = t;
    }
    // HQ = B^T (H B), column by column: T[., r] = H B[., r], then HQ[k][r] = sum_a B[a][k] T[a][r] for k >= r
    double C6[6], C7[6], h66 = 0.0, h76 = 0.0, h77 = 0.0;  // rows 6 and 7 of HQ (EST)
#pragma unroll
    for (int r = 0; r < Q; ++r) {
        __asm__ volatile("" ::: "memory");  // (the sums are read again per column instead of being held across all of them)
        double Tc[N];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < N; ++b) {
                const double hb = bs[a <= b ? align_vw_packed(a, b) : align_vw_packed(b, a)] * B[b][r];
                t = t + hb;
            }
            Tc[a] = t;
        }
#pragma unroll
        for (int k = r; k < Q; ++k) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) {
                const double bt = B[a][k] * Tc[a];
                t = t + bt;
            }
            rec[align_group_tri(k, r)] = t;
            if (EST) {
                if (k == 6 && r < 6) C6[r] = t;
                if (k == 7 && r < 6) C7[r] = t;
                if (k == 6 && r == 6) h66 = t;
                if (k == 7 && r == 6) h76 = t;
                if (k == 7 && r == 7) h77 = t;
            }
        }
    }
    if (EST) {
        const double lam = p.scal[(size_t)y * ALIGN_GROUP_SCAL + 2], inf = __builtin_inf();
        const double l6 = lam * h66, l7 = lam * h77;
        const double d0 = h66 + l6, a11 = h77 + l7;
        const double L = h76 / d0, ll = L * L;
        const double d1 = a11 - ll * d0;
        const bool elim = d0 > 0.0 && d0 < inf && d1 > 0.0 && d1 < inf && bs[0] >= 2.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {  // six columns of C, then c
            const double b0 = k < 6 ? C6[k < 6 ? k : 0] : -0.5 * t6, b1 = k < 6 ? C7[k < 6 ? k : 0] : -0.5 * t7;
            double x0 = b0, x1 = b1 - L * x0;
            x0 = x0 / d0, x1 = x1 / d1;
            x0 = x0 - L * x1;
            if (!elim) x0 = 0.0, x1 = 0.0;
            if (k < 6) rec[ALIGN_GROUP_REC_X + k] = x0, rec[ALIGN_GROUP_REC_X + 6 + k] = x1;
            else rec[ALIGN_GROUP_REC_Y] = x0, rec[ALIGN_GROUP_REC_Y + 1] = x1;
        }
        rec[ALIGN_GROUP_REC_ELIM] = elim ? 1.0 : 0.0;
    }
}

// one thread per group behind the records: M and tm over the members in ascending order from the first member's term, the damping, minus the
// Schur term C^T X (and C^T y on the right) of every eliminating member in ascending order, d = ldl_solve(A, rhs, 6), the Cayley update of
// align_volume_step_w_kernel on the group's best state -> rigid_trial, d, flags; behind the last evaluation the group's outputs.  The loops over
// the members have run-time bounds; a member's record is addressed at run time, the systems are not.
template <int EST>
__global__ __launch_bounds__(256) void align_group_step_kernel(AlignGroupParams p) {
#pragma clang fp contract(off)
    const int y = blockIdx.x * 256 + threadIdx.x;
    if (y >= p.G) return;
    const int lo = p.group_start[y], hi = p.group_start[y + 1];
    double* sc = p.scal + (size_t)y * ALIGN_GROUP_SCAL;
    const double lam = sc[2];
    double A[6][6], rhs[6], d[6];
    {
        const double* rec = p.rec + (size_t)lo * ALIGN_GROUP_REC;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            rhs[k] = rec[k];
#pragma unroll
            for (int r = 0; r <= k; ++r) A[k][r] = rec[align_group_tri(k, r)];
        }
    }
    for (int q = lo + 1; q < hi; ++q) {
        const double* rec = p.rec + (size_t)q * ALIGN_GROUP_REC;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            rhs[k] = rhs[k] + rec[k];
#pragma unroll
            for (int r = 0; r <= k; ++r) A[k][r] = A[k][r] + rec[align_group_tri(k, r)];
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double lh = lam * A[k][k];
        A[k][k] = A[k][k] + lh;
        rhs[k] = -0.5 * rhs[k];
    }
    if (EST) {
        for (int q = lo; q < hi; ++q) {
            const double* rec = p.rec + (size_t)q * ALIGN_GROUP_REC;
            if (rec[ALIGN_GROUP_REC_ELIM] != 0.0) {
                const double y0 = rec[ALIGN_GROUP_REC_Y], y1 = rec[ALIGN_GROUP_REC_Y + 1];
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const double c6 = rec[align_group_tri(6, k)], c7 = rec[align_group_tri(7, k)];
#pragma unroll
                    for (int r = 0; r <= k; ++r) {
                        const double s0 = c6 * rec[ALIGN_GROUP_REC_X + r], s1 = c7 * rec[ALIGN_GROUP_REC_X + 6 + r];
                        const double s = s0 + s1;
                        A[k][r] = A[k][r] - s;
                    }
                    const double s0 = c6 * y0, s1 = c7 * y1;
                    const double s = s0 + s1;
                    rhs[k] = rhs[k] - s;
                }
            }
        }
    }
    const bool ok = align_ldl_solve<6>(A, rhs, d);
    __asm__ volatile("" ::: "memory");
    double rb[12], rt[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) rb[a] = p.rigid_best[(size_t)y * 12 + a];
    align_cayley_update(d, rb, rt);
#pragma unroll
    for (int a = 0; a < 12; ++a) p.rigid_trial[(size_t)y * 12 + a] = rt[a];
#pragma unroll
    for (int a = 0; a < 6; ++a) sc[3 + a] = d[a];
    const double mean_best = sc[0], mean_first = sc[1];
    int* cn = p.cnt + (size_t)y * ALIGN_GROUP_CNT;
    const int flags = (ok ? 0 : ALIGN_SINGULAR) | (mean_first == __builtin_inf() ? ALIGN_NO_OVERLAP : 0);
    cn[1] = flags;
    if (p.last) {
        constexpr int S = ALIGN_VOLUME_SUMS_W;
        double C = p.sums_best[(size_t)lo * S], W = p.sums_best[(size_t)lo * S + 1];
        for (int q = lo + 1; q < hi; ++q) {
            C = C + p.sums_best[(size_t)q * S];
            W = W + p.sums_best[(size_t)q * S + 1];
        }
        if (p.rigid_out) {
#pragma unroll
            for (int a = 0; a < 12; ++a) p.rigid_out[(size_t)y * 12 + a] = rb[a];
        }
        double* rp = p.report + (size_t)y * 7;
        rp[0] = (double)cn[0], rp[1] = mean_first, rp[2] = mean_best, rp[3] = C, rp[4] = W, rp[5] = lam, rp[6] = (double)flags;
    }
}

// one thread per target behind its group's step: trial := the map of rigid_trial on its plane; EST and the target eliminated:
// (dg, db) = y - X d, (g, b)' = (float)((double)(g, b)_best + (dg, db)); otherwise (g, b)' = (g, b)_best.  Behind the last evaluation the
// target's outputs: the best map and (g, b), count, wsum and cost at the best state.
template <int EST>
__global__ __launch_bounds__(256) void align_group_apply_kernel(AlignGroupParams p) {
#pragma clang fp contract(off)
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= p.m) return;
    const int y = p.group_of[q];
    double rt[12], pl[12];
    float trial[9];
#pragma unroll
    for (int a = 0; a < 12; ++a) rt[a] = p.rigid_trial[(size_t)y * 12 + a], pl[a] = p.planes[(size_t)q * 12 + a];
    align_rigid_map3(rt, pl, p.spacing, trial);
    const float gbest = p.gb_best[(size_t)q * 2], bbest = p.gb_best[(size_t)q * 2 + 1];
    float gt = gbest, bt = bbest;
    if (EST) {
        const double* rec = p.rec + (size_t)q * ALIGN_GROUP_REC;
        if (rec[ALIGN_GROUP_REC_ELIM] != 0.0) {
            const double* d = p.scal + (size_t)y * ALIGN_GROUP_SCAL + 3;
            double x0 = 0.0, x1 = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double m0 = rec[ALIGN_GROUP_REC_X + a] * d[a], m1 = rec[ALIGN_GROUP_REC_X + 6 + a] * d[a];
                x0 = x0 + m0, x1 = x1 + m1;
            }
            const double dg = rec[ALIGN_GROUP_REC_Y] - x0, db = rec[ALIGN_GROUP_REC_Y + 1] - x1;
            gt = (float)((double)gbest + dg), bt = (float)((double)bbest + db);
        }
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) p.trial[(size_t)q * 9 + a] = trial[a];
    p.gb_trial[(size_t)q * 2] = gt, p.gb_trial[(size_t)q * 2 + 1] = bt;
    if (p.last) {
#pragma unroll
        for (int a = 0; a < 9; ++a) p.maps_out[(size_t)q * 9 + a] = p.best[(size_t)q * 9 + a];
        p.intensity_out[(size_t)q * 2] = gbest, p.intensity_out[(size_t)q * 2 + 1] = bbest;
        if (p.target_report) {
            const double* bs = p.sums_best + (size_t)q * ALIGN_VOLUME_SUMS_W;
            p.target_report[(size_t)q * 3] = bs[0], p.target_report[(size_t)q * 3 + 1] = bs[1], p.target_report[(size_t)q * 3 + 2] = bs[2];
        }
    }
}

}  // namespace msiren
