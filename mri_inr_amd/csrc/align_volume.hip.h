// Target slices scored against a stack read as a volume, each under its own 3 x 3 map (msiren_align_volume*): the steps
// either side of the ragged jet trunk.  Target q of m is read on its th x tw lattice under (z0, z1, tz, y0, y1, ty, x0, x1, tx): pixel (i, j) at
//     Z = ((z0 i) + (z1 j)) + tz      Y = ((y0 i) + (y1 j)) + ty      X = ((x0 i) + (x1 j)) + tx      fp32, every operation rounded on its own
// Z in slice units, (Y, X) in reconstruction pixel coordinates: align_point's rule (align.hip.h) with a third row.  Everything behind the point is
// resample_volume.hip.h's gradient form (both = 1): the pair z0' = min(floor Z, n - 2) with f', the bins (slice, tile), the slots of
// ResampleVolumeParams with M = m th tw.  R, gZ, gY, gX are the bits of msiren_resample_volume_grad at (Z, Y, X).
//
//   bin      align_volume_count_kernel    one thread per (target, pixel): the point from the target's map, then resample_volume_count_kernel's logic
//            resample_scan_kernel         (resample.hip.h) exclusive scan over the n nV nH bins -> the ragged offsets
//            align_volume_fill_kernel     the point again, then resample_volume_fill_kernel's logic: entry per slot (2 g + j) K + k, tile and weight per g K + k,
//                                         pair and f per g;  g = q th tw + p
//   trunk    the exact-fp32 jet ragged trunk over T = 2 m th tw K entries at most, one replica, on the plan's rows
//   reduce   align_volume_partial_kernel  one workgroup per (target, chunk of ALIGN_CHUNK pixels): per pixel and plane the blend of both slices
//                                         of the pair (volume_slice_blend), resample_volume_blend_kernel's selection and R1 - R0, [warped],
//                                         [wgrad], the 56 fp64 sums of the chunk -> one partial record
//            align_volume_combine_kernel  one workgroup per target: its partial records added in index order -> sums (m, 56)
// A pixel is VALID iff target, R, gZ, gY, gX are all finite; per valid pixel, in fp64 from the fp32 numbers, contraction off:
//     r = R - T,  J = (gZ i, gZ j, gZ, gY i, gY j, gY, gX i, gX j, gX),  count += 1, cost += r r, dcost[a] += (2 r) J[a], jtj[a, b] += J[a] J[b]
// record = [count, cost, dcost 9, jtj packed upper triangle row-major 45].  The order of every sum is align.hip.h's: thread t of a chunk adds
// its pixels lo + t, lo + t + 256, ..., score_block_sum's combine for all 56 behind one barrier, the chunks of a target in index order.  No
// floating-point atomics.
//
// What the volume families share lives here (align_volume_w.hip.h, align_volume_r.hip.h and align_group.hip.h call it; LAB_NOTES.md section 30):
//   align_volume_pixel            R, gZ, gY, gX of one pixel with the optional warped / wgrad stores: all three partial kernels
//   align_rigid_jacobian3<N, Q>   B of the rigid modes: both step kernels and align_group_project_kernel
//   align_cayley_update           Rot' = Cay Rot, u' = u + d[3:6]: align_volume_step_w_kernel and align_group_step_kernel.  align_volume_step_kernel<RIGID>
//                                 keeps these lines in its own body (through the function it spills), as it keeps its projection on the unpacked H
#pragma once
#include <hip/hip_runtime.h>

#include "align.hip.h"

namespace msiren {

constexpr int ALIGN_VOLUME_SUMS = 56;  // count, cost, dcost[9], jtj[45]

struct AlignVolumeParams {
    ResampleVolumeParams v;  // points unused (null); M = m th tw; both = 1
    const float* maps;       // (m, 9)
    int th, tw, Mt;          // Mt = th tw pixels per target
};

// where pixel (i, j) of the lattice is read under map a[0..8]: fp32, one rounding per operation
__device__ __forceinline__ void align_point3(const float* __restrict__ a, int i, int j, float* Z, float* Y, float* X) {
#pragma clang fp contract(off)
    const float fi = (float)i, fj = (float)j;  // (below 2^24: exact)
    const float z0 = a[0] * fi, z1 = a[1] * fj, y0 = a[3] * fi, y1 = a[4] * fj, x0 = a[6] * fi, x1 = a[7] * fj;
    const float zs = z0 + z1, ys = y0 + y1, xs = x0 + x1;
    *Z = zs + a[2];
    *Y = ys + a[5];
    *X = xs + a[8];
}

// thread g of the grid -> its point, placed by its target's map; false beyond the last pixel
__device__ __forceinline__ bool align_volume_thread_point(const AlignVolumeParams& p, int g, float* Z, float* Y, float* X) {
    *Z = 0.f, *Y = 0.f, *X = 0.f;
    if (g >= p.v.M) return false;  // (m th tw < 2^28: checked by the host)
    const int q = g / p.Mt, px = g - q * p.Mt, i = px / p.tw;
    align_point3(p.maps + 9 * (size_t)q, i, px - i * p.tw, Z, Y, X);
    return true;
}

// resample_volume_count_kernel behind the map: the same pair (volume_pair, both = 1), covers (cover_axis) and election (wave_bin_add)
__global__ __launch_bounds__(256) void align_volume_count_kernel(AlignVolumeParams ap) {
    const ResampleVolumeParams& p = ap.v;
    const int m = blockIdx.x * 256 + threadIdx.x;
    int z0 = -1, v0 = 0, h0 = 0, nv = 0, nh = 0, J = 0;
    float f, Z, Y, X;
    if (align_volume_thread_point(ap, m, &Z, &Y, &X)) {
        J = volume_pair(Z, p.n, p.both, &z0, &f);
        nv = cover_axis(Y, p.nV, p.S, p.I, p.pad, &v0), nh = cover_axis(X, p.nH, p.S, p.I, p.pad, &h0);
    }
    const int NPt = p.nV * p.nH;
    for (int j = 0; j < 2; ++j)
        for (int a = 0; a < p.KA; ++a)
            for (int b = 0; b < p.KA; ++b) {
                const bool has = j < J && a < nv && b < nh;
                (void)wave_bin_add(p.counts, has ? (z0 + j) * NPt + (v0 + a) * p.nH + h0 + b : 0, has);
            }
}

// resample_volume_fill_kernel behind the map: its slots, with its fp64 expressions (volume_tile_offset, volume_local_coord, volume_fold_weight)
__global__ __launch_bounds__(256) void align_volume_fill_kernel(AlignVolumeParams ap) {
    const ResampleVolumeParams& p = ap.v;
    const int m = blockIdx.x * 256 + threadIdx.x;
    const int K = p.KA * p.KA;
    int z0 = -1, v0 = 0, h0 = 0, nv = 0, nh = 0, J = 0;
    float f = 0.f, Z, Y, X;
    const bool in = align_volume_thread_point(ap, m, &Z, &Y, &X);
    if (in) {
        J = volume_pair(Z, p.n, p.both, &z0, &f);
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

// R, gZ, gY, gX of pixel gp, the bits of msiren_resample_volume_grad at its point: per plane the blend of both slices of the pair, then
// resample_volume_blend_kernel's selection; gZ = R1 - R0 of the value plane; an invalid Z: NaN in all four.  [warped], [wgrad] (3, M) get them.
// The three partial kernels (here, align_volume_w.hip.h, align_volume_r.hip.h) read their pixels through this.
__device__ __forceinline__ void align_volume_pixel(const float* __restrict__ vals, const int* __restrict__ ent, const int* __restrict__ tile, const float* __restrict__ w,
                                                   const int* __restrict__ black, const int* __restrict__ pair, const float* __restrict__ fz, float* __restrict__ warped,
                                                   float* __restrict__ wgrad, size_t gp, size_t M, int K, int NPt, int T, float* R, float* gZ, float* gY, float* gX) {
#pragma clang fp contract(off)
    const int z0 = pair[gp];
    float pl[3], dz;
    if (z0 < 0) {  // invalid Z: NaN in every plane, as resample_volume_blend_kernel writes it
        pl[0] = pl[1] = pl[2] = dz = __builtin_nanf("");
    } else {
        const float f = fz[gp], a0 = 1.0f - f;
        const int* e0 = ent + 2 * gp * K;
        const int* tl = tile + gp * K;
        const float* ww = w + gp * K;
        const int *b0 = black + (size_t)z0 * NPt, *b1 = black + (size_t)(z0 + 1) * NPt;
        dz = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* v = vals + (size_t)c * T;
            const float R0 = volume_slice_blend(v, e0, tl, ww, b0, K);
            const float R1 = volume_slice_blend(v, e0 + K, tl, ww, b1, K);
            pl[c] = f == 0.f ? R0 : f == 1.f ? R1 : __builtin_fmaf(f, R1, a0 * R0);
            if (c == 0) dz = R1 - R0;
        }
    }
    *R = pl[0], *gZ = dz, *gY = pl[1], *gX = pl[2];
    if (warped) warped[gp] = pl[0];
    if (wgrad) {
        wgrad[gp] = dz;
        wgrad[M + gp] = pl[1];
        wgrad[2 * M + gp] = pl[2];
    }
}

// vals (3, T): the jet ragged trunk's outputs by entry, T = 2 M K.  ent (2 M K), tile / w (M K), pair / fz (M): the fill kernel's.  black (n NPt).
// targets (m, Mt).  warped (m, Mt) and wgrad (3, m, Mt) may be null.  partials (m chunks, ALIGN_VOLUME_SUMS).
// grid: m * chunks workgroups (target-major), chunks = ceil(Mt / ALIGN_CHUNK)
__global__ __launch_bounds__(256) void align_volume_partial_kernel(const float* __restrict__ vals, const int* __restrict__ ent, const int* __restrict__ tile,
                                                                   const float* __restrict__ w, const int* __restrict__ black, const int* __restrict__ pair,
                                                                   const float* __restrict__ fz, const float* __restrict__ targets, float* __restrict__ warped,
                                                                   float* __restrict__ wgrad, double* __restrict__ partials, int m, int Mt, int tw, int K, int NPt,
                                                                   int T, int chunks) {
#pragma clang fp contract(off)
    __shared__ double red[ALIGN_VOLUME_SUMS][4];
    const int q = blockIdx.x / chunks, chunk = blockIdx.x - q * chunks;
    const int lo = chunk * ALIGN_CHUNK, hi = lo + ALIGN_CHUNK < Mt ? lo + ALIGN_CHUNK : Mt;
    const size_t M = (size_t)m * Mt;
    double acc[ALIGN_VOLUME_SUMS];
#pragma unroll
    for (int a = 0; a < ALIGN_VOLUME_SUMS; ++a) acc[a] = 0.0;
    for (int px = lo + threadIdx.x; px < hi; px += 256) {
        const size_t g = (size_t)q * Mt + px;
        float R, gZ, gY, gX;
        align_volume_pixel(vals, ent, tile, w, black, pair, fz, warped, wgrad, g, M, K, NPt, T, &R, &gZ, &gY, &gX);
        const float tv = targets[g];
        if (align_finite(tv) && align_finite(R) && align_finite(gZ) && align_finite(gY) && align_finite(gX)) {
            const int i = px / tw, j = px - i * tw;
            const double r = (double)R - (double)tv, r2 = 2.0 * r, di = (double)i, dj = (double)j;
            double J[9];
            J[0] = (double)gZ * di, J[1] = (double)gZ * dj, J[2] = (double)gZ;
            J[3] = (double)gY * di, J[4] = (double)gY * dj, J[5] = (double)gY;
            J[6] = (double)gX * di, J[7] = (double)gX * dj, J[8] = (double)gX;
            acc[0] += 1.0;
            acc[1] += r * r;
            int s = 11;
#pragma unroll
            for (int a = 0; a < 9; ++a) {
                acc[2 + a] += r2 * J[a];
#pragma unroll
                for (int b = a; b < 9; ++b, ++s) acc[s] += J[a] * J[b];
            }
        }
    }
    align_block_reduce<ALIGN_VOLUME_SUMS>(acc, red, partials);
}

// sums[q, a] = the target's partial records added in index order
__global__ __launch_bounds__(256) void align_volume_combine_kernel(const double* __restrict__ partials, double* __restrict__ sums, int chunks) {
    align_combine<ALIGN_VOLUME_SUMS>(partials, sums, chunks);
}

// ---- msiren_align_volume_solve* (DESIGN.md section 5.13): section 5.11's damped Gauss-Newton loop around the pipeline above --------------------
// One thread per target between two evaluations.  State per target, in the stream's scratch behind the partials:
//     trial, best (9 fp32 each)   the map the next evaluation reads / the best map so far
//     rigid_trial, rigid_best     (Rot 9 row-major, u 3) fp64 each (rigid mode)
//     sums_best (56 fp64)         the sums at the best map;  scal = (mean_best, mean_first, lam);  cnt = (accepted, flags)
// The rule is restated by mri_inr_amd/align_volume.py: lm_step_v -- fp64 + - * / one at a time (contraction off), every sum in the order written
// there.  The step kernel is instantiated per mode, so each instantiation carries one system (align_ldl_solve factorises it in place).
// Every loop has constant bounds and is unrolled: nothing is indexed at run time.  Plain stores, no atomics.
constexpr int ALIGN_VOLUME_AFFINE = 0, ALIGN_VOLUME_RIGID = 1;

struct AlignVolumeSolveParams {
    const double* sums;                  // (m, 56) of the evaluation at `trial`
    const double* planes;                // (m, 12) = (e_i, e_j, o, c), rigid mode
    float *trial, *best;                 // (m, 9)
    double *rigid_trial, *rigid_best;    // (m, 12)
    double* sums_best;                   // (m, 56)
    double* scal;                        // (m, 3)
    int* cnt;                            // (m, 2)
    double* trace;                       // (iterations, m, 11) or null
    float* maps_out;                     // (m, 9)      written behind the last evaluation
    double* rigid_out;                   // (m, 12) or null
    double* report;                      // (m, 6)
    int m, k, last;                      // k: the evaluation just done; last: k == iterations - 1
    double down, up, lam_min, lam_max, spacing;
};

// y = Rot x, rows in order, each ((r0 x0) + (r1 x1)) + r2 x2
__device__ __forceinline__ void align_rot_apply(const double (&R)[9], const double (&x)[3], double (&y)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double p0 = R[3 * r] * x[0], p1 = R[3 * r + 1] * x[1], p2 = R[3 * r + 2] * x[2];
        const double s = p0 + p1;
        y[r] = s + p2;
    }
}

// the lattice under the rigid state: v_i = Rot e_i, v_j = Rot e_j, v_o = Rot (o - c)
__device__ __forceinline__ void align_rigid_vectors3(const double (&st)[12], const double (&pl)[12], double (&vi)[3], double (&vj)[3], double (&vo)[3]) {
#pragma clang fp contract(off)
    double R[9], ei[3], ej[3], oc[3];
#pragma unroll
    for (int a = 0; a < 9; ++a) R[a] = st[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) ei[a] = pl[a], ej[a] = pl[3 + a], oc[a] = pl[6 + a] - pl[9 + a];
    align_rot_apply(R, ei, vi);
    align_rot_apply(R, ej, vj);
    align_rot_apply(R, oc, vo);
}

// rigid_maps3's formula (mri_inr_amd/align_volume.py) for one state: fp64, the Z row over the spacing, rounded once per entry
__device__ __forceinline__ void align_rigid_map3(const double (&st)[12], const double (&pl)[12], double spacing, float* mp) {
#pragma clang fp contract(off)
    double vi[3], vj[3], vo[3];
    align_rigid_vectors3(st, pl, vi, vj, vo);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double tc = vo[r] + pl[9 + r];
        const double t = tc + st[9 + r];
        if (r == 0) mp[0] = (float)(vi[0] / spacing), mp[1] = (float)(vj[0] / spacing), mp[2] = (float)(t / spacing);
        else mp[3 * r] = (float)vi[r], mp[3 * r + 1] = (float)vj[r], mp[3 * r + 2] = (float)t;
    }
}

// B (N x Q), N = 9 or 11, Q = 6 or 8: d map / d (w, u) at the rigid state rb on the plane pl, rigid_jacobian3's entries (mri_inr_amd/align_volume.py):
// B[3 r + col][k] = (e_k x v_col)[r], v_col = v_i, v_j, v_o;  B[3 r + 2][3 + k] = [r == k];  the rows of Z over the spacing;  N = 11: then
// B[9][6] = B[10][7] = 1 for the intensity;  every other entry 0.  Both step kernels and align_group_project_kernel form their B here.
template <int N, int Q>
__device__ __forceinline__ void align_rigid_jacobian3(const double (&rb)[12], const double (&pl)[12], double spacing, double (&B)[N][Q]) {
#pragma clang fp contract(off)
    static_assert((N == 9 && Q == 6) || (N == 11 && Q == 8), "the map's nine over the motion's six, or both with the intensity's two");
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int k = 0; k < Q; ++k) B[a][k] = 0.0;
    double vi[3], vj[3], vo[3];
    align_rigid_vectors3(rb, pl, vi, vj, vo);
#pragma unroll
    for (int col = 0; col < 3; ++col) {
        const double v0 = col == 0 ? vi[0] : col == 1 ? vj[0] : vo[0];
        const double v1 = col == 0 ? vi[1] : col == 1 ? vj[1] : vo[1];
        const double v2 = col == 0 ? vi[2] : col == 1 ? vj[2] : vo[2];
        // e_0 x v = (0, -v2, v1);  e_1 x v = (v2, 0, -v0);  e_2 x v = (-v1, v0, 0)
        B[col][1] = v2 / spacing, B[col][2] = (-v1) / spacing;
        B[3 + col][0] = -v2, B[3 + col][2] = v0;
        B[6 + col][0] = v1, B[6 + col][1] = -v0;
    }
    B[2][3] = 1.0 / spacing, B[5][4] = 1.0, B[8][5] = 1.0;
    if (N == 11) B[N - 2][Q - 2] = 1.0, B[N - 1][Q - 1] = 1.0;
}

// the rigid state rt behind the step d = (w 3, u 3, ...) from the state rb, cayley_update's rule (mri_inr_amd/align_volume.py):
// Cayley: a = d[0:3] / 2, Cay = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a);  Rot' = Cay Rot, u' = u + d[3:6]
template <int Q>
__device__ __forceinline__ void align_cayley_update(const double (&d)[Q], const double (&rb)[12], double (&rt)[12]) {
#pragma clang fp contract(off)
    const double a0 = d[0] / 2.0, a1 = d[1] / 2.0, a2 = d[2] / 2.0;
    const double q0 = a0 * a0, q1 = a1 * a1, q2 = a2 * a2;
    const double q01 = q0 + q1, aa = q01 + q2;
    const double den = 1.0 + aa, sc = 1.0 - aa;
    const double t0 = 2.0 * a0, t1 = 2.0 * a1, t2 = 2.0 * a2;
    double C[3][3];
    C[0][0] = (sc + t0 * a0) / den, C[0][1] = (t0 * a1 - t2) / den, C[0][2] = (t0 * a2 + t1) / den;
    C[1][0] = (t1 * a0 + t2) / den, C[1][1] = (sc + t1 * a1) / den, C[1][2] = (t1 * a2 - t0) / den;
    C[2][0] = (t2 * a0 - t1) / den, C[2][1] = (t2 * a1 + t0) / den, C[2][2] = (sc + t2 * a2) / den;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p0 = C[r][0] * rb[c], p1 = C[r][1] * rb[3 + c], p2 = C[r][2] * rb[6 + c];
            const double s = p0 + p1;
            rt[3 * r + c] = s + p2;
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) rt[9 + a] = rb[9 + a] + d[3 + a];
}

// before the first evaluation: trial := best := the input (rigid: the map of the input state), lam := damping, nothing accepted
template <int MODE>
__global__ __launch_bounds__(256) void align_volume_solve_init_kernel(AlignVolumeSolveParams p, const float* __restrict__ maps_in, const double* __restrict__ rigid_in,
                                                                      double damping) {
#pragma clang fp contract(off)
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= p.m) return;
    float mp[9];
    double st[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) st[a] = 0.0;
    if (MODE == ALIGN_VOLUME_RIGID) {
        double pl[12];
#pragma unroll
        for (int a = 0; a < 12; ++a) st[a] = rigid_in[(size_t)q * 12 + a], pl[a] = p.planes[(size_t)q * 12 + a];
        align_rigid_map3(st, pl, p.spacing, mp);
    } else {
#pragma unroll
        for (int a = 0; a < 9; ++a) mp[a] = maps_in[(size_t)q * 9 + a];
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) p.trial[(size_t)q * 9 + a] = mp[a], p.best[(size_t)q * 9 + a] = mp[a];
#pragma unroll
    for (int a = 0; a < 12; ++a) p.rigid_trial[(size_t)q * 12 + a] = st[a], p.rigid_best[(size_t)q * 12 + a] = st[a];
#pragma unroll
    for (int a = 0; a < ALIGN_VOLUME_SUMS; ++a) p.sums_best[(size_t)q * ALIGN_VOLUME_SUMS + a] = 0.0;
    p.scal[(size_t)q * 3] = __builtin_inf(), p.scal[(size_t)q * 3 + 1] = __builtin_inf(), p.scal[(size_t)q * 3 + 2] = damping;
    p.cnt[(size_t)q * 2] = 0, p.cnt[(size_t)q * 2 + 1] = 0;
}

// behind evaluation k: accept or reject the trial, then propose the next one from the best map.  grid: ceil(m / 256) workgroups of 256.
// What the proposal does not need while the system is formed and solved (the best map, the rigid state, the plane) is read again from the state
// behind a compiler barrier instead of being held in registers across it: the 9 x 9 matrix, B and the 6 x 6 system fill the file.
template <int MODE>
__global__ __launch_bounds__(256) void align_volume_step_kernel(AlignVolumeSolveParams p) {
#pragma clang fp contract(off)
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= p.m) return;
    constexpr int P = MODE == ALIGN_VOLUME_RIGID ? 6 : 9;
    const double inf = __builtin_inf();
    double mean_best = p.scal[(size_t)q * 3], mean_first = p.scal[(size_t)q * 3 + 1], lam = p.scal[(size_t)q * 3 + 2];
    int accepted = p.cnt[(size_t)q * 2];
    const double* ev = p.sums + (size_t)q * ALIGN_VOLUME_SUMS;
    const double count = ev[0], cost = ev[1];
    {
        float trial[9];
#pragma unroll
        for (int a = 0; a < 9; ++a) trial[a] = p.trial[(size_t)q * 9 + a];
        if (p.trace) {
            double* tr = p.trace + ((size_t)p.k * p.m + q) * 11;
#pragma unroll
            for (int a = 0; a < 9; ++a) tr[a] = (double)trial[a];
            tr[9] = cost, tr[10] = count;
        }
    }
    const double mean = count >= (double)P ? cost / count : inf;
    const bool accept = align_lm_decide(p.k, mean, &mean_best, &mean_first, &lam, &accepted, p.down, p.up, p.lam_min, p.lam_max);
    if (accept) {  // best := trial, in the state
#pragma unroll
        for (int a = 0; a < ALIGN_VOLUME_SUMS; ++a) p.sums_best[(size_t)q * ALIGN_VOLUME_SUMS + a] = ev[a];
#pragma unroll
        for (int a = 0; a < 9; ++a) p.best[(size_t)q * 9 + a] = p.trial[(size_t)q * 9 + a];
#pragma unroll
        for (int a = 0; a < 12; ++a) p.rigid_best[(size_t)q * 12 + a] = p.rigid_trial[(size_t)q * 12 + a];
    }
    __asm__ volatile("" ::: "memory");
    double bs[ALIGN_VOLUME_SUMS];  // the sums at the best map
#pragma unroll
    for (int a = 0; a < ALIGN_VOLUME_SUMS; ++a) bs[a] = p.sums_best[(size_t)q * ALIGN_VOLUME_SUMS + a];
    const double count_best = bs[0];
    bool ok;
    float trial[9];
    if (MODE == ALIGN_VOLUME_AFFINE) {
        // A = H damped on its diagonal: H[a][b] = bs[11 + packed(a, b)] for a <= b
        double A[9][9], rhs[9], d[9];
        {
            int s = 11;
#pragma unroll
            for (int a = 0; a < 9; ++a)
#pragma unroll
                for (int b = a; b < 9; ++b, ++s) A[b][a] = bs[s], A[a][b] = bs[s];
        }
#pragma unroll
        for (int a = 0; a < 9; ++a) {
            const double h = A[a][a], lh = lam * h;
            A[a][a] = h + lh;
            rhs[a] = -0.5 * bs[2 + a];
        }
        ok = align_ldl_solve<9>(A, rhs, d);
#pragma unroll
        for (int a = 0; a < 9; ++a) trial[a] = (float)((double)p.best[(size_t)q * 9 + a] + d[a]);
    } else {
        double B[9][6];
        {
            double rb[12], pl[12];
#pragma unroll
            for (int a = 0; a < 12; ++a) rb[a] = p.rigid_best[(size_t)q * 12 + a], pl[a] = p.planes[(size_t)q * 12 + a];
            align_rigid_jacobian3<9, 6>(rb, pl, p.spacing, B);
        }
        double A[6][6], rhs[6], d[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < 9; ++a) {
                const double bg = B[a][k] * bs[2 + a];
                t = t + bg;
            }
            rhs[k] = -0.5 * t;
        }
        double H[9][9];
        {
            int s = 11;
#pragma unroll
            for (int a = 0; a < 9; ++a)
#pragma unroll
                for (int b = a; b < 9; ++b, ++s) H[a][b] = bs[s], H[b][a] = bs[s];
        }
        // H6 = B^T (H B), column by column: T[., r] = H B[., r], then A[k][r] = sum_a B[a][k] T[a][r] for k >= r (the triangle the solve reads)
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double Tc[9];
#pragma unroll
            for (int a = 0; a < 9; ++a) {
                double t = 0.0;
#pragma unroll
                for (int b = 0; b < 9; ++b) {
                    const double hb = H[a][b] * B[b][r];
                    t = t + hb;
                }
                Tc[a] = t;
            }
#pragma unroll
            for (int k = r; k < 6; ++k) {
                double t = 0.0;
#pragma unroll
                for (int a = 0; a < 9; ++a) {
                    const double bt = B[a][k] * Tc[a];
                    t = t + bt;
                }
                A[k][r] = t;
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double lh = lam * A[k][k];
            A[k][k] = A[k][k] + lh;
        }
        ok = align_ldl_solve<6>(A, rhs, d);
        __asm__ volatile("" ::: "memory");
        // align_cayley_update's expressions in line: through the function this instantiation, which fills the register file, spills four registers
        const double a0 = d[0] / 2.0, a1 = d[1] / 2.0, a2 = d[2] / 2.0;
        const double q0 = a0 * a0, q1 = a1 * a1, q2 = a2 * a2;
        const double q01 = q0 + q1, aa = q01 + q2;
        const double den = 1.0 + aa, sc = 1.0 - aa;
        const double t0 = 2.0 * a0, t1 = 2.0 * a1, t2 = 2.0 * a2;
        double C[3][3];
        C[0][0] = (sc + t0 * a0) / den, C[0][1] = (t0 * a1 - t2) / den, C[0][2] = (t0 * a2 + t1) / den;
        C[1][0] = (t1 * a0 + t2) / den, C[1][1] = (sc + t1 * a1) / den, C[1][2] = (t1 * a2 - t0) / den;
        C[2][0] = (t2 * a0 - t1) / den, C[2][1] = (t2 * a1 + t0) / den, C[2][2] = (sc + t2 * a2) / den;
        double rb[12], pl[12], rt[12];
#pragma unroll
        for (int a = 0; a < 12; ++a) rb[a] = p.rigid_best[(size_t)q * 12 + a], pl[a] = p.planes[(size_t)q * 12 + a];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double p0 = C[r][0] * rb[c], p1 = C[r][1] * rb[3 + c], p2 = C[r][2] * rb[6 + c];
                const double s = p0 + p1;
                rt[3 * r + c] = s + p2;
            }
#pragma unroll
        for (int a = 0; a < 3; ++a) rt[9 + a] = rb[9 + a] + d[3 + a];
        align_rigid_map3(rt, pl, p.spacing, trial);
#pragma unroll
        for (int a = 0; a < 12; ++a) p.rigid_trial[(size_t)q * 12 + a] = rt[a];
    }
    const int flags = (ok ? 0 : ALIGN_SINGULAR) | (mean_first == inf ? ALIGN_NO_OVERLAP : 0);
#pragma unroll
    for (int a = 0; a < 9; ++a) p.trial[(size_t)q * 9 + a] = trial[a];
    p.scal[(size_t)q * 3] = mean_best, p.scal[(size_t)q * 3 + 1] = mean_first, p.scal[(size_t)q * 3 + 2] = lam;
    p.cnt[(size_t)q * 2] = accepted, p.cnt[(size_t)q * 2 + 1] = flags;
    if (p.last) {
#pragma unroll
        for (int a = 0; a < 9; ++a) p.maps_out[(size_t)q * 9 + a] = p.best[(size_t)q * 9 + a];
        if (p.rigid_out) {
#pragma unroll
            for (int a = 0; a < 12; ++a) p.rigid_out[(size_t)q * 12 + a] = p.rigid_best[(size_t)q * 12 + a];
        }
        double* rp = p.report + (size_t)q * 6;
        rp[0] = (double)accepted, rp[1] = mean_first, rp[2] = mean_best, rp[3] = count_best, rp[4] = lam, rp[5] = (double)flags;
    }
}

}  // namespace msiren
