// Aligned target slices gathered back onto the stack's voxel grid (msiren_fuse_targets*): per output voxel a normalised,
// windowed bilinear read of every target whose plane passes within `thickness` of it.  The rule is include/msiren.h's, restated in numpy by
// mri_inr_amd/fuse.py (fuse_on_host): fp64 + - * /, contraction off, one rounding per operation, the associations written there -- the two agree
// bit for bit.
//
//   set-up   fuse_setup_kernel    one thread per target: the record of kFuseRecord doubles (fuse_plan.h, FuseRecordField: a, b, t, the Gram entries,
//                                 det, dt, the normal c, gain, bias, flags) into the stream's scratch, [flags]
//   gather   fuse_gather_kernel   one workgroup of 256 per 16 x 16 (y, x) tile of one slice z, one thread per voxel (fuse_tile_lane); the loop over the
//                                 targets is fuse_visit_targets, shared with solve_volume.hip.h's transpose; num and den stay in registers; no LDS, no
//                                 atomics, no barrier; voxels of a ragged tile outside (H, W) store nothing
// What the family shares on the device lives here and in project.hip.h: the record and the tile (fuse_plan.h), fuse_tile_lane, fuse_visit_targets (the
// voxel side: per voxel over the targets) and project_visit_voxels (the pixel side: per target pixel over the voxels).
#pragma once
#include <hip/hip_runtime.h>

#include "fuse_plan.h"

namespace msiren {

// maps (m, 9), intensity (m, 2) or null -> rec (m, kFuseRecord), flags (m) or null
__global__ __launch_bounds__(256) void fuse_setup_kernel(const float* __restrict__ maps, const float* __restrict__ intensity, double spacing, double thickness, int m,
                                                         double* __restrict__ rec, int* __restrict__ flags) {
#pragma clang fp contract(off)
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    const float* mp = maps + (size_t)q * 9;
    bool finite = true;
    for (int e = 0; e < 9; ++e) finite = finite && __builtin_isfinite(mp[e]);
    const double a0 = (double)mp[0] * spacing, a1 = (double)mp[3], a2 = (double)mp[6];
    const double b0 = (double)mp[1] * spacing, b1 = (double)mp[4], b2 = (double)mp[7];
    const double t0 = (double)mp[2] * spacing, t1 = (double)mp[5], t2 = (double)mp[8];
    const double G11 = ((a0 * a0) + (a1 * a1)) + (a2 * a2), G12 = ((a0 * b0) + (a1 * b1)) + (a2 * b2), G22 = ((b0 * b0) + (b1 * b1)) + (b2 * b2);
    const double det = (G11 * G22) - (G12 * G12), tt = thickness * thickness, dt = det * tt;
    const double c0 = (a1 * b2) - (a2 * b1), c1 = (a2 * b0) - (a0 * b2), c2 = (a0 * b1) - (a1 * b0);
    const float gf = intensity ? intensity[2 * q] : 1.f, bf = intensity ? intensity[2 * q + 1] : 0.f;
    int f = 0;
    if (!finite || !(det > 0) || !__builtin_isfinite(det)) f |= MSIREN_FUSE_DEGENERATE;
    if (!__builtin_isfinite(gf) || !__builtin_isfinite(bf) || gf == 0.f) f |= MSIREN_FUSE_BAD_INTENSITY;
    double* r = rec + (size_t)q * kFuseRecord;
    r[FUSE_A] = a0, r[FUSE_A + 1] = a1, r[FUSE_A + 2] = a2, r[FUSE_B] = b0, r[FUSE_B + 1] = b1, r[FUSE_B + 2] = b2, r[FUSE_T] = t0, r[FUSE_T + 1] = t1, r[FUSE_T + 2] = t2;
    r[FUSE_G11] = G11, r[FUSE_G12] = G12, r[FUSE_G22] = G22, r[FUSE_DET] = det, r[FUSE_DT] = dt, r[FUSE_C] = c0, r[FUSE_C + 1] = c1, r[FUSE_C + 2] = c2;
    r[FUSE_GAIN] = (double)gf, r[FUSE_BIAS] = (double)bf, r[FUSE_FLAGS] = (double)f;
    if (flags) flags[q] = f;
}

// One workgroup of 256 per kFuseTile x kFuseTile tile, the tile's column fastest in the flat grid of tiles_y tiles_x `outer` workgroups: the tile, the
// outer index (a slice of the grid, or a target) and the lane's row and column (a voxel's y, x or a pixel's pi, pj), which may lie beyond a ragged edge
struct FuseTileLane {
    int bx, by, outer, row, col;
};
__device__ __forceinline__ FuseTileLane fuse_tile_lane(int tiles_x, int tiles_y) {
    const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, outer = blockIdx.x / (tiles_x * tiles_y);
    return FuseTileLane{bx, by, outer, by * kFuseTile + (int)(threadIdx.x / kFuseTile), bx * kFuseTile + (int)(threadIdx.x & (kFuseTile - 1))};
}

__device__ __forceinline__ double fuse_min4(double a, double b, double c, double d) { return fmin(fmin(a, b), fmin(c, d)); }
__device__ __forceinline__ double fuse_max4(double a, double b, double c, double d) { return fmax(fmax(a, b), fmax(c, d)); }

// The loop over the targets of the lane's voxel (z = l.outer, y = l.row, x = l.col), for fuse_gather_kernel and solve_transpose_kernel: the flag test, the
// tile-level cull, then the rule's p, pa, pb, cp, i, j, k and contribution test.  For every target q that reaches the voxel, q ascending, it calls
// tap(r, k, at, gi, gj, fi, fj): r the record, `at` the flat index of the first of the four taps (the others at + 1, at + tw, at + tw + 1), and
// (gi gj, gi fj, fi gj, fi fj) their bilinear weights.  The bound m is a run-time one and record q is read with a wave-uniform index (scalar loads: the
// record sits in SGPRs).
// The tile-level cull, computed identically by every lane in front of the per-voxel work: at fixed z the computed cp, i and j of a voxel are within a
// rounding error of functions that are AFFINE in (y, x), whose extremes over the tile's rectangle are at its four corners.  With S the sum of the
// absolute products of the dot product at the corner farthest from t (every |p| of the tile is below its entries), the computed value of any voxel
// of the tile and of any corner differs from the affine function by less than 8 u S, u = 2^-53 (three products, two sums and p's own subtraction,
// each relative u; for i and j the two Gram products, their difference and the division on top, with S = (|G22| Sa + |G12| Sb) / det, which also
// bounds |i|).  The cull uses the margin 2^-40 S, 2^10 times that, and asks of the squared window 2^-40 relative on top:
//     window   all four corners' cp on one side of 0 and lo = min |cp| - margin > 0 and (lo lo) (1 - 2^-40) > dt:  then every voxel has
//              fl(fl(cp cp) / dt) >= 1, i.e. k <= 0
//     rows     max i + margin < 0 or min i - margin > th - 1;  columns likewise with j and tw
// A pair is skipped only then; a quantity of the test that is not finite skips nothing.  A skipped pair would have called no tap, so the cull is
// invisible in what either kernel sums (tests/test_gpu_fuse.py: the graze cases put cp cp = dt and i = th - 1 on tile corners).
template <class Tap>
__device__ __forceinline__ void fuse_visit_targets(const double* __restrict__ rec, int m, int th, int tw, const FuseTileLane& l, double spacing, Tap tap) {
#pragma clang fp contract(off)
    constexpr double MARGIN = 0x1p-40;
    const double v0 = (double)l.outer * spacing, vy = (double)l.row, vx = (double)l.col;
    const double yl = (double)(l.by * kFuseTile), yh = (double)(l.by * kFuseTile + kFuseTile - 1), xl = (double)(l.bx * kFuseTile), xh = (double)(l.bx * kFuseTile + kFuseTile - 1);
    const double th1 = (double)(th - 1), tw1 = (double)(tw - 1), th2 = (double)(th - 2), tw2 = (double)(tw - 2);
    const int Mt = th * tw;
    for (int q = 0; q < m; ++q) {
        const double* r = rec + (size_t)q * kFuseRecord;  // wave-uniform: scalar loads
        if (r[FUSE_FLAGS] != 0.0) continue;
        const double t0 = r[FUSE_T], t1 = r[FUSE_T + 1], t2 = r[FUSE_T + 2], c0 = r[FUSE_C], c1 = r[FUSE_C + 1], c2 = r[FUSE_C + 2], dt = r[FUSE_DT];
        const double p0 = v0 - t0;
        // ---- the tile-level cull: the same values in every lane ----
        const double pyl = yl - t1, pyh = yh - t1, pxl = xl - t2, pxh = xh - t2;
        const double pym = fmax(fabs(pyl), fabs(pyh)), pxm = fmax(fabs(pxl), fabs(pxh));
        {
            const double e0 = c0 * p0, eyl = c1 * pyl, eyh = c1 * pyh, exl = c2 * pxl, exh = c2 * pxh;
            const double k00 = (e0 + eyl) + exl, k01 = (e0 + eyl) + exh, k10 = (e0 + eyh) + exl, k11 = (e0 + eyh) + exh;
            const double S = (fabs(e0) + fabs(c1) * pym) + fabs(c2) * pxm, margin = S * MARGIN;
            const double lo_pos = fuse_min4(k00, k01, k10, k11) - margin, lo_neg = -(fuse_max4(k00, k01, k10, k11) + margin);
            const double lo = fmax(lo_pos, lo_neg);  // > 0: every voxel's |cp| is at least this
            const bool finite = __builtin_isfinite(((k00 + k01) + (k10 + k11)) + S);
            if (finite && lo > 0.0 && (lo * lo) * (1.0 - MARGIN) > dt) continue;
        }
        const double a0 = r[FUSE_A], a1 = r[FUSE_A + 1], a2 = r[FUSE_A + 2], b0 = r[FUSE_B], b1 = r[FUSE_B + 1], b2 = r[FUSE_B + 2];
        const double G11 = r[FUSE_G11], G12 = r[FUSE_G12], G22 = r[FUSE_G22], det = r[FUSE_DET];
        {
            const double ea = a0 * p0, eb = b0 * p0;
            const double ayl = a1 * pyl, ayh = a1 * pyh, axl = a2 * pxl, axh = a2 * pxh, byl = b1 * pyl, byh = b1 * pyh, bxl = b2 * pxl, bxh = b2 * pxh;
            const double pa00 = (ea + ayl) + axl, pa01 = (ea + ayl) + axh, pa10 = (ea + ayh) + axl, pa11 = (ea + ayh) + axh;
            const double pb00 = (eb + byl) + bxl, pb01 = (eb + byl) + bxh, pb10 = (eb + byh) + bxl, pb11 = (eb + byh) + bxh;
            const double Sa = (fabs(ea) + fabs(a1) * pym) + fabs(a2) * pxm, Sb = (fabs(eb) + fabs(b1) * pym) + fabs(b2) * pxm;
            const double mi = ((fabs(G22) * Sa + fabs(G12) * Sb) / det) * MARGIN, mj = ((fabs(G11) * Sb + fabs(G12) * Sa) / det) * MARGIN;
            const double i00 = ((G22 * pa00) - (G12 * pb00)) / det, i01 = ((G22 * pa01) - (G12 * pb01)) / det;
            const double i10 = ((G22 * pa10) - (G12 * pb10)) / det, i11 = ((G22 * pa11) - (G12 * pb11)) / det;
            const double j00 = ((G11 * pb00) - (G12 * pa00)) / det, j01 = ((G11 * pb01) - (G12 * pa01)) / det;
            const double j10 = ((G11 * pb10) - (G12 * pa10)) / det, j11 = ((G11 * pb11) - (G12 * pa11)) / det;
            const bool finite = __builtin_isfinite((((i00 + i01) + (i10 + i11)) + ((j00 + j01) + (j10 + j11))) + (mi + mj));
            const bool out_i = fuse_max4(i00, i01, i10, i11) + mi < 0.0 || fuse_min4(i00, i01, i10, i11) - mi > th1;
            const bool out_j = fuse_max4(j00, j01, j10, j11) + mj < 0.0 || fuse_min4(j00, j01, j10, j11) - mj > tw1;
            if (finite && (out_i || out_j)) continue;
        }
        // ---- the voxel ----
        const double p1 = vy - t1, p2 = vx - t2;
        const double pa = ((a0 * p0) + (a1 * p1)) + (a2 * p2), pb = ((b0 * p0) + (b1 * p1)) + (b2 * p2), cp = ((c0 * p0) + (c1 * p1)) + (c2 * p2);
        const double i = ((G22 * pa) - (G12 * pb)) / det, j = ((G11 * pb) - (G12 * pa)) / det;
        const double k = 1.0 - ((cp * cp) / dt);
        if (k > 0.0 && i >= 0.0 && i <= th1 && j >= 0.0 && j <= tw1) {
            const double fi0 = fmin(floor(i), th2), fj0 = fmin(floor(j), tw2);
            const double fi = i - fi0, fj = j - fj0, gi = 1.0 - fi, gj = 1.0 - fj;
            const int at = q * Mt + (int)fi0 * tw + (int)fj0;  // i0 <= th - 2, j0 <= tw - 2: the four taps are inside the target
            tap(r, k, at, gi, gj, fi, fj);
        }
    }
}

// targets (m, th, tw), weights (m, th, tw) or null, rec (m, kFuseRecord) -> volume (n, H, W) or null, coverage (n, H, W) or null.
// grid: tiles_y tiles_x n workgroups (fuse_tile_lane)
__global__ __launch_bounds__(256) void fuse_gather_kernel(const float* __restrict__ targets, const float* __restrict__ weights, const double* __restrict__ rec, int m,
                                                          int th, int tw, int H, int W, int tiles_x, int tiles_y, double spacing, double min_coverage,
                                                          float* __restrict__ volume, float* __restrict__ coverage) {
#pragma clang fp contract(off)
    const FuseTileLane l = fuse_tile_lane(tiles_x, tiles_y);
    const int z = l.outer, y = l.row, x = l.col;
    double num = 0.0, den = 0.0;
    fuse_visit_targets(rec, m, th, tw, l, spacing, [&](const double* r, double k, int at, double gi, double gj, double fi, double fj) {
        const double g = r[FUSE_GAIN], bias = r[FUSE_BIAS];
        const double beta[4] = {gi * gj, gi * fj, fi * gj, fi * fj};
        // unsigned, so that at + off stays one 32-bit add (the sum is below 2^30): a signed add inside this callable is split into a 64-bit offset
        // whose sign-extended tw costs the kernel two SGPRs over the 68 its code-object test records (LAB_NOTES.md section 34)
        const unsigned off[4] = {0u, 1u, (unsigned)tw, (unsigned)tw + 1u};
        double sn = 0.0, sd = 0.0;
#pragma unroll
        for (int tap = 0; tap < 4; ++tap) {
            const float T = targets[(int)(at + off[tap])];
            const float w = weights ? weights[(int)(at + off[tap])] : 1.f;
            if (__builtin_isfinite(T) && __builtin_isfinite(w) && w > 0.f) {
                const double bw = beta[tap] * (double)w;
                sn += bw * (((double)T - bias) / g);
                sd += bw;
            }
        }
        num += k * sn;
        den += k * sd;
    });
    if (y < H && x < W) {
        const size_t at = ((size_t)z * H + y) * W + x;
        if (volume) volume[at] = den > min_coverage ? (float)(num / den) : __builtin_nanf("");
        if (coverage) coverage[at] = (float)den;
    }
}

}  // namespace msiren
