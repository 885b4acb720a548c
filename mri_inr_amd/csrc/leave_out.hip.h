// Every target predicted from the targets outside its own group (msiren_leave_out_targets*): the fusion's two sums per voxel
// formed once, and per target pixel a projection in which every voxel first takes the terms of the pixel's own group out of its sums.  The rule is
// include/msiren.h's, restated in numpy by mri_inr_amd/leave_out.py (leave_out_on_host): fp64 + - * /, contraction off, one rounding per operation -- the
// two agree bit for bit.  The per-target record is fuse_setup_kernel's; p, pa, pb, cp, i, j, k, i0, j0, fi, fj, the four beta, a tap's validity and the
// per-target terms k sn, k sd are fuse.hip.h's expressions; the box is project_plan.h's.
//
//   upload   loo_upload_kernel   up to 512 offsets of group_start, carried by value in the kernel's arguments -> the scratch (no host sync)
//   sums     loo_sums_kernel     one workgroup of 256 per 16 x 16 (y, x) tile of one slice through fuse_visit_targets with its cull: (num_v, den_v) as
//                                two doubles per voxel into the scratch, [volume], [volume_coverage] exactly as fuse_gather_kernel stores them
//   gather   loo_gather_kernel   one workgroup of 256 per 16 x 16 tile of one target's pixels, one thread per pixel (fuse_tile_lane); the record of q and
//                                its group [lo, hi) are wave-uniform.  Each thread visits the voxels of project_plan.h's box through loo_visit_voxels,
//                                project_visit_voxels' sibling that hands over the voxel and its tap BEFORE anyone asks whether the voxel takes part:
//                                that question costs the loop over the group's members at the voxel, so it is asked only of voxels that have the
//                                pixel among their taps.  The member loop has no tile cull (the voxels differ per lane); its trip count hi - lo is
//                                wave-uniform; the members' records are read through vector registers (below).  N and D stay in registers; no LDS, no atomics, no barrier;
//                                pixels of a ragged tile outside (th, tw) store nothing
// The residual and the four sums per target are project_stats_kernel's (project.hip.h), launched as it is.
// A member's terms at a voxel are computed by loo_member_terms with the expressions of fuse_visit_targets' voxel part and fuse_gather_kernel's tap loop, so
// that where a group is a voxel's only contributor its own sums ARE the voxel's sums (0.0 + x = x, the same order) and denL = 0 excludes it exactly.
#pragma once
#include <hip/hip_runtime.h>

#include "leave_out_plan.h"
#include "project.hip.h"

namespace msiren {

struct LooOffsets { int v[kLooOffsets]; };

// dst[base + i] = s.v[i] for i < count: group_start reaches the device in kernel arguments.  grid: 512 / 256 workgroups of 256.
__global__ __launch_bounds__(256) void loo_upload_kernel(LooOffsets s, int* __restrict__ dst, int base, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) dst[base + i] = s.v[i];
}

// targets, weights or null, rec -> sums (n, H, W, 2) = (num_v, den_v), [volume], [coverage] (n, H, W).  grid: tiles_y tiles_x n workgroups (fuse_tile_lane)
__global__ __launch_bounds__(256) void loo_sums_kernel(const float* __restrict__ targets, const float* __restrict__ weights, const double* __restrict__ rec, int m, int th,
                                                       int tw, int H, int W, int tiles_x, int tiles_y, double spacing, double min_coverage, double2* __restrict__ sums,
                                                       float* __restrict__ volume, float* __restrict__ coverage) {
#pragma clang fp contract(off)
    const FuseTileLane l = fuse_tile_lane(tiles_x, tiles_y);
    const int z = l.outer, y = l.row, x = l.col;
    double num = 0.0, den = 0.0;
    fuse_visit_targets(rec, m, th, tw, l, spacing, [&](const double* r, double k, int at, double gi, double gj, double fi, double fj) {
        const double g = r[FUSE_GAIN], bias = r[FUSE_BIAS];
        const double beta[4] = {gi * gj, gi * fj, fi * gj, fi * fj};
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
        sums[at] = make_double2(num, den);
        if (volume) volume[at] = den > min_coverage ? (float)(num / den) : __builtin_nanf("");
        if (coverage) coverage[at] = (float)den;
    }
}

// What the unflagged target with record r adds to (num_v, den_v) of the voxel at p = v - t ... (p0 = z spacing - t0 is formed here as fuse_visit_targets
// forms it): false where it does not contribute; else kn = k sn, kd = k sd.  `first`: the flat index of the target's pixel (0, 0)
__device__ __forceinline__ bool loo_member_terms(const double* r, const float* __restrict__ targets, const float* __restrict__ weights, int first, int th, int tw, double v0,
                                                 double vy, double vx, double* kn, double* kd) {
#pragma clang fp contract(off)
    // the window first, from seven of the record's twenty doubles: most members of a large group fail it at most voxels
    const double t0 = r[FUSE_T], t1 = r[FUSE_T + 1], t2 = r[FUSE_T + 2], c0 = r[FUSE_C], c1 = r[FUSE_C + 1], c2 = r[FUSE_C + 2], dt = r[FUSE_DT];
    const double th1 = (double)(th - 1), tw1 = (double)(tw - 1), th2 = (double)(th - 2), tw2 = (double)(tw - 2);
    const double p0 = v0 - t0, p1 = vy - t1, p2 = vx - t2;
    const double cp = ((c0 * p0) + (c1 * p1)) + (c2 * p2);
    const double k = 1.0 - ((cp * cp) / dt);
    if (!(k > 0.0)) return false;
    const double a0 = r[FUSE_A], a1 = r[FUSE_A + 1], a2 = r[FUSE_A + 2], b0 = r[FUSE_B], b1 = r[FUSE_B + 1], b2 = r[FUSE_B + 2];
    const double G11 = r[FUSE_G11], G12 = r[FUSE_G12], G22 = r[FUSE_G22], det = r[FUSE_DET];
    const double pa = ((a0 * p0) + (a1 * p1)) + (a2 * p2), pb = ((b0 * p0) + (b1 * p1)) + (b2 * p2);
    const double i = ((G22 * pa) - (G12 * pb)) / det, j = ((G11 * pb) - (G12 * pa)) / det;
    if (!(i >= 0.0 && i <= th1 && j >= 0.0 && j <= tw1)) return false;
    const double fi0 = fmin(floor(i), th2), fj0 = fmin(floor(j), tw2);
    const double fi = i - fi0, fj = j - fj0, gi = 1.0 - fi, gj = 1.0 - fj;
    const int at = first + (int)fi0 * tw + (int)fj0;  // i0 <= th - 2, j0 <= tw - 2: the four taps are inside the target
    const double g = r[FUSE_GAIN], bias = r[FUSE_BIAS];
    const double beta[4] = {gi * gj, gi * fj, fi * gj, fi * fj};
    const int off[4] = {0, 1, tw, tw + 1};
    double sn = 0.0, sd = 0.0;
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) {
        const float T = targets[at + off[tap]];
        const float w = weights ? weights[at + off[tap]] : 1.f;
        if (__builtin_isfinite(T) && __builtin_isfinite(w) && w > 0.f) {
            const double bw = beta[tap] * (double)w;
            sn += bw * (((double)T - bias) / g);
            sd += bw;
        }
    }
    *kn = k * sn, *kd = k * sd;
    return true;
}

// project_visit_voxels' sibling (project.hip.h: the box, the order z, y, x ascending, the window tested as cp cp < dt in front of the divisions, all
// as there and for the reasons given there): pair(z, y, x, at, k, beta) receives every voxel that contributes to the target and has pixel (pi, pj)
// among its four taps, with the window k and the pixel's bilinear weight beta -- whether the voxel takes part is the callable's business.
template <class Pair>
__device__ __forceinline__ void loo_visit_voxels(const double* r, int pi, int pj, int th, int tw, int n, int H, int W, double spacing, double thickness, Pair pair) {
#pragma clang fp contract(off)
    const double a0 = r[FUSE_A], a1 = r[FUSE_A + 1], a2 = r[FUSE_A + 2], b0 = r[FUSE_B], b1 = r[FUSE_B + 1], b2 = r[FUSE_B + 2];
    const double t0 = r[FUSE_T], t1 = r[FUSE_T + 1], t2 = r[FUSE_T + 2];
    const double G11 = r[FUSE_G11], G12 = r[FUSE_G12], G22 = r[FUSE_G22], det = r[FUSE_DET], dt = r[FUSE_DT], c0 = r[FUSE_C], c1 = r[FUSE_C + 1], c2 = r[FUSE_C + 2];
    double R[3];
    const bool boxed = project_box(r, thickness, spacing, n, H, W, R);
    const int nz = project_count(boxed, R[0], n), ny = project_count(boxed, R[1], H), nx = project_count(boxed, R[2], W);
    const double dpi = (double)pi, dpj = (double)pj;
    const int z0 = project_base(((t0 + a0 * dpi) + b0 * dpj) / spacing, R[0], n, nz);
    const int y0 = project_base((t1 + a1 * dpi) + b1 * dpj, R[1], H, ny);
    const int x0 = project_base((t2 + a2 * dpi) + b2 * dpj, R[2], W, nx);
    const double th1 = (double)(th - 1), tw1 = (double)(tw - 1), th2 = (double)(th - 2), tw2 = (double)(tw - 2);
    // what only the two outer loops read waits in VGPRs: 16 SGPRs less across the callable (the values are the same bits wherever they wait)
    double za = a0, zb = b0, zc = c0, zt = t0, ya = a1, yb = b1, yc = c1, yt = t1;
    asm("" : "+v"(za), "+v"(zb), "+v"(zc), "+v"(zt), "+v"(ya), "+v"(yb), "+v"(yc), "+v"(yt));
    for (int dz = 0; dz < nz; ++dz) {
        const int z = z0 + dz;  // 0 <= z0 and z0 + nz <= n (project_base): every index is inside the grid
        const double p0 = ((double)z * spacing) - zt;
        const double ea = za * p0, eb = zb * p0, ec = zc * p0;
        for (int dy = 0; dy < ny; ++dy) {
            const int y = y0 + dy;
            const double p1 = (double)y - yt;
            const double fa = ea + (ya * p1), fb = eb + (yb * p1), fc = ec + (yc * p1);
            const size_t row = ((size_t)z * H + y) * W;
            for (int dx = 0; dx < nx; ++dx) {
                const int x = x0 + dx;
                const double p2 = (double)x - t2;
                const double cp = fc + (c2 * p2), cc = cp * cp;
                if (!(cc < dt)) continue;  // k <= 0
                const double pa = fa + (a2 * p2), pb = fb + (b2 * p2);
                const double i = ((G22 * pa) - (G12 * pb)) / det, j = ((G11 * pb) - (G12 * pa)) / det;
                const double k = 1.0 - (cc / dt);
                if (k > 0.0 && i >= 0.0 && i <= th1 && j >= 0.0 && j <= tw1) {
                    const double fi0 = fmin(floor(i), th2), fj0 = fmin(floor(j), tw2);
                    const double di = dpi - fi0, dj = dpj - fj0;  // exact: small integers
                    if ((di == 0.0 || di == 1.0) && (dj == 0.0 || dj == 1.0)) {
                        const double fi = i - fi0, fj = j - fj0, gi = 1.0 - fi, gj = 1.0 - fj;
                        pair(z, y, x, row + x, k, (di == 0.0 ? gi : fi) * (dj == 0.0 ? gj : fj));
                    }
                }
            }
        }
    }
}

// targets, weights or null, rec, sums (n, H, W, 2), group_start (G + 1) or null (every target its own group) -> simulated (m, th, tw), coverage (m, th, tw)
// or null.  grid: tiles_y tiles_x m workgroups (fuse_tile_lane)
__global__ __launch_bounds__(256) void loo_gather_kernel(const float* __restrict__ targets, const float* __restrict__ weights, const double* __restrict__ rec,
                                                         const double2* __restrict__ sums, const int* __restrict__ group_start, int G, int th, int tw, int n, int H, int W,
                                                         int tiles_x, int tiles_y, double spacing, double thickness, double min_coverage, float* __restrict__ simulated,
                                                         float* __restrict__ coverage) {
#pragma clang fp contract(off)
    const FuseTileLane l = fuse_tile_lane(tiles_x, tiles_y);
    const int q = l.outer, pi = l.row, pj = l.col;
    const bool inside = pi < th && pj < tw;
    const size_t at = ((size_t)q * th + (inside ? pi : 0)) * tw + (inside ? pj : 0);
    const double* r = rec + (size_t)q * kFuseRecord;  // wave-uniform: scalar loads
    if (r[FUSE_FLAGS] != 0.0) {                       // a flagged target: NaN, coverage 0
        if (inside) {
            simulated[at] = __builtin_nanf("");
            if (coverage) coverage[at] = 0.f;
        }
        return;
    }
    int lo = q, hi = q + 1;  // the group of q: the last y with group_start[y] <= q.  The same in every lane
    if (group_start) {
        int a = 0, b = G;  // group_start[a] <= q < group_start[b]
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (group_start[mid] <= q) a = mid;
            else b = mid;
        }
        lo = group_start[a], hi = group_start[a + 1];
    }
    const int Mt = th * tw;
    double N = 0.0, D = 0.0;
    loo_visit_voxels(r, pi, pj, th, tw, n, H, W, spacing, thickness, [&](int z, int y, int x, size_t v, double k, double beta) {
        const double2 s = sums[v];  // (num_v, den_v)
        const double v0 = (double)z * spacing, vy = (double)y, vx = (double)x;
        double own_n = 0.0, own_d = 0.0;
        for (int qq = lo; qq < hi; ++qq) {
            const double* rr = rec + (size_t)qq * kFuseRecord;
            // the member's record goes through VGPRs: the record of q and the box already hold some 90 SGPRs across this loop, and a second record
            // beside them spilled 25 (LAB_NOTES.md section 42).  The pointer is the same in every lane, so each load is one broadcast line
            asm("" : "+v"(rr));
            if (rr[FUSE_FLAGS] != 0.0) continue;
            double kn, kd;
            if (loo_member_terms(rr, targets, weights, qq * Mt, th, tw, v0, vy, vx, &kn, &kd)) own_n += kn, own_d += kd;
        }
        const double numL = s.x - own_n, denL = s.y - own_d;
        if (denL > min_coverage && denL > s.y * MSIREN_LEAVE_OUT_FLOOR) {
            const double U = numL / denL, kb = k * beta;
            N += kb * U;
            D += kb;
        }
    });
    if (inside) {
        const double g = r[FUSE_GAIN], bias = r[FUSE_BIAS];
        simulated[at] = D > min_coverage ? (float)((g * (N / D)) + bias) : __builtin_nanf("");
        if (coverage) coverage[at] = (float)D;
    }
}

}  // namespace msiren
