// msiren_project_volume(_dev) on the host side, plain C++ without HIP (unit-tested on the CPU by tests/test_project_reference.py):
// what the call refuses before any launch, its tiling, its block of the stream's scratch
//     [records m x 20 doubles]     fuse_plan.h's, written by fuse_setup_kernel
//     [column sums m x tw x 4]     doubles, only when stats are asked for: project_stats_kernel parks (count, sum w, sum w r, sum w r r) per column
// and the BOX of voxels that project_gather_kernel visits per target pixel (also compiled into the kernel: MSIREN_HD).
//
// The box.  Pixel (pi, pj) of a target sits at x = t + a pi + b pj.  A voxel v that adds a term to the pixel has (pi, pj) among its four taps, so its
// computed in-plane coordinates obey |i - pi| <= 1 and |j - pj| <= 1 (i0 <= i <= i0 + 1 with i0 = min(floor i, th - 2), and pi is i0 or i0 + 1), and it
// passed the window: k > 0, i.e. cp cp < dt.  In exact arithmetic v - t = a i + b j + nhat d with nhat = c / |c|, |c|^2 = det (Lagrange) and |d| <
// thickness, so on every axis e
//     |v_e - x_e| <= R_e = |a_e| + |b_e| + |c_e| thickness / sqrt(det)                                            (pixels; axis 0 / spacing: slices)
// The computed i, j, cp differ from the exact ones by rounding.  project_box pads R_e by the relative 2^-20 and by 2^-10 pixel, and vouches for that
// padding only where the plane is well conditioned and near: G11 G22 <= 2^10 det and every |p_e| of the grid <= 2^24.  Then det, the entries of c and
// the computed i, j and cp / sqrt(det) are each within 16 u kappa^2 |p| <= 2^-49 2^10 2^24 = 2^-15 (u = 2^-53) of the exact ones, in pixels or relative,
// and the handful of such terms (two per coordinate, the pixel's own x, the division by spacing) stays far below the padding.  Where the condition
// fails, or any quantity of the box is not finite, project_box returns false and the whole grid is visited: nothing is skipped.
// The span along an axis of N voxels: count = floor(2 R) + 2 consecutive indices starting at floor(x - R) contain [x - R, x + R]; the start is then
// moved into [0, N - count] (count >= N: the whole axis), which loses no index of the grid and leaves every visited index inside it.  The count
// depends on the target alone, so the three loops of a workgroup have wave-uniform trip counts.
#pragma once
#include <cmath>

#include "fuse_plan.h"

#if defined(__HIPCC__)
#define MSIREN_HD __host__ __device__
#else
#define MSIREN_HD
#endif

namespace msiren {

constexpr int kProjectTile = kFuseTile;  // target pixels per tile edge: the targets' lattices are tiled as the voxel grid is
constexpr int kProjectSums = 4;    // doubles per column: count, sum w, sum w r, sum (w r) r

// the radii without padding, in voxels of each axis (axis 0 in slices): what the proof above calls R
MSIREN_HD inline void project_radius(const double* r, double thickness, double spacing, double R[3]) {
    const double s = thickness / std::sqrt(r[FUSE_DET]);
    R[0] = ((std::fabs(r[FUSE_A + 0]) + std::fabs(r[FUSE_B + 0])) + std::fabs(r[FUSE_C + 0]) * s) / spacing;
    R[1] = (std::fabs(r[FUSE_A + 1]) + std::fabs(r[FUSE_B + 1])) + std::fabs(r[FUSE_C + 1]) * s;
    R[2] = (std::fabs(r[FUSE_A + 2]) + std::fabs(r[FUSE_B + 2])) + std::fabs(r[FUSE_C + 2]) * s;
}

// true: R holds the padded radii and every voxel outside them adds nothing to the pixel.  false: visit the whole grid.
MSIREN_HD inline bool project_box(const double* r, double thickness, double spacing, int n, int H, int W, double R[3]) {
    project_radius(r, thickness, spacing, R);
    const double far0 = std::fmax(std::fabs(r[FUSE_T + 0]), std::fabs((double)(n - 1) * spacing - r[FUSE_T + 0]));
    const double far1 = std::fmax(std::fabs(r[FUSE_T + 1]), std::fabs((double)(H - 1) - r[FUSE_T + 1]));
    const double far2 = std::fmax(std::fabs(r[FUSE_T + 2]), std::fabs((double)(W - 1) - r[FUSE_T + 2]));
    const double far = std::fmax(far0, std::fmax(far1, far2));
    const bool well = r[FUSE_G11] * r[FUSE_G22] <= 0x1p10 * r[FUSE_DET] && far <= 0x1p24;  // (a NaN fails both)
    R[0] = (R[0] * (1.0 + 0x1p-20)) + 0x1p-10 / spacing;
    R[1] = (R[1] * (1.0 + 0x1p-20)) + 0x1p-10;
    R[2] = (R[2] * (1.0 + 0x1p-20)) + 0x1p-10;
    return well && R[0] < 0x1p30 && R[1] < 0x1p30 && R[2] < 0x1p30;  // (finite, and floor(2 R) + 2 fits an int)
}

// how many consecutive voxels of an axis of N a pixel visits: the same for every pixel of the target
MSIREN_HD inline int project_count(bool boxed, double R, int N) {
    if (!boxed) return N;
    const double c = std::floor(2.0 * R) + 2.0;
    return c < (double)N ? (int)c : N;
}

// the first of them for the pixel at x (in voxels of the axis): floor(x - R) moved into [0, N - count]
MSIREN_HD inline int project_base(double x, double R, int N, int count) {
    if (count >= N) return 0;
    const double lo = std::floor(x - R);
    return (int)std::fmin(std::fmax(lo, 0.0), (double)(N - count));  // (fmax(NaN, 0) = 0: inside the grid whatever x is)
}

struct ProjectLayout {
    size_t records;   // offset of the records
    size_t columns;   // offset of the column sums
    size_t total;     // bytes of the call's block
};
inline ProjectLayout project_layout(int64_t m, int32_t tw, bool stats) {
    const size_t rec = fuse_records_bytes(m);
    const size_t col = stats && m > 0 ? (size_t)m * (size_t)tw * kProjectSums * sizeof(double) : 0;
    return ProjectLayout{0, rec, rec + col};
}

// fuse_plan.h's tile counts under the names of the lattice they count here
inline int64_t project_tiles_y(int32_t th) { return fuse_tiles_y(th); }
inline int64_t project_tiles_x(int32_t tw) { return fuse_tiles_x(tw); }
inline int64_t project_tiles(int64_t m, int32_t th, int32_t tw) { return fuse_tiles(m, th, tw); }

// What one call is given.  `device`: the pointers are device pointers, whose alignment is checked.
struct ProjectArgs {
    const void* volume;
    int64_t n;
    int32_t H, W;
    const void *maps, *intensity;
    const msiren_fuse_opts* opts;
    int64_t m;
    int32_t th, tw;
    const void *targets, *weights, *simulated, *coverage, *residual, *stats, *flags;
    bool device;
};

// true: the call is accepted.  false: `msg` names the argument that is refused.
inline bool project_check(const ProjectArgs& a, char* msg, size_t cap) {
#define MSIREN_PROJECT_REFUSE(...) return std::snprintf(msg, cap, __VA_ARGS__), false
    if (!fuse_check_sizes(a.m, a.th, a.tw, a.opts, a.n, a.H, a.W, msg, cap)) return false;
    if (a.m > 0 && !a.volume) MSIREN_PROJECT_REFUSE("null argument (volume)");
    if (a.m > 0 && !a.maps) MSIREN_PROJECT_REFUSE("null argument (maps)");
    if (a.m > 0 && !a.simulated) MSIREN_PROJECT_REFUSE("null argument (simulated)");
    if (!a.targets && a.weights) MSIREN_PROJECT_REFUSE("weights given without targets");
    if (!a.targets && a.residual) MSIREN_PROJECT_REFUSE("residual asked for without targets");
    if (!a.targets && a.stats) MSIREN_PROJECT_REFUSE("stats asked for without targets");
    if (a.device) {
        const struct { const void* p; const char* name; } ptrs[] = {{a.volume, "volume"}, {a.maps, "maps"}, {a.intensity, "intensity"}, {a.targets, "targets"},
                                                                    {a.weights, "weights"}, {a.simulated, "simulated"}, {a.coverage, "coverage"}, {a.residual, "residual"},
                                                                    {a.flags, "flags"}};
        for (const auto& e : ptrs)
            if ((uintptr_t)e.p % 4) MSIREN_PROJECT_REFUSE("device %s must be 4-byte aligned", e.name);
        if ((uintptr_t)a.stats % 8) MSIREN_PROJECT_REFUSE("device stats must be 8-byte aligned");
    }
#undef MSIREN_PROJECT_REFUSE
    return true;
}

}  // namespace msiren
