// msiren_fuse_targets(_dev) (include/msiren.h): the aligned targets of the volume alignment calls gathered back onto the
// stack's voxel grid.  Kernels: fuse.hip.h; what the call refuses, its tiling and its scratch: fuse_plan.h.  No images, no trunk: the handle need not
// hold committed weights.
// msiren_project_volume(_dev): the way back, the stack gathered onto the targets' lattices with the same weights.  Kernels:
// project.hip.h (fuse_setup_kernel is shared: this is the one unit that includes fuse.hip.h); refusals, tiling, scratch and the box: project_plan.h.
// msiren_solve_volume(_dev): conjugate gradients on those two operators, the stack that best explains all targets.  Kernels:
// solve_volume.hip.h (fuse_setup_kernel and fuse_gather_kernel are reused as they are); refusals, scratch and the launch plan: solve_volume_plan.h.
#include "fuse.hip.h"
#include "fuse_plan.h"
#include "project.hip.h"
#include "project_plan.h"
#include "solve_volume.hip.h"
#include "solve_volume_plan.h"
#include "host_buffers.h"
#include "host_ctx.h"

using namespace mh;

static_assert(msiren::kFuseTile == msiren::FUSE_TILE && msiren::kFuseRecord == msiren::FUSE_RECORD, "fuse_plan.h and the kernels disagree");
static_assert(msiren::FUSE_DEGENERATE == MSIREN_FUSE_DEGENERATE && msiren::FUSE_BAD_INTENSITY == MSIREN_FUSE_BAD_INTENSITY, "the header and the kernels disagree");
static_assert(sizeof(msiren_fuse_opts) == 32, "msiren_fuse_opts is 32 bytes");
static_assert(msiren::kProjectTile == msiren::PROJECT_TILE && msiren::kProjectSums == 4, "project_plan.h and the kernels disagree");
static_assert(sizeof(msiren_solve_opts) == 40, "msiren_solve_opts is 40 bytes");
static_assert(msiren::SOLVE_TILE == msiren::kFuseTile && msiren::SOLVE_TILE == msiren::kProjectTile, "the solve's gathers use the tilings of fuse_plan.h and project_plan.h");

namespace {

int fuse_refusal(const msiren::FuseArgs& a) {
    char msg[256];
    return msiren::fuse_check(a, msg, sizeof msg) ? 0 : fail(MSIREN_E_INVALID, "%s", msg);
}

// the two kernels on the call's stream, one profile entry; every pointer is the device's, `a` has passed fuse_check
int fuse_on_stream(msiren_ctx* h, const Call& c, const msiren::FuseArgs& a) {
    int rc;
    auto& sc = h->sc[c.stream];
    const msiren::FuseLayout lay = msiren::fuse_layout(a.m);
    if (lay.total && (rc = ensure(h, sc.ragged, lay.total))) return rc;
    double* const rec = a.m > 0 ? (double*)((char*)sc.ragged.p + lay.records) : nullptr;
    const double spacing = a.opts ? a.opts->spacing : 1.0, thickness = a.opts ? a.opts->thickness : 1.0, min_coverage = a.opts ? a.opts->min_coverage : 0.0;
    const int64_t voxels = a.n * a.H * a.W;
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1))) return rc;
    if (a.m > 0) {
        hipLaunchKernelGGL(msiren::fuse_setup_kernel, dim3((unsigned)((a.m + 255) / 256)), dim3(256), 0, sc.s, (const float*)a.maps, (const float*)a.intensity, spacing,
                           thickness, (int)a.m, rec, (int*)a.flags);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(msiren::fuse_gather_kernel, dim3((unsigned)msiren::fuse_tiles(a.n, a.H, a.W)), dim3(256), 0, sc.s, (const float*)a.targets, (const float*)a.weights,
                       (const double*)rec, (int)a.m, a.th, a.tw, a.H, a.W, (int)msiren::fuse_tiles_x(a.W), (int)msiren::fuse_tiles_y(a.H), spacing, min_coverage,
                       (float*)a.volume, (float*)a.coverage);
    HIPCHK(hipGetLastError());
    return profile_end(h, c.stream, e1, voxels, "fuse_kernels");
}

int project_refusal(const msiren::ProjectArgs& a) {
    char msg[256];
    return msiren::project_check(a, msg, sizeof msg) ? 0 : fail(MSIREN_E_INVALID, "%s", msg);
}

// set-up, gather and (with targets) the residual and the sums on the call's stream, one profile entry; every pointer is the device's, `a` has passed
// project_check and a.m > 0
int project_on_stream(msiren_ctx* h, const Call& c, const msiren::ProjectArgs& a) {
    int rc;
    auto& sc = h->sc[c.stream];
    const msiren::ProjectLayout lay = msiren::project_layout(a.m, a.tw, a.stats != nullptr);
    if ((rc = ensure(h, sc.ragged, lay.total))) return rc;
    double* const rec = (double*)((char*)sc.ragged.p + lay.records);
    double* const columns = a.stats ? (double*)((char*)sc.ragged.p + lay.columns) : nullptr;
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1))) return rc;
    hipLaunchKernelGGL(msiren::fuse_setup_kernel, dim3((unsigned)((a.m + 255) / 256)), dim3(256), 0, sc.s, (const float*)a.maps, (const float*)a.intensity, a.opts->spacing,
                       a.opts->thickness, (int)a.m, rec, (int*)a.flags);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(msiren::project_gather_kernel, dim3((unsigned)msiren::project_tiles(a.m, a.th, a.tw)), dim3(256), 0, sc.s, (const float*)a.volume, (const double*)rec,
                       a.th, a.tw, (int)a.n, a.H, a.W, (int)msiren::project_tiles_x(a.tw), (int)msiren::project_tiles_y(a.th), a.opts->spacing, a.opts->thickness,
                       a.opts->min_coverage, (float*)a.simulated, (float*)a.coverage);
    HIPCHK(hipGetLastError());
    if (a.targets && (a.residual || a.stats)) {
        hipLaunchKernelGGL(msiren::project_stats_kernel, dim3((unsigned)a.m), dim3(256), 0, sc.s, (const float*)a.targets, (const float*)a.weights, (const float*)a.simulated,
                           a.th, a.tw, columns, (float*)a.residual, (double*)a.stats);
        HIPCHK(hipGetLastError());
    }
    return profile_end(h, c.stream, e1, a.m * a.th * a.tw, "project_kernels");
}

int solve_refusal(const msiren::SolveArgs& a) {
    char msg[256];
    return msiren::solve_check(a, msg, sizeof msg) ? 0 : fail(MSIREN_E_INVALID, "%s", msg);
}

// the whole solve on the call's stream, one profile entry; every pointer is the device's, `a` has passed solve_check.  The sequence of launches
// depends on m > 0, start, coverage and iterations alone (solve_volume_plan.h: solve_launches counts them): nothing is read back
int solve_on_stream(msiren_ctx* h, const Call& c, const msiren::SolveArgs& a) {
    using namespace msiren;
    int rc;
    auto& sc = h->sc[c.stream];
    const SolveLayout lay = solve_layout(a.m, a.th, a.tw, a.n, a.H, a.W);
    if ((rc = ensure(h, sc.ragged, lay.total))) return rc;
    char* const base = (char*)sc.ragged.p;
    double* const rec = a.m > 0 ? (double*)(base + lay.records) : nullptr;
    double *const x = (double*)(base + lay.x), *const r = (double*)(base + lay.r), *const p = (double*)(base + lay.p), *const q = (double*)(base + lay.q);
    double *const D = (double*)(base + lay.D), *const Wt = (double*)(base + lay.Wt), *const zz = (double*)(base + lay.z);
    double *const columns = (double*)(base + lay.columns), *const slices = (double*)(base + lay.slices), *const state = (double*)(base + lay.state);
    const msiren_solve_opts& o = *a.opts;
    const double cz = 1.0 / (o.spacing * o.spacing);
    const int n = (int)a.n, H = a.H, W = a.W, m = (int)a.m, voxels = n * H * W;
    const dim3 wg(256), tiles((unsigned)fuse_tiles(a.n, H, W)), pixels((unsigned)(m > 0 ? project_tiles(a.m, a.th, a.tw) : 0));
    const dim3 pointwise((unsigned)solve_pointwise_blocks(a.n, H, W)), dots((unsigned)solve_dot_blocks(a.n, W));
    const int tx = (int)fuse_tiles_x(W), ty = (int)fuse_tiles_y(H), ptx = (int)project_tiles_x(a.tw), pty = (int)project_tiles_y(a.th);
    float* const volume = (float*)a.volume;
    const float* const sup = a.start ? (const float*)a.start : volume;  // the support: the finite voxels of the start
    double* const history = (double*)a.history;
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1))) return rc;
#define MSIREN_SOLVE_LAUNCH(kernel, grid, ...)                              \
    do {                                                                    \
        hipLaunchKernelGGL(kernel, grid, wg, 0, sc.s, __VA_ARGS__);         \
        HIPCHK(hipGetLastError());                                          \
    } while (0)
    auto forward = [&](const double* v) -> int {  // z = (Wt (P v)) / D
        if (m > 0) MSIREN_SOLVE_LAUNCH(solve_forward_kernel, pixels, v, (const double*)rec, (const double*)D, (const double*)Wt, a.th, a.tw, n, H, W, ptx, pty, o.spacing, o.thickness, zz);
        return 0;
    };
    auto transpose = [&](const double* v, double* out) -> int {  // out = Pt z [+ lambda L v]
        MSIREN_SOLVE_LAUNCH(solve_transpose_kernel, tiles, (const double*)zz, (const double*)rec, sup, v, m, a.th, a.tw, n, H, W, tx, ty, o.spacing, o.lambda, cz, out);
        return 0;
    };
    auto dot = [&](const double* u, const double* v, int mode, int it) -> int {
        MSIREN_SOLVE_LAUNCH(solve_dot_kernel, dots, u, v, sup, n, H, W, columns);
        MSIREN_SOLVE_LAUNCH(solve_reduce_kernel, dim3(1), (const double*)columns, n, W, mode, it, slices, state, history);
        return 0;
    };
    if (m > 0) MSIREN_SOLVE_LAUNCH(fuse_setup_kernel, dim3((unsigned)((m + 255) / 256)), (const float*)a.maps, (const float*)a.intensity, o.spacing, o.thickness, m, rec, (int*)a.flags);
    if (!a.start || a.coverage)  // the start and / or the coverage: msiren_fuse_targets' gather, untouched
        MSIREN_SOLVE_LAUNCH(fuse_gather_kernel, tiles, (const float*)a.targets, (const float*)a.weights, (const double*)rec, m, a.th, a.tw, H, W, tx, ty, o.spacing, o.min_coverage,
                            a.start ? (float*)nullptr : volume, (float*)a.coverage);
    MSIREN_SOLVE_LAUNCH(solve_start_kernel, pointwise, sup, voxels, x);
    if (m > 0)
        MSIREN_SOLVE_LAUNCH(solve_coverage_kernel, pixels, sup, (const float*)a.targets, (const float*)a.weights, (const double*)rec, a.th, a.tw, n, H, W, ptx, pty, o.spacing,
                            o.thickness, o.min_coverage, D, Wt, zz);
    if ((rc = transpose(nullptr, r))) return rc;                     // r = Pt Omega tau
    if ((rc = forward(x)) || (rc = transpose(x, q))) return rc;      // q = A x
    MSIREN_SOLVE_LAUNCH(solve_residual_kernel, pointwise, (const double*)q, voxels, r, p);
    if ((rc = dot(r, r, SOLVE_REDUCE_FIRST, 0))) return rc;
    for (int it = 0; it < o.iterations; ++it) {
        if ((rc = forward(p)) || (rc = transpose(p, q))) return rc;  // q = A p
        if ((rc = dot(p, q, SOLVE_REDUCE_GAMMA, it))) return rc;
        MSIREN_SOLVE_LAUNCH(solve_update_xr_kernel, pointwise, (const double*)state, sup, (const double*)p, (const double*)q, voxels, x, r);
        if ((rc = dot(r, r, SOLVE_REDUCE_RHO, it))) return rc;
        MSIREN_SOLVE_LAUNCH(solve_update_p_kernel, pointwise, (const double*)state, sup, (const double*)r, voxels, p);
    }
    MSIREN_SOLVE_LAUNCH(solve_store_kernel, pointwise, (const double*)x, (const double*)state, sup, voxels, volume, (int*)a.stopped_at);
#undef MSIREN_SOLVE_LAUNCH
    return profile_end(h, c.stream, e1, (int64_t)voxels, "solve_volume_kernels");
}

}  // namespace

extern "C" {

int msiren_solve_volume_dev(msiren_handle h, const float* targets_dev, int64_t m, int32_t th, int32_t tw, const float* maps_dev, const float* weights_dev,
                            const float* intensity_dev, const msiren_solve_opts* opts, int64_t n, int32_t height, int32_t width, const float* start_dev, float* volume_dev,
                            float* coverage_dev, double* history_dev, int32_t* flags_dev, int32_t* stopped_at_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::SolveArgs a{targets_dev, m, th, tw, maps_dev, weights_dev, intensity_dev, opts, n, height, width, start_dev, volume_dev, coverage_dev, history_dev, flags_dev,
                              stopped_at_dev, true};
    if ((rc = solve_refusal(a))) return rc;  // (before the stream rotates)
    return solve_on_stream(h, dev_call(h), a);
}

int msiren_solve_volume(msiren_handle h, const float* targets_host, int64_t m, int32_t th, int32_t tw, const float* maps_host, const float* weights_host,
                        const float* intensity_host, const msiren_solve_opts* opts, int64_t n, int32_t height, int32_t width, const float* start_host, float* volume_host,
                        float* coverage_host, double* history_host, int32_t* flags_host, int32_t* stopped_at_host) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::SolveArgs host{targets_host, m, th, tw, maps_host, weights_host, intensity_host, opts, n, height, width, start_host, volume_host, coverage_host, history_host,
                                 flags_host, stopped_at_host, false};
    if ((rc = solve_refusal(host))) return rc;
    const Call c = make_call(h, true);
    const size_t nt = (size_t)(m > 0 ? m * th * tw : 0) * sizeof(float), nv = (size_t)n * height * width * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_t = io.in(targets_host, nt, HOST_COPY), i_m = io.in(maps_host, (size_t)m * 9 * sizeof(float), HOST_COPY), i_w = io.in(weights_host, nt, HOST_COPY);
    const int i_gb = io.in(intensity_host, (size_t)m * 2 * sizeof(float), HOST_COPY), i_s = io.in(start_host, nv, HOST_COPY);
    // the volume is copied: with start NULL it holds the fusion, which every kernel of the loop reads as the support
    const int o_v = io.out(volume_host, nv, HOST_COPY), o_c = io.out(coverage_host, nv, HOST_IN_PLACE);
    const int o_h = io.out(history_host, (size_t)(opts->iterations + 1) * 2 * sizeof(double), HOST_COPY), o_f = io.out(flags_host, (size_t)m * sizeof(int32_t), HOST_COPY);
    const int o_st = io.out(stopped_at_host, sizeof(int32_t), HOST_COPY);
    if ((rc = io.begin())) return rc;
    const msiren::SolveArgs dev{io.src<float>(i_t), m, th, tw, io.src<float>(i_m), io.src<float>(i_w), io.src<float>(i_gb), opts, n, height, width, io.src<float>(i_s),
                                io.dst<float>(o_v), io.dst<float>(o_c), io.dst<double>(o_h), io.dst<int32_t>(o_f), io.dst<int32_t>(o_st), true};
    if ((rc = solve_on_stream(h, c, dev))) return rc;
    return io.finish();
}

int msiren_project_volume_dev(msiren_handle h, const float* volume_dev, int64_t n, int32_t height, int32_t width, const float* maps_dev, const float* intensity_dev,
                              const msiren_fuse_opts* opts, int64_t m, int32_t th, int32_t tw, const float* targets_dev, const float* weights_dev, float* simulated_dev,
                              float* coverage_dev, float* residual_dev, double* stats_dev, int32_t* flags_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::ProjectArgs a{volume_dev, n, height, width, maps_dev, intensity_dev, opts, m, th, tw, targets_dev, weights_dev, simulated_dev, coverage_dev, residual_dev,
                                stats_dev, flags_dev, true};
    if ((rc = project_refusal(a))) return rc;  // (before the stream rotates)
    if (m == 0) return 0;                      // (no pixel: nothing to write)
    return project_on_stream(h, dev_call(h), a);
}

int msiren_project_volume(msiren_handle h, const float* volume_host, int64_t n, int32_t height, int32_t width, const float* maps_host, const float* intensity_host,
                          const msiren_fuse_opts* opts, int64_t m, int32_t th, int32_t tw, const float* targets_host, const float* weights_host, float* simulated_host,
                          float* coverage_host, float* residual_host, double* stats_host, int32_t* flags_host) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::ProjectArgs host{volume_host, n, height, width, maps_host, intensity_host, opts, m, th, tw, targets_host, weights_host, simulated_host, coverage_host,
                                   residual_host, stats_host, flags_host, false};
    if ((rc = project_refusal(host))) return rc;
    if (m == 0) return 0;
    const Call c = make_call(h, true);
    const size_t nt = (size_t)m * th * tw * sizeof(float), nv = (size_t)n * height * width * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_v = io.in(volume_host, nv, HOST_COPY), i_m = io.in(maps_host, (size_t)m * 9 * sizeof(float), HOST_COPY);
    const int i_gb = io.in(intensity_host, (size_t)m * 2 * sizeof(float), HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY), i_w = io.in(weights_host, nt, HOST_COPY);
    const int o_s = io.out(simulated_host, nt, HOST_COPY), o_c = io.out(coverage_host, nt, HOST_IN_PLACE), o_r = io.out(residual_host, nt, HOST_IN_PLACE);
    const int o_st = io.out(stats_host, (size_t)m * 4 * sizeof(double), HOST_COPY), o_f = io.out(flags_host, (size_t)m * sizeof(int32_t), HOST_COPY);
    if ((rc = io.begin())) return rc;
    const msiren::ProjectArgs dev{io.src<float>(i_v), n, height, width, io.src<float>(i_m), io.src<float>(i_gb), opts, m, th, tw, io.src<float>(i_t), io.src<float>(i_w),
                                  io.dst<float>(o_s), io.dst<float>(o_c), io.dst<float>(o_r), io.dst<double>(o_st), io.dst<int32_t>(o_f), true};
    if ((rc = project_on_stream(h, c, dev))) return rc;
    return io.finish();
}

int msiren_fuse_targets_dev(msiren_handle h, const float* targets_dev, int64_t m, int32_t th, int32_t tw, const float* maps_dev, const float* weights_dev,
                            const float* intensity_dev, const msiren_fuse_opts* opts, int64_t n, int32_t height, int32_t width, float* volume_dev, float* coverage_dev,
                            int32_t* flags_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::FuseArgs a{targets_dev, m, th, tw, maps_dev, weights_dev, intensity_dev, opts, n, height, width, volume_dev, coverage_dev, flags_dev, true};
    if ((rc = fuse_refusal(a))) return rc;  // (before the stream rotates)
    if (!volume_dev && !coverage_dev) return 0;  // (m = 0 without an output)
    return fuse_on_stream(h, dev_call(h), a);
}

int msiren_fuse_targets(msiren_handle h, const float* targets_host, int64_t m, int32_t th, int32_t tw, const float* maps_host, const float* weights_host,
                        const float* intensity_host, const msiren_fuse_opts* opts, int64_t n, int32_t height, int32_t width, float* volume_host, float* coverage_host,
                        int32_t* flags_host) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::FuseArgs host{targets_host, m, th, tw, maps_host, weights_host, intensity_host, opts, n, height, width, volume_host, coverage_host, flags_host, false};
    if ((rc = fuse_refusal(host))) return rc;
    if (!volume_host && !coverage_host) return 0;
    const Call c = make_call(h, true);
    const size_t nt = (size_t)(m > 0 ? m * th * tw : 0) * sizeof(float), nv = (size_t)n * height * width * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_t = io.in(targets_host, nt, HOST_COPY), i_m = io.in(maps_host, (size_t)m * 9 * sizeof(float), HOST_COPY), i_w = io.in(weights_host, nt, HOST_COPY);
    const int i_gb = io.in(intensity_host, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int o_v = io.out(volume_host, nv, HOST_IN_PLACE), o_c = io.out(coverage_host, nv, HOST_IN_PLACE), o_f = io.out(flags_host, (size_t)m * sizeof(int32_t), HOST_COPY);
    if ((rc = io.begin())) return rc;
    const msiren::FuseArgs dev{io.src<float>(i_t), m, th, tw, io.src<float>(i_m), io.src<float>(i_w), io.src<float>(i_gb), opts, n, height, width, io.dst<float>(o_v),
                               io.dst<float>(o_c), io.dst<int32_t>(o_f), true};
    if ((rc = fuse_on_stream(h, c, dev))) return rc;
    return io.finish();
}

}  // extern "C"
