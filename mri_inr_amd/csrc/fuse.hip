// msiren_fuse_targets(_dev) (include/msiren.h): the aligned targets of the volume alignment calls gathered back onto the
// stack's voxel grid.  Kernels: fuse.hip.h; what the call refuses, its tiling and its scratch: fuse_plan.h.  No images, no trunk: the handle need not
// hold committed weights.
// msiren_project_volume(_dev): the way back, the stack gathered onto the targets' lattices with the same weights.  Kernels:
// project.hip.h; refusals, scratch and the box: project_plan.h.
// msiren_solve_volume(_dev): conjugate gradients on those two operators, the stack that best explains all targets.  Kernels:
// solve_volume.hip.h; refusals, scratch and the launch plan: solve_volume_plan.h.
// msiren_solve_volume_r(_dev): rounds of that solve, each reweighted by the Geman-McClure weight of the pixels' residuals
// against the current iterate.  Kernels: solve_volume_r.hip.h and, launched as they are, solve_volume.hip.h's; refusals, scratch, the schedule and
// the launch plan: solve_volume_r_plan.h.
// msiren_leave_out_targets(_dev): every target predicted from the fusion of the targets outside its own group.  Kernels:
// leave_out.hip.h and, launched as they are, fuse_setup_kernel and project_stats_kernel; refusals, scratch and the launch count: leave_out_plan.h.
// The calls share the record of fuse_setup_kernel, the tiling and the two loops (fuse_visit_targets, project_visit_voxels), and on this side
// the refusal, the checked launch and the launches of the set-up and of the fusion below.
#include "solve_volume_r.hip.h"  // (and through it solve_volume.hip.h, project.hip.h, fuse.hip.h and the four plans)
#include "leave_out.hip.h"
#include "host_buffers.h"
#include "host_ctx.h"

using namespace mh;

static_assert(sizeof(msiren_fuse_opts) == 32, "msiren_fuse_opts is 32 bytes");
static_assert(msiren::kProjectSums == 4, "project_stats_kernel parks four sums per column");
static_assert(sizeof(msiren_solve_opts) == 40, "msiren_solve_opts is 40 bytes");
static_assert(sizeof(msiren_solve_r_opts) == 56, "msiren_solve_r_opts is 56 bytes");
static_assert(msiren::kSolveRSums == 4, "irls_stats_kernel parks four sums per column");
static_assert(sizeof(msiren::LooOffsets) == 4 * msiren::kLooOffsets && msiren::kLooOffsets % 256 == 0, "loo_upload_kernel's argument and grid");

namespace {

// 0, or MSIREN_E_INVALID with the words of `check` (fuse_check, project_check, solve_check)
template <class Args>
int refusal(bool (*check)(const Args&, char*, size_t), const Args& a) {
    char msg[256];
    return check(a, msg, sizeof msg) ? 0 : fail(MSIREN_E_INVALID, "%s", msg);
}

// Kernels onto one stream in workgroups of 256, every launch checked: after one that failed nothing more is launched and `rc` is its code
struct Launcher {
    hipStream_t s;
    int rc = 0;
    template <class... P, class... A>
    void operator()(void (*kernel)(P...), dim3 grid, A... args) {
        if (!rc) rc = launch(kernel, grid, args...);
    }

private:
    template <class... P, class... A>
    int launch(void (*kernel)(P...), dim3 grid, A... args) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, args...);
        HIPCHK(hipGetLastError());
        return 0;
    }
};

// the records of m > 0 targets into `rec`, [flags]
void launch_setup(Launcher& go, const void* maps, const void* intensity, double spacing, double thickness, int64_t m, double* rec, const void* flags) {
    if (m > 0) go(msiren::fuse_setup_kernel, dim3((unsigned)((m + 255) / 256)), (const float*)maps, (const float*)intensity, spacing, thickness, (int)m, rec, (int*)flags);
}

// msiren_fuse_targets' gather: [volume], [coverage] (n, H, W)
void launch_fusion(Launcher& go, const void* targets, const void* weights, const double* rec, int64_t m, int32_t th, int32_t tw, int64_t n, int32_t H, int32_t W,
                   double spacing, double min_coverage, float* volume, float* coverage) {
    go(msiren::fuse_gather_kernel, dim3((unsigned)msiren::fuse_tiles(n, H, W)), (const float*)targets, (const float*)weights, rec, (int)m, th, tw, H, W,
       (int)msiren::fuse_tiles_x(W), (int)msiren::fuse_tiles_y(H), spacing, min_coverage, volume, coverage);
}

// the two kernels on the call's stream, one profile entry; every pointer is the device's, `a` has passed fuse_check
int fuse_on_stream(msiren_ctx* h, const Call& c, const msiren::FuseArgs& a) {
    int rc;
    auto& sc = h->sc[c.stream];
    const msiren::FuseLayout lay = msiren::fuse_layout(a.m);
    if (lay.total && (rc = ensure(h, sc.ragged, lay.total))) return rc;
    double* const rec = a.m > 0 ? (double*)((char*)sc.ragged.p + lay.records) : nullptr;
    const double spacing = a.opts ? a.opts->spacing : 1.0, thickness = a.opts ? a.opts->thickness : 1.0, min_coverage = a.opts ? a.opts->min_coverage : 0.0;
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1))) return rc;
    Launcher go{sc.s};
    launch_setup(go, a.maps, a.intensity, spacing, thickness, a.m, rec, a.flags);
    launch_fusion(go, a.targets, a.weights, rec, a.m, a.th, a.tw, a.n, a.H, a.W, spacing, min_coverage, (float*)a.volume, (float*)a.coverage);
    return go.rc ? go.rc : profile_end(h, c.stream, e1, a.n * a.H * a.W, "fuse_kernels");
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
    const msiren_fuse_opts& o = *a.opts;
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1))) return rc;
    Launcher go{sc.s};
    launch_setup(go, a.maps, a.intensity, o.spacing, o.thickness, a.m, rec, a.flags);
    go(msiren::project_gather_kernel, dim3((unsigned)msiren::project_tiles(a.m, a.th, a.tw)), (const float*)a.volume, (const double*)rec, a.th, a.tw, (int)a.n, a.H, a.W,
       (int)msiren::project_tiles_x(a.tw), (int)msiren::project_tiles_y(a.th), o.spacing, o.thickness, o.min_coverage, (float*)a.simulated, (float*)a.coverage);
    if (a.targets && (a.residual || a.stats))
        go(msiren::project_stats_kernel, dim3((unsigned)a.m), (const float*)a.targets, (const float*)a.weights, (const float*)a.simulated, a.th, a.tw, columns,
           (float*)a.residual, (double*)a.stats);
    return go.rc ? go.rc : profile_end(h, c.stream, e1, a.m * a.th * a.tw, "project_kernels");
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
    const dim3 tiles((unsigned)fuse_tiles(a.n, H, W)), pixels((unsigned)(m > 0 ? project_tiles(a.m, a.th, a.tw) : 0));
    const dim3 pointwise((unsigned)solve_pointwise_blocks(a.n, H, W)), dots((unsigned)solve_dot_blocks(a.n, W));
    const int tx = (int)fuse_tiles_x(W), ty = (int)fuse_tiles_y(H), ptx = (int)project_tiles_x(a.tw), pty = (int)project_tiles_y(a.th);
    float* const volume = (float*)a.volume;
    const float* const sup = a.start ? (const float*)a.start : volume;  // the support: the finite voxels of the start
    double* const history = (double*)a.history;
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1))) return rc;
    Launcher go{sc.s};
    auto forward = [&](const double* v) {  // z = (Wt (P v)) / D
        if (m > 0) go(solve_forward_kernel, pixels, v, (const double*)rec, (const double*)D, (const double*)Wt, a.th, a.tw, n, H, W, ptx, pty, o.spacing, o.thickness, zz);
    };
    auto transpose = [&](const double* v, double* out) {  // out = Pt z [+ lambda L v]
        go(solve_transpose_kernel, tiles, (const double*)zz, (const double*)rec, sup, v, m, a.th, a.tw, n, H, W, tx, ty, o.spacing, o.lambda, cz, out);
    };
    auto dot = [&](const double* u, const double* v, int mode, int it) {
        go(solve_dot_kernel, dots, u, v, sup, n, H, W, columns);
        go(solve_reduce_kernel, dim3(1), (const double*)columns, n, W, mode, it, slices, state, history);
    };
    launch_setup(go, a.maps, a.intensity, o.spacing, o.thickness, a.m, rec, a.flags);
    if (!a.start || a.coverage)  // the start and / or the coverage: msiren_fuse_targets' gather
        launch_fusion(go, a.targets, a.weights, rec, a.m, a.th, a.tw, a.n, H, W, o.spacing, o.min_coverage, a.start ? (float*)nullptr : volume, (float*)a.coverage);
    go(solve_start_kernel, pointwise, sup, voxels, x);
    if (m > 0)
        go(solve_coverage_kernel, pixels, sup, (const float*)a.targets, (const float*)a.weights, (const double*)rec, a.th, a.tw, n, H, W, ptx, pty, o.spacing, o.thickness,
           o.min_coverage, D, Wt, zz);
    transpose(nullptr, r);  // r = Pt Omega tau
    forward(x), transpose(x, q);  // q = A x
    go(solve_residual_kernel, pointwise, (const double*)q, voxels, r, p);
    dot(r, r, SOLVE_REDUCE_FIRST, 0);
    for (int it = 0; it < o.iterations; ++it) {
        forward(p), transpose(p, q);  // q = A p
        dot(p, q, SOLVE_REDUCE_GAMMA, it);
        go(solve_update_xr_kernel, pointwise, (const double*)state, sup, (const double*)p, (const double*)q, voxels, x, r);
        dot(r, r, SOLVE_REDUCE_RHO, it);
        go(solve_update_p_kernel, pointwise, (const double*)state, sup, (const double*)r, voxels, p);
    }
    go(solve_store_kernel, pointwise, (const double*)x, (const double*)state, sup, voxels, volume, (int*)a.stopped_at);
    return go.rc ? go.rc : profile_end(h, c.stream, e1, (int64_t)voxels, "solve_volume_kernels");
}

// the robust solve on the call's stream, one profile entry; every pointer is the device's, `a` has passed solve_r_check.  The sequence of launches
// depends on m > 0, start, coverage, rounds, iterations and whether a final pass is asked for (solve_volume_r_plan.h: solve_r_launches counts them):
// nothing is read back.  The schedule is computed here, in fp64, and handed to the reweighting kernel as a value
int solve_r_on_stream(msiren_ctx* h, const Call& c, const msiren::SolveRArgs& a) {
    using namespace msiren;
    int rc;
    auto& sc = h->sc[c.stream];
    const SolveRLayout lay = solve_r_layout(a.m, a.th, a.tw, a.n, a.H, a.W);
    if ((rc = ensure(h, sc.ragged, lay.total))) return rc;
    char* const base = (char*)sc.ragged.p;
    double* const rec = a.m > 0 ? (double*)(base + lay.base.records) : nullptr;
    double *const x = (double*)(base + lay.base.x), *const r = (double*)(base + lay.base.r), *const p = (double*)(base + lay.base.p), *const q = (double*)(base + lay.base.q);
    double *const D = (double*)(base + lay.base.D), *const Wt = (double*)(base + lay.base.Wt), *const zz = (double*)(base + lay.base.z);
    double *const columns = (double*)(base + lay.base.columns), *const slices = (double*)(base + lay.base.slices), *const state = (double*)(base + lay.base.state);
    double *const Wt0 = (double*)(base + lay.Wt0), *const zp = (double*)(base + lay.zp), *const stat_columns = (double*)(base + lay.stat_columns);
    const msiren_solve_r_opts& o = *a.opts;
    const double cz = 1.0 / (o.spacing * o.spacing);
    const int n = (int)a.n, H = a.H, W = a.W, m = (int)a.m, voxels = n * H * W;
    const dim3 tiles((unsigned)fuse_tiles(a.n, H, W)), pixels((unsigned)(m > 0 ? project_tiles(a.m, a.th, a.tw) : 0));
    const dim3 pointwise((unsigned)solve_pointwise_blocks(a.n, H, W)), dots((unsigned)solve_dot_blocks(a.n, W));
    const int tx = (int)fuse_tiles_x(W), ty = (int)fuse_tiles_y(H), ptx = (int)project_tiles_x(a.tw), pty = (int)project_tiles_y(a.th);
    float* const volume = (float*)a.volume;
    const float* const sup = a.start ? (const float*)a.start : volume;  // the support: the finite voxels of the start
    const bool final_pass = a.rweight || a.residual || a.stats;
    double factor[kSolveRMaxRounds];
    solve_r_schedule(o.rounds, o.anneal, factor);
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1))) return rc;
    Launcher go{sc.s};
    auto reweight = [&](double f, int last) {  // Wt, z, z' of x under the scales f scale; last: the final pass
        if (m > 0)
            go(irls_reweight_kernel, pixels, (const double*)x, (const float*)a.targets, (const double*)rec, (const double*)D, (const double*)Wt0, (const double*)a.scale, f, last,
               a.th, a.tw, n, H, W, ptx, pty, o.spacing, o.thickness, Wt, zz, zp, (float*)a.rweight, (float*)a.residual);
    };
    auto forward = [&](const double* v) {  // z = (Wt (P v)) / D
        if (m > 0) go(solve_forward_kernel, pixels, v, (const double*)rec, (const double*)D, (const double*)Wt, a.th, a.tw, n, H, W, ptx, pty, o.spacing, o.thickness, zz);
    };
    auto transpose = [&](const double* y, const double* v, double* out) {  // out = Pt y [+ lambda L v]
        go(solve_transpose_kernel, tiles, y, (const double*)rec, sup, v, m, a.th, a.tw, n, H, W, tx, ty, o.spacing, o.lambda, cz, out);
    };
    launch_setup(go, a.maps, a.intensity, o.spacing, o.thickness, a.m, rec, a.flags);
    if (!a.start || a.coverage)  // the start and / or the coverage: msiren_fuse_targets' gather
        launch_fusion(go, a.targets, a.weights, rec, a.m, a.th, a.tw, a.n, H, W, o.spacing, o.min_coverage, a.start ? (float*)nullptr : volume, (float*)a.coverage);
    go(solve_start_kernel, pointwise, sup, voxels, x);
    if (m > 0)  // D, the active pixels and Wt0 = (w g) g, once (its z is overwritten by the first reweighting pass)
        go(solve_coverage_kernel, pixels, sup, (const float*)a.targets, (const float*)a.weights, (const double*)rec, a.th, a.tw, n, H, W, ptx, pty, o.spacing, o.thickness,
           o.min_coverage, D, Wt0, zz);
    for (int t = 0; t < o.rounds; ++t) {
        double* const history = a.history ? (double*)a.history + (size_t)t * (o.iterations + 1) * 2 : nullptr;
        auto dot = [&](const double* u, const double* v, int mode, int it) {
            go(solve_dot_kernel, dots, u, v, sup, n, H, W, columns);
            go(solve_reduce_kernel, dim3(1), (const double*)columns, n, W, mode, it, slices, state, history);
        };
        reweight(factor[t], 0);
        transpose(zz, nullptr, r);  // r = Pt z
        transpose(zp, x, q);        // q = Pt z' + lambda L x = A x
        go(solve_residual_kernel, pointwise, (const double*)q, voxels, r, p);
        dot(r, r, SOLVE_REDUCE_FIRST, 0);  // (resets the stop state)
        for (int it = 0; it < o.iterations; ++it) {
            forward(p), transpose(zz, p, q);  // q = A p
            dot(p, q, SOLVE_REDUCE_GAMMA, it);
            go(solve_update_xr_kernel, pointwise, (const double*)state, sup, (const double*)p, (const double*)q, voxels, x, r);
            dot(r, r, SOLVE_REDUCE_RHO, it);
            go(solve_update_p_kernel, pointwise, (const double*)state, sup, (const double*)r, voxels, p);
        }
        go(irls_stop_kernel, dim3(1), (const double*)state, t, (int*)a.stopped_at);
    }
    if (final_pass) {
        reweight(1.0, 1);
        if (m > 0)
            go(irls_stats_kernel, dim3((unsigned)m), (const float*)a.weights, (const double*)Wt, (const double*)zz, (const double*)zp, a.th, a.tw, stat_columns,
               (double*)a.stats);
    }
    go(solve_store_kernel, pointwise, (const double*)x, (const double*)state, sup, voxels, volume, (int*)nullptr);
    return go.rc ? go.rc : profile_end(h, c.stream, e1, (int64_t)voxels, "solve_volume_r_kernels");
}

// the whole leave-out call on the call's stream, one profile entry; every pointer but opts and group_start is the device's, `a` has passed
// leave_out_check and has something to write.  The sequence of launches depends on m > 0, the number of groups and which outputs are given alone
// (leave_out_plan.h: leave_out_launches counts them): nothing is read back
int leave_out_on_stream(msiren_ctx* h, const Call& c, const msiren::LeaveOutArgs& a) {
    using namespace msiren;
    int rc;
    auto& sc = h->sc[c.stream];
    const int G = a.m > 0 ? (int)a.n_groups : 0;
    const LeaveOutLayout lay = leave_out_layout(a.m, a.tw, a.n_groups, a.n, a.H, a.W, a.stats != nullptr);
    if ((rc = ensure(h, sc.ragged, lay.total))) return rc;
    char* const base = (char*)sc.ragged.p;
    double* const rec = a.m > 0 ? (double*)(base + lay.records) : nullptr;
    int* const gs = G > 0 ? (int*)(base + lay.group_start) : nullptr;
    double2* const sums = (double2*)(base + lay.sums);
    double* const columns = a.stats && a.m > 0 ? (double*)(base + lay.columns) : nullptr;
    const double spacing = a.opts ? a.opts->spacing : 1.0, thickness = a.opts ? a.opts->thickness : 1.0, min_coverage = a.opts ? a.opts->min_coverage : 0.0;
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1))) return rc;
    Launcher go{sc.s};
    launch_setup(go, a.maps, a.intensity, spacing, thickness, a.m, rec, a.flags);
    // group_start: up to 512 offsets per launch, by value in the kernel's arguments (no copy from a host buffer that the caller may reuse, no sync)
    for (int64_t at = 0; at < (G > 0 ? (int64_t)G + 1 : 0); at += kLooOffsets) {
        LooOffsets off{};
        const int count = (int)std::min<int64_t>(kLooOffsets, (int64_t)G + 1 - at);
        for (int i = 0; i < count; ++i) off.v[i] = a.group_start[at + i];
        go(loo_upload_kernel, dim3(kLooOffsets / 256), off, gs, (int)at, count);
    }
    go(loo_sums_kernel, dim3((unsigned)fuse_tiles(a.n, a.H, a.W)), (const float*)a.targets, (const float*)a.weights, (const double*)rec, (int)a.m, a.th, a.tw, a.H, a.W,
       (int)fuse_tiles_x(a.W), (int)fuse_tiles_y(a.H), spacing, min_coverage, sums, (float*)a.volume, (float*)a.volume_coverage);
    if (a.m > 0) {
        go(loo_gather_kernel, dim3((unsigned)project_tiles(a.m, a.th, a.tw)), (const float*)a.targets, (const float*)a.weights, (const double*)rec, (const double2*)sums,
           (const int*)gs, G, a.th, a.tw, (int)a.n, a.H, a.W, (int)project_tiles_x(a.tw), (int)project_tiles_y(a.th), spacing, thickness, min_coverage, (float*)a.simulated,
           (float*)a.coverage);
        if (a.residual || a.stats)
            go(project_stats_kernel, dim3((unsigned)a.m), (const float*)a.targets, (const float*)a.weights, (const float*)a.simulated, a.th, a.tw, columns, (float*)a.residual,
               (double*)a.stats);
    }
    return go.rc ? go.rc : profile_end(h, c.stream, e1, a.m * a.th * a.tw, "leave_out_kernels");
}

// (m = 0 without the plain fusion: nothing to write)
bool leave_out_has_work(const msiren::LeaveOutArgs& a) { return a.m > 0 || a.volume || a.volume_coverage; }

}  // namespace

extern "C" {

int msiren_leave_out_targets_dev(msiren_handle h, const float* targets_dev, int64_t m, int32_t th, int32_t tw, const float* maps_dev, const float* weights_dev,
                                 const float* intensity_dev, const msiren_fuse_opts* opts, const int32_t* group_start, int64_t n_groups, int64_t n, int32_t height,
                                 int32_t width, float* simulated_dev, float* coverage_dev, float* residual_dev, double* stats_dev, int32_t* flags_dev, float* volume_dev,
                                 float* volume_coverage_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::LeaveOutArgs a{targets_dev, m, th, tw, maps_dev, weights_dev, intensity_dev, opts, group_start, n_groups, n, height, width, simulated_dev, coverage_dev,
                                 residual_dev, stats_dev, flags_dev, volume_dev, volume_coverage_dev, true};
    if ((rc = refusal(msiren::leave_out_check, a))) return rc;  // (before the stream rotates)
    if (!leave_out_has_work(a)) return 0;
    return leave_out_on_stream(h, dev_call(h), a);
}

int msiren_leave_out_targets(msiren_handle h, const float* targets_host, int64_t m, int32_t th, int32_t tw, const float* maps_host, const float* weights_host,
                             const float* intensity_host, const msiren_fuse_opts* opts, const int32_t* group_start, int64_t n_groups, int64_t n, int32_t height, int32_t width,
                             float* simulated_host, float* coverage_host, float* residual_host, double* stats_host, int32_t* flags_host, float* volume_host,
                             float* volume_coverage_host) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::LeaveOutArgs host{targets_host, m, th, tw, maps_host, weights_host, intensity_host, opts, group_start, n_groups, n, height, width, simulated_host,
                                    coverage_host, residual_host, stats_host, flags_host, volume_host, volume_coverage_host, false};
    if ((rc = refusal(msiren::leave_out_check, host))) return rc;
    if (!leave_out_has_work(host)) return 0;
    const Call c = make_call(h, true);
    const size_t nt = (size_t)(m > 0 ? m * th * tw : 0) * sizeof(float), nv = (size_t)n * height * width * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_t = io.in(targets_host, nt, HOST_COPY), i_m = io.in(maps_host, (size_t)m * 9 * sizeof(float), HOST_COPY), i_w = io.in(weights_host, nt, HOST_COPY);
    const int i_gb = io.in(intensity_host, (size_t)m * 2 * sizeof(float), HOST_COPY);
    // simulated is copied: project_stats_kernel reads it back
    const int o_s = io.out(simulated_host, nt, HOST_COPY), o_c = io.out(coverage_host, nt, HOST_IN_PLACE), o_r = io.out(residual_host, nt, HOST_IN_PLACE);
    const int o_st = io.out(stats_host, (size_t)m * 4 * sizeof(double), HOST_COPY), o_f = io.out(flags_host, (size_t)m * sizeof(int32_t), HOST_COPY);
    const int o_v = io.out(volume_host, nv, HOST_IN_PLACE), o_vc = io.out(volume_coverage_host, nv, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    const msiren::LeaveOutArgs dev{io.src<float>(i_t), m, th, tw, io.src<float>(i_m), io.src<float>(i_w), io.src<float>(i_gb), opts, group_start, n_groups, n, height, width,
                                   io.dst<float>(o_s), io.dst<float>(o_c), io.dst<float>(o_r), io.dst<double>(o_st), io.dst<int32_t>(o_f), io.dst<float>(o_v),
                                   io.dst<float>(o_vc), true};
    if ((rc = leave_out_on_stream(h, c, dev))) return rc;
    return io.finish();
}

int msiren_solve_volume_r_dev(msiren_handle h, const float* targets_dev, int64_t m, int32_t th, int32_t tw, const float* maps_dev, const float* weights_dev,
                              const float* intensity_dev, const double* scale_dev, const msiren_solve_r_opts* opts, int64_t n, int32_t height, int32_t width,
                              const float* start_dev, float* volume_dev, float* coverage_dev, double* history_dev, int32_t* flags_dev, int32_t* stopped_at_dev,
                              float* rweight_dev, float* residual_dev, double* stats_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::SolveRArgs a{targets_dev, m, th, tw, maps_dev, weights_dev, intensity_dev, scale_dev, opts, n, height, width, start_dev, volume_dev, coverage_dev,
                               history_dev, flags_dev, stopped_at_dev, rweight_dev, residual_dev, stats_dev, true};
    if ((rc = refusal(msiren::solve_r_check, a))) return rc;  // (before the stream rotates)
    return solve_r_on_stream(h, dev_call(h), a);
}

int msiren_solve_volume_r(msiren_handle h, const float* targets_host, int64_t m, int32_t th, int32_t tw, const float* maps_host, const float* weights_host,
                          const float* intensity_host, const double* scale_host, const msiren_solve_r_opts* opts, int64_t n, int32_t height, int32_t width,
                          const float* start_host, float* volume_host, float* coverage_host, double* history_host, int32_t* flags_host, int32_t* stopped_at_host,
                          float* rweight_host, double* stats_host) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::SolveRArgs host{targets_host, m, th, tw, maps_host, weights_host, intensity_host, scale_host, opts, n, height, width, start_host, volume_host, coverage_host,
                                  history_host, flags_host, stopped_at_host, rweight_host, nullptr, stats_host, false};
    if ((rc = refusal(msiren::solve_r_check, host))) return rc;
    const Call c = make_call(h, true);
    const size_t nt = (size_t)(m > 0 ? m * th * tw : 0) * sizeof(float), nv = (size_t)n * height * width * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_t = io.in(targets_host, nt, HOST_COPY), i_m = io.in(maps_host, (size_t)m * 9 * sizeof(float), HOST_COPY), i_w = io.in(weights_host, nt, HOST_COPY);
    const int i_gb = io.in(intensity_host, (size_t)m * 2 * sizeof(float), HOST_COPY), i_s = io.in(start_host, nv, HOST_COPY);
    const int i_sc = io.in(scale_host, (size_t)m * sizeof(double), HOST_COPY);
    // the volume is copied: with start NULL it holds the fusion, which every kernel of the loop reads as the support
    const int o_v = io.out(volume_host, nv, HOST_COPY), o_c = io.out(coverage_host, nv, HOST_IN_PLACE);
    const int o_h = io.out(history_host, (size_t)opts->rounds * (opts->iterations + 1) * 2 * sizeof(double), HOST_COPY);
    const int o_f = io.out(flags_host, (size_t)m * sizeof(int32_t), HOST_COPY), o_st = io.out(stopped_at_host, (size_t)opts->rounds * sizeof(int32_t), HOST_COPY);
    const int o_rw = io.out(rweight_host, nt, HOST_IN_PLACE), o_ss = io.out(stats_host, (size_t)m * 4 * sizeof(double), HOST_COPY);
    if ((rc = io.begin())) return rc;
    const msiren::SolveRArgs dev{io.src<float>(i_t), m, th, tw, io.src<float>(i_m), io.src<float>(i_w), io.src<float>(i_gb), io.src<double>(i_sc), opts, n, height, width,
                                 io.src<float>(i_s), io.dst<float>(o_v), io.dst<float>(o_c), io.dst<double>(o_h), io.dst<int32_t>(o_f), io.dst<int32_t>(o_st),
                                 io.dst<float>(o_rw), nullptr, io.dst<double>(o_ss), true};
    if ((rc = solve_r_on_stream(h, c, dev))) return rc;
    return io.finish();
}

int msiren_solve_volume_dev(msiren_handle h, const float* targets_dev, int64_t m, int32_t th, int32_t tw, const float* maps_dev, const float* weights_dev,
                            const float* intensity_dev, const msiren_solve_opts* opts, int64_t n, int32_t height, int32_t width, const float* start_dev, float* volume_dev,
                            float* coverage_dev, double* history_dev, int32_t* flags_dev, int32_t* stopped_at_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::SolveArgs a{targets_dev, m, th, tw, maps_dev, weights_dev, intensity_dev, opts, n, height, width, start_dev, volume_dev, coverage_dev, history_dev, flags_dev,
                              stopped_at_dev, true};
    if ((rc = refusal(msiren::solve_check, a))) return rc;  // (before the stream rotates)
    return solve_on_stream(h, dev_call(h), a);
}

int msiren_solve_volume(msiren_handle h, const float* targets_host, int64_t m, int32_t th, int32_t tw, const float* maps_host, const float* weights_host,
                        const float* intensity_host, const msiren_solve_opts* opts, int64_t n, int32_t height, int32_t width, const float* start_host, float* volume_host,
                        float* coverage_host, double* history_host, int32_t* flags_host, int32_t* stopped_at_host) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::SolveArgs host{targets_host, m, th, tw, maps_host, weights_host, intensity_host, opts, n, height, width, start_host, volume_host, coverage_host, history_host,
                                 flags_host, stopped_at_host, false};
    if ((rc = refusal(msiren::solve_check, host))) return rc;
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
    if ((rc = refusal(msiren::project_check, a))) return rc;  // (before the stream rotates)
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
    if ((rc = refusal(msiren::project_check, host))) return rc;
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
    if ((rc = refusal(msiren::fuse_check, a))) return rc;  // (before the stream rotates)
    if (!volume_dev && !coverage_dev) return 0;  // (m = 0 without an output)
    return fuse_on_stream(h, dev_call(h), a);
}

int msiren_fuse_targets(msiren_handle h, const float* targets_host, int64_t m, int32_t th, int32_t tw, const float* maps_host, const float* weights_host,
                        const float* intensity_host, const msiren_fuse_opts* opts, int64_t n, int32_t height, int32_t width, float* volume_host, float* coverage_host,
                        int32_t* flags_host) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::FuseArgs host{targets_host, m, th, tw, maps_host, weights_host, intensity_host, opts, n, height, width, volume_host, coverage_host, flags_host, false};
    if ((rc = refusal(msiren::fuse_check, host))) return rc;
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
