// One coordinate set per patch (include/msiren.h): msiren_sample_ragged_* -- SirenNet.forward, and its spatial
// gradient, with patch b evaluated at coords[offsets[b] : offsets[b + 1]].  The exact-fp32 trunks, on handles of every precision
// (siren_trunk_f32_ragged.hip.h; the launches: launch_dispatch.hip): a layer-0 table per (patch, coordinate) would be 4 H bytes an entry.
// The *_native value forms run the handle's own trunk arithmetic instead, layer 0 computed in the kernel (launch_trunk_ragged_native).
// msiren_resample_slices*, msiren_resample_volume*, msiren_align_slices*, msiren_align_solve* and their weighted forms msiren_align_slices_w*,
// msiren_align_solve_w*, and msiren_align_volume*, msiren_align_volume_solve* (DESIGN.md sections 5.8 - 5.13) are built on these trunks: launch_dispatch.hip.
#include "host_buffers.h"
#include "host_ctx.h"

using namespace mh;

namespace {

// what both forms check before anything is enqueued; `grad`: the jet's limits on the model (jet_supported)
int check_ragged_args(msiren_ctx* h, const float* coords, const int32_t* offsets, const float* mods, int64_t B, int64_t T, const float* out, const float* grad_out,
                      bool grad, RaggedSet* r) {
    int rc = check(h);
    if (rc || (grad && (rc = jet_supported(h)))) return rc;
    if (!grad && h->HP > 512) return fail(MSIREN_E_INVALID, "dim_hidden=%d (padded %d) is not supported by the exact-fp32 trunks", h->H, h->HP);
    if (B < 0 || T < 0) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld, T=%lld)", (long long)B, (long long)T);
    *r = RaggedSet{coords, offsets, T, B, 1, nullptr, B, nullptr};
    if ((rc = ragged_check(*r, grad ? 32 : 64))) return rc;
    if (B > 0 && T > 0 && (!coords || !offsets || !mods || (grad ? !grad_out : !out))) return fail(MSIREN_E_INVALID, "null argument");
    return 0;
}

int ragged_dev(msiren_ctx* h, const float* coords_dev, const int32_t* offsets_dev, const float* mods_dev, int64_t B, int64_t T, float* out_dev, float* grad_dev, bool grad,
               bool native = false) {
    RaggedSet r;
    int rc = check_ragged_args(h, coords_dev, offsets_dev, mods_dev, B, T, out_dev, grad_dev, grad, &r);
    if (rc || B == 0 || T == 0) return rc;
    if ((rc = check_pairs_aligned(coords_dev, "coordinates"))) return rc;
    if ((uintptr_t)offsets_dev % 4) return fail(MSIREN_E_INVALID, "device offsets must be 4-byte aligned");
    const Call c = dev_call(h);
    auto& sc = h->sc[c.stream];
    if ((rc = ensure(h, sc.ragged, (size_t)(B + 1) * sizeof(int)))) return rc;
    r.items = (int*)sc.ragged.p;
    if (grad) return launch_trunk_f32_jet_ragged(h, c, r, mods_dev, out_dev, grad_dev, 1.0f);
    return native ? launch_trunk_ragged_native(h, c, r, mods_dev, out_dev) : launch_trunk_f32_ragged(h, c, r, mods_dev, out_dev);
}

// one synchronous one-chunk call on host pointers, as the sampling calls: coords + offsets + mods -> [out], [grad]
int ragged_host(msiren_ctx* h, const float* coords_host, const int32_t* offsets_host, const float* mods_host, int64_t B, int64_t T, float* out_host, float* grad_host,
                bool grad, bool native = false) {
    RaggedSet r;
    int rc = check_ragged_args(h, coords_host, offsets_host, mods_host, B, T, out_host, grad_host, grad, &r);
    if (rc || B == 0 || T == 0) return rc;
    if (offsets_host[0] != 0 || offsets_host[B] != T) return fail(MSIREN_E_INVALID, "offsets must run from 0 to T=%lld, got %d .. %d", (long long)T, offsets_host[0], offsets_host[B]);
    for (int64_t b = 0; b < B; ++b)
        if (offsets_host[b + 1] < offsets_host[b]) return fail(MSIREN_E_INVALID, "offsets must be non-decreasing: offsets[%lld] = %d > offsets[%lld] = %d", (long long)b, offsets_host[b], (long long)b + 1, offsets_host[b + 1]);
    Call c = make_call(h, true);
    auto& sc = h->sc[c.stream];
    const size_t nc = (size_t)T * 2 * sizeof(float), nf = (size_t)(B + 1) * sizeof(int), no = (size_t)T * sizeof(float);
    const size_t ni = (size_t)h->L * B * h->H * sizeof(float);
    if ((rc = ensure(h, sc.coords, nc)) || (rc = ensure(h, sc.ragged, 2 * nf))) return rc;
    int* const d_off = (int*)sc.ragged.p;  // [offsets (B + 1)][item table (B + 1)]
    SyncHostCall io(h, c.stream);
    const int i_c = io.in(coords_host, nc, HOST_COPY, sc.coords.p), i_off = io.in(offsets_host, nf, HOST_COPY, d_off);
    const int i_m = io.in(mods_host, ni, HOST_COPY);  // (modulations are read once per item: copied)
    const int o_out = io.out(out_host, no, HOST_IN_PLACE), o_grad = io.out(grad ? grad_host : nullptr, 2 * no, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    r.coords = io.src<float>(i_c), r.offsets = io.src<int>(i_off), r.items = d_off + (B + 1);
    if (grad) rc = launch_trunk_f32_jet_ragged(h, c, r, io.src<float>(i_m), io.dst<float>(o_out), io.dst<float>(o_grad), 1.0f);
    else if (native) rc = launch_trunk_ragged_native(h, c, r, io.src<float>(i_m), io.dst<float>(o_out));
    else rc = launch_trunk_f32_ragged(h, c, r, io.src<float>(i_m), io.dst<float>(o_out));
    if (rc || (rc = io.finish())) return rc;
    if (native) (void)take_range_flag(h);  // informational: a flagged call holds the exact-fp32 trunk's bits already
    return 0;
}

// the reconstruction at points, one synchronous one-chunk call on host pointers: images + points -> [out], [grad]
int resample_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* points_host, int64_t M, float* out_host,
                  float* grad_host, bool grad, bool native = false) {
    int rc = check(h);
    if (rc || (rc = resample_check(h, n, height, width, M, grad))) return rc;
    if (n == 0 || M == 0) return 0;
    if (!images_host || !points_host || (grad ? !grad_host : !out_host)) return fail(MSIREN_E_INVALID, "null argument");
    if (n * (int64_t)height * width > 0x1fffffffLL) return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld slices of %dx%d", (long long)n, height, width);
    Call c = make_call(h, true);
    auto& sc = h->sc[c.stream];
    const size_t ni = (size_t)n * height * width * sizeof(float), np = (size_t)M * 2 * sizeof(float), no = (size_t)n * M * sizeof(float);
    if ((rc = ensure(h, sc.coords, np))) return rc;
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_p = io.in(points_host, np, HOST_COPY, sc.coords.p);
    const int o_out = io.out(out_host, no, HOST_IN_PLACE), o_grad = io.out(grad ? grad_host : nullptr, 2 * no, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    if ((rc = resample_slices(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_p), M, io.dst<float>(o_out), io.dst<float>(o_grad), grad, native))) return rc;
    if ((rc = io.finish())) return rc;
    if (native) (void)take_range_flag(h);  // informational, as above
    return 0;
}

// a stack read as a volume at points (Z, Y, X), one synchronous one-chunk call on host pointers: images + points -> [out (M)], [grad (3, M)]
int volume_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* points_host, int64_t M, float* out_host,
                float* grad_host, bool grad, bool native = false) {
    int rc = check(h);
    if (rc || (rc = resample_volume_check(h, n, height, width, M, grad))) return rc;
    if (n == 0 || M == 0) return 0;
    if (!images_host || !points_host || (grad ? !grad_host : !out_host)) return fail(MSIREN_E_INVALID, "null argument");
    if (n * (int64_t)height * width > 0x1fffffffLL) return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld slices of %dx%d", (long long)n, height, width);
    Call c = make_call(h, true);
    auto& sc = h->sc[c.stream];
    const size_t ni = (size_t)n * height * width * sizeof(float), np = (size_t)M * 3 * sizeof(float), no = (size_t)M * sizeof(float);
    if ((rc = ensure(h, sc.coords, np))) return rc;
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_p = io.in(points_host, np, HOST_COPY, sc.coords.p);
    const int o_out = io.out(out_host, no, HOST_IN_PLACE), o_grad = io.out(grad ? grad_host : nullptr, 3 * no, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    if ((rc = resample_volume(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_p), M, io.dst<float>(o_out), io.dst<float>(o_grad), grad, native))) return rc;
    if ((rc = io.finish())) return rc;
    if (native) (void)take_range_flag(h);  // informational, as above
    return 0;
}

// slices scored under affine maps against targets, one synchronous one-chunk call on host pointers: images + targets + maps -> sums, [warped], [wgrad]
int align_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int32_t th, int32_t tw,
               const float* maps_host, double* sums_host, float* warped_host, float* wgrad_host) {
    int rc = check(h);
    if (rc || (rc = align_check(h, n, height, width, th, tw))) return rc;
    const int64_t M = (int64_t)th * tw;
    if (n == 0 || M == 0) return 0;
    if (!images_host || !targets_host || !maps_host || !sums_host) return fail(MSIREN_E_INVALID, "null argument");
    if (n * (int64_t)height * width > 0x1fffffffLL) return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld slices of %dx%d", (long long)n, height, width);
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)n * M * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY), i_m = io.in(maps_host, (size_t)n * 6 * sizeof(float), HOST_COPY);
    const int o_s = io.out(sums_host, (size_t)n * kAlignSums * sizeof(double), HOST_IN_PLACE);
    const int o_w = io.out(warped_host, nt, HOST_IN_PLACE), o_g = io.out(wgrad_host, 2 * nt, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    if ((rc = align_slices(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), th, tw, io.src<float>(i_m), io.dst<double>(o_s), io.dst<float>(o_w),
                           io.dst<float>(o_g))))
        return rc;
    return io.finish();
}

// slices aligned to their targets, one synchronous one-chunk call on host pointers: images + targets + the start go up once, the loop runs on the
// device, maps, [rigid states], report and [trace] come back
int align_solve_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int32_t th, int32_t tw,
                     const msiren_align_solve_opts* o, const float* maps_in, const double* rigid_in, float* maps_out, double* rigid_out, double* report, double* trace) {
    int rc = check(h);
    if (rc || (rc = align_solve_check(h, n, height, width, th, tw, o, maps_in, rigid_in, maps_out, report))) return rc;
    const int64_t M = (int64_t)th * tw;
    if (n == 0 || M == 0) return 0;
    if (!images_host || !targets_host) return fail(MSIREN_E_INVALID, "null argument");
    if (n * (int64_t)height * width > 0x1fffffffLL) return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld slices of %dx%d", (long long)n, height, width);
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)n * M * sizeof(float);
    const bool rigid = o->mode == 1;
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY);
    const int i_m = io.in(rigid ? nullptr : maps_in, (size_t)n * 6 * sizeof(float), HOST_COPY), i_r = io.in(rigid ? rigid_in : nullptr, (size_t)n * 4 * sizeof(double), HOST_COPY);
    const int o_m = io.out(maps_out, (size_t)n * 6 * sizeof(float), HOST_COPY), o_r = io.out(rigid_out, (size_t)n * 4 * sizeof(double), HOST_COPY);
    const int o_rep = io.out(report, (size_t)n * 6 * sizeof(double), HOST_COPY), o_tr = io.out(trace, (size_t)o->iterations * n * 8 * sizeof(double), HOST_COPY);
    if ((rc = io.begin())) return rc;
    if ((rc = align_solve(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), th, tw, o, io.src<float>(i_m), io.src<double>(i_r), io.dst<float>(o_m),
                          io.dst<double>(o_r), io.dst<double>(o_rep), io.dst<double>(o_tr))))
        return rc;
    return io.finish();
}

// the weighted forms: as the two above; the weights and the intensities go up once per call
int align_w_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int32_t th, int32_t tw,
                 const float* maps_host, const float* weights_host, const float* intensity_host, double* sums_host, float* warped_host, float* wgrad_host) {
    int rc = check(h);
    if (rc || (rc = align_w_check(h, n, height, width, th, tw))) return rc;
    const int64_t M = (int64_t)th * tw;
    if (n == 0 || M == 0) return 0;
    if (!images_host || !targets_host || !maps_host || !sums_host) return fail(MSIREN_E_INVALID, "null argument");
    if (n * (int64_t)height * width > 0x1fffffffLL) return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld slices of %dx%d", (long long)n, height, width);
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)n * M * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY), i_m = io.in(maps_host, (size_t)n * 6 * sizeof(float), HOST_COPY);
    const int i_w = io.in(weights_host, nt, HOST_COPY), i_gb = io.in(intensity_host, (size_t)n * 2 * sizeof(float), HOST_COPY);
    const int o_s = io.out(sums_host, (size_t)n * kAlignSumsW * sizeof(double), HOST_IN_PLACE);
    const int o_w = io.out(warped_host, nt, HOST_IN_PLACE), o_g = io.out(wgrad_host, 2 * nt, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    if ((rc = align_slices_w(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), th, tw, io.src<float>(i_m), io.src<float>(i_w), io.src<float>(i_gb),
                             io.dst<double>(o_s), io.dst<float>(o_w), io.dst<float>(o_g))))
        return rc;
    return io.finish();
}

int align_solve_w_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int32_t th, int32_t tw,
                       const msiren_align_solve_w_opts* o, const float* maps_in, const double* rigid_in, const float* weights_host, const float* intensity_in,
                       float* maps_out, float* intensity_out, double* rigid_out, double* report, double* trace) {
    int rc = check(h);
    if (rc || (rc = align_solve_w_check(h, n, height, width, th, tw, o, maps_in, rigid_in, maps_out, intensity_out, report))) return rc;
    const int64_t M = (int64_t)th * tw;
    if (n == 0 || M == 0) return 0;
    if (!images_host || !targets_host) return fail(MSIREN_E_INVALID, "null argument");
    if (n * (int64_t)height * width > 0x1fffffffLL) return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld slices of %dx%d", (long long)n, height, width);
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)n * M * sizeof(float);
    const bool rigid = o->mode == 1;
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY);
    const int i_m = io.in(rigid ? nullptr : maps_in, (size_t)n * 6 * sizeof(float), HOST_COPY), i_r = io.in(rigid ? rigid_in : nullptr, (size_t)n * 4 * sizeof(double), HOST_COPY);
    const int i_w = io.in(weights_host, nt, HOST_COPY), i_gb = io.in(intensity_in, (size_t)n * 2 * sizeof(float), HOST_COPY);
    const int o_m = io.out(maps_out, (size_t)n * 6 * sizeof(float), HOST_COPY), o_gb = io.out(intensity_out, (size_t)n * 2 * sizeof(float), HOST_COPY);
    const int o_r = io.out(rigid_out, (size_t)n * 4 * sizeof(double), HOST_COPY);
    const int o_rep = io.out(report, (size_t)n * 7 * sizeof(double), HOST_COPY), o_tr = io.out(trace, (size_t)o->iterations * n * 11 * sizeof(double), HOST_COPY);
    if ((rc = io.begin())) return rc;
    if ((rc = align_solve_w(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), th, tw, o, io.src<float>(i_m), io.src<double>(i_r), io.src<float>(i_w),
                            io.src<float>(i_gb), io.dst<float>(o_m), io.dst<float>(o_gb), io.dst<double>(o_r), io.dst<double>(o_rep), io.dst<double>(o_tr))))
        return rc;
    return io.finish();
}

// target slices scored against the stack read as a volume, one synchronous one-chunk call on host pointers
int align_volume_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                      const float* maps_host, double* sums_host, float* warped_host, float* wgrad_host) {
    int rc = check(h);
    if (rc || (rc = align_volume_check(h, n, height, width, m, th, tw))) return rc;
    const int64_t M = m * (int64_t)th * tw;
    if (M == 0) return 0;
    if (!images_host || !targets_host || !maps_host || !sums_host) return fail(MSIREN_E_INVALID, "null argument");
    if (n * (int64_t)height * width > 0x1fffffffLL) return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld slices of %dx%d", (long long)n, height, width);
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)M * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY), i_m = io.in(maps_host, (size_t)m * 9 * sizeof(float), HOST_COPY);
    const int o_s = io.out(sums_host, (size_t)m * kAlignVolumeSums * sizeof(double), HOST_IN_PLACE);
    const int o_w = io.out(warped_host, nt, HOST_IN_PLACE), o_g = io.out(wgrad_host, 3 * nt, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    if ((rc = align_volume(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), m, th, tw, io.src<float>(i_m), io.dst<double>(o_s), io.dst<float>(o_w),
                           io.dst<float>(o_g))))
        return rc;
    return io.finish();
}

// targets aligned to the volume, one synchronous one-chunk call on host pointers: images + targets + the start go up once, the loop runs on the device
int align_volume_solve_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                            const msiren_align_volume_solve_opts* o, const float* maps_in, const double* planes, const double* rigid_in, float* maps_out, double* rigid_out,
                            double* report, double* trace) {
    int rc = check(h);
    if (rc || (rc = align_volume_solve_check(h, n, height, width, m, th, tw, o, maps_in, planes, rigid_in, maps_out, report))) return rc;
    const int64_t M = m * (int64_t)th * tw;
    if (M == 0) return 0;
    if (!images_host || !targets_host) return fail(MSIREN_E_INVALID, "null argument");
    if (n * (int64_t)height * width > 0x1fffffffLL) return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld slices of %dx%d", (long long)n, height, width);
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)M * sizeof(float);
    const bool rigid = o->mode == 1;
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY);
    const int i_m = io.in(rigid ? nullptr : maps_in, (size_t)m * 9 * sizeof(float), HOST_COPY), i_p = io.in(rigid ? planes : nullptr, (size_t)m * 12 * sizeof(double), HOST_COPY);
    const int i_r = io.in(rigid ? rigid_in : nullptr, (size_t)m * 12 * sizeof(double), HOST_COPY);
    const int o_m = io.out(maps_out, (size_t)m * 9 * sizeof(float), HOST_COPY), o_r = io.out(rigid_out, (size_t)m * 12 * sizeof(double), HOST_COPY);
    const int o_rep = io.out(report, (size_t)m * 6 * sizeof(double), HOST_COPY), o_tr = io.out(trace, (size_t)o->iterations * m * 11 * sizeof(double), HOST_COPY);
    if ((rc = io.begin())) return rc;
    if ((rc = align_volume_solve(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), m, th, tw, o, io.src<float>(i_m), io.src<double>(i_p), io.src<double>(i_r),
                                 io.dst<float>(o_m), io.dst<double>(o_r), io.dst<double>(o_rep), io.dst<double>(o_tr))))
        return rc;
    return io.finish();
}

}  // namespace

extern "C" {

int msiren_align_slices_w(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int32_t th, int32_t tw,
                          const float* maps_host, const float* weights_host, const float* intensity_host, double* sums_host, float* warped_host, float* wgrad_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_w_host(h, images_host, n, height, width, targets_host, th, tw, maps_host, weights_host, intensity_host, sums_host, warped_host, wgrad_host);
}
int msiren_align_slices_w_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                              const float* maps_dev, const float* weights_dev, const float* intensity_dev, double* sums_dev, float* warped_dev, float* wgrad_dev) {
    int rc = check(h);
    if (rc) return rc;
    if ((rc = align_w_check(h, n, height, width, th, tw))) return rc;  // (before the stream rotates)
    return align_slices_w(h, dev_call(h), images_dev, n, height, width, targets_dev, th, tw, maps_dev, weights_dev, intensity_dev, sums_dev, warped_dev, wgrad_dev);
}
int msiren_align_solve_w(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int32_t th, int32_t tw,
                         const msiren_align_solve_w_opts* opts, const float* maps_in, const double* rigid_in, const float* weights_host, const float* intensity_in,
                         float* maps_out, float* intensity_out, double* rigid_out, double* report, double* trace) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_solve_w_host(h, images_host, n, height, width, targets_host, th, tw, opts, maps_in, rigid_in, weights_host, intensity_in, maps_out, intensity_out, rigid_out,
                              report, trace);
}
int msiren_align_solve_w_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                             const msiren_align_solve_w_opts* opts, const float* maps_in_dev, const double* rigid_in_dev, const float* weights_dev,
                             const float* intensity_in_dev, float* maps_out_dev, float* intensity_out_dev, double* rigid_out_dev, double* report_dev, double* trace_dev) {
    int rc = check(h);
    if (rc) return rc;
    if ((rc = align_solve_w_check(h, n, height, width, th, tw, opts, maps_in_dev, rigid_in_dev, maps_out_dev, intensity_out_dev, report_dev))) return rc;  // (before the stream rotates)
    return align_solve_w(h, dev_call(h), images_dev, n, height, width, targets_dev, th, tw, opts, maps_in_dev, rigid_in_dev, weights_dev, intensity_in_dev, maps_out_dev,
                         intensity_out_dev, rigid_out_dev, report_dev, trace_dev);
}

int msiren_align_volume(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                        const float* maps_host, double* sums_host, float* warped_host, float* wgrad_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_volume_host(h, images_host, n, height, width, targets_host, m, th, tw, maps_host, sums_host, warped_host, wgrad_host);
}
int msiren_align_volume_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th, int32_t tw,
                            const float* maps_dev, double* sums_dev, float* warped_dev, float* wgrad_dev) {
    int rc = check(h);
    if (rc) return rc;
    if ((rc = align_volume_check(h, n, height, width, m, th, tw))) return rc;  // (before the stream rotates)
    return align_volume(h, dev_call(h), images_dev, n, height, width, targets_dev, m, th, tw, maps_dev, sums_dev, warped_dev, wgrad_dev);
}
int msiren_align_volume_solve(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th,
                              int32_t tw, const msiren_align_volume_solve_opts* opts, const float* maps_in, const double* planes, const double* rigid_in, float* maps_out,
                              double* rigid_out, double* report, double* trace) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_volume_solve_host(h, images_host, n, height, width, targets_host, m, th, tw, opts, maps_in, planes, rigid_in, maps_out, rigid_out, report, trace);
}
int msiren_align_volume_solve_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                                  int32_t tw, const msiren_align_volume_solve_opts* opts, const float* maps_in_dev, const double* planes_dev, const double* rigid_in_dev,
                                  float* maps_out_dev, double* rigid_out_dev, double* report_dev, double* trace_dev) {
    int rc = check(h);
    if (rc) return rc;
    if ((rc = align_volume_solve_check(h, n, height, width, m, th, tw, opts, maps_in_dev, planes_dev, rigid_in_dev, maps_out_dev, report_dev))) return rc;  // (before the stream rotates)
    return align_volume_solve(h, dev_call(h), images_dev, n, height, width, targets_dev, m, th, tw, opts, maps_in_dev, planes_dev, rigid_in_dev, maps_out_dev, rigid_out_dev,
                              report_dev, trace_dev);
}

int msiren_align_solve(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int32_t th, int32_t tw,
                       const msiren_align_solve_opts* opts, const float* maps_in, const double* rigid_in, float* maps_out, double* rigid_out, double* report,
                       double* trace) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_solve_host(h, images_host, n, height, width, targets_host, th, tw, opts, maps_in, rigid_in, maps_out, rigid_out, report, trace);
}
int msiren_align_solve_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                           const msiren_align_solve_opts* opts, const float* maps_in_dev, const double* rigid_in_dev, float* maps_out_dev, double* rigid_out_dev,
                           double* report_dev, double* trace_dev) {
    int rc = check(h);
    if (rc) return rc;
    if ((rc = align_solve_check(h, n, height, width, th, tw, opts, maps_in_dev, rigid_in_dev, maps_out_dev, report_dev))) return rc;  // (before the stream rotates)
    return align_solve(h, dev_call(h), images_dev, n, height, width, targets_dev, th, tw, opts, maps_in_dev, rigid_in_dev, maps_out_dev, rigid_out_dev, report_dev, trace_dev);
}

int msiren_resample_volume(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* points_host, int64_t M, float* out_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return volume_host(h, images_host, n, height, width, points_host, M, out_host, nullptr, false);
}
int msiren_resample_volume_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* points_dev, int64_t M, float* out_dev) {
    int rc = check(h);
    if (rc) return rc;
    return resample_volume(h, dev_call(h), images_dev, n, height, width, points_dev, M, out_dev, nullptr, false);
}
int msiren_resample_volume_native(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* points_host, int64_t M, float* out_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return volume_host(h, images_host, n, height, width, points_host, M, out_host, nullptr, false, true);
}
int msiren_resample_volume_native_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* points_dev, int64_t M, float* out_dev) {
    int rc = check(h);
    if (rc) return rc;
    return resample_volume(h, dev_call(h), images_dev, n, height, width, points_dev, M, out_dev, nullptr, false, true);
}
int msiren_resample_volume_grad(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* points_host, int64_t M, float* out_host,
                                float* grad_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return volume_host(h, images_host, n, height, width, points_host, M, out_host, grad_host, true);
}
int msiren_resample_volume_grad_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* points_dev, int64_t M, float* out_dev,
                                    float* grad_dev) {
    int rc = check(h);
    if (rc) return rc;
    return resample_volume(h, dev_call(h), images_dev, n, height, width, points_dev, M, out_dev, grad_dev, true);
}

int msiren_align_slices(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int32_t th, int32_t tw,
                        const float* maps_host, double* sums_host, float* warped_host, float* wgrad_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_host(h, images_host, n, height, width, targets_host, th, tw, maps_host, sums_host, warped_host, wgrad_host);
}
int msiren_align_slices_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                            const float* maps_dev, double* sums_dev, float* warped_dev, float* wgrad_dev) {
    int rc = check(h);
    if (rc) return rc;
    return align_slices(h, dev_call(h), images_dev, n, height, width, targets_dev, th, tw, maps_dev, sums_dev, warped_dev, wgrad_dev);
}

int msiren_resample_slices(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* points_host, int64_t M, float* out_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return resample_host(h, images_host, n, height, width, points_host, M, out_host, nullptr, false);
}
int msiren_resample_slices_native(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* points_host, int64_t M, float* out_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return resample_host(h, images_host, n, height, width, points_host, M, out_host, nullptr, false, true);
}
int msiren_resample_slices_native_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* points_dev, int64_t M, float* out_dev) {
    int rc = check(h);
    if (rc) return rc;
    return resample_slices(h, dev_call(h), images_dev, n, height, width, points_dev, M, out_dev, nullptr, false, true);
}
int msiren_resample_slices_grad(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* points_host, int64_t M, float* out_host,
                                float* grad_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return resample_host(h, images_host, n, height, width, points_host, M, out_host, grad_host, true);
}
int msiren_resample_slices_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* points_dev, int64_t M, float* out_dev) {
    int rc = check(h);
    if (rc) return rc;
    return resample_slices(h, dev_call(h), images_dev, n, height, width, points_dev, M, out_dev, nullptr, false);
}
int msiren_resample_slices_grad_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* points_dev, int64_t M, float* out_dev,
                                    float* grad_dev) {
    int rc = check(h);
    if (rc) return rc;
    return resample_slices(h, dev_call(h), images_dev, n, height, width, points_dev, M, out_dev, grad_dev, true);
}

int msiren_sample_ragged_mods(msiren_handle h, const float* coords_host, const int32_t* offsets_host, const float* mods_host, int64_t B, int64_t T, float* out_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return ragged_host(h, coords_host, offsets_host, mods_host, B, T, out_host, nullptr, false);
}
int msiren_sample_ragged_mods_dev(msiren_handle h, const float* coords_dev, const int32_t* offsets_dev, const float* mods_dev, int64_t B, int64_t T, float* out_dev) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return ragged_dev(h, coords_dev, offsets_dev, mods_dev, B, T, out_dev, nullptr, false);
}
int msiren_sample_ragged_mods_native(msiren_handle h, const float* coords_host, const int32_t* offsets_host, const float* mods_host, int64_t B, int64_t T, float* out_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return ragged_host(h, coords_host, offsets_host, mods_host, B, T, out_host, nullptr, false, true);
}
int msiren_sample_ragged_mods_native_dev(msiren_handle h, const float* coords_dev, const int32_t* offsets_dev, const float* mods_dev, int64_t B, int64_t T, float* out_dev) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return ragged_dev(h, coords_dev, offsets_dev, mods_dev, B, T, out_dev, nullptr, false, true);
}
int msiren_sample_ragged_grad_mods(msiren_handle h, const float* coords_host, const int32_t* offsets_host, const float* mods_host, int64_t B, int64_t T, float* out_host,
                                   float* grad_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return ragged_host(h, coords_host, offsets_host, mods_host, B, T, out_host, grad_host, true);
}
int msiren_sample_ragged_grad_mods_dev(msiren_handle h, const float* coords_dev, const int32_t* offsets_dev, const float* mods_dev, int64_t B, int64_t T, float* out_dev,
                                       float* grad_dev) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return ragged_dev(h, coords_dev, offsets_dev, mods_dev, B, T, out_dev, grad_dev, true);
}

}  // extern "C"
