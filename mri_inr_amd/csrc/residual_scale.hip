// msiren_residual_scale(_dev) (include/msiren.h): a robust scale per target from an exact order statistic of the residuals,
// computed on the device with nothing read back, so that the scale of the robust calls never has to leave it.  Kernels: residual_scale.hip.h; what the
// call refuses, its chunking, its launch count and its scratch: residual_scale_plan.h.  No images, no trunk: the handle need not hold committed
// weights.  A unit of its own: it includes none of the other families' kernel headers, so none of their kernels is instantiated a second time.
#include "residual_scale.hip.h"
#include "host_buffers.h"
#include "host_ctx.h"

using namespace mh;

static_assert(sizeof(msiren_scale_opts) == 32, "msiren_scale_opts is 32 bytes");
static_assert(sizeof(msiren::RscaleOffsets) == 4 * msiren::kRscaleOffsets && msiren::kRscaleOffsets % 256 == 0, "rscale_upload_kernel's argument and grid");

namespace {

// 0, or MSIREN_E_INVALID with rscale_check's words
int refusal(const msiren::RscaleArgs& a) {
    char msg[256];
    return msiren::rscale_check(a, msg, sizeof msg) ? 0 : fail(MSIREN_E_INVALID, "%s", msg);
}

// The whole call on the call's stream, one profile entry; every pointer but group_start is the device's, `a` has passed rscale_check and has work.
// The sequence of launches depends on centre and the number of groups alone (residual_scale_plan.h: rscale_launches counts them): nothing is read back
int rscale_on_stream(msiren_ctx* h, const Call& c, const msiren::RscaleArgs& a) {
    using namespace msiren;
    int rc;
    auto& sc = h->sc[c.stream];
    const int pixels = a.th * a.tw, m = (int)a.m, G = (int)a.n_groups, chunks = (int)rscale_chunks(pixels);
    const RscaleLayout lay = rscale_layout(a.m, pixels, a.n_groups);
    if ((rc = ensure(h, sc.ragged, lay.total))) return rc;
    char* const base = (char*)sc.ragged.p;
    unsigned *const keys = (unsigned*)(base + lay.keys), *const partials = (unsigned*)(base + lay.partials), *const state = (unsigned*)(base + lay.state);
    int* const gs = G > 0 ? (int*)(base + lay.group_start) : nullptr;
    const msiren_scale_opts& o = *a.opts;
    const dim3 per_chunk((unsigned)((int64_t)m * chunks)), per_segment((unsigned)rscale_segments(a.m, a.n_groups)), block(256);
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1))) return rc;
    hipStream_t st = sc.s;
    // group_start: up to 512 offsets per launch, by value in the kernel's arguments (no copy from a host buffer that the caller may reuse, no sync)
    for (int64_t at = 0; at < (G > 0 ? (int64_t)G + 1 : 0); at += kRscaleOffsets) {
        RscaleOffsets off{};
        const int count = (int)std::min<int64_t>(kRscaleOffsets, (int64_t)G + 1 - at);
        for (int i = 0; i < count; ++i) off.v[i] = a.group_start[at + i];
        hipLaunchKernelGGL(rscale_upload_kernel, dim3(kRscaleOffsets / 256), block, 0, st, off, gs, (int)at, count);
        HIPCHK(hipGetLastError());
    }
    for (int selection = 0; selection <= o.centre; ++selection) {
        const int by_bits = o.centre && selection == 0;  // the first of two selections orders the e themselves; every other the bits of a magnitude
        if (selection == 0)
            hipLaunchKernelGGL(rscale_keys_kernel, per_chunk, block, 0, st, (const float*)a.targets, (const float*)a.simulated, (const float*)a.weights,
                               (const float*)a.intensity, pixels, chunks, by_bits, keys, partials);
        else
            hipLaunchKernelGGL(rscale_rekey_kernel, per_chunk, block, 0, st, keys, (const int*)gs, G, (const unsigned*)state, pixels, chunks, partials);
        HIPCHK(hipGetLastError());
        for (int pass = 0; pass < kRscalePasses; ++pass) {
            if (pass > 0) {
                hipLaunchKernelGGL(rscale_hist_kernel, per_chunk, block, 0, st, (const unsigned*)keys, (const int*)gs, G, (const unsigned*)state, pixels, chunks, 24 - 8 * pass,
                                   partials);
                HIPCHK(hipGetLastError());
            }
            hipLaunchKernelGGL(rscale_choose_kernel, per_segment, block, 0, st, (const unsigned*)partials, (const int*)gs, G, chunks, pass == 0, selection == 1, o.quantile,
                               state);
            HIPCHK(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(rscale_finish_kernel, dim3((unsigned)((m + 255) / 256)), block, 0, st, (const unsigned*)state, (const int*)gs, G, m, o.centre, o.tune, o.floor,
                       (double*)a.scale, (double*)a.stats);
    HIPCHK(hipGetLastError());
    return profile_end(h, c.stream, e1, a.m * pixels, "residual_scale_kernels");
}

bool has_work(const msiren::RscaleArgs& a) { return a.m > 0 && (int64_t)a.th * a.tw > 0; }

}  // namespace

extern "C" {

int msiren_residual_scale_dev(msiren_handle h, const float* targets_dev, const float* simulated_dev, const float* weights_dev, const float* intensity_dev, int64_t m,
                              int32_t th, int32_t tw, const msiren_scale_opts* opts, const int32_t* group_start, int64_t n_groups, double* scale_dev, double* stats_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::RscaleArgs a{targets_dev, simulated_dev, weights_dev, intensity_dev, m, th, tw, opts, group_start, n_groups, scale_dev, stats_dev, true};
    if ((rc = refusal(a))) return rc;  // (before the stream rotates)
    if (!has_work(a)) return 0;       // (no pixel: nothing to write)
    return rscale_on_stream(h, dev_call(h), a);
}

int msiren_residual_scale(msiren_handle h, const float* targets_host, const float* simulated_host, const float* weights_host, const float* intensity_host, int64_t m,
                          int32_t th, int32_t tw, const msiren_scale_opts* opts, const int32_t* group_start, int64_t n_groups, double* scale_host, double* stats_host) {
    int rc = check(h, false);
    if (rc) return rc;
    const msiren::RscaleArgs host{targets_host, simulated_host, weights_host, intensity_host, m, th, tw, opts, group_start, n_groups, scale_host, stats_host, false};
    if ((rc = refusal(host))) return rc;
    if (!has_work(host)) return 0;
    const Call c = make_call(h, true);
    const size_t nt = (size_t)m * th * tw * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_t = io.in(targets_host, nt, HOST_COPY), i_s = io.in(simulated_host, nt, HOST_COPY), i_w = io.in(weights_host, nt, HOST_COPY);
    const int i_gb = io.in(intensity_host, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int o_sc = io.out(scale_host, (size_t)m * sizeof(double), HOST_COPY);
    const int o_st = io.out(stats_host, (size_t)msiren::rscale_segments(m, n_groups) * 4 * sizeof(double), HOST_COPY);
    if ((rc = io.begin())) return rc;
    const msiren::RscaleArgs dev{io.src<float>(i_t), io.src<float>(i_s), io.src<float>(i_w), io.src<float>(i_gb), m, th, tw, opts, group_start, n_groups, io.dst<double>(o_sc),
                                 io.dst<double>(o_st), true};
    if ((rc = rscale_on_stream(h, c, dev))) return rc;
    return io.finish();
}

}  // extern "C"
