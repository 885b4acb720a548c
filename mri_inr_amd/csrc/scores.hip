// msiren_score_images(_dev): the evaluation harness's PSNR / SSIM / NRMSE on the device (scores.hip.h: the kernels, their order).
#include <algorithm>

#include "host_buffers.h"
#include "host_ctx.h"
#include "scores.hip.h"

using namespace mh;

namespace {

// the three launches on the handle's CURRENT stream: a call right behind a *_dev forward call sees its output without a sync
int score_on_current_stream(msiren_ctx* h, const float* o, const float* p, int64_t n, int32_t H, int32_t W, double* scores) {
    const int64_t hw = (int64_t)H * W;
    const int64_t chunks = (hw + msiren::SCORE_CHUNK - 1) / msiren::SCORE_CHUNK;
    const int64_t tiles_x = (W - msiren::SCORE_WIN + msiren::SCORE_TW) / msiren::SCORE_TW;  // ceil((W-6) / 32)
    const int64_t tiles = tiles_x * ((H - msiren::SCORE_WIN + msiren::SCORE_TH) / msiren::SCORE_TH);
    if (n * std::max(chunks, tiles) > 0x7fffffffLL)
        return fail(MSIREN_E_INVALID, "too many images for one call: %lld of %dx%d", (long long)n, H, W);
    auto& c = h->sc[h->cur];
    const size_t stat_bytes = (size_t)(n * chunks) * sizeof(msiren::ScoreStat);
    int rc = ensure(h, c.score, stat_bytes + (size_t)(n * tiles) * sizeof(double));
    if (rc) return rc;
    auto* stats = (msiren::ScoreStat*)c.score.p;
    auto* ssim_part = (double*)((char*)c.score.p + stat_bytes);
    hipLaunchKernelGGL(msiren::score_stats_kernel, dim3((unsigned)(n * chunks)), dim3(msiren::SCORE_THREADS), 0, c.s, o, p, stats, hw, (int)chunks);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(msiren::score_ssim_kernel, dim3((unsigned)(n * tiles)), dim3(msiren::SCORE_THREADS), 0, c.s, o, p, stats, ssim_part, H, W,
                       (int)chunks, (int)tiles_x, (int)tiles);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(msiren::score_combine_kernel, dim3((unsigned)n), dim3(msiren::SCORE_THREADS), 0, c.s, stats, ssim_part, scores, H, W,
                       (int)chunks, (int)tiles);
    HIPCHK(hipGetLastError());
    return 0;
}

int score_args(msiren_ctx* h, const void* o, const void* p, int64_t n, int32_t H, int32_t W, const void* scores) {
    int rc = check(h, false);
    if (rc) return rc;
    if (n < 0) return fail(MSIREN_E_INVALID, "n_images must be >= 0, got %lld", (long long)n);
    // skimage refuses images smaller than its 7 x 7 window too
    if (H < msiren::SCORE_WIN || W < msiren::SCORE_WIN)
        return fail(MSIREN_E_INVALID, "images of %dx%d are smaller than the 7x7 SSIM window", H, W);
    if (n > 0 && (!o || !p || !scores)) return fail(MSIREN_E_INVALID, "null image or score pointer");
    return 0;
}

}  // namespace

extern "C" {

int msiren_score_images_dev(msiren_handle h, const float* original_dev, const float* predicted_dev, int64_t n, int32_t height, int32_t width,
                            double* scores_dev) {
    int rc = score_args(h, original_dev, predicted_dev, n, height, width, scores_dev);
    if (rc || n == 0) return rc;
    return score_on_current_stream(h, original_dev, predicted_dev, n, height, width, scores_dev);
}

int msiren_score_images(msiren_handle h, const float* original_host, const float* predicted_host, int64_t n, int32_t height, int32_t width,
                        double* scores_host) {
    int rc = score_args(h, original_host, predicted_host, n, height, width, scores_host);
    if (rc || n == 0) return rc;
    const size_t ni = (size_t)n * height * width * sizeof(float), ns = (size_t)n * 3 * sizeof(double);
    SyncHostCall io(h, h->cur);
    const int i_o = io.in(original_host, ni, HOST_COPY), i_p = io.in(predicted_host, ni, HOST_COPY | HOST_PACKED), o_s = io.out(scores_host, ns, HOST_COPY);
    if ((rc = io.begin()) || (rc = score_on_current_stream(h, io.src<float>(i_o), io.src<float>(i_p), n, height, width, io.dst<double>(o_s)))) return rc;
    return io.finish();
}

}  // extern "C"
