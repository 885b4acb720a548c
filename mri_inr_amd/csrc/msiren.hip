// libmsiren.so -- the C ABI declared in include/msiren.h: lifecycle, weights, the forward and slice entry points, memory, timing, info.
// Owns the device context (one device, up to three streams), the weight store keyed by the reference's state_dict names and the grow-only
// device workspaces; the launch sequence lives in launch_dispatch.hip, the weight layouts in weights_pack.hip (host_ctx.h: the map).
// Nothing here falls back to the CPU: every forward entry point launches HIP kernels or fails.
#include <dlfcn.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host_ctx.h"
#include "host_buffers.h"
#include "host_plan.h"
#include "weights_blob.h"

namespace mh {

namespace {
thread_local std::string g_err;
}

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
const char* last_error() { return g_err.c_str(); }

int use_device(msiren_ctx* h) {
    HIPCHK(hipSetDevice(h->cfg.device));
    return 0;
}

int ensure(msiren_ctx* h, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    if (b.p) HIPCHK(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    size_t cap = bytes + bytes / 4 + 256;
    HIPCHK(hipMalloc(&b.p, cap));
    b.cap = cap;
    (void)h;
    return 0;
}

int upload(float** dst, const std::vector<float>& src) {
    if (*dst) HIPCHK(hipFree(*dst));
    *dst = nullptr;
    HIPCHK(hipMalloc((void**)dst, src.size() * sizeof(float)));
    HIPCHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

bool take_range_flag(msiren_ctx* h) {
    if (!h->status_host || !*h->status_host) return false;
    *h->status_host = 0;
    h->range_events++;
    return true;
}

int sync_all(msiren_ctx* h) {
    for (auto& c : h->sc)
        if (c.s) HIPCHK(hipStreamSynchronize(c.s));
    (void)take_range_flag(h);  // informational: the outputs are the exact-fp32 trunk's already
    return 0;
}

// behind a synchronous host call: the domain flag in host memory is informational (the outputs are the exact-fp32 trunk's already)
static int take_range_flag_after(msiren_ctx* h, int rc) {
    (void)take_range_flag(h);
    return rc;
}

// asynchronous forward entry points rotate over the configured streams
void next_stream(msiren_ctx* h) {
    if (h->nstreams > 1) h->cur = (h->cur + 1) % h->nstreams;
}

Call dev_call(msiren_ctx* h) {
    next_stream(h);
    return make_call(h, false);
}

// event pairs recorded since the last collection -> totals (the streams have been synchronised by the caller)
int profile_collect(msiren_ctx* h) {
    for (size_t i = 0; i < h->prof_used; ++i) {
        const auto& r = h->prof_events[i];
        if (r.kernel < 0) continue;  // (the launch between the pair failed)
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
        auto& k = h->prof_kernels[r.kernel];
        if (k.trunk) {  // (the layer-0 table kernel of a sampling call is listed per kernel only)
            h->prof_ms += ms;
            h->prof_launches++;
        }
        k.ms += ms;
        k.launches++;
        k.coords += r.coords;
    }
    h->prof_used = 0;
    return 0;
}

int check(msiren_ctx* h, bool need_commit) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    if (need_commit && !h->committed) return fail(MSIREN_E_STATE, "weights not committed: call msiren_set_tensor for every net.* key, then msiren_commit_weights");
    return use_device(h);
}

int check_tile_size(const msiren_ctx* h, bool cite) {
    if (h->O == 32) return 0;
    return cite ? fail(MSIREN_E_INVALID, "the custom encoder is hard-wired to 32x32 tiles (siren_encoder.py:499), outer_patch_size=%d", h->O)
                : fail(MSIREN_E_INVALID, "the custom encoder is hard-wired to 32x32 tiles, outer_patch_size=%d", h->O);
}

int check_reflect_padding(const msiren_ctx* h, int32_t height, int32_t width) {
    const int pad = (h->O - h->I) / 2;
    const int vpad = (h->I - height % h->I) % h->I, hpad = (h->I - width % h->I) % h->I;
    if (pad + vpad >= height || pad + hpad >= width)
        return fail(MSIREN_E_INVALID, "image %dx%d is too small for reflect padding of %d/%d", height, width, pad + vpad, pad + hpad);
    return 0;
}

int check_pairs_aligned(const void* dev, const char* what) {
    if ((uintptr_t)dev % 8) return fail(MSIREN_E_INVALID, "device %s must be 8-byte aligned (they are read as (row, column) pairs)", what);
    return 0;
}

}  // namespace mh

using namespace mh;

// =================================================================================================
extern "C" {

int msiren_abi_version(void) { return MSIREN_ABI_VERSION; }

const char* msiren_last_error(void) { return mh::last_error(); }

int msiren_device_count(int32_t* count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    if (count) *count = n;
    return 0;
}

int msiren_create(const msiren_config* cfg, msiren_handle* out) {
    if (!cfg || !out) return fail(MSIREN_E_INVALID, "null argument");
    if (cfg->abi_version != MSIREN_ABI_VERSION)
        return fail(MSIREN_E_INVALID, "ABI version mismatch: header %d, library %d", cfg->abi_version, MSIREN_ABI_VERSION);
    if (cfg->dim_in != 2) return fail(MSIREN_E_INVALID, "dim_in must be 2 (the coordinate grid is a 2-D meshgrid), got %d", cfg->dim_in);
    if (cfg->dim_out != 1) return fail(MSIREN_E_INVALID, "dim_out must be 1 (the reference's squeeze(2)+rearrange only works for 1), got %d", cfg->dim_out);
    if (cfg->dim_hidden < 1 || cfg->dim_hidden > 512) return fail(MSIREN_E_INVALID, "dim_hidden must be in [1,512], got %d", cfg->dim_hidden);
    if (cfg->num_layers < 1 || cfg->num_layers > 64) return fail(MSIREN_E_INVALID, "num_layers must be in [1,64], got %d", cfg->num_layers);
    if (cfg->latent_dim < 1) return fail(MSIREN_E_INVALID, "latent_dim must be positive, got %d", cfg->latent_dim);
    // (shapes off the MFMA Linear kernels run the VALU Modulator, whose input rows live in the LDS of a plain launch: dispatch.h)
    if (!msiren::modulator_valu_fits(cfg->dim_hidden, cfg->latent_dim, cfg->num_layers))
        return fail(MSIREN_E_INVALID, "latent_dim too large for dim_hidden %% 16 != 0 or latent_dim %% 16 != 0: need %s + latent_dim <= 1792, got %d + %d",
                    cfg->num_layers > 1 ? "dim_hidden" : "0", cfg->num_layers > 1 ? cfg->dim_hidden : 0, cfg->latent_dim);
    if (cfg->siren_patch_size < 2) return fail(MSIREN_E_INVALID, "siren_patch_size must be >= 2, got %d", cfg->siren_patch_size);
    if (cfg->inner_patch_size < 1 || cfg->outer_patch_size < cfg->inner_patch_size)
        return fail(MSIREN_E_INVALID, "need outer_patch_size >= inner_patch_size >= 1");
    if (cfg->activation != MSIREN_ACT_SINE && cfg->activation != MSIREN_ACT_MORLET) return fail(MSIREN_E_INVALID, "unknown activation %d", cfg->activation);
    if (cfg->precision < MSIREN_PREC_F32 || cfg->precision > MSIREN_PREC_F16)
        return fail(MSIREN_E_INVALID, "unknown precision %d", cfg->precision);
    if (cfg->w0 == 0.f || cfg->w0_initial == 0.f) return fail(MSIREN_E_INVALID, "w0 and w0_initial must be non-zero");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(MSIREN_E_INVALID, "device %d out of range (%d visible)", cfg->device, ndev);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MSIREN_E_INVALID, "device %d is %s; libmsiren is built for gfx950 (MI355X) only", cfg->device, prop.gcnArchName);
    auto* h = new msiren_ctx();
    h->cfg = *cfg;
    h->H = cfg->dim_hidden;
    h->HP = (cfg->dim_hidden + 127) / 128 * 128;
    h->L = cfg->num_layers;
    h->Z = cfg->latent_dim;
    h->S = cfg->siren_patch_size;
    h->P = h->S * h->S;
    h->O = cfg->outer_patch_size;
    h->I = cfg->inner_patch_size;
    h->num_cus = prop.multiProcessorCount;
    if (const char* e = std::getenv("MSIREN_F16_HALF")) h->dh.half_allowed = std::atoi(e) != 0;
    if (const char* e = std::getenv("MSIREN_HOST_PIPE_MIN")) h->dh.host_pipe_min = std::max(128, std::atoi(e));
    if (const char* e = std::getenv("MSIREN_QUEUE_START")) h->queue_start = (unsigned)std::strtoul(e, nullptr, 0);
    if (const char* e = std::getenv("MSIREN_F16_WS")) h->dh.f16_ws = std::atoi(e) != 0;
    if (const char* e = std::getenv("MSIREN_TRACE_HOST")) h->trace_host = std::atoi(e);
    if (const char* e = std::getenv("MSIREN_PROLOGUE_F16X3")) h->em_enabled = std::atoi(e) != 0;
    if (const char* e = std::getenv("MSIREN_EM_DEPTH")) h->dh.em_depth = std::atoi(e);
    declare_expected(h);
    hipError_t e = hipSetDevice(cfg->device);
    for (auto& c : h->sc)
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->status_host, 64, hipHostMallocMapped);
    if (e == hipSuccess) {
        for (int i = 0; i < 16; ++i) h->status_host[i] = 0;  // [0] f16x3 domain guard (informational), [8] the flag word of synchronous host calls
        e = hipHostGetDevicePointer((void**)&h->status_dev, (void*)h->status_host, 0);
    }

    if (e == hipSuccess) e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    if (e != hipSuccess) {
        msiren_destroy(h);  // releases whatever was created
        return fail(MSIREN_E_HIP, "context creation failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return 0;
}

int msiren_destroy(msiren_handle h) {
    if (!h) return 0;
    (void)hipSetDevice(h->cfg.device);
    for (auto& c : h->sc)
        if (c.s) (void)hipStreamSynchronize(c.s);
    if (h->comm) (void)comm_destroy(h);
    drop_lattices(h);
    if (h->status_host) (void)hipHostFree((void*)h->status_host);
    if (h->ws_comm.p) (void)hipFree(h->ws_comm.p);
    if (h->d_wp16n) (void)hipFree(h->d_wp16n);
    if (h->d_emw) (void)hipFree(h->d_emw);
    if (h->d_emc2) (void)hipFree(h->d_emc2);
    for (void* q : {h->d_woutx1, h->d_wpx1n, h->d_wpx1w, (void*)h->d_bias32x1})
        if (q) (void)hipFree(q);
    float* ptrs[] = {h->d_w0raw, h->d_b0raw, h->d_dump, h->d_s0t512, h->d_s0t, h->d_bias16, h->d_wout16, h->d_grid, h->d_l0, h->d_wp, h->d_bias, h->d_wout, h->d_modw, h->d_modw_rm, h->d_modb, h->d_encw, h->d_foldw, h->d_embias};
    for (float* p : ptrs)
        if (p) (void)hipFree(p);
    std::vector<DevBuf*> bufs = {&h->stage_in, &h->stage_out};
    for (auto& c : h->sc)
        for (DevBuf* b : {&c.cscratch, &c.mods, &c.modpad, &c.latent, &c.patches, &c.keep, &c.rec, &c.queue, &c.feat, &c.plan, &c.score, &c.coords, &c.l0tab, &c.ragged}) bufs.push_back(b);
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (auto& pr : h->prof_events) {
        (void)hipEventDestroy(pr.a);
        (void)hipEventDestroy(pr.b);
    }
    for (auto& c : h->sc)
        if (c.ev_join) (void)hipEventDestroy(c.ev_join);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    for (auto& c : h->sc)
        if (c.s) (void)hipStreamDestroy(c.s);
    delete h;
    return 0;
}

int msiren_set_tensor(msiren_handle h, const char* name, const float* host_data, size_t n) {
    if (!h || !name || (!host_data && n)) return fail(MSIREN_E_INVALID, "null argument");
    auto it = h->expected.find(name);
    if (it == h->expected.end()) return fail(MSIREN_E_INVALID, "Unexpected key in state_dict: \"%s\"", name);
    if (it->second != n)
        return fail(MSIREN_E_SHAPE, "size mismatch for %s: got %zu elements, the configuration implies %zu", name, n, it->second);
    h->tensors[name].assign(host_data, host_data + n);
    h->committed = false;
    return 0;
}

int msiren_get_tensor(msiren_handle h, const char* name, float* host_out, size_t n) {
    if (!h || !name || (!host_out && n)) return fail(MSIREN_E_INVALID, "null argument");
    auto ex = h->expected.find(name);
    if (ex == h->expected.end()) return fail(MSIREN_E_INVALID, "Unexpected key in state_dict: \"%s\"", name);
    auto it = h->tensors.find(name);
    if (it == h->tensors.end()) return fail(MSIREN_E_STATE, "tensor %s has not been set", name);
    if (it->second.size() != n) return fail(MSIREN_E_SHAPE, "size mismatch for %s: asked for %zu elements, it has %zu", name, n, it->second.size());
    std::copy(it->second.begin(), it->second.end(), host_out);
    return 0;
}

int msiren_commit_weights(msiren_handle h) {
    int rc = check(h, false);
    if (rc) return rc;
    if ((rc = sync_all(h))) return rc;
    drop_lattices(h);  // (the kept layer-0 tables of other output strides depend on net.layers.0: sample_grid.hip)
    if ((rc = pack_trunk(h))) return rc;
    if ((rc = pack_trunk_f16x3(h))) return rc;
    if ((rc = pack_trunk_x1(h))) return rc;
    if ((rc = pack_fold_weights(h))) return rc;
    rc = pack_modulator(h);
    if (rc < 0) return rc;
    h->have_modulator = (rc == 0);
    rc = pack_encoder(h);
    if (rc < 0) return rc;
    h->have_encoder = (rc == 0);
    if ((rc = pack_prologue_f16x3(h))) return rc;
    describe_for_dispatch(h);
    h->committed = true;
    return 0;
}

int msiren_forward_mods_dev(msiren_handle h, const float* mods_dev, int64_t B, float* out_dev) {
    int rc = check(h);
    if (rc) return rc;
    const Call c = dev_call(h);
    if (B < 0 || (B > 0 && (!mods_dev || !out_dev))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    return launch_trunk(h, c, mods_dev, B, out_dev);
}

static int msiren_forward_mods_impl(msiren_handle h, const float* mods_host, int64_t B, float* out_host) {
    int rc = check(h);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!mods_host || !out_host))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if (B == 0) return 0;
    const Call c = make_call(h, true);
    auto& sc = h->sc[c.stream];
    const size_t nm = (size_t)h->L * B * h->H * sizeof(float), no = (size_t)B * h->P * sizeof(float);
    if ((rc = ensure(h, sc.mods, nm))) return rc;
    SyncHostCall io(h, c.stream);
    const int i_m = io.in(mods_host, nm, HOST_COPY, sc.mods.p), o_out = io.out(out_host, no, HOST_COPY);
    if ((rc = io.begin()) || (rc = launch_trunk(h, c, io.src<float>(i_m), B, io.dst<float>(o_out)))) return rc;
    return io.finish();
}

int msiren_forward_mods(msiren_handle h, const float* mods_host, int64_t B, float* out_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return take_range_flag_after(h, msiren_forward_mods_impl(h, mods_host, B, out_host));
}

int msiren_forward_latent_dev(msiren_handle h, const float* z_dev, int64_t B, float* out_dev, float* mods_out_dev) {
    int rc = check(h);
    if (rc) return rc;
    const Call c = dev_call(h);
    if (B < 0 || (B > 0 && (!z_dev || !out_dev))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    return forward_latent_dev(h, c, z_dev, B, out_dev, mods_out_dev);
}

static int msiren_forward_latent_impl(msiren_handle h, const float* z_host, int64_t B, float* out_host, float* mods_out_host) {
    int rc = check(h);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!z_host || !out_host))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if (B == 0) return 0;
    const Call c = make_call(h, true);
    auto& sc = h->sc[c.stream];
    const size_t nz = (size_t)B * h->Z * sizeof(float), no = (size_t)B * h->P * sizeof(float);
    const size_t nm = (size_t)h->L * B * h->H * sizeof(float);
    if ((rc = ensure(h, sc.latent, nz)) || (rc = ensure(h, sc.mods, nm))) return rc;
    SyncHostCall io(h, c.stream);
    const int i_z = io.in(z_host, nz, HOST_COPY, sc.latent.p), o_out = io.out(out_host, no, HOST_COPY);
    io.out(mods_out_host, nm, HOST_COPY, sc.mods.p);  // (the modulations are in the stream's scratch whether the caller takes them or not)
    if ((rc = io.begin()) || (rc = forward_latent_dev(h, c, io.src<float>(i_z), B, io.dst<float>(o_out), (float*)sc.mods.p))) return rc;
    return io.finish();
}

int msiren_forward_latent(msiren_handle h, const float* z_host, int64_t B, float* out_host, float* mods_out_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return take_range_flag_after(h, msiren_forward_latent_impl(h, z_host, B, out_host, mods_out_host));
}

// ---- the two producers alone: model.encoder(tiles) and model.modulator(z) of the reference (modulated_siren.py:420, 416) ----
int msiren_encode_tiles_dev(msiren_handle h, const float* tiles_dev, int64_t B, float* z_dev) {
    int rc = check(h);
    if (rc) return rc;
    const Call c = dev_call(h);
    if (B < 0 || (B > 0 && (!tiles_dev || !z_dev))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if ((rc = check_tile_size(h))) return rc;
    return launch_encoder(h, c, tiles_dev, B, z_dev);
}

int msiren_modulate_dev(msiren_handle h, const float* z_dev, int64_t B, float* mods_dev) {
    int rc = check(h);
    if (rc) return rc;
    const Call c = dev_call(h);
    if (B < 0 || (B > 0 && (!z_dev || !mods_dev))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    return launch_modulator(h, c, z_dev, B, mods_dev);
}

int msiren_encode_tiles(msiren_handle h, const float* tiles_host, int64_t B, float* z_host) {
    int rc = check(h);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!tiles_host || !z_host))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if ((rc = check_tile_size(h))) return rc;
    if (B == 0) return 0;
    const size_t nt = (size_t)B * h->O * h->O * sizeof(float), nz = (size_t)B * h->Z * sizeof(float);
    const Call call = make_call(h, false);  // (the prologue's MODE 1 / 2 instances have one ring depth, no prefetch: nothing to tell)
    auto& c = h->sc[call.stream];
    if ((rc = ensure(h, c.latent, nz))) return rc;
    SyncHostCall io(h, call.stream);
    const int i_t = io.in(tiles_host, nt, HOST_COPY), o_z = io.out(z_host, nz, HOST_COPY, c.latent.p);
    if ((rc = io.begin()) || (rc = launch_encoder(h, call, io.src<float>(i_t), B, io.dst<float>(o_z)))) return rc;
    return io.finish();
}

int msiren_modulate(msiren_handle h, const float* z_host, int64_t B, float* mods_host) {
    int rc = check(h);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!z_host || !mods_host))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if (B == 0) return 0;
    const size_t nz = (size_t)B * h->Z * sizeof(float), nm = (size_t)h->L * B * h->H * sizeof(float);
    const Call call = make_call(h, false);  // (as msiren_encode_tiles)
    auto& c = h->sc[call.stream];
    if ((rc = ensure(h, c.latent, nz)) || (rc = ensure(h, c.mods, nm))) return rc;
    SyncHostCall io(h, call.stream);
    const int i_z = io.in(z_host, nz, HOST_COPY, c.latent.p), o_m = io.out(mods_host, nm, HOST_COPY, c.mods.p);
    if ((rc = io.begin()) || (rc = launch_modulator(h, call, io.src<float>(i_z), B, io.dst<float>(o_m)))) return rc;
    return io.finish();
}

// ---- the prologue of msiren_forward_tiles(_dev) alone: tiles -> [latent] -> modulations, by the launches that call would make ----
int msiren_encode_modulate_tiles_dev(msiren_handle h, const float* tiles_dev, int64_t B, float* latent_dev, float* mods_dev) {
    int rc = check(h);
    if (rc) return rc;
    const Call c = dev_call(h);
    if (B < 0 || (B > 0 && (!tiles_dev || !mods_dev))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if ((rc = check_tile_size(h))) return rc;
    if (B == 0) return 0;
    return encode_modulate_dev(h, c, tiles_dev, B, latent_dev, mods_dev);
}

int msiren_encode_modulate_tiles(msiren_handle h, const float* tiles_host, int64_t B, float* latent_host, float* mods_host) {
    int rc = check(h);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!tiles_host || !mods_host))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if ((rc = check_tile_size(h))) return rc;
    if (B == 0) return 0;
    const size_t tile_elems = (size_t)h->O * h->O, nt = (size_t)B * tile_elems * sizeof(float), nz = (size_t)B * h->Z * sizeof(float);
    const size_t nm = (size_t)h->L * B * h->H * sizeof(float);
    // the chunks, streams and CallMode of msiren_forward_tiles_impl (which see): every chunk reaches the instance it reaches there
    std::vector<msiren::HostChunk> plan;
    if (msiren::host_call_pipelines(h->dh, B)) plan = msiren::pipelined_host_plan(B, h->host_first, h->host_piece, h->cur);
    else plan.push_back({0, B, h->cur, 0, false});
    // device staging for the whole call (chunk k's modulations, (L, n_k, H), sit at L * lo_k * H): nothing is reallocated while a chunk runs
    SyncHostCall io(h, h->cur, true);
    const int i_t = io.in(tiles_host, nt, HOST_OWN_COPIES), o_z = io.out(latent_host, nz, HOST_OWN_COPIES), o_m = io.out(mods_host, nm, HOST_OWN_COPIES);
    if ((rc = io.begin())) return rc;
    Call call = make_call(h, true);
    for (const msiren::HostChunk& c : plan) {
        call.stream = c.stream;
        call.mode.trunk = c.trunk;
        call.mode.beside = c.beside;
        hipStream_t s = h->sc[c.stream].s;
        float* const d_t = (float*)io.src<float>(i_t) + (size_t)c.lo * tile_elems;
        float* const d_z = latent_host ? io.dst<float>(o_z) + (size_t)c.lo * h->Z : nullptr;
        float* const d_m = io.dst<float>(o_m) + (size_t)h->L * c.lo * h->H;
        HIPCHK(hipMemcpyAsync(d_t, io.host_src<float>(i_t) + (size_t)c.lo * tile_elems, (size_t)c.n * tile_elems * sizeof(float), hipMemcpyHostToDevice, s));
        if ((rc = encode_modulate_dev(h, call, d_t, c.n, d_z, d_m))) return rc;
        if (d_z) HIPCHK(hipMemcpyAsync(io.host_dst<float>(o_z) + (size_t)c.lo * h->Z, d_z, (size_t)c.n * h->Z * sizeof(float), hipMemcpyDeviceToHost, s));
        const size_t row = (size_t)c.n * h->H * sizeof(float);  // layer l of the chunk -> rows [lo, lo + n) of layer l of the call
        HIPCHK(hipMemcpy2DAsync(io.host_dst<float>(o_m) + (size_t)c.lo * h->H, (size_t)B * h->H * sizeof(float), d_m, row, row, (size_t)h->L, hipMemcpyDeviceToHost, s));
    }
    return io.finish();
}

int msiren_forward_tiles_dev(msiren_handle h, const float* tiles_dev, int64_t B, float* out_dev) {
    int rc = check(h);
    if (rc) return rc;
    const Call c = dev_call(h);
    if (B < 0 || (B > 0 && (!tiles_dev || !out_dev))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if ((rc = check_tile_size(h))) return rc;
    return forward_tiles_dev(h, c, tiles_dev, B, out_dev);
}

static int msiren_forward_tiles_impl(msiren_handle h, const float* tiles_host, int64_t B, float* out_host) {
    int rc = check(h);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!tiles_host || !out_host))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if ((rc = check_tile_size(h))) return rc;
    if (B == 0) return 0;
    const size_t nt = (size_t)B * h->O * h->O * sizeof(float), no = (size_t)B * h->P * sizeof(float);
    // From host_pipe_min tiles (2400 = six slices) up the call pipelines itself (round 5).  The device side of a slice is ~325 us; uploading
    // its 1.6 MB first and downloading its 0.9 MB afterwards added ~90 us in front and behind.  Patches are independent
    // (modulated_siren.py:435-457), so the batch is cut into chunks that alternate between the handle's two streams:
    //     H2D_0 | launch_0 | H2D_1 | launch_1 | D2H_0 | H2D_2 | launch_2 | D2H_1 | ... | D2H_last
    // (a pageable copy blocks the host until it is done -- so each is issued where the device has other work queued).
    // Chunk 0 is SMALL (112 tiles = two rounds of the register-resident trunk): its upload is short, so the device starts early,
    // and its trunk runs while the next chunk's tiles arrive and its encoder / Modulator run beside it: 8 slices per call 2.57 -> 2.27 ms.
    // Every chunk but the last takes the register-resident trunk (room beside it for the next chunk's prologue), the last one the
    // weight-stationary trunk (the faster kernel; nothing is left to run beside it but the previous chunk's download).  Below the
    // threshold ONE chunk whose kernels read / write page-locked caller buffers in place is faster: 800 tiles 658 against 818 us,
    // 1600 tiles 1220 against 1227, 3200 tiles 2353 against 2284 (profiles/r5/04_host_call_pipelining.txt).  All trunk and prologue
    // instances give the same bits, so the cut does not change results (tests/test_gpu_host_calls.py).
    using Chunk = msiren::HostChunk;
    std::vector<Chunk> plan;
    const int cur0 = h->cur;
    const bool pipelined = msiren::host_call_pipelines(h->dh, B);
    if (pipelined) plan = msiren::pipelined_host_plan(B, h->host_first, h->host_piece, cur0);  // (host_plan.h: unit-tested on the CPU)
    else plan.push_back({0, B, cur0, 0, false});
    const int nchunks = (int)plan.size();
    const size_t tile_elems = (size_t)h->O * h->O;
    // In place (round 5): where the caller's OUTPUT array is page-locked memory (msiren_host_alloc; the Python mirror's outputs come from a
    // recycling pool of such blocks by default; a pinned torch tensor) the trunk stores its 0.9 MB per slice straight into it over the course
    // of its 265 us -- no download, no wait for one behind the stream; page-locked TILES are read in place by the conv kernel.  Pageable
    // memory (a plain numpy array) is copied by the runtime.  One-chunk calls only: same box, 400 tiles: 390 us with both copies, 369 with
    // the output in place, 360 with the tiles in place as well; a cut call of 3 200 tiles: 2.24 ms with copies (they run beside the other
    // chunk's kernels anyway), 2.35-2.87 ms in place (profiles/r5/04_host_call_pipelining.txt).
    // Who copies (a range that is page-locked in part goes through a bounce buffer either way: host_range_kind):
    //   own   a cut call (nchunks > 1): never in place; this function enqueues every chunk's upload and download itself, on that chunk's
    //         stream (HOST_OWN_COPIES: the helper classifies, bounces, reserves the staging and waits);
    //   !own  one chunk: in place where page-locked, else the helper's copies -- the upload in begin(), the download in finish() -- so
    //         the loop's H2D and the `download` lambda below have nothing to enqueue (they still take the trace's stamps: for one chunk
    //         `h2d` is the time behind classification and upload, `d2h` the time at which finish() is about to be called).
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    auto us = [&]() { return std::chrono::duration<double, std::micro>(clk::now() - t0).count(); };
    const bool own = nchunks > 1;
    SyncHostCall io(h, cur0, true);
    const int i_t = io.in(tiles_host, nt, own ? HOST_OWN_COPIES : HOST_IN_PLACE), o_out = io.out(out_host, no, own ? HOST_OWN_COPIES : HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    tiles_host = io.host_src<float>(i_t);
    out_host = io.host_dst<float>(o_out);
    const float* const d_tiles = io.src<float>(i_t);
    float* const out_base = io.dst<float>(o_out);
    std::vector<double> tr_h2d(nchunks, 0.0), tr_launch(nchunks, 0.0), tr_d2h(nchunks, 0.0);
    HostCheck hc;
    Call call = make_call(h, true);
    call.mode.host_check = nchunks == 1;
    call.hc = &hc;
    auto download = [&](int k) {
        const Chunk& c = plan[k];
        tr_d2h[k] = us();
        if (!own) return;  // (finish() downloads what one chunk did not store in place)
        hipError_t e = hipMemcpyAsync(out_host + (size_t)c.lo * h->P, out_base + (size_t)c.lo * h->P, (size_t)c.n * h->P * sizeof(float),
                                      hipMemcpyDeviceToHost, h->sc[c.stream].s);
        if (e != hipSuccess && !rc) rc = fail(MSIREN_E_HIP, "hipMemcpyAsync(D2H): %s", hipGetErrorString(e));
        tr_d2h[k] = us();
    };
    for (int k = 0; k < nchunks && !rc; ++k) {
        const Chunk& c = plan[k];
        call.stream = c.stream;
        call.mode.trunk = c.trunk;
        call.mode.beside = c.beside;
        const float* d_t = d_tiles + (size_t)c.lo * tile_elems;
        if (own) {
            hipError_t e = hipMemcpyAsync((void*)d_t, tiles_host + (size_t)c.lo * tile_elems, (size_t)c.n * tile_elems * sizeof(float), hipMemcpyHostToDevice, h->sc[c.stream].s);
            if (e != hipSuccess) rc = fail(MSIREN_E_HIP, "hipMemcpyAsync(H2D): %s", hipGetErrorString(e));
        }
        tr_h2d[k] = us();
        // (the weight-stationary trunk owns its CUs: queued beside the previous chunk's conditional exact-fp32 launch it would start first,
        //  and that launch -- and the download behind it -- would wait for it to end)
        call.trunk_wait = pipelined && c.trunk == 2 && k >= 1 ? h->sc[plan[k - 1].stream].ev_join : nullptr;
        if (!rc) rc = forward_tiles_dev(h, call, d_t, c.n, out_base + (size_t)c.lo * h->P);
        if (pipelined && !rc) {
            auto& sc = h->sc[c.stream];
            if (!sc.ev_join) { hipError_t e2 = hipEventCreateWithFlags(&sc.ev_join, hipEventDisableTiming); if (e2 != hipSuccess) rc = fail(MSIREN_E_HIP, "hipEventCreate: %s", hipGetErrorString(e2)); }
            if (!rc) { hipError_t e2 = hipEventRecord(sc.ev_join, sc.s); if (e2 != hipSuccess) rc = fail(MSIREN_E_HIP, "hipEventRecord: %s", hipGetErrorString(e2)); }
        }
        tr_launch[k] = us();
        // (pipelined: the previous chunk's download is issued once this chunk's work is queued behind it on the other stream;
        //  otherwise all downloads follow all launches, as a pageable D2H blocks the host until its chunk is done)
        if (pipelined && k >= 1 && !rc) download(k - 1);
    }
    for (int k = pipelined ? nchunks - 1 : 0; k < nchunks && !rc; ++k) download(k);
    if (!rc) rc = io.finish();
    if (!rc) rc = io.recheck(hc, CoordSet{});  // (the domain check: one-chunk calls only, hc is armed by them)
    if (h->trace_host) {  // (whatever the outcome; a call that failed is drained by the helper when it goes)
        std::fprintf(stderr, "msiren_forward_tiles B=%lld chunks=%d%s (us since entry): ", (long long)B, nchunks, pipelined ? " pipelined" : "");
        for (int k = 0; k < nchunks; ++k) std::fprintf(stderr, "[%lld tiles: h2d %.0f launched %.0f d2h %.0f] ", (long long)plan[k].n, tr_h2d[k], tr_launch[k], tr_d2h[k]);
        std::fprintf(stderr, "synced %.0f\n", us());
    }
    return rc;
}

int msiren_forward_tiles(msiren_handle h, const float* tiles_host, int64_t B, float* out_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return take_range_flag_after(h, msiren_forward_tiles_impl(h, tiles_host, B, out_host));
}

// out_stride: 0 or inner_patch_size = the model's own output side; another: msiren_reconstruct_slices_scaled
static int msiren_reconstruct_slices_impl(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, float* recon_host,
                                          int32_t out_stride = 0) {
    int rc = check(h);
    if (rc) return rc;
    if (out_stride == 0) out_stride = h->I;
    if (n < 0 || (n > 0 && (!images_host || !recon_host))) return fail(MSIREN_E_INVALID, "bad arguments");
    if (n == 0) return 0;
    int32_t nV, nH;
    if ((rc = msiren_recon_shape(h, height, width, &nV, &nH))) return rc;
    const size_t ni = (size_t)n * height * width * sizeof(float);
    const size_t nr = (size_t)n * nV * out_stride * nH * out_stride * sizeof(float);
    // As in msiren_forward_tiles: where the caller's reconstruction array is page-locked memory (the Python mirror's outputs are, by default)
    // the fold stores straight into it; the image always arrives by a copy (host_buffers.h: HOST_COPY).
    Call c = make_call(h, true);
    OutGeom og;
    if (out_stride != h->I && (rc = scaled_call(h, c, out_stride, &og))) return rc;
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), o_rec = io.out(recon_host, nr, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    if ((rc = reconstruct_slices(h, c, io.src<float>(i_img), n, height, width, io.dst<float>(o_rec), out_stride != h->I ? &og : nullptr))) return rc;
    return io.finish();
}

int msiren_reconstruct_slices(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, float* recon_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return take_range_flag_after(h, msiren_reconstruct_slices_impl(h, images_host, n, height, width, recon_host));
}

int msiren_reconstruct_slices_scaled(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, int32_t out_stride,
                                     float* recon_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    if (out_stride < 1) return fail(MSIREN_E_INVALID, "out_stride must be positive, got %d", out_stride);
    return take_range_flag_after(h, msiren_reconstruct_slices_impl(h, images_host, n, height, width, recon_host, out_stride));
}

int msiren_set_streams(msiren_handle h, int32_t n) {
    int rc = check(h, false);
    if (rc) return rc;
    if (n < 1 || n > 3) return fail(MSIREN_E_INVALID, "streams must be 1, 2 or 3, got %d", n);
    if ((rc = sync_all(h))) return rc;
    h->nstreams = n;
    h->cur = 0;
    return 0;
}

int msiren_sync(msiren_handle h) {
    int rc = check(h, false);
    if (rc) return rc;
    if ((rc = sync_all(h))) return rc;
    return 0;
}

int msiren_dev_alloc(msiren_handle h, size_t bytes, void** dev_ptr) {
    int rc = check(h, false);
    if (rc) return rc;
    if (!dev_ptr) return fail(MSIREN_E_INVALID, "null argument");
    *dev_ptr = nullptr;
    if (bytes == 0) return 0;
    HIPCHK(hipMalloc(dev_ptr, bytes));
    return 0;
}

int msiren_dev_free(msiren_handle h, void* dev_ptr) {
    int rc = check(h, false);
    if (rc) return rc;
    if (dev_ptr) {
        if ((rc = sync_all(h))) return rc;
        HIPCHK(hipFree(dev_ptr));
    }
    return 0;
}

int msiren_host_alloc(msiren_handle h, size_t bytes, void** host_ptr) {
    int rc = check(h, false);
    if (rc) return rc;
    if (!host_ptr) return fail(MSIREN_E_INVALID, "null argument");
    *host_ptr = nullptr;
    if (bytes == 0) return 0;
    HIPCHK(hipHostMalloc(host_ptr, bytes, hipHostMallocDefault));
    return 0;
}

int msiren_host_free(msiren_handle h, void* host_ptr) {
    if (!h) {  // a block that has outlived its handle (msiren_destroy waited for the handle's streams: nothing of it is in flight)
        if (host_ptr) HIPCHK(hipHostFree(host_ptr));
        return 0;
    }
    int rc = check(h, false);
    if (rc) return rc;
    if (host_ptr) {
        if ((rc = sync_all(h))) return rc;  // (a copy to or from it may still be in flight)
        HIPCHK(hipHostFree(host_ptr));
    }
    return 0;
}

int msiren_memcpy_h2d(msiren_handle h, void* dst_dev, const void* src_host, size_t bytes) {
    int rc = check(h, false);
    if (rc) return rc;
    if (bytes == 0) return 0;
    if ((rc = sync_all(h))) return rc;
    // (to the helper a null host pointer is an output left out and a null device side is staging: neither may be null here)
    if (!dst_dev || !src_host) return fail(MSIREN_E_HIP, "msiren_memcpy_h2d: null pointer (invalid argument)");
    SyncHostCall io(h, h->cur);
    io.in(src_host, bytes, HOST_COPY, dst_dev);
    return (rc = io.begin()) ? rc : io.finish();
}

int msiren_memcpy_d2h(msiren_handle h, void* dst_host, const void* src_dev, size_t bytes) {
    int rc = check(h, false);
    if (rc) return rc;
    if (bytes == 0) return 0;
    if ((rc = sync_all(h))) return rc;
    if (!dst_host || !src_dev) return fail(MSIREN_E_HIP, "msiren_memcpy_d2h: null pointer (invalid argument)");  // (as msiren_memcpy_h2d)
    SyncHostCall io(h, h->cur);
    io.out(dst_host, bytes, HOST_COPY, src_dev);
    return (rc = io.begin()) ? rc : io.finish();
}

int msiren_timer_start(msiren_handle h) {
    int rc = check(h, false);
    if (rc) return rc;
    if ((rc = sync_all(h))) return rc;
    HIPCHK(hipEventRecord(h->ev0, h->sc[0].s));
    return 0;
}

int msiren_timer_stop(msiren_handle h, float* elapsed_ms) {
    int rc = check(h, false);
    if (rc) return rc;
    if ((rc = sync_all(h))) return rc;
    HIPCHK(hipEventRecord(h->ev1, h->sc[0].s));
    HIPCHK(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    if (elapsed_ms) *elapsed_ms = ms;
    return 0;
}

int msiren_profile_enable(msiren_handle h, int32_t on) {
    int rc = check(h, false);
    if (rc) return rc;
    if ((rc = sync_all(h))) return rc;
    h->profile = on != 0;
    h->prof_used = 0;
    h->prof_launches = 0;
    h->prof_ms = 0.0;
    h->prof_kernels.clear();
    return 0;
}

int msiren_profile_read(msiren_handle h, int64_t* launches, double* trunk_ms_total) {
    int rc = check(h, false);
    if (rc) return rc;
    if ((rc = sync_all(h))) return rc;
    if ((rc = profile_collect(h))) return rc;
    if (launches) *launches = h->prof_launches;
    if (trunk_ms_total) *trunk_ms_total = h->prof_ms;
    return 0;
}

int msiren_profile_read_kernel(msiren_handle h, int32_t index, char* name128, int64_t* launches, double* ms_total, int64_t* coords_total) {
    int rc = check(h, false);
    if (rc) return rc;
    if ((rc = sync_all(h))) return rc;
    if ((rc = profile_collect(h))) return rc;
    if (index < 0 || index >= (int32_t)h->prof_kernels.size())
        return fail(MSIREN_E_INVALID, "profile: %d trunk instance(s) were launched since msiren_profile_enable, index %d asked for",
                    (int)h->prof_kernels.size(), index);
    const auto& k = h->prof_kernels[index];
    if (name128) std::snprintf(name128, 128, "%s", k.name.c_str());
    if (launches) *launches = k.launches;
    if (ms_total) *ms_total = k.ms;
    if (coords_total) *coords_total = k.coords;
    return 0;
}

int msiren_last_trunk_kernel(msiren_handle h, char* name128) {
    if (!h || !name128) return fail(MSIREN_E_INVALID, "null argument");
    std::snprintf(name128, 128, "%s", h->last_trunk);
    return 0;
}

int msiren_last_prologue_kernel(msiren_handle h, char* name128) {
    if (!h || !name128) return fail(MSIREN_E_INVALID, "null argument");
    std::snprintf(name128, 128, "%s", h->last_prologue);
    return 0;
}

int msiren_device_info(msiren_handle h, char* name256, int32_t* cus, int32_t* mhz, uint64_t* hbm) {
    int rc = check(h, false);
    if (rc) return rc;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, h->cfg.device));
    if (name256) {
        std::snprintf(name256, 256, "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (cus) *cus = prop.multiProcessorCount;
    if (mhz) *mhz = prop.clockRate / 1000;
    if (hbm) *hbm = (uint64_t)prop.totalGlobalMem;
    return 0;
}

int msiren_runtime_info(int32_t* runtime_version, int32_t* built_against, int32_t* driver_version, char* lib_path, size_t lib_path_bytes) {
    // Which HIP runtime this process's libmsiren calls end up in.  The library's only HIP dependency is NEEDED libamdhip64.so.7; a
    // PyTorch-ROCm wheel ships its own libamdhip64.so under the SAME soname (torch/lib, ROCm 7.0 in this image), so in a process that
    // imported torch first the dynamic loader resolves every hip* call of this library to torch's copy and its libhsa-runtime64 -- not
    // to /opt/rocm's.  dladdr on a HIP entry point names the file that is really mapped.
    int rv = 0, dv = 0;
    if (hipRuntimeGetVersion(&rv) != hipSuccess) { (void)hipGetLastError(); rv = 0; }
    if (hipDriverGetVersion(&dv) != hipSuccess) { (void)hipGetLastError(); dv = 0; }
    if (runtime_version) *runtime_version = rv;
    if (built_against) *built_against = HIP_VERSION;
    if (driver_version) *driver_version = dv;
    if (lib_path && lib_path_bytes) {
        Dl_info di{};
        const char* name = (dladdr((void*)&hipGetDeviceCount, &di) && di.dli_fname) ? di.dli_fname : "";
        std::snprintf(lib_path, lib_path_bytes, "%s", name);
    }
    return 0;
}

int msiren_host_range_kind(const void* host_ptr, size_t bytes, int32_t* kind) {
    if (!kind) return fail(MSIREN_E_INVALID, "null argument");
    void* dev = nullptr;
    *kind = (int32_t)host_range_kind(host_ptr, bytes, &dev);
    return 0;
}

int msiren_device_pci(msiren_handle h, char* busid32) {
    int rc = check(h, false);
    if (rc) return rc;
    if (!busid32) return fail(MSIREN_E_INVALID, "null argument");
    HIPCHK(hipDeviceGetPCIBusId(busid32, 32, h->cfg.device));
    return 0;
}

int msiren_range_events(msiren_handle h, int64_t* count) {
    if (!h || !count) return fail(MSIREN_E_INVALID, "null argument");
    *count = h->range_events;
    return 0;
}

int msiren_flops_per_coord(msiren_handle h, double* flops) {
    if (!h || !flops) return fail(MSIREN_E_INVALID, "null argument");
    const double H = h->H, L = h->L;
    *flops = 2.0 * 2.0 * H + (L - 1.0) * 2.0 * H * H + 2.0 * H;
    return 0;
}

}  // extern "C"
