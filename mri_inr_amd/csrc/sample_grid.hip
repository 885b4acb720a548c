// The representation off its own grid (include/msiren.h): msiren_sample_* -- SirenNet.forward at coordinates the
// caller chooses -- and the slice pipeline at another output stride (msiren_upsampled_*, the *_scaled_dev entry points).  What is new on
// the device is the call's layer-0 table (sample_grid.hip.h); everything else is the existing launch sequence run with the call's
// coordinate set (Call::cs) in place of the handle's.
#include "host_buffers.h"
#include "host_ctx.h"
#include "sample_grid.hip.h"

using namespace mh;

namespace {

constexpr int64_t kMaxCoords = 65536;  // the table is 4 H bytes per coordinate: <= 64 MB at H = 256

// the 16-bit trunks read layer 0 from a table; the fp32 trunk forms it from the coordinates
bool needs_table(const msiren_ctx* h) { return h->dh.x1_ready || msiren::use_f16x3(h->dh); }

int launch_table(msiren_ctx* h, int s, const float* coords_dev, int Q, float* table) {
    msiren::Layer0TableParams p{coords_dev, h->d_w0raw, h->d_b0raw, table, Q, h->H / 4, h->cfg.w0_initial, h->cfg.activation == MSIREN_ACT_MORLET ? 1 : 0};
    const int64_t n = (int64_t)p.groups * Q;
    hipLaunchKernelGGL(msiren::layer0_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->sc[s].s, p);
    HIPCHK(hipGetLastError());
    return 0;
}

int check_coords(const float* coords, int64_t Q) {
    if (Q < 1 || Q > kMaxCoords) return fail(MSIREN_E_INVALID, "the number of coordinates must be in [1, %lld], got %lld", (long long)kMaxCoords, (long long)Q);
    if (!coords) return fail(MSIREN_E_INVALID, "null coordinates");
    return 0;
}

// the call's coordinate set: device coordinates as given, the table (16-bit trunks) built into the stream's scratch in front of the trunk
int attach_coords(msiren_ctx* h, Call& c, const float* coords_dev, int64_t Q) {
    if ((uintptr_t)coords_dev % 8) return fail(MSIREN_E_INVALID, "device coordinates must be 8-byte aligned (they are read as (row, column) pairs)");
    CoordSet cs{coords_dev, nullptr, (int)Q};
    if (needs_table(h)) {
        auto& sc = h->sc[c.stream];
        hipEvent_t e1 = nullptr;  // (msiren_profile_enable: the table kernel is reported beside the trunks, under its own name)
        int rc = ensure(h, sc.l0tab, (size_t)h->H * Q * sizeof(float));
        if (rc || (rc = profile_begin(h, c.stream, &e1)) || (rc = launch_table(h, c.stream, coords_dev, (int)Q, (float*)sc.l0tab.p)) ||
            (rc = profile_end(h, c.stream, e1, Q, "layer0_table_kernel")))
            return rc;
        cs.table = (const float*)sc.l0tab.p;
    }
    c = with_coords(c, cs);
    return 0;
}

// msiren_upsampled_geometry's rule; 0 or the error code
int geometry(int32_t S, int32_t I, int32_t out_stride, int32_t* tile, int32_t* pad) {
    if (S < 2 || I < 1 || out_stride < 1) return fail(MSIREN_E_INVALID, "need siren_patch_size >= 2, inner_patch_size >= 1, out_stride >= 1; got %d, %d, %d", S, I, out_stride);
    const int64_t num = (int64_t)S * out_stride;
    const int64_t t = num / I;
    if (num % I != 0 || t < 2 || (t - out_stride) % 2 != 0 || t < out_stride || t * t > kMaxCoords)
        return fail(MSIREN_E_INVALID,
                    "out_stride=%d does not fit siren_patch_size=%d at inner_patch_size=%d: the output tile S*out_stride/I and the fold padding "
                    "(tile - out_stride)/2 must be integers, 2 <= tile <= 256",
                    out_stride, S, I);
    if (tile) *tile = (int32_t)t;
    if (pad) *pad = (int32_t)((t - out_stride) / 2);
    return 0;
}

// lin'[j] = (-1 - d/2) + (d/r)(j + 1/2): fp64, every operation rounded on its own (the order is part of the definition), then fp32
void lattice(int32_t S, int32_t I, int32_t out_stride, int32_t tile, float* lin) {
#pragma clang fp contract(off)
    const double d = 2.0 / (double)(S - 1);
    const double r = (double)out_stride / (double)I;
    const double lo = -1.0 - d / 2, step = d / r;
    for (int j = 0; j < tile; ++j) lin[j] = (float)(lo + step * ((double)j + 0.5));
}

using Lattice = msiren_ctx::StreamCtx::Lattice;

// The lattice of an output stride on stream `s`: coordinates, table and fold weights, built on first use (uploads and the table kernel
// on that stream, so whatever the stream runs next sees them) and kept until msiren_commit_weights.
int get_lattice(msiren_ctx* h, int s, int32_t out_stride, const Lattice** out) {
    auto& sc = h->sc[s];
    for (const Lattice& l : sc.lattices)
        if (l.out_stride == out_stride) {
            *out = &l;
            return 0;
        }
    int32_t T, pad;
    int rc = geometry(h->S, h->I, out_stride, &T, &pad);
    if (rc) return rc;
    Lattice l;
    l.out_stride = out_stride, l.tile = T, l.pad = pad;
    const size_t Q = (size_t)T * T;
    l.host.resize(Q * 2);
    std::vector<float> lin(T);
    lattice(h->S, h->I, out_stride, T, lin.data());
    for (int a = 0; a < T; ++a)
        for (int b = 0; b < T; ++b) {
            l.host[((size_t)a * T + b) * 2 + 0] = lin[a];
            l.host[((size_t)a * T + b) * 2 + 1] = lin[b];
        }
    const std::vector<float> w = fold_weight_matrix(T);  // the reference's formula at size S'
    l.host.insert(l.host.end(), w.begin(), w.end());     // [coords (Q, 2)][fold weights (T, T)]
    sc.lattices.push_back(std::move(l));
    Lattice& k = sc.lattices.back();  // (in place first: the uploads read k.host, which has to outlive this call)
    rc = 0;
    if (hipMalloc((void**)&k.coords, Q * 2 * sizeof(float)) != hipSuccess || hipMalloc((void**)&k.foldw, Q * sizeof(float)) != hipSuccess ||
        (needs_table(h) && hipMalloc((void**)&k.table, (size_t)h->H * Q * sizeof(float)) != hipSuccess))
        rc = fail(MSIREN_E_NOMEM, "no device memory for the lattice of out_stride=%d: %s", out_stride, hipGetErrorString(hipGetLastError()));
    else if (hipMemcpyAsync(k.coords, k.host.data(), Q * 2 * sizeof(float), hipMemcpyHostToDevice, sc.s) != hipSuccess ||
        hipMemcpyAsync(k.foldw, k.host.data() + Q * 2, Q * sizeof(float), hipMemcpyHostToDevice, sc.s) != hipSuccess)
        rc = fail(MSIREN_E_HIP, "uploading the lattice of out_stride=%d failed: %s", out_stride, hipGetErrorString(hipGetLastError()));
    if (!rc && k.table) rc = launch_table(h, s, k.coords, (int)Q, k.table);
    if (rc) {  // not kept: the next call builds it again
        (void)hipStreamSynchronize(sc.s);
        for (float* q : {k.coords, k.table, k.foldw})
            if (q) (void)hipFree(q);
        sc.lattices.pop_back();
        return rc;
    }
    *out = &k;
    return 0;
}

// one synchronous one-chunk call on host pointers: coords + (tiles | mods) -> out, as msiren_forward_tiles does below its pipelining
// threshold (page-locked tiles and outputs in place, the domain guard read on the host behind the wait)
int sample_host_impl(msiren_ctx* h, const float* coords_host, int64_t Q, const float* in_host, int64_t B, float* out_host, bool tiles) {
    int rc = check(h);
    if (rc) return rc;
    if ((rc = check_coords(coords_host, Q))) return rc;
    if (B < 0 || (B > 0 && (!in_host || !out_host))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if (tiles && h->O != 32) return fail(MSIREN_E_INVALID, "the custom encoder is hard-wired to 32x32 tiles (siren_encoder.py:499), outer_patch_size=%d", h->O);
    if (B == 0) return 0;
    HostCheck hc;
    Call c = make_call(h, true);
    c.mode.host_check = true;
    c.hc = &hc;
    auto& sc = h->sc[c.stream];
    const size_t nc = (size_t)Q * 2 * sizeof(float), no = (size_t)B * Q * sizeof(float);
    const size_t ni = tiles ? (size_t)B * h->O * h->O * sizeof(float) : (size_t)h->L * B * h->H * sizeof(float);
    DevBuf& in_buf = tiles ? h->ws_tiles : sc.mods;
    if ((rc = ensure(h, sc.coords, nc)) || (rc = ensure(h, in_buf, ni)) || (rc = ensure(h, h->ws_out, no))) return rc;
    const HostSrc csrc(coords_host, nc), src(in_host, ni);
    const HostDst dst(out_host, no);
    HOSTBUF_OK(csrc);
    HOSTBUF_OK(src);
    HOSTBUF_OK(dst);
    DrainOnExit drain(h);
    HIPCHK(hipMemcpyAsync(sc.coords.p, csrc.as<float>(), nc, hipMemcpyHostToDevice, sc.s));
    if ((rc = attach_coords(h, c, (const float*)sc.coords.p, Q))) return rc;
    const float* d_in = tiles ? src.dev<float>() : nullptr;  // (page-locked tiles are read in place; modulations are read once per unit: copied)
    if (!d_in) {
        HIPCHK(hipMemcpyAsync(in_buf.p, src.as<float>(), ni, hipMemcpyHostToDevice, sc.s));
        d_in = (const float*)in_buf.p;
    }
    float* const d_out = dst.dev<float>() ? dst.dev<float>() : (float*)h->ws_out.p;
    if ((rc = tiles ? forward_tiles_dev(h, c, d_in, B, d_out) : launch_trunk(h, c, d_in, B, d_out))) return rc;
    auto download = [&]() -> int {
        if (d_out == (float*)h->ws_out.p) HIPCHK(hipMemcpyAsync(dst.as<float>(), h->ws_out.p, no, hipMemcpyDeviceToHost, sc.s));
        HIPCHK(hipStreamSynchronize(sc.s));
        return 0;
    };
    if ((rc = download())) return rc;
    if (hc.armed && (unsigned)h->status_host[8] == hc.epoch) {
        // a modulation outside the fp16 domain: the batch once more on the exact-fp32 trunk, at the call's coordinates
        Call fix = with_coords(make_call(h, true), c.cs);
        fix.stream = c.stream;
        if ((rc = launch_trunk_f32_cond(h, fix, hc.mods, hc.B, hc.out, h->status_dev + 8, hc.epoch)) || (rc = download())) return rc;
    }
    drain.disarm();
    dst.finish();
    return 0;
}

int sample_host(msiren_ctx* h, const float* coords_host, int64_t Q, const float* in_host, int64_t B, float* out_host, bool tiles) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    const int rc = sample_host_impl(h, coords_host, Q, in_host, B, out_host, tiles);
    (void)take_range_flag(h);  // informational: the outputs are the exact-fp32 trunk's already
    return rc;
}

int sample_dev(msiren_ctx* h, const float* coords_dev, int64_t Q, const float* in_dev, int64_t B, float* out_dev, bool tiles) {
    int rc = check(h);
    if (rc) return rc;
    Call c = dev_call(h);
    if ((rc = check_coords(coords_dev, Q))) return rc;
    if (B < 0 || (B > 0 && (!in_dev || !out_dev))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if (tiles && h->O != 32) return fail(MSIREN_E_INVALID, "the custom encoder is hard-wired to 32x32 tiles (siren_encoder.py:499), outer_patch_size=%d", h->O);
    if (B == 0) return 0;
    if ((rc = attach_coords(h, c, coords_dev, Q))) return rc;
    return tiles ? forward_tiles_dev(h, c, in_dev, B, out_dev) : launch_trunk(h, c, in_dev, B, out_dev);
}

}  // namespace

namespace mh {

void drop_lattices(msiren_ctx* h) {
    for (auto& sc : h->sc) {
        for (auto& l : sc.lattices)
            for (float* q : {l.coords, l.table, l.foldw})
                if (q) (void)hipFree(q);
        sc.lattices.clear();
    }
}

int scaled_call(msiren_ctx* h, Call& c, int32_t out_stride, OutGeom* og) {
    const Lattice* l;
    int rc = get_lattice(h, c.stream, out_stride, &l);
    if (rc) return rc;
    c = with_coords(c, CoordSet{l->coords, l->table, l->tile * l->tile});
    *og = OutGeom{l->tile, l->out_stride, l->pad, l->foldw};
    return 0;
}

}  // namespace mh

extern "C" {

int msiren_upsampled_geometry(int32_t S, int32_t I, int32_t out_stride, int32_t* out_tile, int32_t* pad) {
    return geometry(S, I, out_stride, out_tile, pad);
}

int msiren_upsampled_lattice(int32_t S, int32_t I, int32_t out_stride, float* lin_out) {
    int32_t T;
    int rc = geometry(S, I, out_stride, &T, nullptr);
    if (rc) return rc;
    if (!lin_out) return fail(MSIREN_E_INVALID, "null argument");
    lattice(S, I, out_stride, T, lin_out);
    return 0;
}

int msiren_sample_mods(msiren_handle h, const float* coords_host, int64_t Q, const float* mods_host, int64_t B, float* out_host) {
    return sample_host(h, coords_host, Q, mods_host, B, out_host, false);
}
int msiren_sample_mods_dev(msiren_handle h, const float* coords_dev, int64_t Q, const float* mods_dev, int64_t B, float* out_dev) {
    return sample_dev(h, coords_dev, Q, mods_dev, B, out_dev, false);
}
int msiren_sample_tiles(msiren_handle h, const float* coords_host, int64_t Q, const float* tiles_host, int64_t B, float* out_host) {
    return sample_host(h, coords_host, Q, tiles_host, B, out_host, true);
}
int msiren_sample_tiles_dev(msiren_handle h, const float* coords_dev, int64_t Q, const float* tiles_dev, int64_t B, float* out_dev) {
    return sample_dev(h, coords_dev, Q, tiles_dev, B, out_dev, true);
}

int msiren_reconstruct_slices_scaled_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, int32_t out_stride,
                                         float* recon_dev) {
    int rc = check(h);
    if (rc) return rc;
    if (out_stride == h->I) return msiren_reconstruct_slices_dev(h, images_dev, n, height, width, recon_dev);
    Call c = dev_call(h);
    OutGeom og;
    if ((rc = scaled_call(h, c, out_stride, &og))) return rc;
    return reconstruct_slices(h, c, images_dev, n, height, width, recon_dev, &og);
}

int msiren_reconstruct_tiles_scaled_dev(msiren_handle h, const float* tiles_dev, int64_t n, int32_t nV, int32_t nH, int32_t out_stride, float* recon_dev) {
    int rc = check(h);
    if (rc) return rc;
    if (out_stride == h->I) return msiren_reconstruct_tiles_dev(h, tiles_dev, n, nV, nH, recon_dev);
    Call c = dev_call(h);
    OutGeom og;
    if ((rc = scaled_call(h, c, out_stride, &og))) return rc;
    return reconstruct_tiles_dev(h, c, tiles_dev, n, nV, nH, recon_dev, &og);
}

int msiren_weighted_fold_scaled_dev(msiren_handle h, const float* tiles_dev, int64_t n, int32_t nV, int32_t nH, int32_t out_stride, float* recon_dev) {
    int rc = check(h);
    if (rc) return rc;
    if (out_stride == h->I) return msiren_weighted_fold_dev(h, tiles_dev, n, nV, nH, recon_dev);
    Call c = make_call(h, false);  // the handle's current stream, as msiren_weighted_fold_dev
    OutGeom og;
    if ((rc = scaled_call(h, c, out_stride, &og))) return rc;
    if (n < 0 || nV < 1 || nH < 1 || (n > 0 && (!tiles_dev || !recon_dev))) return fail(MSIREN_E_INVALID, "bad arguments");
    if (n == 0) return 0;
    return weighted_fold_dev(h, c, tiles_dev, n, nV, nH, recon_dev, og);
}

}  // extern "C"
