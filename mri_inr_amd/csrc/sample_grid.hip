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

// the call's coordinate set: device coordinates as given, the table (16-bit trunks) built into the stream's scratch in front of the trunk;
// `table` false (the gradient calls: the jet trunk forms layer 0 itself): the coordinates as they are
int attach_coords(msiren_ctx* h, Call& c, const float* coords_dev, int64_t Q, bool table = true) {
    if (int rc = check_pairs_aligned(coords_dev, "coordinates")) return rc;
    CoordSet cs{coords_dev, nullptr, (int)Q};
    if (table && needs_table(h)) {
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
// on that stream, so whatever the stream runs next sees them) and kept until msiren_commit_weights.  `table` false (the gradient calls:
// the exact-fp32 jet trunk reads the coordinates): no layer-0 table is built; a later call that needs it adds it to the kept lattice.
int get_lattice(msiren_ctx* h, int s, int32_t out_stride, const Lattice** out, bool table = true) {
    auto& sc = h->sc[s];
    table = table && needs_table(h);
    for (Lattice& l : sc.lattices)
        if (l.out_stride == out_stride) {
            if (table && !l.table) {
                const size_t Q = (size_t)l.tile * l.tile;
                if (hipMalloc((void**)&l.table, (size_t)h->H * Q * sizeof(float)) != hipSuccess) {
                    l.table = nullptr;
                    return fail(MSIREN_E_NOMEM, "no device memory for the lattice of out_stride=%d: %s", out_stride, hipGetErrorString(hipGetLastError()));
                }
                const int rc = launch_table(h, s, l.coords, (int)Q, l.table);
                if (rc) return rc;
            }
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
        (table && hipMalloc((void**)&k.table, (size_t)h->H * Q * sizeof(float)) != hipSuccess))
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
    if (tiles && (rc = check_tile_size(h))) return rc;
    if (B == 0) return 0;
    HostCheck hc;
    Call c = make_call(h, true);
    c.mode.host_check = true;
    c.hc = &hc;
    auto& sc = h->sc[c.stream];
    const size_t nc = (size_t)Q * 2 * sizeof(float), no = (size_t)B * Q * sizeof(float);
    const size_t ni = tiles ? (size_t)B * h->O * h->O * sizeof(float) : (size_t)h->L * B * h->H * sizeof(float);
    if ((rc = ensure(h, sc.coords, nc)) || (!tiles && (rc = ensure(h, sc.mods, ni)))) return rc;
    SyncHostCall io(h, c.stream);
    const int i_c = io.in(coords_host, nc, HOST_COPY, sc.coords.p);
    const int i_in = tiles ? io.in(in_host, ni, HOST_IN_PLACE) : io.in(in_host, ni, HOST_COPY, sc.mods.p);
    const int o_out = io.out(out_host, no, HOST_IN_PLACE);
    if ((rc = io.begin()) || (rc = attach_coords(h, c, io.src<float>(i_c), Q))) return rc;  // (the coordinates are on the stream in front of the table kernel)
    const float* const d_in = io.src<float>(i_in);
    float* const d_out = io.dst<float>(o_out);
    if ((rc = tiles ? forward_tiles_dev(h, c, d_in, B, d_out) : launch_trunk(h, c, d_in, B, d_out)) || (rc = io.finish())) return rc;
    return io.recheck(hc, c.cs);
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
    if (tiles && (rc = check_tile_size(h))) return rc;
    if (B == 0) return 0;
    if ((rc = attach_coords(h, c, coords_dev, Q))) return rc;
    return tiles ? forward_tiles_dev(h, c, in_dev, B, out_dev) : launch_trunk(h, c, in_dev, B, out_dev);
}

// ---- value and spatial gradient: the exact-fp32 jet trunk on handles of every precision (siren_trunk_f32_jet.hip.h) -----------------

int check_grad_args(msiren_ctx* h, const float* coords, int64_t Q, const float* in, int64_t B, const float* grad, bool tiles) {
    int rc = check_coords(coords, Q);
    if (rc || (rc = jet_supported(h))) return rc;
    if (B < 0 || (B > 0 && (!in || !grad))) return fail(MSIREN_E_INVALID, "bad arguments (B=%lld)", (long long)B);
    if (tiles && (rc = check_tile_size(h))) return rc;
    return 0;
}

// [encoder -> Modulator ->] jet trunk on the call's stream
int grad_dev_impl(msiren_ctx* h, const Call& c, const float* in_dev, int64_t B, float* out_dev, float* grad_dev, bool tiles) {
    const float* mods = in_dev;
    if (tiles) {
        if (!h->have_encoder || !h->have_modulator) return fail(MSIREN_E_STATE, "encoder.* / modulator.* weights were not loaded");
        auto& sc = h->sc[c.stream];
        int rc = ensure(h, sc.mods, (size_t)h->L * B * h->H * sizeof(float));
        if (rc || (rc = encode_modulate_dev(h, c, in_dev, B, nullptr, (float*)sc.mods.p))) return rc;
        mods = (const float*)sc.mods.p;
    }
    return launch_trunk_f32_jet(h, c, mods, B, out_dev, grad_dev, 1.0f);
}

int sample_grad_dev(msiren_ctx* h, const float* coords_dev, int64_t Q, const float* in_dev, int64_t B, float* out_dev, float* grad_dev, bool tiles) {
    int rc = check(h);
    if (rc || (rc = check_grad_args(h, coords_dev, Q, in_dev, B, grad_dev, tiles))) return rc;
    if ((rc = check_pairs_aligned(coords_dev, "coordinates"))) return rc;
    if (B == 0) return 0;
    Call c = dev_call(h);
    if ((rc = attach_coords(h, c, coords_dev, Q, false))) return rc;
    return grad_dev_impl(h, c, in_dev, B, out_dev, grad_dev, tiles);
}

// one synchronous one-chunk call on host pointers, as sample_host_impl: coords + (tiles | mods) -> [out], grad
int sample_grad_host(msiren_ctx* h, const float* coords_host, int64_t Q, const float* in_host, int64_t B, float* out_host, float* grad_host, bool tiles) {
    int rc = check(h);
    if (rc || (rc = check_grad_args(h, coords_host, Q, in_host, B, grad_host, tiles))) return rc;
    if (B == 0) return 0;
    Call c = make_call(h, true);
    auto& sc = h->sc[c.stream];
    const size_t nc = (size_t)Q * 2 * sizeof(float), no = (size_t)B * Q * sizeof(float);
    const size_t ni = tiles ? (size_t)B * h->O * h->O * sizeof(float) : (size_t)h->L * B * h->H * sizeof(float);
    if ((rc = ensure(h, sc.coords, nc))) return rc;
    SyncHostCall io(h, c.stream);
    const int i_c = io.in(coords_host, nc, HOST_COPY, sc.coords.p);
    // (page-locked tiles are read in place; modulations go to staging: sc.mods is where the _tiles form's prologue writes)
    const int i_in = io.in(in_host, ni, tiles ? HOST_IN_PLACE : HOST_COPY);
    const int o_out = io.out(out_host, no, HOST_IN_PLACE), o_grad = io.out(grad_host, 2 * no, HOST_IN_PLACE);
    if ((rc = io.begin()) || (rc = attach_coords(h, c, io.src<float>(i_c), Q, false))) return rc;
    if ((rc = grad_dev_impl(h, c, io.src<float>(i_in), B, io.dst<float>(o_out), io.dst<float>(o_grad), tiles))) return rc;
    return io.finish();
}

// The slice pipeline with its gradient at output stride out_stride: coordinates, fold geometry and the factor d/r that turns a gradient per
// coordinate unit into one per OUTPUT PIXEL (d = 2/(S-1): one pixel of the model's grid; r = I'/I), fp64 rounded once.  out_stride =
// inner_patch_size is the model's own grid and fold weights.
int grad_slices_call(msiren_ctx* h, Call& c, int32_t out_stride, OutGeom* og, float* gscale) {
    if (out_stride < 1) return fail(MSIREN_E_INVALID, "out_stride must be positive, got %d", out_stride);
    if (out_stride == h->I) {
        c = with_coords(c, CoordSet{h->d_grid, nullptr, h->P});
        *og = OutGeom{h->S, h->I, (h->S - h->I) / 2, h->d_foldw};
    } else {
        const int rc = scaled_call(h, c, out_stride, og, false);
        if (rc) return rc;
    }
    const double d = 2.0 / (double)(h->S - 1), r = (double)out_stride / (double)h->I;
    *gscale = (float)(d / r);
    return 0;
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

int scaled_call(msiren_ctx* h, Call& c, int32_t out_stride, OutGeom* og, bool table) {
    const Lattice* l;
    int rc = get_lattice(h, c.stream, out_stride, &l, table);
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

int msiren_sample_grad_mods(msiren_handle h, const float* coords_host, int64_t Q, const float* mods_host, int64_t B, float* out_host, float* grad_host) {
    return sample_grad_host(h, coords_host, Q, mods_host, B, out_host, grad_host, false);
}
int msiren_sample_grad_mods_dev(msiren_handle h, const float* coords_dev, int64_t Q, const float* mods_dev, int64_t B, float* out_dev, float* grad_dev) {
    return sample_grad_dev(h, coords_dev, Q, mods_dev, B, out_dev, grad_dev, false);
}
int msiren_sample_grad_tiles(msiren_handle h, const float* coords_host, int64_t Q, const float* tiles_host, int64_t B, float* out_host, float* grad_host) {
    return sample_grad_host(h, coords_host, Q, tiles_host, B, out_host, grad_host, true);
}
int msiren_sample_grad_tiles_dev(msiren_handle h, const float* coords_dev, int64_t Q, const float* tiles_dev, int64_t B, float* out_dev, float* grad_dev) {
    return sample_grad_dev(h, coords_dev, Q, tiles_dev, B, out_dev, grad_dev, true);
}

int msiren_reconstruct_slices_grad_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, int32_t out_stride,
                                       float* recon_dev, float* grad_dev) {
    int rc = check(h);
    if (rc || (rc = jet_supported(h))) return rc;
    if (n < 0 || (n > 0 && (!images_dev || !grad_dev))) return fail(MSIREN_E_INVALID, "bad arguments");
    if (n == 0) return 0;
    Call c = dev_call(h);
    OutGeom og;
    GradOut go{grad_dev, 1.f};
    if ((rc = grad_slices_call(h, c, out_stride, &og, &go.gscale))) return rc;
    return reconstruct_slices(h, c, images_dev, n, height, width, recon_dev, &og, &go);
}

int msiren_reconstruct_slices_grad(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, int32_t out_stride,
                                   float* recon_host, float* grad_host) {
    int rc = check(h);
    if (rc || (rc = jet_supported(h))) return rc;
    if (n < 0 || (n > 0 && (!images_host || !grad_host))) return fail(MSIREN_E_INVALID, "bad arguments");
    if (n == 0) return 0;
    if (out_stride < 1) return fail(MSIREN_E_INVALID, "out_stride must be positive, got %d", out_stride);
    int32_t nV, nH;
    if ((rc = msiren_recon_shape(h, height, width, &nV, &nH))) return rc;
    const size_t ni = (size_t)n * height * width * sizeof(float);
    const size_t nr = (size_t)n * nV * out_stride * nH * out_stride * sizeof(float);
    Call c = make_call(h, true);
    OutGeom og;
    GradOut go;
    if ((rc = grad_slices_call(h, c, out_stride, &og, &go.gscale))) return rc;
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), o_rec = io.out(recon_host, nr, HOST_IN_PLACE), o_grad = io.out(grad_host, 2 * nr, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    go.grad = io.dst<float>(o_grad);
    if ((rc = reconstruct_slices(h, c, io.src<float>(i_img), n, height, width, io.dst<float>(o_rec), &og, &go))) return rc;
    return io.finish();
}

}  // extern "C"
