// One coordinate set per patch (include/msiren.h): msiren_sample_ragged_* -- SirenNet.forward, and its spatial
// gradient, with patch b evaluated at coords[offsets[b] : offsets[b + 1]].  The exact-fp32 trunks, on handles of every precision
// (siren_trunk_f32_ragged.hip.h; the launches: launch_dispatch.hip): a layer-0 table per (patch, coordinate) would be 4 H bytes an entry.
// The *_native value forms run the handle's own trunk arithmetic instead, layer 0 computed in the kernel (launch_trunk_ragged_native).
// msiren_resample_slices*, msiren_resample_volume*, msiren_align_slices*, msiren_align_solve* and their weighted forms msiren_align_slices_w*,
// msiren_align_solve_w*, msiren_align_volume*, msiren_align_volume_solve* and their weighted forms msiren_align_volume_w*, msiren_align_volume_solve_w*,
// the grouped msiren_align_volume_solve_group* and the robust msiren_align_volume_r*, msiren_align_volume_solve_group_r* (DESIGN.md sections
// 5.8 - 5.16) are built on these trunks: the five
// geometry pipelines below (namespace mh), each behind launch_dispatch.hip's slice_prologue on the call's stream, then their host-pointer forms
// and the entry points.  Where each call's scratch sections lie and what it refuses as too large: align_plan.h.
// msiren_align_stack_r* and msiren_align_stack_solve_group_r* (align_stack.hip.h) stand beside them on none of the trunks: the
// robust volume family's reduce and grouped solve with the pixel read trilinearly from a plain voxel stack, on a handle that needs no weights.
#include "host_buffers.h"
#include "host_ctx.h"
#include "align_plan.h"
#include "resample.hip.h"
#include "resample_volume.hip.h"
#include "align.hip.h"
#include "align_w.hip.h"
#include "align_volume.hip.h"
#include "align_volume_w.hip.h"
#include "align_volume_r.hip.h"
#include "align_group.hip.h"
#include "align_stack.hip.h"

namespace mh {

static_assert(kAlignSums == msiren::ALIGN_SUMS && kAlignSumsW == msiren::ALIGN_SUMS_W && kAlignVolumeSums == msiren::ALIGN_VOLUME_SUMS,
              "host and kernels disagree about a record");
static_assert(kAlignVolumeSumsW == msiren::ALIGN_VOLUME_SUMS_W, "host and kernels disagree about a record");
static_assert(msiren::kAlignChunk == msiren::ALIGN_CHUNK, "align_plan.h and the kernels disagree about a chunk");

// ---- what the five pipelines share ------------------------------------------------------------------------------------------------------------
// a slice's tiling as these calls see it: KA x KA tiles at most cover a point, nV x nH tiles per slice
struct Geom { int KA = 0, K = 0; int32_t nV = 0, nH = 0; int64_t NPt = 0; };

// the refusals every geometry call shares, in this order: the tile size, the cover, the reconstruction's shape.  (Each check asks
// jet_supported and its own arguments first.)
static int geom_check(msiren_ctx* h, int32_t height, int32_t width, Geom* g) {
    int rc;
    if ((rc = check_tile_size(h, false))) return rc;
    g->KA = (h->S + h->I - 1) / h->I, g->K = g->KA * g->KA;
    if (g->KA > msiren::RESAMPLE_MAX_KA)
        return fail(MSIREN_E_INVALID, "siren_patch_size=%d over inner_patch_size=%d: more than %d tiles per axis would cover a point", h->S, h->I, msiren::RESAMPLE_MAX_KA);
    if ((rc = msiren_recon_shape(h, height, width, &g->nV, &g->nH))) return rc;
    g->NPt = (int64_t)g->nV * g->nH;
    return 0;
}
static int fail_slices(int64_t n, const Geom& g) {
    return fail(MSIREN_E_INVALID, "too many slices for one call: %lld slices x %d x %d tiles (16 n nV nH must stay below 2^30)", (long long)n, g.nV, g.nH);
}

// a kernel parameter struct's pointers into the block at `base` (align_plan.h)
template <typename P>
static void carve(P& p, char* base, const msiren::GeomLayout& l) {
    p.counts = (int*)(base + l.counts), p.cursors = (int*)(base + l.cursors), p.offsets = (int*)(base + l.offsets);
    p.ent = (int*)(base + l.ent), p.tile = (int*)(base + l.tile), p.coords = (float*)(base + l.coords), p.w = (float*)(base + l.w);
}
static void carve_volume(msiren::ResampleVolumeParams& p, char* base, const msiren::GeomLayout& l) {
    carve(p, base, l);
    p.pair = (int*)(base + l.pair), p.f = (float*)(base + l.f);
}

// the bin bracket, one profile entry `name`: memset of counts and cursors -> count -> scan over the bins -> fill, one thread per point
template <typename P>
static int bin_bracket(msiren_ctx* h, const Call& c, void (*count)(P), void (*fill)(P), const P& p, char* base, const msiren::GeomLayout& l, int64_t bins,
                       int64_t points, const char* name) {
    int rc;
    hipStream_t st = h->sc[c.stream].s;
    const unsigned gm = (unsigned)((points + 255) / 256);
    hipEvent_t e1 = nullptr;
    if ((rc = profile_begin(h, c.stream, &e1))) return rc;
    HIPCHK(hipMemsetAsync(base + l.counts, 0, l.zero_bytes, st));
    hipLaunchKernelGGL(count, dim3(gm), dim3(256), 0, st, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(msiren::resample_scan_kernel, dim3(1), dim3(256), 0, st, (const int*)(base + l.counts), (int)bins, (int*)(base + l.offsets));
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(fill, dim3(gm), dim3(256), 0, st, p);
    HIPCHK(hipGetLastError());
    return profile_end(h, c.stream, e1, points, name);
}

// the filled bins as the ragged trunks take them: T entries in `bins` patches, `reps` replicas, on the plan's rows of the NP tiles
static RaggedSet bins_set(msiren_ctx* h, const Call& c, char* base, const msiren::GeomLayout& l, int64_t T, int64_t bins, int64_t reps, int64_t NP) {
    return RaggedSet{(const float*)(base + l.coords), (const int*)(base + l.offsets), T, bins, reps, (const int*)h->sc[c.stream].plan.p + 2 + NP, NP, (int*)(base + l.items)};
}
static float pixel_gscale(const msiren_ctx* h) { return (float)(2.0 / (double)(h->S - 1)); }  // coordinate units per reconstruction pixel

// ---- the reconstruction at arbitrary points (kernels: resample.hip.h) ------------------------------------------------------
// The slice prologue, then on the same stream bin the points by covering tile -> ragged exact-fp32 trunk (`native`: the handle's own,
// launch_trunk_ragged_native), replicated over the slices, patch s NP + t on the plan's row -> blend.
// `grad`: value (out_dev may be null) and the two gradient planes grad_dev (2, n, M), per reconstruction pixel.
int resample_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t M, bool grad) {
    int rc;
    Geom g;
    if (grad ? (rc = jet_supported(h)) : 0) return rc;
    if (n < 0 || M < 0) return fail(MSIREN_E_INVALID, "bad arguments (n=%lld, M=%lld)", (long long)n, (long long)M);
    if ((rc = geom_check(h, height, width, &g))) return rc;
    if (!msiren::resample_fits(n, M, g.K, g.NPt))
        return fail(MSIREN_E_INVALID, "too many points for one call: %lld points x %d covering tiles x %lld slices (8 M K and 12 n M K must stay below 2^31)",
                    (long long)M, g.K, (long long)n);
    return 0;
}

int resample_slices(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* points_dev, int64_t M,
                    float* out_dev, float* grad_dev, bool grad, bool native) {
    int rc = resample_check(h, n, height, width, M, grad);
    if (rc) return rc;
    if (n > 0 && M > 0 && (!images_dev || !points_dev || (grad ? !grad_dev : !out_dev))) return fail(MSIREN_E_INVALID, "null argument");
    if (n == 0 || M == 0) return 0;
    Geom g;
    (void)geom_check(h, height, width, &g);
    const int K = g.K;
    const int64_t NPt = g.NPt, NP = n * NPt, T = M * K;
    if ((rc = check_pairs_aligned(points_dev, "points")) || (rc = check_reflect_padding(h, height, width))) return rc;
    auto& sc = h->sc[c.stream];
    const msiren::GeomLayout lay = msiren::resample_layout(NPt, M, K);
    if ((rc = ensure(h, sc.patches, (size_t)NP * h->O * h->O * sizeof(float))) || (rc = ensure(h, sc.ragged, lay.total)) ||
        (rc = ensure(h, sc.rec, (size_t)n * T * sizeof(float) * (grad ? 3 : 1))))
        return rc;
    Call pc;
    bool fused;
    if ((rc = slice_prologue(h, c, images_dev, height, width, (float*)sc.patches.p, nullptr, n, g.nV, g.nH, &pc, &fused))) return rc;
    hipStream_t st = sc.s;
    char* const base = (char*)sc.ragged.p;
    msiren::ResampleParams rp{points_dev, (int)M, g.nV, g.nH, h->S, h->I, (h->S - h->I) / 2, g.KA};
    carve(rp, base, lay);
    if ((rc = bin_bracket(h, c, msiren::resample_count_kernel, msiren::resample_fill_kernel, rp, base, lay, NPt, M, "resample_bin_kernels"))) return rc;
    float* const rec = (float*)sc.rec.p;  // [value (n, T)][d/d row][d/d column]
    const RaggedSet r = bins_set(h, c, base, lay, T, NPt, n, NP);
    if (grad) rc = launch_trunk_f32_jet_ragged(h, pc, r, (const float*)sc.mods.p, out_dev ? rec : nullptr, rec + (size_t)n * T, pixel_gscale(h));
    else rc = native ? launch_trunk_ragged_native(h, pc, r, (const float*)sc.mods.p, rec) : launch_trunk_f32_ragged(h, pc, r, (const float*)sc.mods.p, rec);
    hipEvent_t e1 = nullptr;
    if (rc || (rc = profile_begin(h, c.stream, &e1))) return rc;
    const unsigned gb = (unsigned)((n * M + 255) / 256);
    if (out_dev) hipLaunchKernelGGL(msiren::resample_blend_kernel, dim3(gb), dim3(256), 0, st, rec, rp.ent, rp.tile, rp.w, (const int*)sc.keep.p, out_dev, (int)n, (int)M, K, (int)NPt, (int)T, 1);
    if (grad) hipLaunchKernelGGL(msiren::resample_blend_kernel, dim3(gb), dim3(256), 0, st, rec + (size_t)n * T, rp.ent, rp.tile, rp.w, (const int*)sc.keep.p, grad_dev, (int)n, (int)M, K, (int)NPt, (int)T, 2);
    HIPCHK(hipGetLastError());
    return profile_end(h, c.stream, e1, n * M, "resample_blend_kernel");
}

// ---- a stack of slices read as a volume at points (Z, Y, X) (kernels: resample_volume.hip.h) -----------------------------
// The slice prologue, then on the same stream bin the points by (slice, tile) -> the ragged trunk over those n nV nH bins as its patches, one
// replica, on the plan's rows (`native`: launch_trunk_ragged_native) -> blend across tiles and the pair of slices.  Scratch grows with 2 M K,
// not with n.  `grad`: value (out_dev may be null) and the three gradient planes grad_dev (3, M): per slice of Z, per reconstruction pixel rows, columns.
int resample_volume_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t M, bool grad) {
    int rc;
    Geom g;
    if (grad ? (rc = jet_supported(h)) : 0) return rc;
    if (n < 0 || M < 0) return fail(MSIREN_E_INVALID, "bad arguments (n=%lld, M=%lld)", (long long)n, (long long)M);
    if (grad && n == 1) return fail(MSIREN_E_INVALID, "the volume's gradient needs two slices at least (n=1)");
    if ((rc = geom_check(h, height, width, &g))) return rc;
    if (!msiren::volume_points_fit(M, g.K))
        return fail(MSIREN_E_INVALID, "too many points for one call: %lld points x %d covering tiles (32 M K + 8 M must stay below 2^30)", (long long)M, g.K);
    if (!msiren::volume_slices_fit(n, g.NPt)) return fail_slices(n, g);
    return 0;
}

int resample_volume(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* points_dev, int64_t M,
                    float* out_dev, float* grad_dev, bool grad, bool native) {
    int rc = resample_volume_check(h, n, height, width, M, grad);
    if (rc) return rc;
    if (n > 0 && M > 0 && (!images_dev || !points_dev || (grad ? !grad_dev : !out_dev))) return fail(MSIREN_E_INVALID, "null argument");
    if (n == 0 || M == 0) return 0;
    if ((uintptr_t)points_dev % 4) return fail(MSIREN_E_INVALID, "device points must be 4-byte aligned");
    Geom g;
    (void)geom_check(h, height, width, &g);
    const int K = g.K;
    const int64_t NPt = g.NPt, NP = n * NPt, T = 2 * M * K;
    if ((rc = check_reflect_padding(h, height, width))) return rc;
    auto& sc = h->sc[c.stream];
    const msiren::GeomLayout lay = msiren::resample_volume_layout(NP, M, K);
    if ((rc = ensure(h, sc.patches, (size_t)NP * h->O * h->O * sizeof(float))) || (rc = ensure(h, sc.ragged, lay.total)) ||
        (rc = ensure(h, sc.rec, (size_t)T * sizeof(float) * (grad ? 3 : 1))))
        return rc;
    Call pc;
    bool fused;
    if ((rc = slice_prologue(h, c, images_dev, height, width, (float*)sc.patches.p, nullptr, n, g.nV, g.nH, &pc, &fused))) return rc;
    hipStream_t st = sc.s;
    char* const base = (char*)sc.ragged.p;
    msiren::ResampleVolumeParams vp{points_dev, (int)M, (int)n, g.nV, g.nH, h->S, h->I, (h->S - h->I) / 2, g.KA, grad ? 1 : 0};
    carve_volume(vp, base, lay);
    if ((rc = bin_bracket(h, c, msiren::resample_volume_count_kernel, msiren::resample_volume_fill_kernel, vp, base, lay, NP, M, "resample_volume_bin_kernels")))
        return rc;
    float* const rec = (float*)sc.rec.p;  // [value (T)][d/d row][d/d column]
    const RaggedSet r = bins_set(h, c, base, lay, T, NP, 1, NP);
    if (grad) rc = launch_trunk_f32_jet_ragged(h, pc, r, (const float*)sc.mods.p, rec, rec + (size_t)T, pixel_gscale(h));  // (grad[0] needs the values)
    else rc = native ? launch_trunk_ragged_native(h, pc, r, (const float*)sc.mods.p, rec) : launch_trunk_f32_ragged(h, pc, r, (const float*)sc.mods.p, rec);
    hipEvent_t e1 = nullptr;
    if (rc || (rc = profile_begin(h, c.stream, &e1))) return rc;
    hipLaunchKernelGGL(msiren::resample_volume_blend_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, rec, vp.ent, vp.tile, vp.w, (const int*)sc.keep.p,
                       vp.pair, vp.f, out_dev, grad ? grad_dev : nullptr, (int)M, K, (int)NPt, (int)T, grad ? 3 : 1, grad ? 1 : 0);
    HIPCHK(hipGetLastError());
    return profile_end(h, c.stream, e1, M, "resample_volume_blend_kernel");
}

// ---- the four align families (DESIGN.md sections 5.10 - 5.14; kernels: align.hip.h, align_w.hip.h, align_volume.hip.h, align_volume_w.hip.h) --------
// Slices scored under one 2 x 3 map each against their targets (plain: 29 fp64 sums per slice; weighted: 47, with a per-pixel weight and a
// per-slice gain and bias), or m targets under one 3 x 3 map each against the stack read as a volume (56 per target; weighted: 80, with a
// per-pixel weight and a per-target gain and bias).  One path: the slice
// prologue over the n slices, then per evaluation on the same stream the pixels of every target lattice, placed by their map in the kernel,
// binned by (slice, tile) -> the exact-fp32 jet ragged trunk over those n nV nH bins, one replica, on the plan's rows -> per (unit, chunk) the
// blend and the sums -> per unit the chunks in index order.  A unit is a slice (plain, weighted) or a target (volume).  What is launched for
// these four is untouched by the fifth:
// ALIGN_VOLUME_ROBUST (align_volume_r.hip.h): the weighted volume family's layout, bins and limits, its 80 sums formed under
// a Geman-McClure loss with one scale per target.
// ALIGN_STACK (align_stack.hip.h): the robust 80 sums with the pixel read trilinearly from a plain voxel stack.  Its own check
// (align_stack_check) and prepare (align_stack_prepare): no model, no prologue, no bins, no trunk; its scratch is the partials.
enum AlignFamily { ALIGN_PLAIN, ALIGN_WEIGHTED, ALIGN_VOLUME, ALIGN_VOLUME_WEIGHTED, ALIGN_VOLUME_ROBUST, ALIGN_STACK };
static int align_nsums(AlignFamily f) {
    return f == ALIGN_PLAIN ? msiren::ALIGN_SUMS : f == ALIGN_WEIGHTED ? msiren::ALIGN_SUMS_W : f == ALIGN_VOLUME ? msiren::ALIGN_VOLUME_SUMS : msiren::ALIGN_VOLUME_SUMS_W;
}
static bool align_is_volume(AlignFamily f) { return f == ALIGN_VOLUME || f == ALIGN_VOLUME_WEIGHTED || f == ALIGN_VOLUME_ROBUST; }

int align_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int32_t th, int32_t tw) {
    int rc;
    Geom g;
    if ((rc = jet_supported(h))) return rc;
    if (n < 0 || th < 0 || tw < 0) return fail(MSIREN_E_INVALID, "bad arguments (n=%lld, th=%d, tw=%d)", (long long)n, th, tw);
    if ((rc = geom_check(h, height, width, &g))) return rc;
    if (!msiren::align_pixels_fit(n, (int64_t)th * tw, g.K, msiren::ALIGN_SUMS))
        return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld slices x %d x %d target pixels x %d covering tiles (20 n th tw K must stay below 2^30)",
                    (long long)n, th, tw, g.K);
    if (!msiren::bins_fit(n, g.NPt)) return fail_slices(n, g);
    return 0;
}

// the weighted form's partial records are 376 bytes per chunk: the bin scratch and they stay below 2^30 together
int align_w_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int32_t th, int32_t tw) {
    int rc = align_check(h, n, height, width, th, tw);
    if (rc) return rc;
    Geom g;
    (void)geom_check(h, height, width, &g);  // (align_check passed it)
    if (!msiren::align_pixels_fit(n, (int64_t)th * tw, g.K, msiren::ALIGN_SUMS_W))
        return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld slices x %d x %d target pixels x %d covering tiles (20 n th tw K must stay below 2^30)",
                    (long long)n, th, tw, g.K);
    return 0;
}

int align_volume_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t m, int32_t th, int32_t tw) {
    int rc;
    Geom g;
    if ((rc = jet_supported(h))) return rc;
    if (n < 0 || m < 0 || th < 0 || tw < 0) return fail(MSIREN_E_INVALID, "bad arguments (n=%lld, m=%lld, th=%d, tw=%d)", (long long)n, (long long)m, th, tw);
    if (n < 2) return fail(MSIREN_E_INVALID, "a volume needs two slices at least (n=%lld)", (long long)n);
    if ((rc = geom_check(h, height, width, &g))) return rc;
    if (!msiren::align_volume_pixels_fit(m, (int64_t)th * tw, g.K, msiren::ALIGN_VOLUME_SUMS))
        return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld targets x %d x %d pixels x %d covering tiles (32 m th tw K + 8 m th tw must stay below 2^30, m th tw below 2^28)",
                    (long long)m, th, tw, g.K);
    if (!msiren::volume_slices_fit(n, g.NPt)) return fail_slices(n, g);
    return 0;
}

// the weighted volume form's partial records are 640 bytes per chunk: the bin scratch and they stay below 2^30 together
int align_volume_w_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t m, int32_t th, int32_t tw) {
    int rc = align_volume_check(h, n, height, width, m, th, tw);
    if (rc) return rc;
    Geom g;
    (void)geom_check(h, height, width, &g);  // (align_volume_check passed it)
    if (!msiren::align_volume_pixels_fit(m, (int64_t)th * tw, g.K, msiren::ALIGN_VOLUME_SUMS_W))
        return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld targets x %d x %d pixels x %d covering tiles (32 m th tw K + 8 m th tw with 640 bytes per chunk of 1024 pixels must stay below 2^30)",
                    (long long)m, th, tw, g.K);
    return 0;
}

// What align_prepare leaves for align_evaluate: the call's geometry, its scratch layout and the trunk's call state.  Nothing of it lives on the handle.
struct AlignPlan {
    AlignFamily fam = ALIGN_PLAIN;
    int64_t n = 0, units = 0, Mt = 0, M = 0, T = 0, chunks = 0;  // units: n slices or m targets; Mt = th tw; M = units Mt pixels; T entries
    int32_t th = 0, tw = 0;
    Geom g;
    msiren::GeomLayout lay{};  // lay.total: what follows in the stream's scratch is the solve's
    const float* targets = nullptr;
    const float *weights = nullptr, *intensity = nullptr;  // weighted: (units, th, tw) and (units, 2), may be null
    Call pc;
    const double* scale = nullptr;  // robust: (units) doubles
    float* rweight = nullptr;       // robust: (units, th, tw) or null
    const float* stack = nullptr;   // stack family: the voxels (n, height, width); n above
    int32_t height = 0, width = 0;
};

// the family's check, every workspace of the call (`extra` bytes more behind the partials: a solve's state) and the slice prologue.
// `units`: n for the slice families, m for the volume.  *todo = false: nothing to do (no unit or th tw = 0).  No workspace moves after this.
static int align_prepare(msiren_handle h, const Call& c, AlignFamily fam, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev,
                         int64_t units, int32_t th, int32_t tw, const void* maps_dev, const void* sums_dev, size_t extra, AlignPlan* a, bool* todo) {
    *todo = false;
    const bool volume = align_is_volume(fam);
    int rc = volume ? align_volume_check(h, n, height, width, units, th, tw) : align_check(h, n, height, width, th, tw);
    if (rc) return rc;
    const int64_t Mt = (int64_t)th * tw, M = units * Mt;
    if (M > 0 && (!images_dev || !targets_dev || !maps_dev || !sums_dev)) return fail(MSIREN_E_INVALID, "null argument");
    if (M == 0) return 0;
    if ((uintptr_t)targets_dev % 4 || (uintptr_t)maps_dev % 4 || (uintptr_t)sums_dev % 8) return fail(MSIREN_E_INVALID, "device targets and maps must be 4-byte aligned, sums 8-byte aligned");
    Geom g;
    (void)geom_check(h, height, width, &g);
    const int64_t NP = n * g.NPt, T = (volume ? 2 : 1) * M * g.K;
    if ((rc = check_reflect_padding(h, height, width))) return rc;
    auto& sc = h->sc[c.stream];
    const int nsums = align_nsums(fam);
    const msiren::GeomLayout lay = volume ? msiren::align_volume_layout(NP, units, Mt, g.K, nsums) : msiren::align_layout(NP, n, Mt, g.K, nsums);
    if ((rc = ensure(h, sc.patches, (size_t)NP * h->O * h->O * sizeof(float))) || (rc = ensure(h, sc.ragged, lay.total + extra)) || (rc = ensure(h, sc.rec, (size_t)T * sizeof(float) * 3)))
        return rc;
    *a = AlignPlan{fam, n, units, Mt, M, T, msiren::align_chunks(Mt), th, tw, g, lay, targets_dev, nullptr, nullptr, Call()};
    bool fused;
    if ((rc = slice_prologue(h, c, images_dev, height, width, (float*)sc.patches.p, nullptr, n, g.nV, g.nH, &a->pc, &fused))) return rc;
    *todo = true;
    return 0;
}

// one evaluation behind align_prepare, on the same stream: the bin bracket, the trunk, then partial and combine as one profile entry
static int align_evaluate(msiren_handle h, const Call& c, const AlignPlan& a, const float* maps_dev, double* sums_dev, float* warped_dev, float* wgrad_dev) {
    int rc;
    auto& sc = h->sc[c.stream];
    const Geom& g = a.g;
    const int64_t NP = a.n * g.NPt, T = a.T;
    hipStream_t st = sc.s;
    char* const base = (char*)sc.ragged.p;
    if (a.fam == ALIGN_STACK) {  // no bins and no trunk: the partial reads the stack itself.  sums_dev (m, 80)
        double* const partials = (double*)(base + a.lay.partials);
        hipEvent_t e1 = nullptr;
        if ((rc = profile_begin(h, c.stream, &e1))) return rc;
        hipLaunchKernelGGL(msiren::align_stack_partial_r_kernel, dim3((unsigned)(a.units * a.chunks)), dim3(256), 0, st, a.stack, maps_dev, a.targets, a.weights, a.intensity,
                           a.scale, warped_dev, wgrad_dev, a.rweight, partials, (int)a.n, a.height, a.width, (int)a.units, (int)a.Mt, a.tw, (int)a.chunks);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(msiren::align_volume_combine_w_kernel, dim3((unsigned)a.units), dim3(256), 0, st, partials, sums_dev, (int)a.chunks);
        HIPCHK(hipGetLastError());
        return profile_end(h, c.stream, e1, a.M, "align_stack_reduce_kernels");
    }
    msiren::AlignVolumeParams avp{};
    msiren::ResampleVolumeParams& vp = avp.v;
    msiren::AlignParams ap{maps_dev, (int)a.n, a.th, a.tw, (int)a.Mt, g.nV, g.nH, h->S, h->I, (h->S - h->I) / 2, g.KA};
    if (align_is_volume(a.fam)) {
        vp = msiren::ResampleVolumeParams{nullptr, (int)a.M, (int)a.n, g.nV, g.nH, h->S, h->I, (h->S - h->I) / 2, g.KA, 1};
        avp.maps = maps_dev, avp.th = a.th, avp.tw = a.tw, avp.Mt = (int)a.Mt;
        carve_volume(vp, base, a.lay);
        rc = bin_bracket(h, c, msiren::align_volume_count_kernel, msiren::align_volume_fill_kernel, avp, base, a.lay, NP, a.M, "align_volume_bin_kernels");
    } else {
        carve(ap, base, a.lay);
        rc = bin_bracket(h, c, msiren::align_count_kernel, msiren::align_fill_kernel, ap, base, a.lay, NP, a.M, "align_bin_kernels");
    }
    if (rc) return rc;
    float* const rec = (float*)sc.rec.p;  // [value (T)][d/d row][d/d column]
    double* const partials = (double*)(base + a.lay.partials);
    const int* const black = (const int*)sc.keep.p;
    const RaggedSet r = bins_set(h, c, base, a.lay, T, NP, 1, NP);
    hipEvent_t e1 = nullptr;
    if ((rc = launch_trunk_f32_jet_ragged(h, a.pc, r, (const float*)sc.mods.p, rec, rec + (size_t)T, pixel_gscale(h))) || (rc = profile_begin(h, c.stream, &e1))) return rc;
    const dim3 gp((unsigned)(a.units * a.chunks)), gc((unsigned)a.units);
    const char* name;
    if (a.fam == ALIGN_VOLUME_ROBUST) {  // sums_dev (m, 80)
        hipLaunchKernelGGL(msiren::align_volume_partial_r_kernel, gp, dim3(256), 0, st, rec, vp.ent, vp.tile, vp.w, black, vp.pair, vp.f, a.targets, a.weights, a.intensity,
                           a.scale, warped_dev, wgrad_dev, a.rweight, partials, (int)a.units, (int)a.Mt, a.tw, g.K, (int)g.NPt, (int)T, (int)a.chunks);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(msiren::align_volume_combine_w_kernel, gc, dim3(256), 0, st, partials, sums_dev, (int)a.chunks);
        name = "align_volume_reduce_r_kernels";
    } else if (a.fam == ALIGN_VOLUME_WEIGHTED) {  // sums_dev (m, 80)
        hipLaunchKernelGGL(msiren::align_volume_partial_w_kernel, gp, dim3(256), 0, st, rec, vp.ent, vp.tile, vp.w, black, vp.pair, vp.f, a.targets, a.weights, a.intensity,
                           warped_dev, wgrad_dev, partials, (int)a.units, (int)a.Mt, a.tw, g.K, (int)g.NPt, (int)T, (int)a.chunks);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(msiren::align_volume_combine_w_kernel, gc, dim3(256), 0, st, partials, sums_dev, (int)a.chunks);
        name = "align_volume_reduce_w_kernels";
    } else if (a.fam == ALIGN_VOLUME) {  // sums_dev (m, 56)
        hipLaunchKernelGGL(msiren::align_volume_partial_kernel, gp, dim3(256), 0, st, rec, vp.ent, vp.tile, vp.w, black, vp.pair, vp.f, a.targets, warped_dev, wgrad_dev,
                           partials, (int)a.units, (int)a.Mt, a.tw, g.K, (int)g.NPt, (int)T, (int)a.chunks);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(msiren::align_volume_combine_kernel, gc, dim3(256), 0, st, partials, sums_dev, (int)a.chunks);
        name = "align_volume_reduce_kernels";
    } else if (a.fam == ALIGN_WEIGHTED) {  // sums_dev (n, 47)
        hipLaunchKernelGGL(msiren::align_partial_w_kernel, gp, dim3(256), 0, st, rec, ap.ent, ap.tile, ap.w, black, a.targets, a.weights, a.intensity, warped_dev, wgrad_dev,
                           partials, (int)a.n, (int)a.Mt, a.tw, g.K, (int)g.NPt, (int)T, (int)a.chunks);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(msiren::align_combine_w_kernel, gc, dim3(256), 0, st, partials, sums_dev, (int)a.chunks);
        name = "align_reduce_w_kernels";
    } else {  // sums_dev (n, 29)
        hipLaunchKernelGGL(msiren::align_partial_kernel, gp, dim3(256), 0, st, rec, ap.ent, ap.tile, ap.w, black, a.targets, warped_dev, wgrad_dev, partials, (int)a.n,
                           (int)a.Mt, a.tw, g.K, (int)g.NPt, (int)T, (int)a.chunks);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(msiren::align_combine_kernel, gc, dim3(256), 0, st, partials, sums_dev, (int)a.chunks);
        name = "align_reduce_kernels";
    }
    HIPCHK(hipGetLastError());
    return profile_end(h, c.stream, e1, a.M, name);
}

// sums_dev (n, 29) doubles; warped_dev (n, th, tw) and wgrad_dev (2, n, th, tw) may be null
int align_slices(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                 const float* maps_dev, double* sums_dev, float* warped_dev, float* wgrad_dev) {
    AlignPlan a;
    bool todo;
    const int rc = align_prepare(h, c, ALIGN_PLAIN, images_dev, n, height, width, targets_dev, n, th, tw, maps_dev, sums_dev, 0, &a, &todo);
    if (rc || !todo) return rc;
    return align_evaluate(h, c, a, maps_dev, sums_dev, warped_dev, wgrad_dev);
}

// sums_dev (n, 47); weights_dev (n, th, tw) and intensity_dev (n, 2) may be null
int align_slices_w(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                   const float* maps_dev, const float* weights_dev, const float* intensity_dev, double* sums_dev, float* warped_dev, float* wgrad_dev) {
    int rc = align_w_check(h, n, height, width, th, tw);
    if (rc) return rc;
    if ((uintptr_t)weights_dev % 4 || (uintptr_t)intensity_dev % 4) return fail(MSIREN_E_INVALID, "device weights and intensity must be 4-byte aligned");
    AlignPlan a;
    bool todo;
    rc = align_prepare(h, c, ALIGN_WEIGHTED, images_dev, n, height, width, targets_dev, n, th, tw, maps_dev, sums_dev, 0, &a, &todo);
    if (rc || !todo) return rc;
    a.weights = weights_dev, a.intensity = intensity_dev;
    return align_evaluate(h, c, a, maps_dev, sums_dev, warped_dev, wgrad_dev);
}

// sums_dev (m, 56); warped_dev (m, th, tw) and wgrad_dev (3, m, th, tw) may be null
int align_volume(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th, int32_t tw,
                 const float* maps_dev, double* sums_dev, float* warped_dev, float* wgrad_dev) {
    if ((uintptr_t)warped_dev % 4 || (uintptr_t)wgrad_dev % 4) return fail(MSIREN_E_INVALID, "device warped and wgrad must be 4-byte aligned");
    AlignPlan a;
    bool todo;
    const int rc = align_prepare(h, c, ALIGN_VOLUME, images_dev, n, height, width, targets_dev, m, th, tw, maps_dev, sums_dev, 0, &a, &todo);
    if (rc || !todo) return rc;
    return align_evaluate(h, c, a, maps_dev, sums_dev, warped_dev, wgrad_dev);
}

// sums_dev (m, 80); weights_dev (m, th, tw) and intensity_dev (m, 2) may be null
int align_volume_w(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th, int32_t tw,
                   const float* maps_dev, const float* weights_dev, const float* intensity_dev, double* sums_dev, float* warped_dev, float* wgrad_dev) {
    int rc = align_volume_w_check(h, n, height, width, m, th, tw);
    if (rc) return rc;
    if ((uintptr_t)warped_dev % 4 || (uintptr_t)wgrad_dev % 4 || (uintptr_t)weights_dev % 4 || (uintptr_t)intensity_dev % 4)
        return fail(MSIREN_E_INVALID, "device warped, wgrad, weights and intensity must be 4-byte aligned");
    AlignPlan a;
    bool todo;
    rc = align_prepare(h, c, ALIGN_VOLUME_WEIGHTED, images_dev, n, height, width, targets_dev, m, th, tw, maps_dev, sums_dev, 0, &a, &todo);
    if (rc || !todo) return rc;
    a.weights = weights_dev, a.intensity = intensity_dev;
    return align_evaluate(h, c, a, maps_dev, sums_dev, warped_dev, wgrad_dev);
}

// sums_dev (m, 80) under the robust loss; scale_dev (m) doubles; rweight_dev (m, th, tw) may be null; the rest: align_volume_w's
int align_volume_r(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th, int32_t tw,
                   const float* maps_dev, const float* weights_dev, const float* intensity_dev, const double* scale_dev, double* sums_dev, float* warped_dev, float* wgrad_dev,
                   float* rweight_dev) {
    int rc = align_volume_w_check(h, n, height, width, m, th, tw);
    if (rc) return rc;
    if (m > 0 && (int64_t)th * tw > 0 && !scale_dev) return fail(MSIREN_E_INVALID, "null argument (scale)");
    if ((uintptr_t)warped_dev % 4 || (uintptr_t)wgrad_dev % 4 || (uintptr_t)rweight_dev % 4 || (uintptr_t)weights_dev % 4 || (uintptr_t)intensity_dev % 4 ||
        (uintptr_t)scale_dev % 8)
        return fail(MSIREN_E_INVALID, "device warped, wgrad, rweight, weights and intensity must be 4-byte aligned, scale 8-byte aligned");
    AlignPlan a;
    bool todo;
    rc = align_prepare(h, c, ALIGN_VOLUME_ROBUST, images_dev, n, height, width, targets_dev, m, th, tw, maps_dev, sums_dev, 0, &a, &todo);
    if (rc || !todo) return rc;
    a.weights = weights_dev, a.intensity = intensity_dev, a.scale = scale_dev, a.rweight = rweight_dev;
    return align_evaluate(h, c, a, maps_dev, sums_dev, warped_dev, wgrad_dev);
}

// ---- targets against a plain voxel stack (kernel: align_stack.hip.h) -------------------------------------------------------
// Nothing of the model is asked: no jet_supported, no geom_check, no reflect padding.  Every refusal that needs no pointer, naming its argument.
int align_stack_check(msiren_ctx*, int64_t n, int32_t height, int32_t width, int64_t m, int32_t th, int32_t tw) {
    if (n < 0 || height < 0 || width < 0 || m < 0 || th < 0 || tw < 0)
        return fail(MSIREN_E_INVALID, "bad arguments (n=%lld, height=%d, width=%d, m=%lld, th=%d, tw=%d)", (long long)n, height, width, (long long)m, th, tw);
    if (!msiren::stack_pixels_fit(m, th, tw))
        return fail(MSIREN_E_INVALID, "too many pixels for one call: m th tw = %lld targets x %d x %d must stay below 2^28", (long long)m, th, tw);
    if (m == 0 || (int64_t)th * tw == 0) return 0;  // nothing to do: the stack is not looked at
    if (n < 2) return fail(MSIREN_E_INVALID, "n = %lld: a stack needs two slices at least", (long long)n);
    if (height < 2) return fail(MSIREN_E_INVALID, "height = %d: a stack needs two rows at least", height);
    if (width < 2) return fail(MSIREN_E_INVALID, "width = %d: a stack needs two columns at least", width);
    if (!msiren::stack_voxels_fit(n, height, width))
        return fail(MSIREN_E_INVALID, "stack too large for one call: n height width = %lld x %d x %d must stay below 2^30, each extent below 2^24", (long long)n, height, width);
    return 0;
}

// the stack family's prepare: its check, the null and alignment refusals of what every stack call takes, and the scratch -- the partials and `extra`
// bytes behind them (a solve's state).  No prologue, no patches, no rec.  *todo = false: nothing to do (m = 0 or th tw = 0).
static int align_stack_prepare(msiren_handle h, const Call& c, const float* stack_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m,
                               int32_t th, int32_t tw, const float* weights_dev, const double* scale_dev, size_t extra, AlignPlan* a, bool* todo) {
    *todo = false;
    int rc = align_stack_check(h, n, height, width, m, th, tw);
    if (rc) return rc;
    const int64_t Mt = (int64_t)th * tw, M = m * Mt;
    if (M == 0) return 0;
    if (!stack_dev) return fail(MSIREN_E_INVALID, "null argument (stack)");
    if (!targets_dev) return fail(MSIREN_E_INVALID, "null argument (targets)");
    if (!scale_dev) return fail(MSIREN_E_INVALID, "null argument (scale)");
    if ((uintptr_t)stack_dev % 4 || (uintptr_t)targets_dev % 4 || (uintptr_t)weights_dev % 4)
        return fail(MSIREN_E_INVALID, "device stack, targets and weights must be 4-byte aligned");
    if ((uintptr_t)scale_dev % 8) return fail(MSIREN_E_INVALID, "device scale must be 8-byte aligned");
    const msiren::GeomLayout lay = msiren::stack_layout(m, Mt, msiren::ALIGN_VOLUME_SUMS_W);
    if ((rc = ensure(h, h->sc[c.stream].ragged, lay.total + extra))) return rc;
    *a = AlignPlan{};
    a->fam = ALIGN_STACK, a->n = n, a->units = m, a->Mt = Mt, a->M = M, a->chunks = msiren::align_chunks(Mt), a->th = th, a->tw = tw, a->lay = lay;
    a->targets = targets_dev, a->weights = weights_dev, a->scale = scale_dev, a->stack = stack_dev, a->height = height, a->width = width;
    *todo = true;
    return 0;
}

// sums_dev (m, 80) under the robust loss; every optional array may be null
int align_stack_r(msiren_handle h, const Call& c, const float* stack_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th, int32_t tw,
                  const float* maps_dev, const float* weights_dev, const float* intensity_dev, const double* scale_dev, double* sums_dev, float* warped_dev, float* wgrad_dev,
                  float* rweight_dev) {
    int rc = align_stack_check(h, n, height, width, m, th, tw);
    if (rc || m == 0 || (int64_t)th * tw == 0) return rc;
    if (!maps_dev || !sums_dev) return fail(MSIREN_E_INVALID, "null argument (%s)", !maps_dev ? "maps" : "sums");
    if ((uintptr_t)maps_dev % 4 || (uintptr_t)intensity_dev % 4 || (uintptr_t)warped_dev % 4 || (uintptr_t)wgrad_dev % 4 || (uintptr_t)rweight_dev % 4)
        return fail(MSIREN_E_INVALID, "device maps, intensity, warped, wgrad and rweight must be 4-byte aligned");
    if ((uintptr_t)sums_dev % 8) return fail(MSIREN_E_INVALID, "device sums must be 8-byte aligned");
    AlignPlan a;
    bool todo;
    rc = align_stack_prepare(h, c, stack_dev, n, height, width, targets_dev, m, th, tw, weights_dev, scale_dev, 0, &a, &todo);
    if (rc || !todo) return rc;
    a.intensity = intensity_dev, a.rweight = rweight_dev;
    return align_evaluate(h, c, a, maps_dev, sums_dev, warped_dev, wgrad_dev);
}

// ---- the solves (DESIGN.md sections 5.11 - 5.14): align_prepare once, then `iterations` x (align_evaluate at the trial maps -> the family's step
// kernel), all on the call's stream, no host sync in between.  State and the per-evaluation sums: the stream's scratch behind the partials
// (align_plan.h: solve_layout), ensured before the prologue.
// the Levenberg-Marquardt options the three option structs share
static int lm_opts_check(int mode, int iterations, double damping, double down, double up, double lam_min, double lam_max) {
    if (mode != 0 && mode != 1) return fail(MSIREN_E_INVALID, "mode = %d (0: affine, 1: rigid)", mode);
    if (iterations < 1 || iterations > 256) return fail(MSIREN_E_INVALID, "iterations = %d outside 1 .. 256", iterations);
    const double inf = __builtin_inf();
    if (!(0.0 < lam_min && lam_min <= damping && damping <= lam_max && lam_max < inf))
        return fail(MSIREN_E_INVALID, "damping: 0 < lam_min <= damping <= lam_max < inf is required (lam_min=%g, damping=%g, lam_max=%g)", lam_min, damping, lam_max);
    if (!(0.0 < down && down <= 1.0) || !(1.0 <= up && up < inf)) return fail(MSIREN_E_INVALID, "0 < down <= 1 <= up < inf is required (down=%g, up=%g)", down, up);
    return 0;
}

// the step kernel's parameters every family has, by name: the state sections at `base` and what the options and the caller give
template <typename SP, typename O>
static void solve_params(SP& sp, char* base, const msiren::SolveLayout& s, const O& o, float* maps_out, double* rigid_out, double* report, double* trace) {
    sp.sums = (double*)(base + s.sums), sp.sums_best = (double*)(base + s.sums_best);
    sp.rigid_trial = (double*)(base + s.rigid_trial), sp.rigid_best = (double*)(base + s.rigid_best), sp.scal = (double*)(base + s.scal);
    sp.trial = (float*)(base + s.trial), sp.best = (float*)(base + s.best), sp.cnt = (int*)(base + s.cnt);
    sp.trace = trace, sp.maps_out = maps_out, sp.rigid_out = rigid_out, sp.report = report;
    sp.down = o.down, sp.up = o.up, sp.lam_min = o.lam_min, sp.lam_max = o.lam_max;
}

// the loop behind a family's init kernel with the step stage as a callable: evaluation k at the trial maps, then `stage(k, last)` as one profile
// entry `name`
template <typename Stage>
static int solve_loop_staged(msiren_handle h, const Call& c, const AlignPlan& a, const float* trial, double* sums, int iterations, const char* name, Stage stage) {
    int rc;
    for (int k = 0; k < iterations; ++k) {
        if ((rc = align_evaluate(h, c, a, trial, sums, nullptr, nullptr))) return rc;
        hipEvent_t e1 = nullptr;
        if ((rc = profile_begin(h, c.stream, &e1)) || (rc = stage(k, k == iterations - 1))) return rc;
        if ((rc = profile_end(h, c.stream, e1, a.units, name))) return rc;
    }
    return 0;
}

// that loop with one kernel `step` over the units as its stage
template <typename SP>
static int solve_loop(msiren_handle h, const Call& c, const AlignPlan& a, SP& sp, int iterations, void (*step)(SP), const char* name) {
    hipStream_t st = h->sc[c.stream].s;
    return solve_loop_staged(h, c, a, sp.trial, const_cast<double*>(sp.sums), iterations, name, [&](int k, bool last) {
        sp.k = k, sp.last = last;
        hipLaunchKernelGGL(step, dim3((unsigned)((a.units + 255) / 256)), dim3(256), 0, st, sp);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

// align_solve_check: every refusal that needs no device pointer (the host-pointer form asks it before it stages anything)
int align_solve_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int32_t th, int32_t tw, const msiren_align_solve_opts* o, const void* maps_in,
                      const void* rigid_in, const void* maps_out, const void* report) {
    int rc = align_check(h, n, height, width, th, tw);
    if (rc) return rc;
    if (!o) return fail(MSIREN_E_INVALID, "null options");
    if (o->struct_size != sizeof(msiren_align_solve_opts))
        return fail(MSIREN_E_INVALID, "msiren_align_solve_opts.struct_size = %u, this library's is %u", o->struct_size, (unsigned)sizeof(msiren_align_solve_opts));
    if ((rc = lm_opts_check(o->mode, o->iterations, o->damping, o->down, o->up, o->lam_min, o->lam_max))) return rc;
    if (o->mode == 1 && !(o->centre_y - o->centre_y == 0.0 && o->centre_x - o->centre_x == 0.0)) return fail(MSIREN_E_INVALID, "rigid mode: the centre must be finite");
    if (n > 0 && (int64_t)th * tw > 0 && (!(o->mode == 1 ? rigid_in : maps_in) || !maps_out || !report))
        return fail(MSIREN_E_INVALID, "null argument (%s)", !maps_out ? "maps_out" : !report ? "report" : o->mode == 1 ? "rigid_in: rigid mode" : "maps_in: affine mode");
    return 0;
}

int align_solve(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                const msiren_align_solve_opts* o, const float* maps_in, const double* rigid_in, float* maps_out, double* rigid_out, double* report, double* trace) {
    int rc = align_solve_check(h, n, height, width, th, tw, o, maps_in, rigid_in, maps_out, report);
    if (rc || n == 0 || (int64_t)th * tw == 0) return rc;
    if (!images_dev || !targets_dev) return fail(MSIREN_E_INVALID, "null argument");
    if ((uintptr_t)targets_dev % 4 || (uintptr_t)maps_in % 4 || (uintptr_t)maps_out % 4 || (uintptr_t)rigid_in % 8 || (uintptr_t)rigid_out % 8 || (uintptr_t)report % 8 || (uintptr_t)trace % 8)
        return fail(MSIREN_E_INVALID, "device maps must be 4-byte aligned, rigid states, report and trace 8-byte aligned");
    AlignPlan a;
    bool todo;
    if ((rc = align_prepare(h, c, ALIGN_PLAIN, images_dev, n, height, width, targets_dev, n, th, tw, maps_out, report, msiren::solve_layout(0, n, msiren::ALIGN_SUMS, 4, 6, false).total,
                            &a, &todo)) || !todo)
        return rc;
    auto& sc = h->sc[c.stream];
    msiren::AlignSolveParams sp{};
    solve_params(sp, (char*)sc.ragged.p, msiren::solve_layout(a.lay.total, n, msiren::ALIGN_SUMS, 4, 6, false), *o, maps_out, rigid_out, report, trace);
    sp.n = (int)n, sp.mode = o->mode, sp.cy = o->centre_y, sp.cx = o->centre_x;
    hipLaunchKernelGGL(msiren::align_solve_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sc.s, sp, maps_in, rigid_in, o->damping);
    HIPCHK(hipGetLastError());
    return solve_loop(h, c, a, sp, o->iterations, msiren::align_step_kernel, "align_step_kernel");
}

int align_solve_w_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int32_t th, int32_t tw, const msiren_align_solve_w_opts* o, const void* maps_in,
                        const void* rigid_in, const void* maps_out, const void* intensity_out, const void* report) {
    if (!o) return fail(MSIREN_E_INVALID, "null options");
    if (o->struct_size != sizeof(msiren_align_solve_w_opts))
        return fail(MSIREN_E_INVALID, "msiren_align_solve_w_opts.struct_size = %u, this library's is %u", o->struct_size, (unsigned)sizeof(msiren_align_solve_w_opts));
    if (o->intensity_mode != 0 && o->intensity_mode != 1) return fail(MSIREN_E_INVALID, "intensity_mode = %d (0: fixed, 1: estimate)", o->intensity_mode);
    const msiren_align_solve_opts base{(uint32_t)sizeof(msiren_align_solve_opts), o->mode, o->iterations, 0, o->damping, o->down, o->up, o->lam_min, o->lam_max,
                                       o->centre_y, o->centre_x};
    int rc = align_solve_check(h, n, height, width, th, tw, &base, maps_in, rigid_in, maps_out, report);  // (everything msiren_align_solve refuses)
    if (rc || (rc = align_w_check(h, n, height, width, th, tw))) return rc;
    if (n > 0 && (int64_t)th * tw > 0 && !intensity_out) return fail(MSIREN_E_INVALID, "null argument (intensity_out)");
    return 0;
}

int align_solve_w(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                  const msiren_align_solve_w_opts* o, const float* maps_in, const double* rigid_in, const float* weights_dev, const float* intensity_in, float* maps_out,
                  float* intensity_out, double* rigid_out, double* report, double* trace) {
    int rc = align_solve_w_check(h, n, height, width, th, tw, o, maps_in, rigid_in, maps_out, intensity_out, report);
    if (rc || n == 0 || (int64_t)th * tw == 0) return rc;
    if (!images_dev || !targets_dev) return fail(MSIREN_E_INVALID, "null argument");
    if ((uintptr_t)targets_dev % 4 || (uintptr_t)maps_in % 4 || (uintptr_t)maps_out % 4 || (uintptr_t)weights_dev % 4 || (uintptr_t)intensity_in % 4 ||
        (uintptr_t)intensity_out % 4 || (uintptr_t)rigid_in % 8 || (uintptr_t)rigid_out % 8 || (uintptr_t)report % 8 || (uintptr_t)trace % 8)
        return fail(MSIREN_E_INVALID, "device maps, weights and intensity must be 4-byte aligned, rigid states, report and trace 8-byte aligned");
    AlignPlan a;
    bool todo;
    if ((rc = align_prepare(h, c, ALIGN_WEIGHTED, images_dev, n, height, width, targets_dev, n, th, tw, maps_out, report,
                            msiren::solve_layout(0, n, msiren::ALIGN_SUMS_W, 4, 6, true).total, &a, &todo)) || !todo)
        return rc;
    auto& sc = h->sc[c.stream];
    char* const base = (char*)sc.ragged.p;
    const msiren::SolveLayout s = msiren::solve_layout(a.lay.total, n, msiren::ALIGN_SUMS_W, 4, 6, true);
    msiren::AlignSolveWParams sp{};
    solve_params(sp, base, s, *o, maps_out, rigid_out, report, trace);
    sp.gb_trial = (float*)(base + s.gb_trial), sp.gb_best = (float*)(base + s.gb_best), sp.intensity_out = intensity_out;
    sp.n = (int)n, sp.mode = o->mode, sp.estimate = o->intensity_mode, sp.cy = o->centre_y, sp.cx = o->centre_x;
    a.weights = weights_dev, a.intensity = sp.gb_trial;
    hipLaunchKernelGGL(msiren::align_solve_init_w_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sc.s, sp, maps_in, rigid_in, intensity_in, o->damping);
    HIPCHK(hipGetLastError());
    return solve_loop(h, c, a, sp, o->iterations, msiren::align_step_w_kernel, "align_step_w_kernel");
}

int align_volume_solve_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t m, int32_t th, int32_t tw, const msiren_align_volume_solve_opts* o,
                             const void* maps_in, const void* planes, const void* rigid_in, const void* maps_out, const void* report) {
    int rc = align_volume_check(h, n, height, width, m, th, tw);
    if (rc) return rc;
    if (!o) return fail(MSIREN_E_INVALID, "null options");
    if (o->struct_size != sizeof(msiren_align_volume_solve_opts))
        return fail(MSIREN_E_INVALID, "msiren_align_volume_solve_opts.struct_size = %u, this library's is %u", o->struct_size, (unsigned)sizeof(msiren_align_volume_solve_opts));
    if ((rc = lm_opts_check(o->mode, o->iterations, o->damping, o->down, o->up, o->lam_min, o->lam_max))) return rc;
    if (o->mode == 1 && !(o->spacing > 0.0 && o->spacing < __builtin_inf())) return fail(MSIREN_E_INVALID, "rigid mode: spacing = %g must be finite and > 0", o->spacing);
    if (m > 0 && (int64_t)th * tw > 0 && (!(o->mode == 1 ? (rigid_in && planes) : maps_in != nullptr) || !maps_out || !report))
        return fail(MSIREN_E_INVALID, "null argument (%s)", !maps_out ? "maps_out" : !report ? "report" : o->mode == 1 ? "planes or rigid_in: rigid mode" : "maps_in: affine mode");
    return 0;
}

int align_volume_solve(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                       int32_t tw, const msiren_align_volume_solve_opts* o, const float* maps_in, const double* planes, const double* rigid_in, float* maps_out,
                       double* rigid_out, double* report, double* trace) {
    int rc = align_volume_solve_check(h, n, height, width, m, th, tw, o, maps_in, planes, rigid_in, maps_out, report);
    if (rc || m == 0 || (int64_t)th * tw == 0) return rc;
    if (!images_dev || !targets_dev) return fail(MSIREN_E_INVALID, "null argument");
    if ((uintptr_t)targets_dev % 4 || (uintptr_t)maps_in % 4 || (uintptr_t)maps_out % 4 || (uintptr_t)planes % 8 || (uintptr_t)rigid_in % 8 || (uintptr_t)rigid_out % 8 ||
        (uintptr_t)report % 8 || (uintptr_t)trace % 8)
        return fail(MSIREN_E_INVALID, "device maps must be 4-byte aligned, planes, rigid states, report and trace 8-byte aligned");
    AlignPlan a;
    bool todo;
    if ((rc = align_prepare(h, c, ALIGN_VOLUME, images_dev, n, height, width, targets_dev, m, th, tw, maps_out, report,
                            msiren::solve_layout(0, m, msiren::ALIGN_VOLUME_SUMS, 12, 9, false).total, &a, &todo)) || !todo)
        return rc;
    auto& sc = h->sc[c.stream];
    msiren::AlignVolumeSolveParams sp{};
    solve_params(sp, (char*)sc.ragged.p, msiren::solve_layout(a.lay.total, m, msiren::ALIGN_VOLUME_SUMS, 12, 9, false), *o, maps_out, rigid_out, report, trace);
    sp.planes = planes, sp.m = (int)m, sp.spacing = o->spacing;
    const bool rigid = o->mode == 1;  // the kernels are instantiated per mode
    const dim3 gs((unsigned)((m + 255) / 256));
    if (rigid) hipLaunchKernelGGL(msiren::align_volume_solve_init_kernel<msiren::ALIGN_VOLUME_RIGID>, gs, dim3(256), 0, sc.s, sp, maps_in, rigid_in, o->damping);
    else hipLaunchKernelGGL(msiren::align_volume_solve_init_kernel<msiren::ALIGN_VOLUME_AFFINE>, gs, dim3(256), 0, sc.s, sp, maps_in, rigid_in, o->damping);
    HIPCHK(hipGetLastError());
    return solve_loop(h, c, a, sp, o->iterations, rigid ? msiren::align_volume_step_kernel<msiren::ALIGN_VOLUME_RIGID> : msiren::align_volume_step_kernel<msiren::ALIGN_VOLUME_AFFINE>,
                      "align_volume_step_kernel");
}

int align_volume_solve_w_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t m, int32_t th, int32_t tw, const msiren_align_volume_solve_w_opts* o,
                               const void* maps_in, const void* planes, const void* rigid_in, const void* maps_out, const void* intensity_out, const void* report) {
    if (!o) return fail(MSIREN_E_INVALID, "null options");
    if (o->struct_size != sizeof(msiren_align_volume_solve_w_opts))
        return fail(MSIREN_E_INVALID, "msiren_align_volume_solve_w_opts.struct_size = %u, this library's is %u", o->struct_size, (unsigned)sizeof(msiren_align_volume_solve_w_opts));
    if (o->intensity_mode != 0 && o->intensity_mode != 1) return fail(MSIREN_E_INVALID, "intensity_mode = %d (0: fixed, 1: estimate)", o->intensity_mode);
    const msiren_align_volume_solve_opts base{(uint32_t)sizeof(msiren_align_volume_solve_opts), o->mode, o->iterations, 0, o->damping, o->down, o->up, o->lam_min, o->lam_max,
                                              o->spacing};
    int rc = align_volume_solve_check(h, n, height, width, m, th, tw, &base, maps_in, planes, rigid_in, maps_out, report);  // (everything msiren_align_volume_solve refuses)
    if (rc || (rc = align_volume_w_check(h, n, height, width, m, th, tw))) return rc;
    if (m > 0 && (int64_t)th * tw > 0 && !intensity_out) return fail(MSIREN_E_INVALID, "null argument (intensity_out)");
    return 0;
}

int align_volume_solve_w(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                         int32_t tw, const msiren_align_volume_solve_w_opts* o, const float* maps_in, const double* planes, const double* rigid_in, const float* weights_dev,
                         const float* intensity_in, float* maps_out, float* intensity_out, double* rigid_out, double* report, double* trace) {
    int rc = align_volume_solve_w_check(h, n, height, width, m, th, tw, o, maps_in, planes, rigid_in, maps_out, intensity_out, report);
    if (rc || m == 0 || (int64_t)th * tw == 0) return rc;
    if (!images_dev || !targets_dev) return fail(MSIREN_E_INVALID, "null argument");
    if ((uintptr_t)targets_dev % 4 || (uintptr_t)maps_in % 4 || (uintptr_t)maps_out % 4 || (uintptr_t)weights_dev % 4 || (uintptr_t)intensity_in % 4 ||
        (uintptr_t)intensity_out % 4 || (uintptr_t)planes % 8 || (uintptr_t)rigid_in % 8 || (uintptr_t)rigid_out % 8 || (uintptr_t)report % 8 || (uintptr_t)trace % 8)
        return fail(MSIREN_E_INVALID, "device maps, weights and intensity must be 4-byte aligned, planes, rigid states, report and trace 8-byte aligned");
    AlignPlan a;
    bool todo;
    if ((rc = align_prepare(h, c, ALIGN_VOLUME_WEIGHTED, images_dev, n, height, width, targets_dev, m, th, tw, maps_out, report,
                            msiren::solve_layout(0, m, msiren::ALIGN_VOLUME_SUMS_W, 12, 9, true).total, &a, &todo)) || !todo)
        return rc;
    auto& sc = h->sc[c.stream];
    char* const base = (char*)sc.ragged.p;
    const msiren::SolveLayout s = msiren::solve_layout(a.lay.total, m, msiren::ALIGN_VOLUME_SUMS_W, 12, 9, true);
    msiren::AlignVolumeSolveWParams sp{};
    solve_params(sp, base, s, *o, maps_out, rigid_out, report, trace);
    sp.gb_trial = (float*)(base + s.gb_trial), sp.gb_best = (float*)(base + s.gb_best), sp.intensity_out = intensity_out;
    sp.planes = planes, sp.m = (int)m, sp.spacing = o->spacing;
    a.weights = weights_dev, a.intensity = sp.gb_trial;
    const bool rigid = o->mode == 1, est = o->intensity_mode == 1;  // the kernels are instantiated per mode; the step also per intensity mode
    const dim3 gs((unsigned)((m + 255) / 256));
    if (rigid) hipLaunchKernelGGL(msiren::align_volume_solve_init_w_kernel<msiren::ALIGN_VOLUME_RIGID>, gs, dim3(256), 0, sc.s, sp, maps_in, rigid_in, intensity_in, o->damping);
    else hipLaunchKernelGGL(msiren::align_volume_solve_init_w_kernel<msiren::ALIGN_VOLUME_AFFINE>, gs, dim3(256), 0, sc.s, sp, maps_in, rigid_in, intensity_in, o->damping);
    HIPCHK(hipGetLastError());
    void (*const step)(msiren::AlignVolumeSolveWParams) =
        rigid ? (est ? msiren::align_volume_step_w_kernel<msiren::ALIGN_VOLUME_RIGID, 1> : msiren::align_volume_step_w_kernel<msiren::ALIGN_VOLUME_RIGID, 0>)
              : (est ? msiren::align_volume_step_w_kernel<msiren::ALIGN_VOLUME_AFFINE, 1> : msiren::align_volume_step_w_kernel<msiren::ALIGN_VOLUME_AFFINE, 0>);
    return solve_loop(h, c, a, sp, o->iterations, step, "align_volume_step_w_kernel");
}

// ---- the grouped rigid solve (kernels: align_group.hip.h): align_volume_solve_w's loop with the step stage for groups of
// consecutive targets under one rigid state per group.  Prologue, bins, trunk and the 80-sum reduce are the weighted volume family's; the loop is
// solve_loop_staged with the four step kernels as its stage.
static int groups_check(const int32_t* group_start, int64_t G, int64_t m);  // what is wrong with group_start, by name and index (below)

// every refusal that needs no device pointer: what align_volume_solve_w_check refuses in rigid mode, then the groups (group_start is a host array)
int align_volume_solve_group_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t m, int32_t th, int32_t tw, const msiren_align_volume_solve_group_opts* o,
                                   const int32_t* group_start, int64_t G, const void* planes, const void* rigid_in, const void* maps_out, const void* intensity_out,
                                   const void* report) {
    if (!o) return fail(MSIREN_E_INVALID, "null options");
    if (o->struct_size != sizeof(msiren_align_volume_solve_group_opts))
        return fail(MSIREN_E_INVALID, "msiren_align_volume_solve_group_opts.struct_size = %u, this library's is %u", o->struct_size,
                    (unsigned)sizeof(msiren_align_volume_solve_group_opts));
    const msiren_align_volume_solve_w_opts w{(uint32_t)sizeof(msiren_align_volume_solve_w_opts), 1, o->iterations, o->intensity_mode, o->damping, o->down, o->up, o->lam_min,
                                             o->lam_max, o->spacing};
    int rc = align_volume_solve_w_check(h, n, height, width, m, th, tw, &w, nullptr, planes, rigid_in, maps_out, intensity_out, report);
    if (rc || m == 0) return rc;
    return groups_check(group_start, G, m);
}

// the stack family's: the same refusals in the same order with align_stack_check in the model's place
int align_stack_solve_group_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t m, int32_t th, int32_t tw, const msiren_align_volume_solve_group_opts* o,
                                  const int32_t* group_start, int64_t G, const void* planes, const void* rigid_in, const void* maps_out, const void* intensity_out,
                                  const void* report) {
    if (!o) return fail(MSIREN_E_INVALID, "null options");
    if (o->struct_size != sizeof(msiren_align_volume_solve_group_opts))
        return fail(MSIREN_E_INVALID, "msiren_align_volume_solve_group_opts.struct_size = %u, this library's is %u", o->struct_size,
                    (unsigned)sizeof(msiren_align_volume_solve_group_opts));
    if (o->intensity_mode != 0 && o->intensity_mode != 1) return fail(MSIREN_E_INVALID, "intensity_mode = %d (0: fixed, 1: estimate)", o->intensity_mode);
    int rc = align_stack_check(h, n, height, width, m, th, tw);
    if (rc || (rc = lm_opts_check(1, o->iterations, o->damping, o->down, o->up, o->lam_min, o->lam_max))) return rc;
    if (!(o->spacing > 0.0 && o->spacing < __builtin_inf())) return fail(MSIREN_E_INVALID, "spacing = %g must be finite and > 0", o->spacing);
    if (m > 0 && (int64_t)th * tw > 0 && (!rigid_in || !planes || !maps_out || !intensity_out || !report))
        return fail(MSIREN_E_INVALID, "null argument (%s)", !maps_out ? "maps_out" : !intensity_out ? "intensity_out" : !report ? "report" : !planes ? "planes" : "rigid_in");
    if (m == 0) return 0;
    return groups_check(group_start, G, m);
}

static int groups_check(const int32_t* group_start, int64_t G, int64_t m) {
    int64_t at = 0;
    switch (msiren::group_start_check(group_start, G, m, &at)) {
        case msiren::GROUPS_OK: return 0;
        case msiren::GROUPS_NONE: return fail(MSIREN_E_INVALID, "n_groups = %lld: one group at least", (long long)G);
        case msiren::GROUPS_NULL: return fail(MSIREN_E_INVALID, "null argument (group_start)");
        case msiren::GROUPS_FIRST: return fail(MSIREN_E_INVALID, "group_start[0] = %d: the first offset must be 0", group_start[0]);
        case msiren::GROUPS_ORDER:
            return fail(MSIREN_E_INVALID, "group_start[%lld] = %d is not above group_start[%lld] = %d: offsets must be strictly ascending", (long long)at, group_start[at],
                        (long long)at - 1, group_start[at - 1]);
        default: return fail(MSIREN_E_INVALID, "group_start[%lld] = %d: the last offset must be m = %lld", (long long)at, group_start[at], (long long)m);
    }
}

// the grouped solve on the sums of `fam`: ALIGN_VOLUME_WEIGHTED (scale_dev unused) or ALIGN_VOLUME_ROBUST (scale_dev (m) doubles,
// fixed for the call, so every evaluation scores one objective).  The step stage reads the 80 sums whatever loss formed them.  ALIGN_STACK (section
// 5.22): images_dev is the voxel stack, the check and the prepare are the stack family's, the rest is the same.
static int group_solve(msiren_handle h, const Call& c, AlignFamily fam, const double* scale_dev, const float* images_dev, int64_t n, int32_t height, int32_t width,
                       const float* targets_dev, int64_t m, int32_t th, int32_t tw, const msiren_align_volume_solve_group_opts* o, const int32_t* group_start, int64_t G,
                       const double* planes, const double* rigid_in, const float* weights_dev, const float* intensity_in, float* maps_out, float* intensity_out,
                       double* rigid_out, double* report, double* target_report, double* trace) {
    const bool stack = fam == ALIGN_STACK;  // images_dev: the voxels
    int rc = stack ? align_stack_solve_group_check(h, n, height, width, m, th, tw, o, group_start, G, planes, rigid_in, maps_out, intensity_out, report)
                   : align_volume_solve_group_check(h, n, height, width, m, th, tw, o, group_start, G, planes, rigid_in, maps_out, intensity_out, report);
    if (rc || m == 0 || (int64_t)th * tw == 0) return rc;
    if (!images_dev || !targets_dev) return fail(MSIREN_E_INVALID, stack ? (!images_dev ? "null argument (stack)" : "null argument (targets)") : "null argument");
    if ((fam == ALIGN_VOLUME_ROBUST || stack) && !scale_dev) return fail(MSIREN_E_INVALID, "null argument (scale)");
    if (fam == ALIGN_VOLUME_ROBUST && (uintptr_t)scale_dev % 8) return fail(MSIREN_E_INVALID, "device scale must be 8-byte aligned");
    if ((uintptr_t)targets_dev % 4 || (uintptr_t)maps_out % 4 || (uintptr_t)weights_dev % 4 || (uintptr_t)intensity_in % 4 || (uintptr_t)intensity_out % 4 ||
        (uintptr_t)planes % 8 || (uintptr_t)rigid_in % 8 || (uintptr_t)rigid_out % 8 || (uintptr_t)report % 8 || (uintptr_t)target_report % 8 || (uintptr_t)trace % 8)
        return fail(MSIREN_E_INVALID, "device maps, weights and intensity must be 4-byte aligned, planes, rigid states, reports and trace 8-byte aligned");
    constexpr int S = msiren::ALIGN_VOLUME_SUMS_W, R = msiren::ALIGN_GROUP_REC, NS = msiren::ALIGN_GROUP_SCAL, NC = msiren::ALIGN_GROUP_CNT;
    AlignPlan a;
    bool todo;
    const size_t extra = msiren::group_solve_layout(0, m, G, S, R, NS, NC).total;
    if ((rc = stack ? align_stack_prepare(h, c, images_dev, n, height, width, targets_dev, m, th, tw, weights_dev, scale_dev, extra, &a, &todo)
                    : align_prepare(h, c, fam, images_dev, n, height, width, targets_dev, m, th, tw, maps_out, report, extra, &a, &todo)) ||
        !todo)
        return rc;
    auto& sc = h->sc[c.stream];
    hipStream_t st = sc.s;
    char* const base = (char*)sc.ragged.p;
    const msiren::GroupSolveLayout s = msiren::group_solve_layout(a.lay.total, m, G, S, R, NS, NC);
    msiren::AlignGroupParams sp{};
    sp.sums = (double*)(base + s.sums), sp.sums_best = (double*)(base + s.sums_best), sp.rec = (double*)(base + s.rec);
    sp.rigid_trial = (double*)(base + s.rigid_trial), sp.rigid_best = (double*)(base + s.rigid_best), sp.scal = (double*)(base + s.scal);
    sp.trial = (float*)(base + s.trial), sp.best = (float*)(base + s.best), sp.gb_trial = (float*)(base + s.gb_trial), sp.gb_best = (float*)(base + s.gb_best);
    sp.group_of = (int*)(base + s.group_of), sp.group_start = (int*)(base + s.group_start), sp.cnt = (int*)(base + s.cnt);
    sp.planes = planes, sp.trace = trace, sp.maps_out = maps_out, sp.intensity_out = intensity_out, sp.rigid_out = rigid_out, sp.report = report;
    sp.target_report = target_report;
    sp.m = (int)m, sp.G = (int)G, sp.est = o->intensity_mode == 1;
    sp.down = o->down, sp.up = o->up, sp.lam_min = o->lam_min, sp.lam_max = o->lam_max, sp.spacing = o->spacing;
    a.weights = weights_dev, a.intensity = sp.gb_trial, a.scale = scale_dev;
    // group_start: up to 512 offsets per launch, by value in the kernel's arguments (no copy from a host buffer that the caller may reuse, no sync)
    for (int64_t at = 0; at < G + 1; at += msiren::ALIGN_GROUP_OFFSETS) {
        msiren::AlignGroupOffsets off{};
        const int count = (int)(G + 1 - at < msiren::ALIGN_GROUP_OFFSETS ? G + 1 - at : msiren::ALIGN_GROUP_OFFSETS);
        for (int i = 0; i < count; ++i) off.v[i] = group_start[at + i];
        hipLaunchKernelGGL(msiren::align_group_upload_kernel, dim3(msiren::ALIGN_GROUP_OFFSETS / 256), dim3(256), 0, st, off, sp.group_start, (int)at, count);
        HIPCHK(hipGetLastError());
    }
    const dim3 gt((unsigned)((m + 255) / 256)), gg((unsigned)((G + 255) / 256));
    hipLaunchKernelGGL(msiren::align_group_init_kernel, gt, dim3(256), 0, st, sp, rigid_in, intensity_in, o->damping);
    HIPCHK(hipGetLastError());
    const bool est = sp.est;
    return solve_loop_staged(h, c, a, sp.trial, const_cast<double*>(sp.sums), o->iterations, "align_group_step_kernels", [&](int k, bool last) {
        sp.k = k, sp.last = last;
        hipLaunchKernelGGL(msiren::align_group_decide_kernel, gg, dim3(256), 0, st, sp);
        HIPCHK(hipGetLastError());
        if (est) hipLaunchKernelGGL(msiren::align_group_project_kernel<1>, gt, dim3(256), 0, st, sp);
        else hipLaunchKernelGGL(msiren::align_group_project_kernel<0>, gt, dim3(256), 0, st, sp);
        HIPCHK(hipGetLastError());
        if (est) hipLaunchKernelGGL(msiren::align_group_step_kernel<1>, gg, dim3(256), 0, st, sp);
        else hipLaunchKernelGGL(msiren::align_group_step_kernel<0>, gg, dim3(256), 0, st, sp);
        HIPCHK(hipGetLastError());
        if (est) hipLaunchKernelGGL(msiren::align_group_apply_kernel<1>, gt, dim3(256), 0, st, sp);
        else hipLaunchKernelGGL(msiren::align_group_apply_kernel<0>, gt, dim3(256), 0, st, sp);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

int align_volume_solve_group(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                             int32_t tw, const msiren_align_volume_solve_group_opts* o, const int32_t* group_start, int64_t G, const double* planes, const double* rigid_in,
                             const float* weights_dev, const float* intensity_in, float* maps_out, float* intensity_out, double* rigid_out, double* report, double* target_report,
                             double* trace) {
    return group_solve(h, c, ALIGN_VOLUME_WEIGHTED, nullptr, images_dev, n, height, width, targets_dev, m, th, tw, o, group_start, G, planes, rigid_in, weights_dev,
                       intensity_in, maps_out, intensity_out, rigid_out, report, target_report, trace);
}

// the same loop on the robust sums; a null scale is refused
int align_volume_solve_group_r(msiren_handle h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                               int32_t tw, const msiren_align_volume_solve_group_opts* o, const int32_t* group_start, int64_t G, const double* planes, const double* rigid_in,
                               const float* weights_dev, const float* intensity_in, const double* scale_dev, float* maps_out, float* intensity_out, double* rigid_out,
                               double* report, double* target_report, double* trace) {
    return group_solve(h, c, ALIGN_VOLUME_ROBUST, scale_dev, images_dev, n, height, width, targets_dev, m, th, tw, o, group_start, G, planes, rigid_in, weights_dev,
                       intensity_in, maps_out, intensity_out, rigid_out, report, target_report, trace);
}

// the same loop on the sums of a plain voxel stack: no prologue, no trunk, no weights of the model
int align_stack_solve_group_r(msiren_handle h, const Call& c, const float* stack_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                              int32_t tw, const msiren_align_volume_solve_group_opts* o, const int32_t* group_start, int64_t G, const double* planes, const double* rigid_in,
                              const float* weights_dev, const float* intensity_in, const double* scale_dev, float* maps_out, float* intensity_out, double* rigid_out,
                              double* report, double* target_report, double* trace) {
    return group_solve(h, c, ALIGN_STACK, scale_dev, stack_dev, n, height, width, targets_dev, m, th, tw, o, group_start, G, planes, rigid_in, weights_dev, intensity_in,
                       maps_out, intensity_out, rigid_out, report, target_report, trace);
}

}  // namespace mh

using namespace mh;

namespace {

// What every host-pointer form of the geometry calls does between its family's check (`rc`: check(h), then that check) and its staging: the
// empty call (*done, success), the null images / points / targets / outputs (`null_arg`), the pixel limit of one upload.
int host_preamble(int rc, bool empty, bool null_arg, int64_t n, int32_t height, int32_t width, bool* done) {
    *done = rc || empty;
    if (*done) return rc;
    if (null_arg) return fail(MSIREN_E_INVALID, "null argument");
    if (n * (int64_t)height * width > 0x1fffffffLL) return fail(MSIREN_E_INVALID, "too many pixels for one call: %lld slices of %dx%d", (long long)n, height, width);
    return 0;
}

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
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : resample_check(h, n, height, width, M, grad),
                            n == 0 || M == 0, !images_host || !points_host || (grad ? !grad_host : !out_host), n, height, width, &done)) || done) return rc;
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
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : resample_volume_check(h, n, height, width, M, grad),
                            n == 0 || M == 0, !images_host || !points_host || (grad ? !grad_host : !out_host), n, height, width, &done)) || done) return rc;
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
    const int64_t M = (int64_t)th * tw;
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : align_check(h, n, height, width, th, tw),
                            n == 0 || M == 0, !images_host || !targets_host || !maps_host || !sums_host, n, height, width, &done)) || done) return rc;
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
    const int64_t M = (int64_t)th * tw;
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : align_solve_check(h, n, height, width, th, tw, o, maps_in, rigid_in, maps_out, report),
                            n == 0 || M == 0, !images_host || !targets_host, n, height, width, &done)) || done) return rc;
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
    const int64_t M = (int64_t)th * tw;
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : align_w_check(h, n, height, width, th, tw),
                            n == 0 || M == 0, !images_host || !targets_host || !maps_host || !sums_host, n, height, width, &done)) || done) return rc;
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
    const int64_t M = (int64_t)th * tw;
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : align_solve_w_check(h, n, height, width, th, tw, o, maps_in, rigid_in, maps_out, intensity_out, report),
                            n == 0 || M == 0, !images_host || !targets_host, n, height, width, &done)) || done) return rc;
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
    const int64_t M = m * (int64_t)th * tw;
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : align_volume_check(h, n, height, width, m, th, tw),
                            M == 0, !images_host || !targets_host || !maps_host || !sums_host, n, height, width, &done)) || done) return rc;
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
    const int64_t M = m * (int64_t)th * tw;
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : align_volume_solve_check(h, n, height, width, m, th, tw, o, maps_in, planes, rigid_in, maps_out, report),
                            M == 0, !images_host || !targets_host, n, height, width, &done)) || done) return rc;
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

// the weighted volume forms: as the two above; the weights and the intensities go up once per call
int align_volume_w_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                        const float* maps_host, const float* weights_host, const float* intensity_host, double* sums_host, float* warped_host, float* wgrad_host) {
    const int64_t M = m * (int64_t)th * tw;
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : align_volume_w_check(h, n, height, width, m, th, tw),
                            M == 0, !images_host || !targets_host || !maps_host || !sums_host, n, height, width, &done)) || done) return rc;
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)M * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY), i_m = io.in(maps_host, (size_t)m * 9 * sizeof(float), HOST_COPY);
    const int i_w = io.in(weights_host, nt, HOST_COPY), i_gb = io.in(intensity_host, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int o_s = io.out(sums_host, (size_t)m * kAlignVolumeSumsW * sizeof(double), HOST_IN_PLACE);
    const int o_w = io.out(warped_host, nt, HOST_IN_PLACE), o_g = io.out(wgrad_host, 3 * nt, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    if ((rc = align_volume_w(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), m, th, tw, io.src<float>(i_m), io.src<float>(i_w), io.src<float>(i_gb),
                             io.dst<double>(o_s), io.dst<float>(o_w), io.dst<float>(o_g))))
        return rc;
    return io.finish();
}

int align_volume_solve_w_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                              const msiren_align_volume_solve_w_opts* o, const float* maps_in, const double* planes, const double* rigid_in, const float* weights_host,
                              const float* intensity_in, float* maps_out, float* intensity_out, double* rigid_out, double* report, double* trace) {
    const int64_t M = m * (int64_t)th * tw;
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : align_volume_solve_w_check(h, n, height, width, m, th, tw, o, maps_in, planes, rigid_in, maps_out, intensity_out, report),
                            M == 0, !images_host || !targets_host, n, height, width, &done)) || done) return rc;
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)M * sizeof(float);
    const bool rigid = o->mode == 1;
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY);
    // six inputs at most per call (SyncHostCall): the start is the maps (affine) or the planes and the states (rigid), never all three
    const int i_s = rigid ? io.in(planes, (size_t)m * 12 * sizeof(double), HOST_COPY) : io.in(maps_in, (size_t)m * 9 * sizeof(float), HOST_COPY);
    const int i_r = io.in(rigid ? rigid_in : nullptr, (size_t)m * 12 * sizeof(double), HOST_COPY);
    const int i_w = io.in(weights_host, nt, HOST_COPY), i_gb = io.in(intensity_in, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int o_m = io.out(maps_out, (size_t)m * 9 * sizeof(float), HOST_COPY), o_gb = io.out(intensity_out, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int o_r = io.out(rigid_out, (size_t)m * 12 * sizeof(double), HOST_COPY);
    const int o_rep = io.out(report, (size_t)m * 7 * sizeof(double), HOST_COPY), o_tr = io.out(trace, (size_t)o->iterations * m * 14 * sizeof(double), HOST_COPY);
    if ((rc = io.begin())) return rc;
    if ((rc = align_volume_solve_w(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), m, th, tw, o, rigid ? nullptr : io.src<float>(i_s), rigid ? io.src<double>(i_s) : nullptr,
                                   io.src<double>(i_r), io.src<float>(i_w), io.src<float>(i_gb), io.dst<float>(o_m), io.dst<float>(o_gb), io.dst<double>(o_r), io.dst<double>(o_rep),
                                   io.dst<double>(o_tr))))
        return rc;
    return io.finish();
}

// the grouped solve: six inputs and six outputs, all staged; group_start stays on the host
int align_volume_solve_group_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                                  const msiren_align_volume_solve_group_opts* o, const int32_t* group_start, int64_t G, const double* planes, const double* rigid_in,
                                  const float* weights_host, const float* intensity_in, float* maps_out, float* intensity_out, double* rigid_out, double* report,
                                  double* target_report, double* trace) {
    const int64_t M = m * (int64_t)th * tw;
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : align_volume_solve_group_check(h, n, height, width, m, th, tw, o, group_start, G, planes, rigid_in, maps_out, intensity_out, report),
                            M == 0, !images_host || !targets_host, n, height, width, &done)) || done) return rc;
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)M * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY);
    const int i_p = io.in(planes, (size_t)m * 12 * sizeof(double), HOST_COPY), i_r = io.in(rigid_in, (size_t)G * 12 * sizeof(double), HOST_COPY);
    const int i_w = io.in(weights_host, nt, HOST_COPY), i_gb = io.in(intensity_in, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int o_m = io.out(maps_out, (size_t)m * 9 * sizeof(float), HOST_COPY), o_gb = io.out(intensity_out, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int o_r = io.out(rigid_out, (size_t)G * 12 * sizeof(double), HOST_COPY), o_rep = io.out(report, (size_t)G * 7 * sizeof(double), HOST_COPY);
    const int o_tr = io.out(target_report, (size_t)m * 3 * sizeof(double), HOST_COPY), o_trace = io.out(trace, (size_t)o->iterations * G * 15 * sizeof(double), HOST_COPY);
    if ((rc = io.begin())) return rc;
    if ((rc = align_volume_solve_group(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), m, th, tw, o, group_start, G, io.src<double>(i_p), io.src<double>(i_r),
                                       io.src<float>(i_w), io.src<float>(i_gb), io.dst<float>(o_m), io.dst<float>(o_gb), io.dst<double>(o_r), io.dst<double>(o_rep),
                                       io.dst<double>(o_tr), io.dst<double>(o_trace))))
        return rc;
    return io.finish();
}

// the robust forms: as align_volume_w_host and align_volume_solve_group_host; the scales go up once per call
int align_volume_r_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                        const float* maps_host, const float* weights_host, const float* intensity_host, const double* scale_host, double* sums_host, float* warped_host,
                        float* wgrad_host, float* rweight_host) {
    const int64_t M = m * (int64_t)th * tw;
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : align_volume_w_check(h, n, height, width, m, th, tw),
                            M == 0, !images_host || !targets_host || !maps_host || !sums_host || !scale_host, n, height, width, &done)) || done) return rc;
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)M * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY), i_m = io.in(maps_host, (size_t)m * 9 * sizeof(float), HOST_COPY);
    const int i_w = io.in(weights_host, nt, HOST_COPY), i_gb = io.in(intensity_host, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int i_s = io.in(scale_host, (size_t)m * sizeof(double), HOST_COPY);
    const int o_s = io.out(sums_host, (size_t)m * kAlignVolumeSumsW * sizeof(double), HOST_IN_PLACE);
    const int o_w = io.out(warped_host, nt, HOST_IN_PLACE), o_g = io.out(wgrad_host, 3 * nt, HOST_IN_PLACE), o_rw = io.out(rweight_host, nt, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    if ((rc = align_volume_r(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), m, th, tw, io.src<float>(i_m), io.src<float>(i_w), io.src<float>(i_gb),
                             io.src<double>(i_s), io.dst<double>(o_s), io.dst<float>(o_w), io.dst<float>(o_g), io.dst<float>(o_rw))))
        return rc;
    return io.finish();
}

// seven inputs: SyncHostCall::kMax
int align_volume_solve_group_r_host(msiren_ctx* h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                                    const msiren_align_volume_solve_group_opts* o, const int32_t* group_start, int64_t G, const double* planes, const double* rigid_in,
                                    const float* weights_host, const float* intensity_in, const double* scale_host, float* maps_out, float* intensity_out, double* rigid_out,
                                    double* report, double* target_report, double* trace) {
    const int64_t M = m * (int64_t)th * tw;
    bool done;
    int rc = check(h);
    if ((rc = host_preamble(rc ? rc : align_volume_solve_group_check(h, n, height, width, m, th, tw, o, group_start, G, planes, rigid_in, maps_out, intensity_out, report),
                            M == 0, !images_host || !targets_host || !scale_host, n, height, width, &done)) || done) return rc;
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)M * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(images_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY);
    const int i_p = io.in(planes, (size_t)m * 12 * sizeof(double), HOST_COPY), i_r = io.in(rigid_in, (size_t)G * 12 * sizeof(double), HOST_COPY);
    const int i_w = io.in(weights_host, nt, HOST_COPY), i_gb = io.in(intensity_in, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int i_s = io.in(scale_host, (size_t)m * sizeof(double), HOST_COPY);
    const int o_m = io.out(maps_out, (size_t)m * 9 * sizeof(float), HOST_COPY), o_gb = io.out(intensity_out, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int o_r = io.out(rigid_out, (size_t)G * 12 * sizeof(double), HOST_COPY), o_rep = io.out(report, (size_t)G * 7 * sizeof(double), HOST_COPY);
    const int o_tr = io.out(target_report, (size_t)m * 3 * sizeof(double), HOST_COPY), o_trace = io.out(trace, (size_t)o->iterations * G * 15 * sizeof(double), HOST_COPY);
    if ((rc = io.begin())) return rc;
    if ((rc = align_volume_solve_group_r(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), m, th, tw, o, group_start, G, io.src<double>(i_p), io.src<double>(i_r),
                                         io.src<float>(i_w), io.src<float>(i_gb), io.src<double>(i_s), io.dst<float>(o_m), io.dst<float>(o_gb), io.dst<double>(o_r),
                                         io.dst<double>(o_rep), io.dst<double>(o_tr), io.dst<double>(o_trace))))
        return rc;
    return io.finish();
}

// the stack forms: as the two above with the stack in the place of the images, on a handle that needs no weights
int align_stack_r_host(msiren_ctx* h, const float* stack_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                       const float* maps_host, const float* weights_host, const float* intensity_host, const double* scale_host, double* sums_host, float* warped_host,
                       float* wgrad_host, float* rweight_host) {
    const int64_t M = m * (int64_t)th * tw;
    int rc = check(h, false);
    if (rc || (rc = align_stack_check(h, n, height, width, m, th, tw)) || M == 0) return rc;
    const char* const missing = !stack_host ? "stack" : !targets_host ? "targets" : !maps_host ? "maps" : !scale_host ? "scale" : !sums_host ? "sums" : nullptr;
    if (missing) return fail(MSIREN_E_INVALID, "null argument (%s)", missing);
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)M * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(stack_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY), i_m = io.in(maps_host, (size_t)m * 9 * sizeof(float), HOST_COPY);
    const int i_w = io.in(weights_host, nt, HOST_COPY), i_gb = io.in(intensity_host, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int i_s = io.in(scale_host, (size_t)m * sizeof(double), HOST_COPY);
    const int o_s = io.out(sums_host, (size_t)m * kAlignVolumeSumsW * sizeof(double), HOST_IN_PLACE);
    const int o_w = io.out(warped_host, nt, HOST_IN_PLACE), o_g = io.out(wgrad_host, 3 * nt, HOST_IN_PLACE), o_rw = io.out(rweight_host, nt, HOST_IN_PLACE);
    if ((rc = io.begin())) return rc;
    if ((rc = align_stack_r(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), m, th, tw, io.src<float>(i_m), io.src<float>(i_w), io.src<float>(i_gb),
                            io.src<double>(i_s), io.dst<double>(o_s), io.dst<float>(o_w), io.dst<float>(o_g), io.dst<float>(o_rw))))
        return rc;
    return io.finish();
}

int align_stack_solve_group_r_host(msiren_ctx* h, const float* stack_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                                   const msiren_align_volume_solve_group_opts* o, const int32_t* group_start, int64_t G, const double* planes, const double* rigid_in,
                                   const float* weights_host, const float* intensity_in, const double* scale_host, float* maps_out, float* intensity_out, double* rigid_out,
                                   double* report, double* target_report, double* trace) {
    const int64_t M = m * (int64_t)th * tw;
    int rc = check(h, false);
    if (rc || (rc = align_stack_solve_group_check(h, n, height, width, m, th, tw, o, group_start, G, planes, rigid_in, maps_out, intensity_out, report)) || M == 0) return rc;
    const char* const missing = !stack_host ? "stack" : !targets_host ? "targets" : !scale_host ? "scale" : nullptr;
    if (missing) return fail(MSIREN_E_INVALID, "null argument (%s)", missing);
    Call c = make_call(h, true);
    const size_t ni = (size_t)n * height * width * sizeof(float), nt = (size_t)M * sizeof(float);
    SyncHostCall io(h, c.stream);
    const int i_img = io.in(stack_host, ni, HOST_COPY), i_t = io.in(targets_host, nt, HOST_COPY);
    const int i_p = io.in(planes, (size_t)m * 12 * sizeof(double), HOST_COPY), i_r = io.in(rigid_in, (size_t)G * 12 * sizeof(double), HOST_COPY);
    const int i_w = io.in(weights_host, nt, HOST_COPY), i_gb = io.in(intensity_in, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int i_s = io.in(scale_host, (size_t)m * sizeof(double), HOST_COPY);
    const int o_m = io.out(maps_out, (size_t)m * 9 * sizeof(float), HOST_COPY), o_gb = io.out(intensity_out, (size_t)m * 2 * sizeof(float), HOST_COPY);
    const int o_r = io.out(rigid_out, (size_t)G * 12 * sizeof(double), HOST_COPY), o_rep = io.out(report, (size_t)G * 7 * sizeof(double), HOST_COPY);
    const int o_tr = io.out(target_report, (size_t)m * 3 * sizeof(double), HOST_COPY), o_trace = io.out(trace, (size_t)o->iterations * G * 15 * sizeof(double), HOST_COPY);
    if ((rc = io.begin())) return rc;
    if ((rc = align_stack_solve_group_r(h, c, io.src<float>(i_img), n, height, width, io.src<float>(i_t), m, th, tw, o, group_start, G, io.src<double>(i_p), io.src<double>(i_r),
                                        io.src<float>(i_w), io.src<float>(i_gb), io.src<double>(i_s), io.dst<float>(o_m), io.dst<float>(o_gb), io.dst<double>(o_r),
                                        io.dst<double>(o_rep), io.dst<double>(o_tr), io.dst<double>(o_trace))))
        return rc;
    return io.finish();
}

}  // namespace

extern "C" {

int msiren_align_stack_r(msiren_handle h, const float* stack_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                         const float* maps_host, const float* weights_host, const float* intensity_host, const double* scale_host, double* sums_host, float* warped_host,
                         float* wgrad_host, float* rweight_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_stack_r_host(h, stack_host, n, height, width, targets_host, m, th, tw, maps_host, weights_host, intensity_host, scale_host, sums_host, warped_host, wgrad_host,
                              rweight_host);
}
int msiren_align_stack_r_dev(msiren_handle h, const float* stack_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th, int32_t tw,
                             const float* maps_dev, const float* weights_dev, const float* intensity_dev, const double* scale_dev, double* sums_dev, float* warped_dev,
                             float* wgrad_dev, float* rweight_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    if ((rc = align_stack_check(h, n, height, width, m, th, tw))) return rc;  // (before the stream rotates)
    return align_stack_r(h, dev_call(h), stack_dev, n, height, width, targets_dev, m, th, tw, maps_dev, weights_dev, intensity_dev, scale_dev, sums_dev, warped_dev, wgrad_dev,
                         rweight_dev);
}
int msiren_align_stack_solve_group_r(msiren_handle h, const float* stack_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th,
                                     int32_t tw, const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start, int64_t n_groups, const double* planes,
                                     const double* rigid_in, const float* weights_host, const float* intensity_in, const double* scale, float* maps_out, float* intensity_out,
                                     double* rigid_out, double* report, double* target_report, double* trace) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_stack_solve_group_r_host(h, stack_host, n, height, width, targets_host, m, th, tw, opts, group_start, n_groups, planes, rigid_in, weights_host, intensity_in,
                                          scale, maps_out, intensity_out, rigid_out, report, target_report, trace);
}
int msiren_align_stack_solve_group_r_dev(msiren_handle h, const float* stack_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                                         int32_t tw, const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start, int64_t n_groups, const double* planes_dev,
                                         const double* rigid_in_dev, const float* weights_dev, const float* intensity_in_dev, const double* scale_dev, float* maps_out_dev,
                                         float* intensity_out_dev, double* rigid_out_dev, double* report_dev, double* target_report_dev, double* trace_dev) {
    int rc = check(h, false);
    if (rc) return rc;
    if ((rc = align_stack_solve_group_check(h, n, height, width, m, th, tw, opts, group_start, n_groups, planes_dev, rigid_in_dev, maps_out_dev, intensity_out_dev, report_dev)))
        return rc;  // (before the stream rotates)
    return align_stack_solve_group_r(h, dev_call(h), stack_dev, n, height, width, targets_dev, m, th, tw, opts, group_start, n_groups, planes_dev, rigid_in_dev, weights_dev,
                                     intensity_in_dev, scale_dev, maps_out_dev, intensity_out_dev, rigid_out_dev, report_dev, target_report_dev, trace_dev);
}

int msiren_align_volume_r(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                          const float* maps_host, const float* weights_host, const float* intensity_host, const double* scale_host, double* sums_host, float* warped_host,
                          float* wgrad_host, float* rweight_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_volume_r_host(h, images_host, n, height, width, targets_host, m, th, tw, maps_host, weights_host, intensity_host, scale_host, sums_host, warped_host, wgrad_host,
                               rweight_host);
}
int msiren_align_volume_r_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th, int32_t tw,
                              const float* maps_dev, const float* weights_dev, const float* intensity_dev, const double* scale_dev, double* sums_dev, float* warped_dev,
                              float* wgrad_dev, float* rweight_dev) {
    int rc = check(h);
    if (rc) return rc;
    if ((rc = align_volume_w_check(h, n, height, width, m, th, tw))) return rc;  // (before the stream rotates)
    return align_volume_r(h, dev_call(h), images_dev, n, height, width, targets_dev, m, th, tw, maps_dev, weights_dev, intensity_dev, scale_dev, sums_dev, warped_dev, wgrad_dev,
                          rweight_dev);
}
int msiren_align_volume_solve_group_r(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th,
                                      int32_t tw, const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start, int64_t n_groups, const double* planes,
                                      const double* rigid_in, const float* weights_host, const float* intensity_in, const double* scale, float* maps_out, float* intensity_out,
                                      double* rigid_out, double* report, double* target_report, double* trace) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_volume_solve_group_r_host(h, images_host, n, height, width, targets_host, m, th, tw, opts, group_start, n_groups, planes, rigid_in, weights_host, intensity_in,
                                           scale, maps_out, intensity_out, rigid_out, report, target_report, trace);
}
int msiren_align_volume_solve_group_r_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                                          int32_t tw, const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start, int64_t n_groups, const double* planes_dev,
                                          const double* rigid_in_dev, const float* weights_dev, const float* intensity_in_dev, const double* scale_dev, float* maps_out_dev,
                                          float* intensity_out_dev, double* rigid_out_dev, double* report_dev, double* target_report_dev, double* trace_dev) {
    int rc = check(h);
    if (rc) return rc;
    if ((rc = align_volume_solve_group_check(h, n, height, width, m, th, tw, opts, group_start, n_groups, planes_dev, rigid_in_dev, maps_out_dev, intensity_out_dev, report_dev)))
        return rc;  // (before the stream rotates)
    return align_volume_solve_group_r(h, dev_call(h), images_dev, n, height, width, targets_dev, m, th, tw, opts, group_start, n_groups, planes_dev, rigid_in_dev, weights_dev,
                                      intensity_in_dev, scale_dev, maps_out_dev, intensity_out_dev, rigid_out_dev, report_dev, target_report_dev, trace_dev);
}

int msiren_align_volume_solve_group(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th,
                                    int32_t tw, const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start, int64_t n_groups, const double* planes,
                                    const double* rigid_in, const float* weights_host, const float* intensity_in, float* maps_out, float* intensity_out, double* rigid_out,
                                    double* report, double* target_report, double* trace) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_volume_solve_group_host(h, images_host, n, height, width, targets_host, m, th, tw, opts, group_start, n_groups, planes, rigid_in, weights_host, intensity_in,
                                         maps_out, intensity_out, rigid_out, report, target_report, trace);
}
int msiren_align_volume_solve_group_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                                        int32_t tw, const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start, int64_t n_groups, const double* planes_dev,
                                        const double* rigid_in_dev, const float* weights_dev, const float* intensity_in_dev, float* maps_out_dev, float* intensity_out_dev,
                                        double* rigid_out_dev, double* report_dev, double* target_report_dev, double* trace_dev) {
    int rc = check(h);
    if (rc) return rc;
    if ((rc = align_volume_solve_group_check(h, n, height, width, m, th, tw, opts, group_start, n_groups, planes_dev, rigid_in_dev, maps_out_dev, intensity_out_dev, report_dev)))
        return rc;  // (before the stream rotates)
    return align_volume_solve_group(h, dev_call(h), images_dev, n, height, width, targets_dev, m, th, tw, opts, group_start, n_groups, planes_dev, rigid_in_dev, weights_dev,
                                    intensity_in_dev, maps_out_dev, intensity_out_dev, rigid_out_dev, report_dev, target_report_dev, trace_dev);
}

int msiren_align_volume_w(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th, int32_t tw,
                          const float* maps_host, const float* weights_host, const float* intensity_host, double* sums_host, float* warped_host, float* wgrad_host) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_volume_w_host(h, images_host, n, height, width, targets_host, m, th, tw, maps_host, weights_host, intensity_host, sums_host, warped_host, wgrad_host);
}
int msiren_align_volume_w_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th, int32_t tw,
                              const float* maps_dev, const float* weights_dev, const float* intensity_dev, double* sums_dev, float* warped_dev, float* wgrad_dev) {
    int rc = check(h);
    if (rc) return rc;
    if ((rc = align_volume_w_check(h, n, height, width, m, th, tw))) return rc;  // (before the stream rotates)
    return align_volume_w(h, dev_call(h), images_dev, n, height, width, targets_dev, m, th, tw, maps_dev, weights_dev, intensity_dev, sums_dev, warped_dev, wgrad_dev);
}
int msiren_align_volume_solve_w(msiren_handle h, const float* images_host, int64_t n, int32_t height, int32_t width, const float* targets_host, int64_t m, int32_t th,
                                int32_t tw, const msiren_align_volume_solve_w_opts* opts, const float* maps_in, const double* planes, const double* rigid_in,
                                const float* weights_host, const float* intensity_in, float* maps_out, float* intensity_out, double* rigid_out, double* report,
                                double* trace) {
    if (!h) return fail(MSIREN_E_INVALID, "null handle");
    return align_volume_solve_w_host(h, images_host, n, height, width, targets_host, m, th, tw, opts, maps_in, planes, rigid_in, weights_host, intensity_in, maps_out,
                                     intensity_out, rigid_out, report, trace);
}
int msiren_align_volume_solve_w_dev(msiren_handle h, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                                    int32_t tw, const msiren_align_volume_solve_w_opts* opts, const float* maps_in_dev, const double* planes_dev, const double* rigid_in_dev,
                                    const float* weights_dev, const float* intensity_in_dev, float* maps_out_dev, float* intensity_out_dev, double* rigid_out_dev,
                                    double* report_dev, double* trace_dev) {
    int rc = check(h);
    if (rc) return rc;
    if ((rc = align_volume_solve_w_check(h, n, height, width, m, th, tw, opts, maps_in_dev, planes_dev, rigid_in_dev, maps_out_dev, intensity_out_dev, report_dev)))
        return rc;  // (before the stream rotates)
    return align_volume_solve_w(h, dev_call(h), images_dev, n, height, width, targets_dev, m, th, tw, opts, maps_in_dev, planes_dev, rigid_in_dev, weights_dev, intensity_in_dev,
                                maps_out_dev, intensity_out_dev, rigid_out_dev, report_dev, trace_dev);
}

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
    // As the resample entry points, and unlike the weighted, volume and solve forms above: no check in front of dev_call, so a call that
    // align_check refuses has rotated the stream already.  Kept: which stream the next call takes is observable.
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
