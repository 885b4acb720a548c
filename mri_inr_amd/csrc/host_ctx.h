// Shared by the host translation units of libmsiren.so (round 6: the former 3 000-line msiren.hip, cut by responsibility):
//     msiren.hip           C ABI: lifecycle, weights, the forward / slice entry points on host pointers, memory, timing, info
//     dispatch.h           which kernel runs for which model and call: pure functions, no HIP (tests/test_dispatch.py)
//     launch_dispatch.hip  the launches of what dispatch.h picks: trunks, prologue, tiling / fold, the *_dev slice pipeline and its
//                          prologue (slice_prologue: what the geometry calls of resample.hip start with)
//     trunk_instances.h    the one list of kernel instances: k_*.hip instantiate it, the host units declare it extern
//     weights_pack.hip     state_dict -> the kernels' weight layouts (host arithmetic + uploads)
//     host_buffers.hip     what a caller's host range is (pageable / page-locked / page-locked in part), bounce buffers, and the one
//                          protocol of a synchronous host-pointer call around them (SyncHostCall: every such entry point uses it)
//     comm_rccl.hip        RCCL through dlopen: communicator, the one weight broadcast, barrier / MAX
//     diagnostics.hip      stamped timeline builds, the sustained-MFMA probe
//     scores.hip           PSNR / SSIM / NRMSE of image pairs (the evaluation harness's metrics; kernels: scores.hip.h)
//     sample_grid.hip      the trunk at caller-chosen coordinates and the slice pipeline at another output stride: the per-call layer-0
//                          table (kernel: sample_grid.hip.h), msiren_sample_*, msiren_upsampled_*, the *_scaled entry points; the
//                          gradient calls (msiren_sample_grad_*, msiren_reconstruct_slices_grad: siren_trunk_f32_jet.hip.h)
//     resample.hip         one coordinate set per patch: msiren_sample_ragged_* (kernels: siren_trunk_f32_ragged.hip.h; the *_native
//                          forms: siren_trunk_f16x3n_ragged.hip.h), and the
//                          reconstruction at arbitrary points built on it: msiren_resample_slices* (bin / blend kernels: resample.hip.h) and
//                          msiren_resample_volume* (a stack read as a volume; resample_volume.hip.h), msiren_align_slices* (slices scored
//                          under affine maps against targets; align.hip.h), msiren_align_solve* (the damped Gauss-Newton loop around it),
//                          msiren_align_slices_w* / msiren_align_solve_w* (the two with a per-pixel weight and a per-slice gain and bias; align_w.hip.h),
//                          msiren_align_volume* / msiren_align_volume_solve* (target slices against the stack read as a volume, 3 x 3 maps; align_volume.hip.h),
//                          msiren_align_volume_w* / msiren_align_volume_solve_w* (those two with a per-pixel weight and a per-target gain and bias; align_volume_w.hip.h).
//                          The whole of these families lives here: checks, pipelines on the call's stream, host-pointer forms, entry points,
//                          and the only inclusion of their six kernel headers
//     align_plan.h         the scratch layouts and size limits of those calls: pure functions, no HIP (tests/test_align_plan.py)
//     fuse.hip             msiren_fuse_targets*: the aligned targets of the volume alignment calls gathered back onto the stack's voxel grid
//                          (kernels: fuse.hip.h); what it refuses, its tiling and scratch: fuse_plan.h, pure functions, no HIP
//                          (tests/test_fuse_reference.py)
//                          and msiren_project_volume*: the way back, a stack gathered onto the targets' lattices (kernels: project.hip.h; refusals,
//                          tiling, scratch and the box of voxels per pixel: project_plan.h, tests/test_project_reference.py)
//                          and msiren_solve_volume*: conjugate gradients on those two operators in one call (kernels: solve_volume.hip.h;
//                          refusals, scratch and the launch plan: solve_volume_plan.h, tests/test_solve_volume_reference.py)
//                          and msiren_solve_volume_r*: that solve in rounds reweighted by a Geman-McClure loss (kernels: solve_volume_r.hip.h;
//                          refusals, scratch, the schedule and the launch plan: solve_volume_r_plan.h, tests/test_solve_volume_robust_reference.py)
//     residual_scale.hip   msiren_residual_scale*: the scale of the robust calls from an exact order statistic of the residuals, on the device
//                          (kernels: residual_scale.hip.h, an MSD radix select per segment of targets; refusals, chunking, launch count and
//                          scratch: residual_scale_plan.h, tests/test_residual_scale_plan.py).  A unit of its own: it includes none of the other
//                          families' kernel headers
// Everything in namespace mh is internal (the library is built with -fvisibility=hidden; only include/msiren.h is exported).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/msiren.h"
#include "dispatch.h"
#include "encoder_params.h"
#include "pass_queue.h"

typedef struct ncclComm* ncclComm_t;  // (<rccl/rccl.h>'s own typedef: the handle only stores the pointer)

namespace mh {

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
const char* last_error();

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return ::mh::fail(MSIREN_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

}  // namespace mh

struct msiren_ctx {
    msiren_config cfg{};
    int H = 0, HP = 0, L = 0, Z = 0, S = 0, P = 0, O = 0, I = 0;
    // Up to three streams with private scratch: with msiren_set_streams(h, 2) consecutive *_dev forward
    // calls alternate between them, so the under-occupied tail of one call's persistent trunk kernel
    // overlaps the encoder / modulator / trunk start of the next call.  Three (round 5): call k+2's prologue no longer queues
    // behind call k's trunk -- for a trunk that OWNS its CUs (config 5: 1.76 rounds per slice) the next trunk is then ready when the
    // half-empty last round begins.
    struct StreamCtx {
        hipStream_t s = nullptr;
        mh::DevBuf mods, modpad, latent, patches, keep, rec, queue, feat, plan;
        mh::DevBuf score;     // partials of msiren_score_images(_dev) (scores.hip.h)
        mh::DevBuf cscratch;  // split-fp16 Modulator: the latent part of layers 1.., lane-private (encoder_modulator_f16x3.hip.h)
        mh::DevBuf coords, l0tab;  // msiren_sample_*: the call's coordinates (host-pointer form) and its layer-0 table (sample_grid.hip)
        mh::DevBuf ragged;         // per-patch coordinate sets (resample.hip): the item table of the ragged trunks, offsets of the host-pointer form
        struct Lattice {           // an output stride's lattice, kept per stream until the next msiren_commit_weights (sample_grid.hip)
            int out_stride = 0, tile = 0, pad = 0;  // I', S', pad'
            float *coords = nullptr, *table = nullptr, *foldw = nullptr;  // (S'S', 2); (H/4, S'S', 4) or null (fp32 trunk); (S', S')
            std::vector<float> host;  // what coords and foldw were uploaded from (alive while the copies may be in flight)
        };
        std::vector<Lattice> lattices;
        hipEvent_t ev_join = nullptr;  // a host call that pipelines itself: this stream's chunk has been enqueued
        msiren::PassQueue pq;  // host view of the never-reset pass counter (pass_queue.h)
    } sc[3];
    int cur = 0, nstreams = 1;  // cur: the stream the next asynchronous (*_dev) call takes (next_stream rotates it)
    msiren::DispatchHandle dh;  // what dispatch.h reads of this handle: the knobs from msiren_create, the rest from msiren_commit_weights
    const char* last_trunk = "";  // name of the trunk instance launched last (msiren_last_trunk_kernel; msiren::kInstances)
    const char* last_prologue = "";  // name of the latent_mods instance launched last, "" behind the per-layer fp32 launches (msiren_last_prologue_kernel)
    struct { const void* k = nullptr; int bytes = 0; } lds_set[8];  // the dynamic-LDS limit raised per kernel (launch_dispatch.hip: launch)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::map<std::string, std::vector<float>> tensors;  // state_dict, host copies
    std::map<std::string, size_t> expected;             // key -> element count
    std::vector<float> grid_host;                       // the coordinate grid in effect (state_dict's, or rebuilt)
    bool committed = false, have_modulator = false, have_encoder = false;
    // trunk
    float *d_grid = nullptr, *d_l0 = nullptr, *d_wp = nullptr, *d_bias = nullptr, *d_wout = nullptr;
    float *d_w0raw = nullptr, *d_b0raw = nullptr;  // net.layers.0.weight (H, 2) / .bias (H; zeros without bias) as stored: layer0_table_kernel
    float bout = 0.f, cg0 = 0.f, cg = 0.f;
    // split-fp16 trunk (MSIREN_PREC_F16X3)
    void* d_wp16n = nullptr;  // weight stream of the 16x16x32 kernel (default)
    // f16x3 domain guard: a word in host memory the trunk kernels set when a scaled modulation does not fit fp16
    volatile int* status_host = nullptr;
    int* status_dev = nullptr;
    unsigned range_epoch = 0;      // number of the split-fp16 trunk launch in flight (what it writes to its stream's flag word)
    int64_t range_events = 0;      // synchronisations that found the conditional exact-fp32 trunk had run, since create
    float* d_dump = nullptr;       // 256 floats: where lanes of the weight-stationary trunk that have nothing to store write
    int trace_host = 0;            // MSIREN_TRACE_HOST=1: msiren_forward_tiles prints the host-side timeline of the call (stderr)
    float *d_bias16 = nullptr, *d_wout16 = nullptr, *d_s0t = nullptr;
    float mscale16[16] = {0};  // 16x16 kernel: factor of each layer's modulation row (the NEXT layer's weight scale, inverted)
    bool f16x3_ready = false;
    // single-product 16-bit trunk (MSIREN_PREC_BF16 / MSIREN_PREC_F16), H = 512
    void *d_woutx1 = nullptr, *d_wpx1n = nullptr;  // last_layer.weight (fp16); weight stream of siren_trunk_x1n.hip.h
    void* d_wpx1w = nullptr;       // weight stream of siren_trunk_x1w.hip.h (weight-stationary: 64 KB per layer, N-pass and wave)
    float* d_bias32x1 = nullptr;   // bias rows: fp32, in revolutions x the layer's weight scale
    float* d_s0t512 = nullptr;
    float winvx1[64] = {0};
    bool x1_ready = false;
    int num_cus = 256;
    // environment knobs (the whole list): read ONCE, at msiren_create -- not on the launch path (dispatch's: dh)
    static constexpr int host_first = 112, host_piece = 400;  // tiles in the first / the further chunks of a pipelined host call (host_plan.h)
    unsigned queue_start = 0;  // MSIREN_QUEUE_START: initial value of the never-reset pass counters (tests: wrap-around)
    // modulator: transposed weights so that consecutive threads read consecutive outputs
    float *d_modw = nullptr, *d_modb = nullptr, *d_modw_rm = nullptr;  // transposed / as stored (row-major)
    // encoder
    float *d_encw = nullptr, *d_c3w_rm = nullptr, *d_fcw_rm = nullptr;  // the latter two point into d_encw
    msiren::EncoderParams enc{};
    // encoder tail + Modulator in split-fp16 arithmetic, one launch (encoder_modulator_f16x3.hip.h); every precision but fp32
    void* d_emw = nullptr;         // packed weight streams of the four waves
    void* d_emc2 = nullptr;        // conv2's MFMA A fragments
    float* d_embias = nullptr;     // [conv3 64][fc Z][modulator L x H]
    float em_winv_c3 = 1.f, em_winv_fc = 1.f, em_winv_z[64] = {0}, em_winv_h[64] = {0};
    int em_wave_stride = 0, em_zp_start = 0;
    bool em_enc = false, em_mod = false;  // which halves of the stream are packed (the checkpoint's key set decides)
    int em_enabled = 1;            // MSIREN_PROLOGUE_F16X3=0: the exact-fp32 launches per layer on a split-fp16 handle (tests, A/B)
    float* d_foldw = nullptr;  // (S,S) overlap-add weights
    // workspaces
    mh::DevBuf stage_in, stage_out;  // staging of the host-pointer entry points, carved per call by SyncHostCall (host_buffers.h)
    // profiling
    bool profile = false;
    int64_t prof_launches = 0;
    double prof_ms = 0.0;
    struct ProfRec { hipEvent_t a, b; int kernel; int64_t coords; };
    struct ProfKernel { std::string name; int64_t launches = 0, coords = 0; double ms = 0.0; bool trunk = true; };  // trunk: counts in msiren_profile_read's totals
    std::vector<ProfRec> prof_events;
    std::vector<ProfKernel> prof_kernels;  // totals per trunk instance since msiren_profile_enable(h, 1), in order of first launch
    size_t prof_used = 0;
    // multi-GPU: RCCL communicator this handle is a rank of (msiren_comm_*), staging buffer of its collectives
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_n = 1;
    mh::DevBuf ws_comm;
};

namespace mh {

// One call's launch state, passed by reference from the entry point down through the launchers: nothing of it lives on the handle.
// Synchronous one-chunk msiren_forward_tiles calls (round 5): the host is going to wait for the stream anyway, so the trunk raises its
// flag in HOST memory (status_host[8]) and the call looks at it after the wait -- no conditional launch (4.4 us of kernel + a launch
// gap per call); a flagged call enqueues the exact-fp32 trunk then and waits once more (profiles/r5/12_*).
struct HostCheck { const float* mods = nullptr; int64_t B = 0; float* out = nullptr; unsigned epoch = 0; bool armed = false; };
// The coordinate set a call evaluates: null / 0 = the model's own grid and the table committed with the weights.
struct CoordSet {
    const float* coords = nullptr;  // device, (Q, 2): what the fp32 trunks read (the conditional ones of the domain guard included)
    const float* table = nullptr;   // device, (H/4, Q, 4): layer 0 of the 16-bit trunks (layer0_table_kernel); null on an fp32 handle
    int Q = 0;
};
struct Call {
    int stream = 0;                    // h->sc[stream]
    msiren::CallMode mode;             // what dispatch.h reads of the call
    const int* plan = nullptr;         // device-side list of kept patches (slice pipeline; mode.plan)
    hipEvent_t trunk_wait = nullptr;  // the trunk waits for this event first (a pipelined host call's weight-stationary last chunk)
    HostCheck* hc = nullptr;           // mode.host_check: where the trunk launch leaves what the host check needs
    CoordSet cs;                       // msiren_sample_* / the *_scaled pipeline (with_coords sets it and mode.coords together)
    int P(const msiren_ctx* h) const { return cs.Q ? cs.Q : h->P; }  // coordinates per patch of this call
};
inline Call with_coords(Call c, const CoordSet& cs) {
    c.cs = cs;
    c.mode.coords = cs.Q;
    return c;
}
inline Call make_call(const msiren_ctx* h, bool sync) {
    Call c;
    c.stream = h->cur;
    c.mode.nstreams = h->nstreams;
    c.mode.sync = sync;
    return c;
}

// the output side of the slice pipeline where it is not the model's own (the call carries the lattice: Call::cs): tile S', stride I',
// padding pad', fold weights (S', S')
struct OutGeom { int tile = 0, stride = 0, pad = 0; const float* foldw = nullptr; };
// the slice pipeline with its spatial gradient (msiren_reconstruct_slices_grad): the exact-fp32 jet trunk in place of the handle's trunk,
// grad (2, n, nV*I', nH*I') folded plane by plane; every gradient multiplied by gscale (coordinate units per output pixel)
struct GradOut { float* grad = nullptr; float gscale = 1.f; };

// msiren.hip
int use_device(msiren_ctx* h);
int ensure(msiren_ctx* h, DevBuf& b, size_t bytes);                 // grow-only device workspace
int upload(float** dst, const std::vector<float>& src);            // (re)allocate + blocking H2D copy
int check(msiren_ctx* h, bool need_commit = true);
// refusals that several entry points share; 0, or MSIREN_E_INVALID
int check_tile_size(const msiren_ctx* h, bool cite = true);  // the custom encoder takes 32 x 32 tiles; cite: the wording that names the reference's line
int check_reflect_padding(const msiren_ctx* h, int32_t height, int32_t width);  // torch's reflect padding requires pad < dim (F.pad raises otherwise)
int check_pairs_aligned(const void* dev, const char* what);  // `what` (coordinates, points) is read as (row, column) pairs: 8-byte aligned
int sync_all(msiren_ctx* h);
bool take_range_flag(msiren_ctx* h);
void next_stream(msiren_ctx* h);   // asynchronous forward entry points rotate over the configured streams
Call dev_call(msiren_ctx* h);      // next_stream, then the call of an asynchronous entry point

// weights_pack.hip: state_dict -> kernel layouts.  pack_modulator / pack_encoder return 1 when their keys are absent.
void declare_expected(msiren_ctx* h);
int pack_trunk(msiren_ctx* h);
int pack_trunk_f16x3(msiren_ctx* h);
int pack_trunk_x1(msiren_ctx* h);
int pack_modulator(msiren_ctx* h);
int pack_encoder(msiren_ctx* h);
int pack_prologue_f16x3(msiren_ctx* h);
int pack_fold_weights(msiren_ctx* h);
std::vector<float> fold_weight_matrix(int S);  // generate_weight_matrix(S) of the reference (tiling.py:67-88), (S, S)

// launch_dispatch.hip: everything below enqueues on h->sc[c.stream].s
void describe_for_dispatch(msiren_ctx* h);  // h->dh from the committed weights (msiren_commit_weights)
// msiren_profile_enable: an event pair around a launch on stream s; `name` null = the trunk launched last
int profile_begin(msiren_ctx* h, int s, hipEvent_t* end_event);
int profile_end(msiren_ctx* h, int s, hipEvent_t end_event, int64_t coords, const char* name = nullptr);
int launch_trunk(msiren_ctx* h, const Call& c, const float* mods_dev, int64_t B, float* out_dev);
int launch_trunk_f32_cond(msiren_ctx* h, const Call& c, const float* mods_dev, int64_t B, float* out_dev, const int* flag_word = nullptr, unsigned flag_val = 0);
int launch_modulator(msiren_ctx* h, const Call& c, const float* z_dev, int64_t B, float* mods_dev);
int launch_encoder(msiren_ctx* h, const Call& c, const float* tiles_dev, int64_t B, float* z_dev);
int encode_modulate_dev(msiren_ctx* h, const Call& c, const float* tiles_dev, int64_t B, float* z_dev, float* mods_dev);  // z_dev may be null
int forward_latent_dev(msiren_ctx* h, const Call& c, const float* z_dev, int64_t B, float* out_dev, float* mods_out_dev);
int forward_tiles_dev(msiren_ctx* h, const Call& c, const float* tiles_dev, int64_t B, float* out_dev);
int reconstruct_slices(msiren_ctx* h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, float* recon_dev, const OutGeom* og = nullptr,
                       const GradOut* go = nullptr);  // go: recon_dev may be null
int reconstruct_tiles_dev(msiren_ctx* h, const Call& c, const float* tiles_dev, int64_t n, int32_t nV, int32_t nH, float* recon_dev, const OutGeom* og = nullptr);
int weighted_fold_dev(msiren_ctx* h, const Call& c, const float* tiles_dev, int64_t n, int32_t nV, int32_t nH, float* recon_dev, const OutGeom& og);
// what every slice call runs in front of its trunk: tiling -> black flags -> plan -> the handle's prologue over the kept tiles.  Leaves the
// flags in sc.keep, the plan in sc.plan, the kept tiles' modulations in sc.mods; *pc: the call with the plan attached
int slice_prologue(msiren_ctx* h, const Call& c, const float* images_dev, int32_t height, int32_t width, float* patches_rw, const float* patches_ro, int64_t n,
                   int32_t nV, int32_t nH, Call* pc, bool* fused_out);
int jet_supported(msiren_ctx* h);  // 0, or MSIREN_E_INVALID: dim_hidden > 256 / residual (what the jet trunk does not take)
int launch_trunk_f32_jet(msiren_ctx* h, const Call& c, const float* mods_dev, int64_t B, float* out_dev /* may be null */, float* grad_dev, float gscale);

// One coordinate set per patch on the exact-fp32 trunks (siren_trunk_f32_ragged.hip.h), on handles of every precision.  Patch t of NP owns
// coords[offsets[t] : offsets[t + 1]] of the T coordinates; `reps` replicas of the item range, replica s with the modulation rows of patch
// s * NP + t (mods: (L, rows, H)), looked up through `pos` where given (negative: not evaluated).  items: scratch of NP + 1 words.
struct RaggedSet { const float* coords; const int* offsets; int64_t T; int64_t NP; int64_t reps; const int* pos; int64_t rows; int* items; };
int ragged_check(const RaggedSet& r, int chunk);  // 0, or MSIREN_E_INVALID: an index of the launch would leave 32 bits
int launch_trunk_f32_ragged(msiren_ctx* h, const Call& c, const RaggedSet& r, const float* mods_dev, float* out_dev /* (reps, T) */);
int launch_trunk_f32_jet_ragged(msiren_ctx* h, const Call& c, const RaggedSet& r, const float* mods_dev, float* out_dev /* may be null */, float* grad_dev /* (2, reps, T) */,
                                float gscale);

// The same sets in the handle's own trunk arithmetic (the *_native entry points): siren_trunk_f16x3n_ragged_kernel where
// ragged_native_pick (dispatch.h) says so, with the exact-fp32 ragged trunk as the conditional launch of the domain guard behind it
// (siren_trunk_f32_ragged_cond_kernel); on every other handle launch_trunk_f32_ragged, bit for bit.  items: NP + 1 words as above.
int launch_trunk_ragged_native(msiren_ctx* h, const Call& c, const RaggedSet& r, const float* mods_dev, float* out_dev /* (reps, T) */);

// resample.hip: the geometry pipelines behind the slice prologue, on h->sc[c.stream].s; their scratch layouts and limits: align_plan.h
// the reconstruction of n slices at M points shared by them (resample.hip.h); grad: out_dev may be null, grad_dev (2, n, M)
int resample_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t M, bool grad);  // 0, or MSIREN_E_INVALID: the model, or too many points
int resample_slices(msiren_ctx* h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* points_dev, int64_t M, float* out_dev,
                    float* grad_dev, bool grad, bool native = false);  // native (values only): launch_trunk_ragged_native
// a stack of n slices read as a volume at M points (Z, Y, X) (resample_volume.hip.h): out_dev (M); grad: out_dev may be null, grad_dev (3, M), n >= 2
int resample_volume_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t M, bool grad);  // 0, or MSIREN_E_INVALID, naming what is too large
int resample_volume(msiren_ctx* h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* points_dev, int64_t M, float* out_dev,
                    float* grad_dev, bool grad, bool native = false);  // native (values only): launch_trunk_ragged_native
// n slices scored under one 2 x 3 affine map each against targets (th, tw) (align.hip.h): sums_dev (n, 29) doubles; warped_dev (n, th, tw) and
// wgrad_dev (2, n, th, tw) may be null
constexpr int kAlignSums = 29;  // doubles per slice: count, cost, dcost[6], jtj[21] (align.hip.h: ALIGN_SUMS)
int align_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int32_t th, int32_t tw);  // 0, or MSIREN_E_INVALID: the model, or naming what is too large
int align_slices(msiren_ctx* h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                 const float* maps_dev, double* sums_dev, float* warped_dev, float* wgrad_dev);
// msiren_align_solve* (align.hip.h): the prologue once, then opts->iterations x (evaluation at the trial maps -> align_step_kernel) on the call's
// stream.  align_solve_check: every refusal that needs no device pointer (the host-pointer form asks it before it stages anything).
int align_solve_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int32_t th, int32_t tw, const msiren_align_solve_opts* o, const void* maps_in,
                      const void* rigid_in, const void* maps_out, const void* report);
int align_solve(msiren_ctx* h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                const msiren_align_solve_opts* o, const float* maps_in, const double* rigid_in, float* maps_out, double* rigid_out, double* report, double* trace);
// msiren_align_slices_w* and msiren_align_solve_w* (align_w.hip.h): the same pipeline with a per-pixel weight and a per-slice
// (gain, bias); weights_dev (n, th, tw) and intensity (n, 2) may be null; sums_dev (n, 47) doubles.  The checks as above; align_w_check also sizes
// the larger partial records.
constexpr int kAlignSumsW = 47;  // doubles per slice: count, wsum, cost, dcost[8], jtj[36] (align_w.hip.h: ALIGN_SUMS_W)
int align_w_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int32_t th, int32_t tw);
int align_slices_w(msiren_ctx* h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                   const float* maps_dev, const float* weights_dev, const float* intensity_dev, double* sums_dev, float* warped_dev, float* wgrad_dev);
int align_solve_w_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int32_t th, int32_t tw, const msiren_align_solve_w_opts* o, const void* maps_in,
                        const void* rigid_in, const void* maps_out, const void* intensity_out, const void* report);
int align_solve_w(msiren_ctx* h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int32_t th, int32_t tw,
                  const msiren_align_solve_w_opts* o, const float* maps_in, const double* rigid_in, const float* weights_dev, const float* intensity_in, float* maps_out,
                  float* intensity_out, double* rigid_out, double* report, double* trace);
// msiren_align_volume* and msiren_align_volume_solve* (align_volume.hip.h): m targets (th, tw) scored against the stack of n slices
// read as a volume, one 3 x 3 map (m, 9) each; sums_dev (m, 56) doubles; warped_dev (m, th, tw) and wgrad_dev (3, m, th, tw) may be null.  The solve:
// the prologue once, then opts->iterations x (evaluation at the trial maps -> align_volume_step_kernel) on the call's stream.
constexpr int kAlignVolumeSums = 56;  // doubles per target: count, cost, dcost[9], jtj[45] (align_volume.hip.h: ALIGN_VOLUME_SUMS)
int align_volume_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t m, int32_t th, int32_t tw);  // 0, or MSIREN_E_INVALID naming what is too large
int align_volume(msiren_ctx* h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th, int32_t tw,
                 const float* maps_dev, double* sums_dev, float* warped_dev, float* wgrad_dev);
int align_volume_solve_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t m, int32_t th, int32_t tw, const msiren_align_volume_solve_opts* o,
                             const void* maps_in, const void* planes, const void* rigid_in, const void* maps_out, const void* report);
int align_volume_solve(msiren_ctx* h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                       int32_t tw, const msiren_align_volume_solve_opts* o, const float* maps_in, const double* planes, const double* rigid_in, float* maps_out,
                       double* rigid_out, double* report, double* trace);
// msiren_align_volume_w* and msiren_align_volume_solve_w* (align_volume_w.hip.h): the same pipeline with a per-pixel weight and a
// per-target (gain, bias); weights_dev (m, th, tw) and intensity (m, 2) may be null; sums_dev (m, 80) doubles.  The checks as above;
// align_volume_w_check also sizes the larger partial records.
constexpr int kAlignVolumeSumsW = 80;  // doubles per target: count, wsum, cost, dcost[11], jtj[66] (align_volume_w.hip.h: ALIGN_VOLUME_SUMS_W)
int align_volume_w_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t m, int32_t th, int32_t tw);
int align_volume_w(msiren_ctx* h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th, int32_t tw,
                   const float* maps_dev, const float* weights_dev, const float* intensity_dev, double* sums_dev, float* warped_dev, float* wgrad_dev);
int align_volume_solve_w_check(msiren_ctx* h, int64_t n, int32_t height, int32_t width, int64_t m, int32_t th, int32_t tw, const msiren_align_volume_solve_w_opts* o,
                               const void* maps_in, const void* planes, const void* rigid_in, const void* maps_out, const void* intensity_out, const void* report);
int align_volume_solve_w(msiren_ctx* h, const Call& c, const float* images_dev, int64_t n, int32_t height, int32_t width, const float* targets_dev, int64_t m, int32_t th,
                         int32_t tw, const msiren_align_volume_solve_w_opts* o, const float* maps_in, const double* planes, const double* rigid_in, const float* weights_dev,
                         const float* intensity_in, float* maps_out, float* intensity_out, double* rigid_out, double* report, double* trace);

// sample_grid.hip
// the call evaluates and folds the lattice of out_stride (built on first use); table = false: without the 16-bit trunks' layer-0 table
int scaled_call(msiren_ctx* h, Call& c, int32_t out_stride, OutGeom* og, bool table = true);
void drop_lattices(msiren_ctx* h);  // msiren_commit_weights (the streams are idle), msiren_destroy

// comm_rccl.hip
int comm_destroy(msiren_ctx* h);

}  // namespace mh
