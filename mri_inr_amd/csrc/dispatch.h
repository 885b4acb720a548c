// Which kernel runs for which model and call: DESIGN.md section 4 as pure functions.  Plain C++, no HIP (unit-tested on the CPU by
// tests/test_dispatch.py): the launchers in launch_dispatch.hip and the host calls in msiren.hip ask these functions and launch what
// they return.  What they read is spelled out in their arguments: the handle as it was committed (DispatchHandle) and the call
// (CallMode); nothing here has state.
#pragma once
#include <cstdint>

#include "../../include/msiren.h"
#include "trunk_instances.h"

namespace msiren {

// ---- the instances (trunk_instances.h), each with its family, template arguments and name ------------------------------------
enum class Kernel : int { f32, f32_cond, f16x3n, f16x3h, f16x3w, x1n, x1w, latent_mods, encoder_conv };
struct Instance {
    Kernel family;
    int arg[4];        // template arguments (absent ones 0: the kernels' defaults)
    const char* name;  // msiren_last_trunk_kernel / the profile's names
};
inline constexpr Instance kInstances[] = {
#define MSIREN_TRUNK_ROW(fam, ...) {Kernel::fam, {__VA_ARGS__}, "siren_trunk_" #fam "_kernel<" #__VA_ARGS__ ">"},
#define MSIREN_PROLOGUE_ROW(fam, ...) {Kernel::fam, {__VA_ARGS__}, #fam "_f16x3_kernel<" #__VA_ARGS__ ">"},
    MSIREN_TRUNK_INSTANCES(MSIREN_TRUNK_ROW) MSIREN_PROLOGUE_INSTANCES(MSIREN_PROLOGUE_ROW)
#undef MSIREN_TRUNK_ROW
#undef MSIREN_PROLOGUE_ROW
};
constexpr int kNumInstances = sizeof kInstances / sizeof kInstances[0];

// row of kInstances, -1 if that instance is not compiled
constexpr int instance(Kernel k, int a0, int a1 = 0, int a2 = 0, int a3 = 0) {
    for (int i = 0; i < kNumInstances; ++i) {
        const Instance& r = kInstances[i];
        if (r.family == k && r.arg[0] == a0 && r.arg[1] == a1 && r.arg[2] == a2 && r.arg[3] == a3) return i;
    }
    return -1;
}

// ---- inputs -------------------------------------------------------------------------------------------------------------------
// What dispatch reads of a handle, fixed at msiren_commit_weights (the LDS facts come from the kernel headers there).
struct DispatchHandle {
    int precision = MSIREN_PREC_F32, H = 0, HP = 0, L = 0, Z = 0, P = 0, act = MSIREN_ACT_SINE, res = 0, num_cus = 256;
    bool f16x3_ready = false, x1_ready = false;  // packed split-fp16 (H = 256) / single-product 16-bit (H = 512) trunk weights
    bool em_enc = false, em_mod = false;         // which halves of the one-launch prologue's weight stream are packed
    bool f16_ring3_fits = false, f16_ring4_fits = false;  // F16Lds<3 | 4>::total(L) <= 160 KB
    bool ws_depth_ok = false;                              // WS_MIN_L <= L <= WS_MAX_L (WsLds<4>::total(L) fits)
    // environment knobs, read at msiren_create
    int f16_ws = 1;            // MSIREN_F16_WS=0: never the weight-stationary trunk
    int half_allowed = 1;      // MSIREN_F16_HALF=0: never the half-unit instance
    int em_depth = 0;          // MSIREN_EM_DEPTH: the split-fp16 prologue's weight-ring depth, forced
    int host_pipe_min = 2400;  // MSIREN_HOST_PIPE_MIN: tiles from which a host call cuts itself into chunks
};

// What dispatch reads of a call.
struct CallMode {
    int nstreams = 1;         // streams of the handle (msiren_set_streams)
    bool sync = false;        // a synchronous host-pointer call: it runs on one stream, nothing of the handle runs beside it
    int trunk = 0;            // a pipelined host call's chunk (HostChunk::trunk): 0 = the rule below, 1 = f16x3n ring 3, 2 = f16x3w
    bool beside = false;      // the prologue runs beside a trunk of the same call (HostChunk::beside)
    bool plan = false;        // a device-side list of kept patches is in effect: the batch size is not known on the host
    bool host_check = false;  // the trunk's domain guard is read on the host behind the call's wait (synchronous one-chunk call)
    int coords = 0;           // coordinates per patch of a call that brings its own set (msiren_sample_*, *_scaled); 0 = the handle's P
    bool alone() const { return nstreams == 1 || sync; }  // no other call of the handle runs beside this one
};

// ---- trunk -------------------------------------------------------------------------------------------------------------------
// what follows a 16-bit trunk launch when a scaled modulation leaves the fp16 domain
enum class Guard : int {
    none,      // the exact-fp32 trunk: nothing to guard
    f32_cond,  // siren_trunk_f32_cond_kernel<ACT> behind it on the same stream (conditional: leaves unless flagged)
    f32_512,   // fp16 and bf16 at H = 512 (both read an fp16 modulation table): siren_trunk_f32_kernel<512,ACT,RES> as the conditional launch
    host,      // the flag in host memory, read by the call after its wait (no launch)
};
struct TrunkPick {
    int inst = -1;        // row of kInstances
    int ring = 0;         // f16x3n / f16x3h: the weight ring R
    bool half = false;    // f16x3h: 16 coordinates per wave
    bool balanced = false;  // x1w: x1w_balanced_grid (the same rounds on fewer CUs) instead of every CU
    Guard guard = Guard::none;
};

inline bool use_f16x3(const DispatchHandle& d) {
    return d.precision == MSIREN_PREC_F16X3 && d.f16x3_ready && !d.res && d.f16_ring3_fits;
}

// The weight-stationary trunk is the faster kernel on its own (it owns the whole register file and LDS of its CUs, so nothing can
// run beside it); with two streams the register-resident trunk wins because the next call's encoder and modulator run beside it.
// Depths 3..5 (its unit images + tables must fit the LDS); modulation buffer below 4 GB.
inline bool ws_capable(const DispatchHandle& d, int64_t B) {
    return d.f16_ws && d.ws_depth_ok && (int64_t)d.L * B * 256 * 4 < (1LL << 32);
}

inline TrunkPick pick_trunk(const DispatchHandle& d, const CallMode& m, int64_t B) {
    TrunkPick t;
    const int act = d.act == MSIREN_ACT_MORLET ? 1 : 0, res = d.res ? 1 : 0;
    if (d.x1_ready) {  // H = 512: weight-stationary where its layer pipeline has a hidden layer before the final one
        const int bf = d.precision == MSIREN_PREC_BF16 ? 1 : 0;
        // (one-stream handles: the balanced grid, 1 % faster alone; two streams: every CU, so that the next call's trunk can start in
        //  the half-empty last round -- 111.2 against 109.3 Mpixel/s, profiles/r4/09_*)
        t.balanced = d.L >= 3 && m.alone();
        t.inst = d.L >= 3 ? instance(Kernel::x1w, bf, act, res) : instance(Kernel::x1n, bf, act, res, 3);
        t.guard = Guard::f32_512;
        return t;
    }
    if (!use_f16x3(d)) {
        t.inst = instance(Kernel::f32, d.HP, act, res);
        return t;
    }
    t.guard = m.host_check ? Guard::host : Guard::f32_cond;
    // Half-unit instance (16 coordinates per wave, twice the waves) for small batches: everything fits in one round even as
    // half-units, so the extra waves are free and the latency drops (a single tile: 76 -> 66 us).  Needs the unit count on the host
    // (no plan) and the depth-5 instance.
    const int64_t units = B * (((m.coords ? m.coords : d.P) + 31) / 32);
    t.half = !m.plan && d.L == 5 && d.half_allowed && units <= 2 * (int64_t)d.num_cus;
    if (m.trunk == 2 || (m.trunk == 0 && ws_capable(d, B) && m.alone() && !t.half)) {
        t.half = false;
        t.inst = instance(Kernel::f16x3w, act, 4);
        return t;
    }
    // R = 3 leaves ~35 KB of LDS per CU free, enough for an encoder / modulator workgroup of the NEXT call (other stream) to run
    // beside the persistent trunk workgroup; R = 4 fills the CU.  Depths other than 5 run the loop form of the kernel: with a ring of 3
    // hipcc gives it all 512 registers (and scratch), so nothing could run beside it anyway -- the ring of 4 has neither.  The ring of 4
    // fits the LDS up to L = 5 only, so depths 6..11 run the ring-of-3 loop form in every mode (L = 2..4: the ring of 4).
    const bool room = !m.alone() || m.trunk == 1;
    t.ring = (!room || d.L != 5) && d.f16_ring4_fits ? 4 : 3;
    t.inst = t.half ? instance(Kernel::f16x3h, act, t.ring, 5) : instance(Kernel::f16x3n, act, t.ring, d.L == 5 ? 5 : 0);
    return t;
}

// ---- per-patch coordinate sets, the *_native forms (msiren_sample_ragged_mods_native, msiren_resample_slices_native) --------------
// The handle's own trunk arithmetic where that is a split-fp16 trunk: siren_trunk_f16x3n_ragged_kernel<ACT,ring,lfix> (a list of its
// own: trunk_instances.h), the instance by depth as pick_trunk chooses the register-resident one for a call on its own -- L = 5: the
// straight-line form on the ring of 3; L = 2..4: the loop form on the ring of 4; L = 6..11: the loop form on the ring of 3.  Everything
// else (fp32 handles, the single-product 16-bit trunks at H = 512, MSIREN_PREC_F16 / BF16 at other widths, residual models, H or L
// outside the split-fp16 shape) is not native: those handles run the exact-fp32 ragged kernels and return their bits.
struct RaggedNativePick {
    bool native = false;
    int ring = 0, lfix = 0;
};
inline RaggedNativePick ragged_native_pick(const DispatchHandle& d) {
    RaggedNativePick r;
    if (d.x1_ready || !use_f16x3(d) || d.H != 256 || d.L < 2) return r;
    r.native = true;
    r.lfix = d.L == 5 ? 5 : 0;
    r.ring = d.L != 5 && d.f16_ring4_fits ? 4 : 3;
    return r;
}

// ---- prologue (tiles -> modulations) ------------------------------------------------------------------------------------------
// The split-fp16 one-launch prologue (handles with em_enc / em_mod; otherwise the exact-fp32 launches per layer).
struct ProloguePick {
    int inst = -1;      // row of kInstances: latent_mods<NPH,NPZ,DEPTH,MODE>
    int pf_blocks = 0;  // workgroups that only pull the weight stream into the L2s
};
// MODE 1 = tiles -> latent, 2 = latent -> modulations, 3 = both; nblk = row blocks of 16 patches
inline ProloguePick pick_prologue(const DispatchHandle& d, const CallMode& m, int mode, int64_t nblk) {
    ProloguePick p;
    const int nph = d.H == 256 ? 2 : 4, npz = d.H == 256 ? 2 : 1;
    // ring depth 4 (more weight fragments in flight per wave) where the workgroups have their CUs to themselves; depth 2 (<= 96
    // registers, 33 KB of LDS) where they run beside the register-resident trunk of the other stream or many to a CU.  Same bits.
    // (the halves alone -- model.encoder(tiles), model.modulator(z) -- have the ring of 4 only)
    const bool alone = m.alone() && !m.beside;
    int depth = 4;
    if (mode == 3) {
        depth = alone ? (nblk <= (int64_t)d.num_cus ? 8 : 4) : 2;
        if (d.em_depth) depth = d.em_depth;
        // (H = 512, config 5: 12.6 MB of weights per workgroup; nothing runs beside its trunk anyway: never below 4)
        depth = depth >= 8 ? 8 : (depth >= 4 || nph > 2) ? 4 : 2;
    }
    // latency sizes of the H = 256 model: 64 more workgroups (8 per XCD) that only pull the 2.9 MB weight stream into the L2s
    if (nph == 2 && alone && nblk <= 64 && mode == 3) p.pf_blocks = 64;
    p.inst = instance(Kernel::latent_mods, nph, npz, depth, mode);
    return p;
}

// One exact-fp32 Linear layer over a batch of B rows: the 32 x 32-tile kernel (throughput sizes: half the operand bytes per FLOP)
// rather than the 16 x 16 one (latency sizes).  Same arithmetic either way.  (1024 rows; a quarter of it for layers of >= 512
// outputs -- at 400 rows the 16 x 16 kernel launches 800 workgroups per 512-wide layer and takes 10.8 us, the tiled one is 1.7 % of a
// config-5 step faster; 256-wide layers: 2.7 % slower.  The tiled kernel addresses rows with 32-bit element offsets.)
constexpr int kLinearTileMin = 1024;
inline bool linear_tiled(int64_t B, int H, int Z, int Kh) {
    const int tile_min = H < 512 ? kLinearTileMin : kLinearTileMin / 4;
    const int64_t widest = H > Z ? (H > Kh ? H : Kh) : (Z > Kh ? Z : Kh);
    return B >= tile_min && (uint64_t)B * (uint64_t)widest < (1ULL << 32);
}

// The exact-fp32 per-layer launches (handles without the split-fp16 prologue: every fp32 handle, and 16-bit handles off the packed
// (H, Z) pairs).  The MFMA Linear kernels read 16-k blocks of whole 16-feature tiles: H and Z multiples of 16.  Other shapes run the
// VALU kernels: modulator_layer_kernel per Modulator layer; for the encoder the one fused per-tile encoder_kernel where Linear(64, Z)
// does not fit (Z % 16; conv3 == Linear(2048, 64) always fits), otherwise encoder_conv_kernel + two MFMA GEMMs.
inline bool modulator_mfma(int H, int Z) { return H % 16 == 0 && Z % 16 == 0; }
inline bool encoder_fused_valu(int Z) { return Z % 16 != 0; }

// LDS of one modulator_layer_kernel workgroup at its widest layer: the static partial sums (4 k-slices x MOD_ROWS x 64 features) plus
// the dynamic input rows (MOD_ROWS x K floats, K = H + Z behind layer 0, Z for a one-layer Modulator).  The launch is a plain one:
// at most 64 KB, which msiren_create checks (K <= 1792).
constexpr int kModRows = 8;  // encoder_modulator.hip.h: MOD_ROWS
constexpr int64_t kPlainLaunchLdsMax = 64 * 1024;
inline int64_t modulator_valu_lds_bytes(int H, int Z, int L) {
    const int64_t K = (int64_t)(L > 1 ? H : 0) + Z;
    return 4 * kModRows * 64 * 4 + kModRows * K * 4;
}
inline bool modulator_valu_fits(int H, int Z, int L) { return modulator_mfma(H, Z) || modulator_valu_lds_bytes(H, Z, L) <= kPlainLaunchLdsMax; }

// ---- call level --------------------------------------------------------------------------------------------------------------
// msiren_forward_tiles cuts itself into chunks over two streams (host_plan.h) from host_pipe_min tiles up
inline bool host_call_pipelines(const DispatchHandle& d, int64_t B) {
    return B >= d.host_pipe_min && use_f16x3(d) && !d.x1_ready && d.L == 5 && d.em_enc && d.em_mod && ws_capable(d, B);
}

// Slice pipeline: tiling + flags + plan as ONE launch, the pass counter's reset inside the fold -- for synchronous host calls that
// tile the images themselves.  The host enqueues into an idle stream there, so every launch saved is ~3 us (370 against 379 us per
// slice); back-to-back asynchronous calls run from a full queue and lose 0.6-1.5 % to the fused kernel's 400 device-wide fences, so
// they keep the separate kernels (profiles/r5/13_*).  Same bits either way.
inline bool fused_slice_tiling(const CallMode& m, bool from_images) { return m.sync && from_images; }

}  // namespace msiren
