// Every kernel instance libmsiren launches, one list per kernel translation unit (k_*.hip: make -j compiles them side by side).
// Plain preprocessor, no HIP: each k_*.hip expands its list into explicit instantiations (MSIREN_DEFINE_*), the host units into
// `extern template` declarations (MSIREN_EXTERN_*) and the table of kernel pointers (launch_dispatch.hip), dispatch.h into the table
// of instance names.  X(family, template arguments): the arguments are written without spaces, since they are part of the name
// (siren_trunk_<family>_kernel<arguments>: msiren_last_trunk_kernel, bench.py's roofline.kernel).
#pragma once

#define MSIREN_F32_INSTANCES(X)                                                   \
    X(f32, 128,0,0) X(f32, 128,0,1) X(f32, 128,1,0) X(f32, 128,1,1)               \
    X(f32, 256,0,0) X(f32, 256,0,1) X(f32, 256,1,0) X(f32, 256,1,1)               \
    X(f32, 384,0,0) X(f32, 384,0,1) X(f32, 384,1,0) X(f32, 384,1,1)               \
    X(f32, 512,0,0) X(f32, 512,0,1) X(f32, 512,1,0) X(f32, 512,1,1)               \
    X(f32, 256,0,0,1) /* stamped build: msiren_trunk_timeline */                  \
    X(f32_cond, 0) X(f32_cond, 1)
#define MSIREN_F16X3N_INSTANCES(X)                                                \
    X(f16x3n, 0,3,5) X(f16x3n, 0,3,0) X(f16x3n, 0,4,5) X(f16x3n, 0,4,0)           \
    X(f16x3n, 1,3,5) X(f16x3n, 1,3,0) X(f16x3n, 1,4,5) X(f16x3n, 1,4,0)           \
    X(f16x3n, 0,4,5,1) /* stamped build: msiren_f16x3_timeline */
#define MSIREN_F16X3H_INSTANCES(X) X(f16x3h, 0,3,5) X(f16x3h, 0,4,5) X(f16x3h, 1,3,5) X(f16x3h, 1,4,5)
#define MSIREN_F16X3W_INSTANCES(X) X(f16x3w, 0,4) X(f16x3w, 1,4) X(f16x3w, 0,4,1) /* stamped build: msiren_f16x3w_timeline */
#define MSIREN_X1N_INSTANCES(X)                                                   \
    X(x1n, 0,0,0,3) X(x1n, 0,0,1,3) X(x1n, 0,1,0,3) X(x1n, 0,1,1,3)               \
    X(x1n, 1,0,0,3) X(x1n, 1,0,1,3) X(x1n, 1,1,0,3) X(x1n, 1,1,1,3)
#define MSIREN_X1W_INSTANCES(X)                                                   \
    X(x1w, 0,0,0) X(x1w, 0,0,1) X(x1w, 0,1,0) X(x1w, 0,1,1)                       \
    X(x1w, 1,0,0) X(x1w, 1,0,1) X(x1w, 1,1,0) X(x1w, 1,1,1)
#define MSIREN_TRUNK_INSTANCES(X)                                                                                          \
    MSIREN_F32_INSTANCES(X) MSIREN_F16X3N_INSTANCES(X) MSIREN_F16X3H_INSTANCES(X) MSIREN_F16X3W_INSTANCES(X) \
    MSIREN_X1N_INSTANCES(X) MSIREN_X1W_INSTANCES(X)

// The exact-fp32 trunk with its spatial gradient (siren_trunk_f32_jet.hip.h; <HP,ACT>): a list of its own, like layer0_table_kernel it is
// no row of the dispatch table -- msiren_sample_grad_* / msiren_reconstruct_slices_grad launch it on every handle with H <= 256.
#define MSIREN_F32_JET_INSTANCES(X) X(f32_jet, 128,0) X(f32_jet, 128,1) X(f32_jet, 256,0) X(f32_jet, 256,1)

// The exact-fp32 trunks over one coordinate set per patch (siren_trunk_f32_ragged.hip.h; <HP,ACT,RES> and the jet's <HP,ACT>): lists of
// their own like the jet's -- msiren_sample_ragged_* / msiren_resample_slices* launch them on handles of every precision.
#define MSIREN_F32_RAGGED_INSTANCES(X)                                                            \
    X(f32_ragged, 128,0,0) X(f32_ragged, 128,0,1) X(f32_ragged, 128,1,0) X(f32_ragged, 128,1,1)   \
    X(f32_ragged, 256,0,0) X(f32_ragged, 256,0,1) X(f32_ragged, 256,1,0) X(f32_ragged, 256,1,1)   \
    X(f32_ragged, 384,0,0) X(f32_ragged, 384,0,1) X(f32_ragged, 384,1,0) X(f32_ragged, 384,1,1)   \
    X(f32_ragged, 512,0,0) X(f32_ragged, 512,0,1) X(f32_ragged, 512,1,0) X(f32_ragged, 512,1,1)
#define MSIREN_F32_JET_RAGGED_INSTANCES(X) X(f32_jet_ragged, 128,0) X(f32_jet_ragged, 128,1) X(f32_jet_ragged, 256,0) X(f32_jet_ragged, 256,1)

// The split-fp16 trunk over one coordinate set per patch (siren_trunk_f16x3n_ragged_kernel<ACT,R,LFIX>: siren_trunk_f16x3n_ragged.hip.h,
// layer 0 computed in the kernel), what the *_native ragged / resample calls run where ragged_native_pick (dispatch.h) says so: L = 5,
// L = 2..4 (ring of 4), L = 6..11 (ring of 3).  Behind each of its launches: the exact-fp32 ragged trunk as a conditional launch
// (siren_trunk_f32_ragged_cond_kernel<ACT>; H = 256, no residual).  Lists of their own as well.
#define MSIREN_F16X3N_RAGGED_INSTANCES(X)                                                         \
    X(f16x3n_ragged, 0,3,5) X(f16x3n_ragged, 0,4,0) X(f16x3n_ragged, 0,3,0)                       \
    X(f16x3n_ragged, 1,3,5) X(f16x3n_ragged, 1,4,0) X(f16x3n_ragged, 1,3,0)
#define MSIREN_F32_RAGGED_COND_INSTANCES(X) X(f32_ragged_cond, 0) X(f32_ragged_cond, 1)

// the one-launch prologue (<family>_f16x3_kernel: encoder_modulator_f16x3.hip.h); latent_mods<NPH,NPZ,DEPTH,MODE>
#define MSIREN_PROLOGUE_INSTANCES(X)                                                              \
    X(latent_mods, 2,2,2,3) X(latent_mods, 2,2,4,3) X(latent_mods, 2,2,8,3)                       \
    X(latent_mods, 2,2,4,1) X(latent_mods, 2,2,4,2)                                               \
    X(latent_mods, 4,1,4,3) X(latent_mods, 4,1,8,3) X(latent_mods, 4,1,4,1) X(latent_mods, 4,1,4,2) \
    X(encoder_conv, 1)

// HIP units only (inside namespace msiren, behind the kernel headers): the parameter list of each family
#define MSIREN_PARAMS_f32 (TrunkParams)
#define MSIREN_PARAMS_f32_cond (TrunkParams)
#define MSIREN_PARAMS_f32_jet (TrunkJetParams)
#define MSIREN_PARAMS_f32_ragged (TrunkRaggedParams)
#define MSIREN_PARAMS_f32_jet_ragged (TrunkRaggedParams)
#define MSIREN_PARAMS_f32_ragged_cond (TrunkRaggedParams)
#define MSIREN_PARAMS_f16x3n_ragged (TrunkF16RaggedParams)
#define MSIREN_PARAMS_f16x3n (TrunkF16Params)
#define MSIREN_PARAMS_f16x3h (TrunkF16Params)
#define MSIREN_PARAMS_f16x3w (TrunkWsParams)
#define MSIREN_PARAMS_x1n (TrunkX1Params)
#define MSIREN_PARAMS_x1w (TrunkX1Params)
#define MSIREN_PARAMS_latent_mods (EmTailParams)
#define MSIREN_PARAMS_encoder_conv (EncoderParams, const float*, em_u4*, float*)
#define MSIREN_DEFINE_TRUNK(fam, ...) template __global__ void siren_trunk_##fam##_kernel<__VA_ARGS__> MSIREN_PARAMS_##fam;
#define MSIREN_DEFINE_PROLOGUE(fam, ...) template __global__ void fam##_f16x3_kernel<__VA_ARGS__> MSIREN_PARAMS_##fam;
#define MSIREN_EXTERN_TRUNK(fam, ...) extern MSIREN_DEFINE_TRUNK(fam, __VA_ARGS__)
#define MSIREN_EXTERN_PROLOGUE(fam, ...) extern MSIREN_DEFINE_PROLOGUE(fam, __VA_ARGS__)
