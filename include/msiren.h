/*
 * msiren.h -- C ABI of libmsiren.so: the MI355X (gfx950) modulated-SIREN inference path.
 *
 * Drop-in boundary for ONE path of MatteoWohlrapp/mri-inr: the dense coordinate-grid forward of
 * `ModulatedSiren` (reference: src/networks/modulated_siren.py:435-457 and everything it calls).
 * The reference has no FFI of its own -- its boundary is the Python nn.Module protocol
 * (ctor kwargs / load_state_dict / __call__) -- so every entry point below names the reference
 * interface it stands in for.  The Python mirror of that protocol (mri_inr_amd/model.py) binds
 * these symbols with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; all tensors are dense row-major float32 unless stated otherwise;
 *   - every function returns 0 on success, a negative MSIREN_E_* code on failure, and leaves a
 *     human-readable message retrievable with msiren_last_error() (thread-local);
 *   - "host" pointers are ordinary process memory; "dev" pointers are HIP device memory on the
 *     handle's device (hipMalloc, msiren_dev_alloc or e.g. torch.Tensor.data_ptr());
 *   - *_dev entry points only enqueue work on the handle's stream: call msiren_sync() (or
 *     msiren_timer_stop()) before reading results;
 *   - one handle = one device + one stream + one weight set; handles are independent and may be
 *     used from different threads (a single handle is not re-entrant);
 *   - threads may hand their handles the same host arrays, or windows of one array that touch or overlap: inputs are only read, and
 *     the library never page-locks, registers or otherwise changes the state of a caller's memory (a range that the CALLER has
 *     page-locked only in part is copied through a bounce buffer: msiren_host_range_kind).  Two calls that WRITE overlapping output
 *     ranges race, as any two writers do.
 */
#ifndef MSIREN_H
#define MSIREN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 9: msiren_resample_volume* (a stack of slices read as a volume at points (Z, Y, X), value, native value and gradient forms) added.
 * Under the same number, as pure additions (no existing symbol or struct changed): msiren_align_slices(_dev) (slices scored under affine maps
 * against targets: cost, gradient, JtJ); msiren_align_solve(_dev) and msiren_align_solve_opts (the damped Gauss-Newton loop around it, on the device);
 * msiren_align_slices_w(_dev), msiren_align_solve_w(_dev) and msiren_align_solve_w_opts (the same two with a per-pixel weight and a per-slice gain and bias);
 * msiren_align_volume(_dev), msiren_align_volume_solve(_dev) and msiren_align_volume_solve_opts (target slices scored against, and aligned to, the stack
 * read as a volume under 3 x 3 maps); msiren_align_volume_w(_dev), msiren_align_volume_solve_w(_dev) and msiren_align_volume_solve_w_opts (the same two
 * with a per-pixel weight and a per-target gain and bias); msiren_align_volume_solve_group(_dev) and msiren_align_volume_solve_group_opts (groups of
 * consecutive targets aligned to the volume under one shared rigid motion per group); msiren_align_volume_r(_dev) and
 * msiren_align_volume_solve_group_r(_dev) (the weighted volume cost and the grouped solve under a Geman-McClure loss with one scale per target);
 * msiren_fuse_targets(_dev) and msiren_fuse_opts (aligned target slices gathered back onto the stack's voxel grid); msiren_project_volume(_dev) (the
 * way back: a stack gathered onto the targets' lattices with the same weights, with the residual against given targets and four sums per target);
 * msiren_solve_volume(_dev) and msiren_solve_opts (the stack that best explains all targets: regularised conjugate gradients on those two operators);
 * msiren_solve_volume_r(_dev) and msiren_solve_r_opts (rounds of that solve, reweighted by a Geman-McClure loss with one annealed scale per target);
 * msiren_align_stack_r(_dev) and msiren_align_stack_solve_group_r(_dev) (the robust volume cost and the grouped solve against a plain voxel stack read
 * trilinearly: no images, no trunk, no weights); msiren_residual_scale(_dev) and msiren_scale_opts (a robust scale per target or per group of targets
 * from an exact order statistic of the residuals, on the device: what every robust call takes as `scale`, without a host read);
 * msiren_leave_out_targets(_dev) (every target predicted from the fusion of the targets outside its own group: the left-out residual, in one call).
 * 8: msiren_sample_ragged_mods_native(_dev) and msiren_resample_slices_native(_dev) (per-patch coordinate sets and the reconstruction at
 * points in the handle's own trunk arithmetic) added.
 * 7: msiren_sample_ragged_* (one coordinate set per patch on the exact-fp32 trunks) and msiren_resample_slices* (the reconstruction at
 * arbitrary points) added.
 * 6: msiren_sample_grad_* and msiren_reconstruct_slices_grad(_dev) (the model's spatial gradient) added.
 * 5: msiren_encode_modulate_tiles(_dev) (the prologue of msiren_forward_tiles alone) and msiren_last_prologue_kernel added.
 * 4: msiren_sample_* (the trunk at caller-chosen coordinates), msiren_upsampled_geometry / _lattice and the *_scaled slice pipeline
 * (another output stride) added.  3 (round 6): msiren_runtime_info, msiren_host_range_kind added; the large-call split (MSIREN_SPLIT_MIN) and the per-call page-locking of
 * caller buffers (MSIREN_HOST_REGISTER) left the library.  2 (round 5): msiren_chain_* gone, msiren_profile_read_kernel /
 * msiren_last_trunk_kernel / msiren_device_pci added; sync no longer returns MSIREN_E_RANGE.  A library of another number refuses
 * msiren_create. */
#define MSIREN_ABI_VERSION 9

#if defined(__GNUC__)
#define MSIREN_API __attribute__((visibility("default")))
#else
#define MSIREN_API
#endif

enum {
    MSIREN_OK = 0,
    MSIREN_E_INVALID = -1,  /* bad argument / unsupported configuration (Python: ValueError)  */
    MSIREN_E_STATE = -2,    /* call order: weights missing or not committed (RuntimeError)    */
    MSIREN_E_SHAPE = -3,    /* tensor size does not match the configuration (load_state_dict) */
    MSIREN_E_HIP = -4,      /* HIP runtime error (message carries hipGetErrorString)          */
    MSIREN_E_NOMEM = -5,
    MSIREN_E_RANGE = -6     /* (rounds 2-3: an operand left the domain of the split-fp16 trunk.  Not returned since round 4:
                               such launches are re-run on the exact-fp32 trunk on the stream itself, "Domain guard" below) */
};

enum { MSIREN_ACT_SINE = 0, MSIREN_ACT_MORLET = 1 };

/* arithmetic of the hidden-layer contractions */
enum {
    MSIREN_PREC_F32 = 0,  /* v_mfma_f32_32x32x2_f32: exact fp32, the parity path (configs 1-4) */
    MSIREN_PREC_BF16 = 1, /* bf16 operands, fp32 accumulate: single-product trunk (weight-stationary from 3
                             layers on), dim_hidden = 512, 2 <= num_layers <= 11: the per-layer tables must
                             fit the 160 KB LDS (BASELINE config 5; own tolerance)                    */
    MSIREN_PREC_F16X3 = 2, /* split-fp16: 3 x v_mfma_f32_16x16x32_f16 per product, fp32 accumulate;
                             fp32-equivalent accuracy (22-bit operands); H = 256, 2 <= L <= 11 (the
                             per-layer tables must fit the 160 KB LDS beside the weight ring; depths
                             3..5 run the weight-stationary kernel on single-stream handles).
                             Other shapes silently use MSIREN_PREC_F32.  A launch that meets a modulation
                             outside what fp16 operands can carry is followed, on the same stream, by the
                             exact-fp32 trunk over the same batch (a conditional launch: "Domain guard"
                             below) -- the output is the reference's fp32 result either way. */
    MSIREN_PREC_F16 = 3   /* as BF16 with fp16 operands (11-bit significand).  fp16 ends at 65 504 where the
                             reference's fp32 does not: a launch that stores a non-finite output (an overflow
                             to inf is NaN one sine later) is followed, on the same stream, by the exact-fp32
                             trunk over the same batch as a conditional launch -- outside the fp16 domain the
                             output is the fp32 trunk's, bit for bit (round 5)                          */
};

/*
 * Mirrors the keyword arguments of ModulatedSiren.__init__ (src/networks/modulated_siren.py:349-368)
 * that influence the forward pass, i.e. the `model:` block of the YAML files
 * (configuration/train_modulated_siren.yaml:14-29).  `dropout`, `modulate`, `encoder_path`
 * have no effect on eval-mode maths and stay on the Python side.
 */
typedef struct msiren_config {
    int32_t abi_version;      /* MSIREN_ABI_VERSION                                             */
    int32_t dim_in;           /* must be 2 (the grid is a 2-D meshgrid, :427-433)               */
    int32_t dim_hidden;       /* H                                                              */
    int32_t dim_out;          /* must be 1 (squeeze(2)+rearrange at :451-455)                   */
    int32_t num_layers;       /* L: number of modulated sine layers before last_layer           */
    int32_t latent_dim;       /* Z; where dim_hidden or latent_dim is not a multiple of 16:
                                 (num_layers > 1 ? dim_hidden : 0) + latent_dim <= 1792 (the
                                 Modulator's input rows fit 64 KB of LDS), else MSIREN_E_INVALID */
    float w0;                 /* frequency of layers 1..L-1 and of last_layer (:196, :211-213)  */
    float w0_initial;         /* frequency of layer 0                                           */
    int32_t use_bias;
    int32_t activation;       /* MSIREN_ACT_*; last_layer is always sine (:120-123)             */
    int32_t outer_patch_size; /* O: encoder tile (32: FixedAutoencoder is hard-wired to it)     */
    int32_t inner_patch_size; /* I: tiling stride                                               */
    int32_t siren_patch_size; /* S: output tile, P = S*S coordinates per patch                  */
    int32_t residual;         /* 0 = reference semantics; 1 = build-defined skip    */
    int32_t precision;        /* MSIREN_PREC_*                                                  */
    int32_t device;           /* HIP device ordinal                                             */
    int32_t reserved[4];
} msiren_config;

typedef struct msiren_ctx* msiren_handle;

/* ---- lifecycle ------------------------------------------------------------------------------ */

/* ModulatedSiren(**kwargs) + .to(device): validates the configuration, selects the device,
 * creates the stream.  Reference: modulated_siren.py:349-433, test_mod_siren.py:96-120. */
MSIREN_API int msiren_create(const msiren_config* cfg, msiren_handle* out);
MSIREN_API int msiren_destroy(msiren_handle h);

/* Thread-local message of the last failing call on this thread ("" if none). */
MSIREN_API const char* msiren_last_error(void);

/* ---- weights: load_state_dict (test_mod_siren.py:116-118) ------------------------------------ */

/* One state_dict entry, by its reference key name, e.g.
 *   "net.layers.0.weight" (H,2) ... "net.layers.{l}.weight" (H,H), "net.layers.{l}.bias" (H),
 *   "net.last_layer.weight" (1,H), "net.last_layer.bias" (1), "grid" (P,2),
 *   "modulator.layers.{l}.0.weight" (H,Z) / (H,H+Z), "modulator.layers.{l}.0.bias" (H),
 *   "encoder.encoder.encoder.{0,2,4}.weight/.bias", "encoder.encoder.encoder.7.weight/.bias".
 * `n` is the element count and must match the shape implied by the configuration
 * (MSIREN_E_SHAPE otherwise, like load_state_dict's size-mismatch error); unknown names are
 * MSIREN_E_INVALID ("unexpected key").  Data is copied; the caller keeps ownership. */
MSIREN_API int msiren_set_tensor(msiren_handle h, const char* name, const float* host_data, size_t n);
/* state_dict()[name]: copies the tensor the handle holds (set by msiren_set_tensor, or received by
 * msiren_broadcast_weights) into host_out; n must be its element count.  MSIREN_E_STATE if absent. */
MSIREN_API int msiren_get_tensor(msiren_handle h, const char* name, float* host_out, size_t n);

/* Packs the tensors into the kernels' layouts and uploads them.  Fails with MSIREN_E_STATE and a
 * list of missing keys if the trunk ("net.*") is incomplete; modulator / encoder keys are only
 * required by msiren_forward_latent / msiren_forward_tiles. */
MSIREN_API int msiren_commit_weights(msiren_handle h);

/* The whole state_dict as ONE flat float32 image ("blob": mri_inr_amd/csrc/weights_blob.h) -- what
 * torch.save / torch.load of the state_dict is to the reference (test_mod_siren.py:116-118) and the exact
 * payload msiren_broadcast_weights sends: header (magic, version, key count, layout hash, payload size),
 * one presence flag per key of the configuration, then every tensor (absent ones as zeros).
 *   msiren_weights_blob_size   number of floats of this configuration's blob
 *   msiren_weights_export      the tensors the handle holds -> blob_host (n_floats must be the blob size)
 *   msiren_weights_import      blob -> the handle's tensors (replacing them; keys absent in the blob stay absent)
 *                              and commit, exactly what a receiving rank of msiren_broadcast_weights executes.
 * A blob of another configuration is MSIREN_E_SHAPE, a corrupt one MSIREN_E_INVALID; the handle keeps its tensors. */
MSIREN_API int msiren_weights_blob_size(msiren_handle h, size_t* n_floats);
MSIREN_API int msiren_weights_export(msiren_handle h, float* blob_host, size_t n_floats);
MSIREN_API int msiren_weights_import(msiren_handle h, const float* blob_host, size_t n_floats);

/* ---- forward ---------------------------------------------------------------------------------- */

/* SirenNet.forward over the fixed grid (modulated_siren.py:215-233 + :448-455):
 * mods (L,B,H) -- the tuple the Modulator returns, stacked -- -> out (B,S,S).  B may be 0. */
MSIREN_API int msiren_forward_mods(msiren_handle h, const float* mods_host, int64_t B, float* out_host);
MSIREN_API int msiren_forward_mods_dev(msiren_handle h, const float* mods_dev, int64_t B, float* out_dev);

/* Modulator.forward + SirenNet.forward (modulated_siren.py:325-343): latent (B,Z) -> out (B,S,S).
 * If mods_out is non-NULL the (L,B,H) modulations are returned as well. */
MSIREN_API int msiren_forward_latent(msiren_handle h, const float* z_host, int64_t B, float* out_host, float* mods_out_host);
MSIREN_API int msiren_forward_latent_dev(msiren_handle h, const float* z_dev, int64_t B, float* out_dev, float* mods_out_dev);

/* The two producers alone, as the reference exposes them as sub-modules: `model.encoder(tiles)` -> latent (B, Z)
 * (modulated_siren.py:420, 282-301; siren_encoder.py:565-577) and `model.modulator(z)` -> the L modulation vectors, stacked
 * (L, B, H) (modulated_siren.py:416, 325-343).  msiren_forward_tiles == trunk(modulate(encode(tiles))), bit for bit. */
MSIREN_API int msiren_encode_tiles(msiren_handle h, const float* tiles_host, int64_t B, float* latent_host);
MSIREN_API int msiren_encode_tiles_dev(msiren_handle h, const float* tiles_dev, int64_t B, float* latent_dev);
MSIREN_API int msiren_modulate(msiren_handle h, const float* latent_host, int64_t B, float* mods_host);
MSIREN_API int msiren_modulate_dev(msiren_handle h, const float* latent_dev, int64_t B, float* mods_dev);
/* The prologue of msiren_forward_tiles(_dev) and nothing else: tiles (B, O, O) -> modulations (L, B, H), by the very launches that call
 * makes in front of its trunk (on a 16-bit handle ONE latent_mods launch in which the latent never leaves the workgroup, with the ring
 * depth and the prefetch workgroups the call's mode -- streams, synchronous or not, batch size, the chunks of a large host call -- gives
 * it; on an fp32 handle the per-layer launches).  `latent` may be NULL; otherwise the latent (B, Z) is stored as well.
 * msiren_forward_mods of these modulations == msiren_forward_tiles, bit for bit. */
MSIREN_API int msiren_encode_modulate_tiles(msiren_handle h, const float* tiles_host, int64_t B, float* latent_host, float* mods_host);
MSIREN_API int msiren_encode_modulate_tiles_dev(msiren_handle h, const float* tiles_dev, int64_t B, float* latent_dev, float* mods_dev);
/* ModulatedSiren.forward (modulated_siren.py:435-457), custom-encoder branch
 * (siren_encoder.py:503-512,565-577): tiles (B,O,O) -> out (B,S,S). */
MSIREN_API int msiren_forward_tiles(msiren_handle h, const float* tiles_host, int64_t B, float* out_host);
MSIREN_API int msiren_forward_tiles_dev(msiren_handle h, const float* tiles_dev, int64_t B, float* out_dev);

/* The slice pipeline around the model call as metrics_error drives it (src/util/error.py:231-249):
 * image (Hh,Ww) -> image_to_patches(O,I) (tiling.py:10-64) -> black-patch filter (mean < 1e-10,
 * tiling.py:184-198,244-271) -> ModulatedSiren.forward on the non-black tiles -> zeros re-inserted
 * (tiling.py:274-303) -> weighted overlap-add (tiling.py:67-140) -> recon (nV*I, nH*I).
 * n_slices images of identical size are processed as one batch.  recon_rows/cols may be NULL.
 * The host-pointer form stores the reconstruction straight into recon_host where that is page-locked memory (see msiren_host_alloc below). */
MSIREN_API int msiren_reconstruct_slices_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height,
                                  int32_t width, float* recon_dev);
MSIREN_API int msiren_reconstruct_slices(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height,
                              int32_t width, float* recon_host);
/* The same chain from tiles that are already cut (what metrics_error receives, error.py:200-249):
 * tiles (n*nV*nH, O, O) -> black filter -> model -> zeros re-inserted -> weighted overlap-add -> (n, nV*I, nH*I). */
MSIREN_API int msiren_reconstruct_tiles_dev(msiren_handle h, const float* tiles_dev, int64_t n_slices, int32_t n_vertical,
                                 int32_t n_horizontal, float* recon_dev);
/* Output geometry of the above: nV = ceil(height/I), nH = ceil(width/I); recon is (nV*I, nH*I). */
MSIREN_API int msiren_recon_shape(msiren_handle h, int32_t height, int32_t width, int32_t* n_vertical, int32_t* n_horizontal);

/* Stand-alone tiling steps on device buffers (same references as above). */
MSIREN_API int msiren_image_to_patches_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height,
                                int32_t width, float* patches_dev /* (n*nV*nH, O, O) */);
MSIREN_API int msiren_weighted_fold_dev(msiren_handle h, const float* tiles_dev /* (n*nV*nH, S, S) */, int64_t n_slices,
                             int32_t n_vertical, int32_t n_horizontal, float* recon_dev);

/* patches_to_image (tiling.py:143-181): plain overlap average fold(tiles) / fold(ones) of O x O tiles at stride I,
 * padding (O-I)/2 -> (n, nV*I, nH*I).  metrics_error folds the fully-sampled and the undersampled tiles with it
 * to get the images it scores against (error.py:250-255). */
MSIREN_API int msiren_patches_to_image_dev(msiren_handle h, const float* tiles_dev /* (n*nV*nH, O, O) */, int64_t n_slices,
                                int32_t n_vertical, int32_t n_horizontal, float* image_dev);
/* The black-patch filter of the reference's callers as separate steps (src/util/tiling.py:184-198, 244-303; used one by one in
 * src/train/training.py:438-445 -- msiren_reconstruct_tiles_dev does all of them in one call).  All on the handle's current
 * stream; tiles / rows float32, flags / indices int32, everything device memory.
 *   msiren_black_patch_flags_dev  flags[t] = 1 where mean(tile t) < 1e-10 (classify_patches; a tile of 1e-12 is black), else 0
 *   msiren_gather_rows_dev        dst[j] = src[idx[j]], j < n_idx            (patches[non_black_indices])
 *   msiren_scatter_rows_dev       dst = zeros(n_rows); dst[idx[j]] = src[j]  (reintegrate_black_patches: black rows stay zeros) */
MSIREN_API int msiren_black_patch_flags_dev(msiren_handle h, const float* tiles_dev, int64_t n_tiles, int64_t tile_elems, int32_t* flags_dev);
MSIREN_API int msiren_gather_rows_dev(msiren_handle h, const float* src_dev, const int32_t* idx_dev, int64_t n_idx, int64_t row_elems, float* dst_dev);
MSIREN_API int msiren_scatter_rows_dev(msiren_handle h, const float* src_dev, const int32_t* idx_dev, int64_t n_idx, int64_t n_rows, int64_t row_elems,
                                       float* dst_dev);

/* ---- the representation off its own grid ------------------------------------------------------ */

/* SirenNet.forward(coords, mods) at coordinates the CALLER chooses (modulated_siren.py:215-233 takes any (..., 2) coordinates):
 * one set coords (Q, 2) float32 shared by all patches of the call -- column 0 the row coordinate, column 1 the column coordinate, as in
 * the "grid" buffer -- and out[b, q] = SirenNet(coords[q], mods[:, b]), out (B, Q).  1 <= Q <= 65 536 (MSIREN_E_INVALID beyond: the
 * layer-0 table of the call is 4 H bytes per coordinate); Q need not be a square; coordinates may lie outside [-1, 1]; a non-finite
 * coordinate gives non-finite outputs at that q only.  The 16-bit trunks read layer 0 from a table that is built on the device, on
 * the call's stream, in front of the trunk (sample_grid.hip.h); the fp32 trunk reads the coordinates themselves.  The _tiles forms
 * run encoder and Modulator first, as ModulatedSiren.forward does (modulated_siren.py:435-457).  The _dev forms enqueue on the stream
 * rotation like the forward calls; coords_dev is read on the stream, so the caller keeps it unchanged until msiren_sync.  The
 * host-pointer forms are synchronous one-chunk calls.  B = 0 does nothing. */
MSIREN_API int msiren_sample_mods(msiren_handle h, const float* coords_host, int64_t Q, const float* mods_host, int64_t B, float* out_host);
MSIREN_API int msiren_sample_mods_dev(msiren_handle h, const float* coords_dev, int64_t Q, const float* mods_dev, int64_t B, float* out_dev);
MSIREN_API int msiren_sample_tiles(msiren_handle h, const float* coords_host, int64_t Q, const float* tiles_host, int64_t B, float* out_host);
MSIREN_API int msiren_sample_tiles_dev(msiren_handle h, const float* coords_dev, int64_t Q, const float* tiles_dev, int64_t B, float* out_dev);

/* Build-defined (the reference has no such mode): the slice pipeline at another OUTPUT stride I' ("out_stride").
 * Tiling stays O / I -- the encoder sees the same tiles -- and every tile is evaluated on the S' x S' pixel centres of the same physical
 * tile, S' = S I'/I, then folded with kernel S', stride I', padding pad' = (S' - I')/2 and the reference's weight formula at size S'
 * (tiling.py:67-88).  S' and pad' must be integers and S' >= 2, MSIREN_E_INVALID otherwise.  With d = 2/(S-1), r = I'/I (fp64):
 *     lin'[j] = (-1 - d/2) + (d/r) (j + 1/2),  j = 0 .. S'-1,  rounded once to fp32;  coords[a S' + b] = (lin'[a], lin'[b]).
 * msiren_upsampled_geometry / _lattice need neither a handle nor a device. */
MSIREN_API int msiren_upsampled_geometry(int32_t S, int32_t I, int32_t out_stride, int32_t* out_tile, int32_t* pad);
MSIREN_API int msiren_upsampled_lattice(int32_t S, int32_t I, int32_t out_stride, float* lin_out /* out_tile floats */);
/* Build-defined: msiren_reconstruct_slices(_dev) / msiren_reconstruct_tiles_dev / msiren_weighted_fold_dev at output stride
 * out_stride: recon (n, nV*out_stride, nH*out_stride).  out_stride = inner_patch_size IS the existing entry point (the model's own
 * grid and committed table: the same bits).  The lattice's table and fold weights are built once per stream and stride and kept until
 * the next msiren_commit_weights.  n = 0 does nothing. */
MSIREN_API int msiren_reconstruct_slices_scaled(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                                int32_t out_stride, float* recon_host);
MSIREN_API int msiren_reconstruct_slices_scaled_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                                    int32_t out_stride, float* recon_dev);
MSIREN_API int msiren_reconstruct_tiles_scaled_dev(msiren_handle h, const float* tiles_dev, int64_t n_slices, int32_t n_vertical,
                                                   int32_t n_horizontal, int32_t out_stride, float* recon_dev);
MSIREN_API int msiren_weighted_fold_scaled_dev(msiren_handle h, const float* tiles_dev /* (n*nV*nH, S', S') */, int64_t n_slices,
                                               int32_t n_vertical, int32_t n_horizontal, int32_t out_stride, float* recon_dev);

/* The model's spatial gradient: what torch.autograd gives the reference for d SirenNet.forward / d coords
 * (modulated_siren.py:215-233 is differentiable in coords), here by a forward-mode pass through the same layers in one kernel
 * (siren_trunk_f32_jet.hip.h).  The arguments are msiren_sample_*'s and so are the coordinate rules: 1 <= Q <= 65 536, device
 * coordinates 8-byte aligned, any real coordinate accepted, a non-finite coordinate makes value and gradient non-finite at that q only,
 * B = 0 does nothing.  out (B, Q) may be NULL (the gradient alone); grad is PLANAR (2, B, Q): grad[0, b, q] = d out[b, q] / d coords[q, 0]
 * (the row coordinate), grad[1, b, q] = d out[b, q] / d coords[q, 1].
 * ALWAYS EXACT FP32, on handles of every precision: the call runs the fp32 jet trunk on the packed fp32 weights every handle holds; no
 * layer-0 table is built and there is no domain guard, since there is no fp16 operand.  The value returned is the bits of an fp32
 * handle's msiren_sample_* -- on a split-fp16 handle it is therefore the fp32 trunk's value, NOT the split-fp16 trunk's (the _tiles
 * forms still run the handle's own prologue in front).  dim_hidden > 256 (value and two tangents of a chunk no longer fit the LDS) or
 * residual = 1: MSIREN_E_INVALID.  msiren_last_trunk_kernel keeps naming the last trunk of the forward calls; under
 * msiren_profile_enable the launch is reported as "siren_trunk_f32_jet_kernel<HP,ACT>".
 * The _dev forms enqueue on the stream rotation like the forward calls; the host-pointer forms are synchronous one-chunk calls. */
MSIREN_API int msiren_sample_grad_mods(msiren_handle h, const float* coords_host, int64_t Q, const float* mods_host, int64_t B,
                                       float* out_host /* (B, Q) or NULL */, float* grad_host /* (2, B, Q) */);
MSIREN_API int msiren_sample_grad_mods_dev(msiren_handle h, const float* coords_dev, int64_t Q, const float* mods_dev, int64_t B,
                                           float* out_dev /* (B, Q) or NULL */, float* grad_dev /* (2, B, Q) */);
MSIREN_API int msiren_sample_grad_tiles(msiren_handle h, const float* coords_host, int64_t Q, const float* tiles_host, int64_t B,
                                        float* out_host /* (B, Q) or NULL */, float* grad_host /* (2, B, Q) */);
MSIREN_API int msiren_sample_grad_tiles_dev(msiren_handle h, const float* coords_dev, int64_t Q, const float* tiles_dev, int64_t B,
                                            float* out_dev /* (B, Q) or NULL */, float* grad_dev /* (2, B, Q) */);
/* Build-defined, like the other output strides: the slice pipeline with the gradient of every tile, tiling -> black flags -> plan ->
 * prologue -> jet trunk on the lattice of out_stride (out_stride = inner_patch_size: the model's own grid) -> the weighted fold, once
 * for recon (n, nV*out_stride, nH*out_stride; may be NULL) and once per plane of grad (2, n, nV*out_stride, nH*out_stride).  The tile
 * gradients are multiplied by float32(d / r), d = 2/(S-1), r = out_stride/inner_patch_size (fp64): grad is per OUTPUT PIXEL, plane 0
 * along the rows, plane 1 along the columns, the fold-weighted average of the covering tiles' analytic gradients (black tiles
 * contribute zeros with their weight).  recon is the exact-fp32 trunk's reconstruction at that stride. */
MSIREN_API int msiren_reconstruct_slices_grad(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                              int32_t out_stride, float* recon_host, float* grad_host);
MSIREN_API int msiren_reconstruct_slices_grad_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                                  int32_t out_stride, float* recon_dev, float* grad_dev);

/* One coordinate set PER PATCH ("ragged" sets): patch b is evaluated at coords[offsets[b] : offsets[b + 1]].
 * coords (T, 2) as msiren_sample_*'s (any real value; a non-finite coordinate spoils only its own output; device coordinates 8-byte
 * aligned), offsets (B + 1) int32, non-decreasing, offsets[0] = 0, offsets[B] = T; a patch may own no coordinate; T = 0 or B = 0 does
 * nothing.  mods (L, B, H); out (T): the patches' outputs one behind the other, as coords; grad PLANAR (2, T).  T and B below 2^30.
 * The host-pointer forms check the offsets (MSIREN_E_INVALID) and are synchronous one-chunk calls; the _dev forms read them on the
 * device only -- offsets outside [0, T] or decreasing are clamped there, never followed outside the call's buffers -- and enqueue on the
 * stream rotation.
 * ALWAYS EXACT FP32, on handles of every precision, as the gradient calls above and for the same reason (a layer-0 table per (patch,
 * coordinate) would be 4 H bytes an entry): out[offsets[b] + i] is the bits of an fp32 handle's msiren_sample_mods of patch b alone at
 * that coordinate, value and gradient of the _grad forms the bits of msiren_sample_grad_mods.  The value forms take what the fp32
 * trunk takes (dim_hidden <= 512, residual); the _grad forms what the gradient calls take (dim_hidden <= 256, no residual), out may be
 * NULL there.  Under msiren_profile_enable the launches are reported as "siren_trunk_f32_ragged_kernel<HP,ACT,RES>" /
 * "siren_trunk_f32_jet_ragged_kernel<HP,ACT>"; msiren_last_trunk_kernel keeps naming the last trunk of the forward calls. */
MSIREN_API int msiren_sample_ragged_mods(msiren_handle h, const float* coords_host /* (T, 2) */, const int32_t* offsets_host /* (B + 1) */,
                                         const float* mods_host, int64_t B, int64_t T, float* out_host /* (T) */);
MSIREN_API int msiren_sample_ragged_mods_dev(msiren_handle h, const float* coords_dev, const int32_t* offsets_dev, const float* mods_dev, int64_t B,
                                             int64_t T, float* out_dev);
/* NATIVE: the value forms above in the handle's OWN trunk arithmetic -- same arguments, same checks, same clamping of device offsets.
 * Where the handle's trunk is a split-fp16 one (MSIREN_PREC_F16X3, dim_hidden = 256, no residual, num_layers 2..11) the launch is
 * "siren_trunk_f16x3n_ragged_kernel<ACT,R,LFIX>": the register-resident split-fp16 trunk with layer 0 computed in the kernel (the exact
 * trunk's two fp32 FMAs and its sine) instead of read from a table, so an output is inside the project norm of the fp64 reference
 * (max <= 1e-4, rms <= 1e-5 of max|ref|) but NOT the exact forms' bits, nor msiren_sample_mods' (whose layer-0 table is built in fp64).
 * A coordinate's bits depend on the coordinate and its modulation rows only, not on its place in the set, the batch or the stream.
 * Domain guard: behind the launch, on the same stream, "siren_trunk_f32_ragged_cond_kernel<ACT>" re-evaluates the whole call in exact fp32
 * iff a scaled modulation row did not fit fp16 -- such a call returns the exact forms' bits, on the synchronous and the _dev form alike
 * (msiren_range_events counts it at the next synchronisation).  On every other handle (fp32, the 16-bit trunks at dim_hidden = 512,
 * MSIREN_PREC_F16 / BF16 elsewhere, residual) these ARE the exact forms: same launch, same bits.  msiren_profile_read_kernel names the
 * kernel that ran.  The gradient forms have no native counterpart. */
MSIREN_API int msiren_sample_ragged_mods_native(msiren_handle h, const float* coords_host, const int32_t* offsets_host, const float* mods_host, int64_t B,
                                                int64_t T, float* out_host);
MSIREN_API int msiren_sample_ragged_mods_native_dev(msiren_handle h, const float* coords_dev, const int32_t* offsets_dev, const float* mods_dev, int64_t B,
                                                    int64_t T, float* out_dev);
MSIREN_API int msiren_sample_ragged_grad_mods(msiren_handle h, const float* coords_host, const int32_t* offsets_host, const float* mods_host, int64_t B,
                                              int64_t T, float* out_host /* (T) or NULL */, float* grad_host /* (2, T) */);
MSIREN_API int msiren_sample_ragged_grad_mods_dev(msiren_handle h, const float* coords_dev, const int32_t* offsets_dev, const float* mods_dev, int64_t B,
                                                  int64_t T, float* out_dev /* (T) or NULL */, float* grad_dev /* (2, T) */);

/* Build-defined: the reconstruction of msiren_reconstruct_slices at arbitrary points, and its gradient.
 * points (M, 2) = (Y, X) in RECONSTRUCTION PIXEL coordinates -- integer (Y, X) is the centre of recon[Y, X] -- one set shared by the n
 * slices; out (n, M); grad PLANAR (2, n, M), per reconstruction pixel, plane 0 along the rows.
 * With pad = (S - I) / 2, tile (v, h) of a slice covers a point iff  v I - pad <= Y <= v I - pad + S - 1  and likewise for X (closed
 * ends; the fp32 coordinate is compared with the integers as it is).  For a covering tile, in fp64 and rounded once to fp32:
 *     ty = Y - (v I - pad),  local coordinate x = -1 + ty 2 / (S - 1),  w = exp(-0.1 sqrt((ty - c)^2 + (tx - c)^2)),  c = (S - 1) / 2
 *     out[s, m] = sum_k w_k val_k / sum_k w_k,   grad[., s, m] = (2 / (S - 1)) sum_k w_k g_k / sum_k w_k       (fp32)
 * over the (at most ceil(S / I)^2) covering tiles in (v, h) row-major order: val_k, g_k the exact-fp32 trunk's value and gradient of tile
 * k at the local coordinate, 0 for a black tile (which still counts with its weight).  At integer pixels this is the weighted fold of
 * msiren_reconstruct_slices (_grad) on an fp32 handle; between pixels the blend jumps where a tile's cover begins or ends, as the
 * fold's does from pixel to pixel.  The derivative of the weights is not part of grad.
 * A point no tile covers and a non-finite point give NaN at that m and touch nothing else; a point under black tiles only gives 0.
 * The pipeline, on the call's stream: tiling -> black flags -> plan -> the handle's own prologue (msiren_reconstruct_slices' steps) ->
 * the points binned by tile -> the ragged exact-fp32 trunk (ALWAYS exact fp32; the _grad forms take what the gradient calls take) ->
 * blend.  The order of the points does not influence any output bit.  8 M K and 12 n M K (K = ceil(S / I)^2) must stay below 2^31
 * (MSIREN_E_INVALID beyond); ceil(S / I) <= 4.  n = 0 or M = 0 does nothing.  Host-pointer forms: synchronous one-chunk calls. */
MSIREN_API int msiren_resample_slices(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                      const float* points_host, int64_t M, float* out_host);
MSIREN_API int msiren_resample_slices_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                          const float* points_dev, int64_t M, float* out_dev);
/* msiren_resample_slices(_dev) with the trunk step in the handle's own arithmetic (msiren_sample_ragged_mods_native above: kernel, domain
 * guard and fallback are the same); binning, weights and blend are unchanged, so val_k is the native trunk's value in the formula above. */
MSIREN_API int msiren_resample_slices_native(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                             const float* points_host, int64_t M, float* out_host);
MSIREN_API int msiren_resample_slices_native_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                                 const float* points_dev, int64_t M, float* out_dev);
MSIREN_API int msiren_resample_slices_grad(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                           const float* points_host, int64_t M, float* out_host /* or NULL */, float* grad_host);
MSIREN_API int msiren_resample_slices_grad_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                               const float* points_dev, int64_t M, float* out_dev /* or NULL */, float* grad_dev);

/* Build-defined: the n slices of a call read as a VOLUME, a stack along Z, at points (M, 3) = (Z, Y, X) float32.
 * (Y, X) are reconstruction pixel coordinates exactly as above; Z is in slice units, an integer Z being slice Z of the call.  out (M);
 * grad PLANAR (3, M): plane 0 per slice of Z, planes 1 and 2 per reconstruction pixel along rows and columns.
 * With R_s(Y, X), G_s(Y, X) what msiren_resample_slices / _grad define for slice s (same cover rule, local coordinate, weights and fp32
 * num / den over the covering tiles, a black tile 0 with its weight):
 *     valid iff 0 <= Z <= n - 1 (the fp32 Z against the integers; false for a NaN);  z0 = floorf(Z),  f = Z - z0 (exact),  a0 = 1.0f - f
 *     value forms:     out[m] = R_z0 if f == 0 (one slice; n = 1 is allowed), else fmaf(f, R_{z0+1}, a0 R_z0).  A slice of weight 0 is not
 *                      evaluated.
 *     gradient forms:  n >= 2 (MSIREN_E_INVALID otherwise), always two slices: z0' = min(z0, n - 2), f' = Z - z0' in [0, 1],
 *                      R0, R1, G0, G1 of slices z0', z0' + 1;  select(A0, A1) = A0 if f' == 0, A1 if f' == 1, else fmaf(f', A1, (1.0f - f') A0)
 *                      out[m] = select(R0, R1) -- the bits of the exact value form;  grad[0] = R1 - R0 (one fp32 subtraction: the slope of
 *                      the segment that contains Z, at an interior integer the one to its right);  grad[1], grad[2] = select over G0, G1.
 *                      The derivative of the fold weights is not part of grad.
 * An invalid Z, a non-finite (Y, X) and a point no tile covers give NaN at that m in every plane and touch nothing else.  At integer Z = s
 * value and in-plane gradient are the bits of msiren_resample_slices / _grad of slice s at (Y, X); a permutation of the points permutes
 * the outputs; the call on slices a .. b - 1 with Z - a gives the bits of the whole stack for points inside [a, b - 1] (grad[0] at
 * Z = b - 1 excepted: the whole stack's segment there is the next one).
 * The pipeline, on the call's stream: msiren_resample_slices' prologue -> the points binned by (slice, tile) -> the ragged trunk over those
 * n nV nH bins, at most 2 M K entries (K = ceil(S / I)^2), whatever n is -> blend.  The plain and _grad forms run the exact-fp32 trunks on
 * handles of every precision (the _grad forms take what the gradient calls take); the _native forms the handle's own trunk arithmetic as
 * msiren_sample_ragged_mods_native does: same kernel, domain guard and fallback.  32 M K + 8 M and 16 n nV nH must stay below 2^30
 * (MSIREN_E_INVALID beyond, naming the product); ceil(S / I) <= 4.  n = 0 or M = 0 does nothing.  Host-pointer forms: synchronous one-chunk
 * calls; the _dev forms enqueue on the stream rotation.  Under msiren_profile_enable: "resample_volume_bin_kernels", the ragged trunk under
 * its name, "resample_volume_blend_kernel". */
MSIREN_API int msiren_resample_volume(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                      const float* points_host /* (M, 3) */, int64_t M, float* out_host /* (M) */);
MSIREN_API int msiren_resample_volume_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                          const float* points_dev, int64_t M, float* out_dev);
MSIREN_API int msiren_resample_volume_native(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                             const float* points_host, int64_t M, float* out_host);
MSIREN_API int msiren_resample_volume_native_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                                 const float* points_dev, int64_t M, float* out_dev);
MSIREN_API int msiren_resample_volume_grad(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                           const float* points_host, int64_t M, float* out_host /* (M) or NULL */, float* grad_host /* (3, M) */);
MSIREN_API int msiren_resample_volume_grad_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                               const float* points_dev, int64_t M, float* out_dev /* (M) or NULL */, float* grad_dev /* (3, M) */);

/* Build-defined: the n slices of a call scored against n targets under one 2 x 3 affine map each -- per slice the
 * sum of squared differences, its gradient over the six map parameters and the Gauss-Newton matrix JtJ, all summed on the device.
 *     images (n, height, width) float32;  targets (n, th, tw) float32;  maps (n, 6) float32 = (a00, a01, t0, a10, a11, t1)
 * Target pixel (i, j) of slice s, 0 <= i < th, 0 <= j < tw, is read at
 *     Y = ((a00 i) + (a01 j)) + t0        X = ((a10 i) + (a11 j)) + t1
 * in fp32, i and j converted exactly, every operation rounded on its own (NO fused multiply-add: float32 arithmetic in numpy gives the same
 * bits).  (Y, X) are reconstruction pixel coordinates exactly as in msiren_resample_slices.  R, gY, gX are THE BITS of
 * msiren_resample_slices_grad of slice s at that point (value, plane 0, plane 1): the same cover rule, fp64-then-rounded local coordinate
 * and weight, fp32 num / den over the covering tiles in (v, h) order, a black tile 0 with its weight; the derivative of the fold weights is
 * not included.  The trunk is always the exact-fp32 jet ragged trunk, on handles of every precision; the model limits are the gradient
 * calls' (dim_hidden <= 256, no residual: MSIREN_E_INVALID otherwise, nothing launched).
 * A pixel is VALID iff targets[s, i, j], R, gY and gX are all finite: a point under black tiles only is valid (R = 0); an uncovered or
 * non-finite point and a NaN target (a cheap mask) are not.  An invalid pixel contributes to nothing and touches nothing else.  Per valid
 * pixel, in fp64 from the fp32 numbers, no fused multiply-add:
 *     r = (double)R - (double)T        J = (gY i, gY j, gY, gX i, gX j, gX)       (parameter order a00, a01, t0, a10, a11, t1)
 *     count += 1;  cost += r r;  dcost[a] += (2 r) J[a];  jtj[a, b] += J[a] J[b]  for a <= b
 * sums (n, 29) float64 = [count, cost, dcost[0..5], jtj: the upper triangle packed row-major (21)].
 * warped (n, th, tw) = R and wgrad (2, n, th, tw) = gY, gX are optional (NULL: not written); at invalid pixels they carry what
 * msiren_resample_slices_grad gives (NaN where no tile covers the point).
 * Every sum has one order: pixel p = i tw + j; chunks of 1024 consecutive pixels of a slice; inside a chunk thread t of 256 adds
 * p = lo + t, lo + t + 256, ... in that order; the 256 totals are combined by a butterfly inside each wave of 64 (xor 32, 16, .. 1), then the
 * four waves in order; a slice's chunks in index order.  So sums are the same bits run to run, a slice alone gives its row of any batch, and
 * passing or omitting warped / wgrad changes no bit.
 * The pipeline, on the call's stream: msiren_resample_slices' prologue -> the pixels binned by (slice, tile) -> the jet ragged trunk over
 * those n nV nH bins, at most T = n th tw K entries (K = ceil(S / I)^2) -> per chunk blend and partial sums -> per slice the total.  20 T and
 * 16 n nV nH must stay below 2^30 (MSIREN_E_INVALID beyond, naming the product); ceil(S / I) <= 4.  n = 0 or th tw = 0 does nothing.  The
 * host-pointer form is a synchronous one-chunk call; the _dev form enqueues on the stream rotation.  Under msiren_profile_enable:
 * "align_bin_kernels", the jet ragged trunk under its name, "align_reduce_kernels". */
MSIREN_API int msiren_align_slices(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                   const float* targets_host, int32_t th, int32_t tw, const float* maps_host /* (n, 6) */,
                                   double* sums_host /* (n, 29) */, float* warped_host /* or NULL */, float* wgrad_host /* or NULL */);
MSIREN_API int msiren_align_slices_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                       const float* targets_dev, int32_t th, int32_t tw, const float* maps_dev /* (n, 6) */,
                                       double* sums_dev /* (n, 29) */, float* warped_dev /* or NULL */, float* wgrad_dev /* or NULL */);

/* Build-defined: slices aligned to their targets on the device -- msiren_align_slices' prologue once, then
 * `iterations` x (its evaluation at the trial maps -> one step kernel), all on the call's stream, no host synchronisation in between.
 * Levenberg-Marquardt with per-slice accept / reject over the six affine parameters (mode 0) or over rotation and in-plane shift about
 * (centre_y, centre_x) (mode 1).  After evaluation k = 0 .. iterations - 1 with sums (count, cost, g[6], H[6][6]) at the trial map:
 *     mean = cost / count if count >= 6 else +inf
 *     k == 0:            accept (best := trial, sums_best := sums, mean_best = mean_first = mean); lam unchanged
 *     mean < mean_best:  accept; accepted += 1; lam = max(lam down, lam_min)
 *     otherwise:         reject (a NaN mean included); lam = min(lam up, lam_max)
 *     then propose from best (also behind the last evaluation), with g, H of sums_best:
 *     affine  A = H, A[a][a] = H[a][a] + lam H[a][a];  d = ldl_solve(A, -g / 2);  trial[a] = (float)((double)best[a] + d[a])
 *     rigid   state (c, s, uY, uX):  B (6 x 3) = d map / d (angle, uY, uX),  g3 = B^T g,  H3 = B^T (H B),  A = H3 damped as above,
 *             d = ldl_solve(A, -g3 / 2);  u = d[0] / 2, cd = (1 - u u) / (1 + u u), sd = 2 u / (1 + u u) (Cayley: an exact rotation);
 *             c' = c cd - s sd, s' = s cd + c sd, uY' = uY + d[1], uX' = uX + d[2];
 *             trial = (float)(c', -s', cy - (c' cy - s' cx) + uY', s', c', cx - (s' cy + c' cx) + uX')
 * ldl_solve: A = L D L^T without pivoting; a pivot that is not positive and finite gives a zero step (flag SINGULAR).  fp64 + - * / one
 * at a time, no fused multiply-add, every sum in one order: mri_inr_amd/align.py: lm_step restates it in Python floats and gives the
 * same bits, so the call equals the same loop on the host around msiren_align_slices bit for bit (DESIGN.md section 5.11 has every order).
 * Affine mode reads maps_in (n, 6); rigid mode reads rigid_in (n, 4) = (cos, sin, uY, uX) and forms the first map from it.
 * maps_out (n, 6): the best map.  rigid_out (n, 4) or NULL: the best rigid state (zeros in affine mode).
 * report (n, 6) float64: accepted, mean_first, mean_best, count at the best map, lam, flags (bit 0 SINGULAR: the last proposal was zero;
 * bit 1 NO_OVERLAP: mean_first is +inf).  trace (iterations, n, 8) float64 or NULL: per evaluation the trial map as six doubles, cost, count.
 * A slice with fewer than six valid pixels at every evaluation, and a black slice (H = 0: SINGULAR), keep their input map.  Every slice's
 * trajectory depends on that slice only: the same bits alone or in any batch, with or without trace.
 * MSIREN_E_INVALID with a message, before any launch: what msiren_align_slices refuses; struct_size != sizeof(msiren_align_solve_opts);
 * mode not 0 or 1; iterations outside 1 .. 256; anything outside 0 < lam_min <= damping <= lam_max < inf, 0 < down <= 1, 1 <= up < inf; a
 * non-finite centre in rigid mode; a missing input of the mode, a null maps_out or report; device pointers not aligned to 4 (floats) / 8
 * (doubles) bytes.  n = 0 or th tw = 0 does nothing.  The host-pointer form is one synchronous call: images and targets go up once.
 * Under msiren_profile_enable: the prologue's entries once per call; "align_bin_kernels", the jet ragged trunk, "align_reduce_kernels" and
 * "align_step_kernel" `iterations` times. */
typedef struct {
    uint32_t struct_size;     /* sizeof(msiren_align_solve_opts) */
    int32_t mode;             /* 0 affine, 1 rigid */
    int32_t iterations;       /* evaluations, 1 .. 256 */
    int32_t reserved;
    double damping, down, up, lam_min, lam_max, centre_y, centre_x;
} msiren_align_solve_opts;
MSIREN_API int msiren_align_solve(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                  const float* targets_host, int32_t th, int32_t tw, const msiren_align_solve_opts* opts,
                                  const float* maps_in /* (n, 6), affine */, const double* rigid_in /* (n, 4), rigid */,
                                  float* maps_out /* (n, 6) */, double* rigid_out /* (n, 4) or NULL */, double* report /* (n, 6) */,
                                  double* trace /* (iterations, n, 8) or NULL */);
MSIREN_API int msiren_align_solve_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                      const float* targets_dev, int32_t th, int32_t tw, const msiren_align_solve_opts* opts,
                                      const float* maps_in_dev /* (n, 6), affine */, const double* rigid_in_dev /* (n, 4), rigid */,
                                      float* maps_out_dev /* (n, 6) */, double* rigid_out_dev /* (n, 4) or NULL */,
                                      double* report_dev /* (n, 6) */, double* trace_dev /* (iterations, n, 8) or NULL */);

/* Build-defined: msiren_align_slices with a per-pixel weight and a per-slice gain and bias.  Everything of
 * msiren_align_slices is unchanged (images, targets, maps, the point rule, R, gY, gX the bits of msiren_resample_slices_grad, the pipeline, the
 * limits); two inputs are added:
 *     weights (n, th, tw) float32 or NULL (every weight 1);   intensity (n, 2) float32 = (g, b) per slice or NULL ((1, 0))
 * A pixel is VALID iff msiren_align_slices' condition holds (target, R, gY, gX all finite) and its weight w is finite and w > 0: a zero,
 * negative, NaN or infinite weight masks the pixel.  An invalid pixel contributes to nothing.  Per valid pixel, in fp64 from the fp32 numbers, no
 * fused multiply-add, each operation rounded on its own, in exactly this association:
 *     m  = ((double)g (double)R) + (double)b          r = m - (double)T
 *     gy = (double)g (double)gY                       gx = (double)g (double)gX
 *     J  = (gy i, gy j, gy, gx i, gx j, gx, (double)R, 1.0)         (parameter order a00, a01, t0, a10, a11, t1, g, b)
 *     wr = w r
 *     count += 1;  wsum += w;  cost += wr r;  dcost[a] += (2 wr) J[a];  jtj[a, b] += (w J[a]) J[b]  for a <= b
 * sums (n, 47) float64 = [count, wsum, cost, dcost[0..7], jtj: the upper triangle of the 8 x 8 matrix packed row-major (36)].
 * warped / wgrad are what msiren_align_slices writes: R, gY, gX BEFORE gain and bias, the bits of msiren_resample_slices_grad.
 * Every sum has msiren_align_slices' one order (chunks of 1024 pixels, thread t adds lo + t, lo + t + 256, ..., the butterfly inside each wave,
 * the four waves in order, the chunks in index order; no floating-point atomics).  So, bit for bit: with g = 1, b = 0, w = 1 every shared
 * entry (count, cost, dcost[0..5], the leading 6 x 6 block of jtj) is msiren_align_slices' and wsum == count; weights in {0, 1} give what
 * msiren_align_slices gives on targets with NaN where the weight is 0; a weight that is a power of two scales wsum, cost, dcost and jtj
 * exactly.  MSIREN_E_INVALID before any launch: what msiren_align_slices refuses (the partial records are 376 bytes per chunk in the
 * 2^30 limit); device weights or intensity not 4-byte aligned.  Under msiren_profile_enable: "align_bin_kernels", the jet ragged trunk,
 * "align_reduce_w_kernels". */
MSIREN_API int msiren_align_slices_w(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                     const float* targets_host, int32_t th, int32_t tw, const float* maps_host /* (n, 6) */,
                                     const float* weights_host /* (n, th, tw) or NULL */, const float* intensity_host /* (n, 2) or NULL */,
                                     double* sums_host /* (n, 47) */, float* warped_host /* or NULL */, float* wgrad_host /* or NULL */);
MSIREN_API int msiren_align_slices_w_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                         const float* targets_dev, int32_t th, int32_t tw, const float* maps_dev /* (n, 6) */,
                                         const float* weights_dev /* (n, th, tw) or NULL */, const float* intensity_dev /* (n, 2) or NULL */,
                                         double* sums_dev /* (n, 47) */, float* warped_dev /* or NULL */, float* wgrad_dev /* or NULL */);

/* Build-defined: msiren_align_solve's loop around msiren_align_slices_w -- the prologue once, then `iterations` x
 * (bin -> jet ragged trunk -> the 47-sum reduce -> one step kernel), no host synchronisation.  intensity_mode 0 (fixed): (g, b) stay at their
 * inputs and the solve is over 6 parameters (affine) or 3 (rigid); 1 (estimate): (g, b) are solved for with the map, over 8 (affine) or 5
 * (rigid).  With P the number of solved parameters and sums (count, wsum, cost, g[8], H[8][8]) at the trial (map, g, b):
 *     mean = cost / wsum if count >= P else +inf;       accept / reject, lam and the flags: msiren_align_solve's
 *     affine, fixed     msiren_align_solve's 6 x 6 system on the leading block of g, H
 *     affine, estimate  the same expressions with 8 in place of 6;  trial[a] = (float)((double)best[a] + d[a]) for a < 6,
 *                       g' = (float)((double)g_best + d[6]),  b' = (float)((double)b_best + d[7])
 *     rigid, fixed      msiren_align_solve's 3 x 3 system on the leading 6 x 6 block
 *     rigid, estimate   B (8 x 5): msiren_align_solve's 6 x 3 block, then B[6][3] = B[7][4] = 1, every other entry 0;  g5 = B^T g,
 *                       H5 = B^T (H B), every sum ascending from 0.0, zero entries included;  the Cayley update on d[0..2];
 *                       g' = (float)((double)g_best + d[3]),  b' = (float)((double)b_best + d[4])
 * fp64 + - * / one at a time; mri_inr_amd/align.py: lm_step_w restates it in Python floats and gives the same bits.  With unit weights
 * wsum == count, so with intensity_mode 0, no weights and no intensity the call returns msiren_align_solve's maps, report and trace columns.
 * weights (n, th, tw) or NULL; intensity_in (n, 2) or NULL ((1, 0)).  maps_out (n, 6), intensity_out (n, 2): the best map and (g, b);
 * rigid_out (n, 4) or NULL.  report (n, 7) float64: accepted, mean_first, mean_best, count at the best map, wsum at the best map, lam, flags.
 * trace (iterations, n, 11) float64 or NULL: per evaluation the trial map (6), the trial g, b, then cost, count, wsum.
 * A black slice (R = 0 everywhere: SINGULAR) and a slice whose weights mask every pixel (NO_OVERLAP) keep their inputs.
 * MSIREN_E_INVALID with a message, before any launch: everything msiren_align_solve refuses; struct_size != sizeof(msiren_align_solve_w_opts);
 * intensity_mode not 0 or 1; a null intensity_out or report; device weights or intensities not 4-byte aligned.
 * Under msiren_profile_enable: the prologue's entries once per call; "align_bin_kernels", the jet ragged trunk, "align_reduce_w_kernels" and
 * "align_step_w_kernel" `iterations` times. */
typedef struct {
    uint32_t struct_size;     /* sizeof(msiren_align_solve_w_opts) */
    int32_t mode;             /* 0 affine, 1 rigid */
    int32_t iterations;       /* evaluations, 1 .. 256 */
    int32_t intensity_mode;   /* 0 fixed, 1 estimate */
    double damping, down, up, lam_min, lam_max, centre_y, centre_x;
} msiren_align_solve_w_opts;
MSIREN_API int msiren_align_solve_w(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                    const float* targets_host, int32_t th, int32_t tw, const msiren_align_solve_w_opts* opts,
                                    const float* maps_in /* (n, 6), affine */, const double* rigid_in /* (n, 4), rigid */,
                                    const float* weights /* (n, th, tw) or NULL */, const float* intensity_in /* (n, 2) or NULL */,
                                    float* maps_out /* (n, 6) */, float* intensity_out /* (n, 2) */, double* rigid_out /* (n, 4) or NULL */,
                                    double* report /* (n, 7) */, double* trace /* (iterations, n, 11) or NULL */);
MSIREN_API int msiren_align_solve_w_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                        const float* targets_dev, int32_t th, int32_t tw, const msiren_align_solve_w_opts* opts,
                                        const float* maps_in_dev /* (n, 6), affine */, const double* rigid_in_dev /* (n, 4), rigid */,
                                        const float* weights_dev /* (n, th, tw) or NULL */, const float* intensity_in_dev /* (n, 2) or NULL */,
                                        float* maps_out_dev /* (n, 6) */, float* intensity_out_dev /* (n, 2) */,
                                        double* rigid_out_dev /* (n, 4) or NULL */, double* report_dev /* (n, 7) */,
                                        double* trace_dev /* (iterations, n, 11) or NULL */);

/* Build-defined: m target slices scored against the stack of n slices READ AS A VOLUME (msiren_resample_volume_grad), each
 * under its own 3 x 3 map -- per target the sum of squared differences, its gradient over the nine map parameters and the Gauss-Newton matrix JtJ.
 *     images (n, height, width) float32, n >= 2;  targets (m, th, tw) float32, m independent of n;
 *     maps (m, 9) float32 = (z0, z1, tz, y0, y1, ty, x0, x1, tx)
 * Pixel (i, j) of target q is read at
 *     Z = ((z0 i) + (z1 j)) + tz      Y = ((y0 i) + (y1 j)) + ty      X = ((x0 i) + (x1 j)) + tx
 * in fp32, i and j converted exactly, every operation rounded on its own (NO fused multiply-add: float32 arithmetic in numpy gives the same bits).
 * Z is in slice units, (Y, X) in reconstruction pixel coordinates.  R, gZ, gY, gX are THE BITS of msiren_resample_volume_grad at (Z, Y, X)
 * (value, planes 0, 1, 2): the pair z0' = min(floor Z, n - 2) with f' = Z - z0', the selection R0 / R1 / fma(f', R1, (1 - f') R0), gZ = R1 - R0,
 * NaN in every plane for a Z outside 0 .. n - 1 or where no tile covers (Y, X), a black tile 0 with its weight, no derivative of the fold weights.
 * A pixel is VALID iff targets[q, i, j], R, gZ, gY and gX are all finite.  Per valid pixel, in fp64 from the fp32 numbers, no fused multiply-add:
 *     r = (double)R - (double)T        J = (gZ i, gZ j, gZ, gY i, gY j, gY, gX i, gX j, gX)       (parameter order: the map's)
 *     count += 1;  cost += r r;  dcost[a] += (2 r) J[a];  jtj[a, b] += J[a] J[b]  for a <= b
 * sums (m, 56) float64 = [count, cost, dcost[0..8], jtj: the upper triangle packed row-major (45)].
 * warped (m, th, tw) = R and wgrad (3, m, th, tw) = gZ, gY, gX are optional (NULL: not written); at invalid pixels they carry what
 * msiren_resample_volume_grad gives.  Every sum has msiren_align_slices' one order (chunks of 1024 consecutive pixels of a target; thread t of 256
 * adds p = lo + t, lo + t + 256, ...; the butterfly inside each wave, the four waves in order; the chunks in index order; no floating-point
 * atomics): the same bits run to run, a target alone gives its row of any batch, passing or omitting warped / wgrad changes no bit.  With
 * m = n and the Z row (0, 0, s) the entries count, cost, dcost[3..8] and the in-plane 6 x 6 block of jtj are msiren_align_slices' of slice s.
 * The pipeline, on the call's stream: msiren_resample_volume's prologue -> the pixels binned by (slice, tile), two slices each -> the jet ragged
 * trunk over those n nV nH bins, at most T = 2 m th tw K entries -> per chunk blend and partial sums -> per target the total.  MSIREN_E_INVALID
 * before any launch, naming the product: n < 2; 32 M K + 8 M (M = m th tw) with 448 bytes per chunk, or 16 n nV nH, not below 2^30; M not below
 * 2^28; the gradient calls' model limits; a null argument.  m = 0 or th tw = 0 does nothing.  The host-pointer form is a synchronous one-chunk
 * call; the _dev form enqueues on the stream rotation.  Under msiren_profile_enable: "align_volume_bin_kernels", the jet ragged trunk under its
 * name, "align_volume_reduce_kernels". */
MSIREN_API int msiren_align_volume(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                   const float* targets_host, int64_t m_targets, int32_t th, int32_t tw, const float* maps_host /* (m, 9) */,
                                   double* sums_host /* (m, 56) */, float* warped_host /* or NULL */, float* wgrad_host /* (3, m, th, tw) or NULL */);
MSIREN_API int msiren_align_volume_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                       const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw, const float* maps_dev /* (m, 9) */,
                                       double* sums_dev /* (m, 56) */, float* warped_dev /* or NULL */, float* wgrad_dev /* or NULL */);

/* Build-defined: targets aligned to the volume on the device -- msiren_align_solve's loop around msiren_align_volume: the
 * prologue once, then `iterations` x (bin -> jet ragged trunk -> the 56-sum reduce -> one step kernel), no host synchronisation.  Accept / reject,
 * lam and the flags are msiren_align_solve's;  mean = cost / count if count >= P else +inf.
 *     mode 0, affine, P = 9   msiren_align_solve's expressions with 9 in place of 6
 *     mode 1, rigid,  P = 6   a rigid motion of the target's nominal plane in physical space, slices `spacing` pixels apart.  planes (m, 12)
 *             float64 = (e_i, e_j, o, c): the lattice's two step vectors, its origin and the rotation centre, triples in (Z, Y, X) order in
 *             pixel units.  State (Rot (9, row-major), u (3)) float64.  With v_i = Rot e_i, v_j = Rot e_j, v_o = Rot (o - c), t = (v_o + c) + u,
 *             row r of the map is (float)(v_i[r], v_j[r], t[r]), the Z row (r = 0) divided by spacing before rounding.
 *             B (9 x 6) over (w0, w1, w2, u0, u1, u2): B[3 r + col][k] = (e_k x v_col)[r] (v_col = v_i, v_j, v_o), B[3 r + 2][3 + k] = [r == k], the
 *             rows r = 0 divided by spacing;  g6 = B^T g, H6 = B^T (H B), every sum ascending from 0.0, zero entries included;  d = ldl_solve(H6
 *             damped, -g6 / 2);  a = d[0..2] / 2, Cay = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a) (an exact rotation, no trigonometry),
 *             Rot' = Cay Rot, u' = u + d[3..5].
 * fp64 + - * / one at a time, no fused multiply-add; DESIGN.md section 5.13 fixes every association and mri_inr_amd/align_volume.py: lm_step_v restates
 * it in Python floats with the same bits, so the call equals the same loop on the host around msiren_align_volume bit for bit.
 * Affine mode reads maps_in (m, 9); rigid mode reads planes (m, 12) and rigid_in (m, 12).  maps_out (m, 9): the best map.  rigid_out (m, 12) or
 * NULL: the best rigid state (zeros in affine mode).  report (m, 6) float64: msiren_align_solve's (accepted, mean_first, mean_best, count at the
 * best map, lam, flags).  trace (iterations, m, 11) float64 or NULL: per evaluation the trial map as nine doubles, cost, count.
 * MSIREN_E_INVALID with a message, before any launch: what msiren_align_volume refuses; struct_size != sizeof(msiren_align_volume_solve_opts); mode
 * not 0 or 1; iterations outside 1 .. 256; anything outside 0 < lam_min <= damping <= lam_max < inf, 0 < down <= 1, 1 <= up < inf; in rigid mode
 * a spacing that is not finite and > 0; a missing input of the mode, a null maps_out or report; device pointers not aligned to 4 (floats) / 8
 * (doubles) bytes.  Under msiren_profile_enable: the prologue's entries once per call; "align_volume_bin_kernels", the jet ragged trunk,
 * "align_volume_reduce_kernels" and "align_volume_step_kernel" `iterations` times. */
typedef struct {
    uint32_t struct_size;     /* sizeof(msiren_align_volume_solve_opts) */
    int32_t mode;             /* 0 affine, 1 rigid */
    int32_t iterations;       /* evaluations, 1 .. 256 */
    int32_t reserved;
    double damping, down, up, lam_min, lam_max, spacing;
} msiren_align_volume_solve_opts;
MSIREN_API int msiren_align_volume_solve(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                         const float* targets_host, int64_t m_targets, int32_t th, int32_t tw,
                                         const msiren_align_volume_solve_opts* opts, const float* maps_in /* (m, 9), affine */,
                                         const double* planes /* (m, 12), rigid */, const double* rigid_in /* (m, 12), rigid */,
                                         float* maps_out /* (m, 9) */, double* rigid_out /* (m, 12) or NULL */, double* report /* (m, 6) */,
                                         double* trace /* (iterations, m, 11) or NULL */);
MSIREN_API int msiren_align_volume_solve_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                             const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw,
                                             const msiren_align_volume_solve_opts* opts, const float* maps_in_dev /* (m, 9), affine */,
                                             const double* planes_dev /* (m, 12), rigid */, const double* rigid_in_dev /* (m, 12), rigid */,
                                             float* maps_out_dev /* (m, 9) */, double* rigid_out_dev /* (m, 12) or NULL */,
                                             double* report_dev /* (m, 6) */, double* trace_dev /* (iterations, m, 11) or NULL */);

/* Build-defined: msiren_align_volume with a per-pixel weight and a per-TARGET gain and bias.  Images, targets, maps, the
 * point rule, R, gZ, gY, gX and the pipeline are msiren_align_volume's, unchanged.
 *     weights (m, th, tw) float32 or NULL (every weight 1);   intensity (m, 2) float32 = (g, b) per target or NULL ((1, 0))
 * A pixel is VALID iff msiren_align_volume's condition holds (T, R, gZ, gY, gX finite) and its weight is finite and > 0.  Per valid pixel, in fp64
 * from the fp32 numbers, no fused multiply-add, in exactly this association:
 *     mm = ((double)g (double)R) + (double)b        r = mm - (double)T
 *     gz = (double)g (double)gZ     gy = (double)g (double)gY     gx = (double)g (double)gX
 *     J  = (gz i, gz j, gz, gy i, gy j, gy, gx i, gx j, gx, (double)R, 1.0)       (parameter order: the map's nine, then g, b)
 *     wr = w r
 *     count += 1;  wsum += w;  cost += wr r;  dcost[a] += (2 wr) J[a];  jtj[a, b] += (w J[a]) J[b]  for a <= b
 * sums (m, 80) float64 = [count, wsum, cost, dcost[0..10], jtj: the upper triangle packed row-major (66)].
 * warped (m, th, tw) = R and wgrad (3, m, th, tw) = gZ, gY, gX are optional and are written BEFORE gain and bias: the bits of
 * msiren_resample_volume_grad.  Every sum has msiren_align_slices' one order, so the determinism properties of msiren_align_volume hold.  With
 * weights and intensity NULL the 56 entries the two calls share are msiren_align_volume's bits and wsum == count; a weight that is a power of
 * two scales wsum, cost, dcost and jtj exactly; weights in {0, 1} equal NaN-masked targets.
 * MSIREN_E_INVALID before any launch: what msiren_align_volume refuses; 32 M K + 8 M (M = m th tw) with 640 bytes per chunk of 1024 pixels not
 * below 2^30; device weights or intensity not 4-byte aligned.  Under msiren_profile_enable: "align_volume_bin_kernels", the jet ragged trunk
 * under its name, "align_volume_reduce_w_kernels". */
MSIREN_API int msiren_align_volume_w(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                     const float* targets_host, int64_t m_targets, int32_t th, int32_t tw, const float* maps_host /* (m, 9) */,
                                     const float* weights_host /* (m, th, tw) or NULL */, const float* intensity_host /* (m, 2) or NULL */,
                                     double* sums_host /* (m, 80) */, float* warped_host /* or NULL */, float* wgrad_host /* (3, m, th, tw) or NULL */);
MSIREN_API int msiren_align_volume_w_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                         const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw, const float* maps_dev /* (m, 9) */,
                                         const float* weights_dev /* (m, th, tw) or NULL */, const float* intensity_dev /* (m, 2) or NULL */,
                                         double* sums_dev /* (m, 80) */, float* warped_dev /* or NULL */, float* wgrad_dev /* or NULL */);

/* Build-defined: msiren_align_volume_solve's loop around msiren_align_volume_w -- the prologue once, then `iterations` x
 * (bin -> jet ragged trunk -> the 80-sum reduce -> one step kernel), no host synchronisation.  intensity_mode 0 (fixed): (g, b) stay at their
 * inputs and the solve is over 9 parameters (affine) or 6 (rigid); 1 (estimate): (g, b) are solved for with the map, over 11 (affine) or 8
 * (rigid).  With P the number of solved parameters and sums (count, wsum, cost, g[11], H[11][11]) at the trial (map, g, b):
 *     mean = cost / wsum if count >= P else +inf;       accept / reject, lam and the flags: msiren_align_solve's
 *     affine, fixed     msiren_align_volume_solve's 9 x 9 system on g[0..8] and the leading 9 x 9 block of H
 *     affine, estimate  the same expressions with 11 in place of 9;  trial[a] = (float)((double)best[a] + d[a]) for a < 9,
 *                       g' = (float)((double)g_best + d[9]),  b' = (float)((double)b_best + d[10])
 *     rigid, fixed      msiren_align_volume_solve's B (9 x 6), g6, H6 and Cayley update on the leading block
 *     rigid, estimate   B (11 x 8): msiren_align_volume_solve's 9 x 6 block, then B[9][6] = B[10][7] = 1, every other entry 0;  g8 = B^T g,
 *                       H8 = B^T (H B), every sum ascending from 0.0, zero entries included;  the Cayley update on d[0..2], u' = u + d[3..5];
 *                       g' = (float)((double)g_best + d[6]),  b' = (float)((double)b_best + d[7])
 * fp64 + - * / one at a time; mri_inr_amd/align_volume.py: lm_step_vw restates it in Python floats and gives the same bits.  With unit weights
 * wsum == count, so with intensity_mode 0, no weights and no intensity the call returns msiren_align_volume_solve's maps, rigid states and the
 * report and trace columns the two calls share.
 * weights (m, th, tw) or NULL; intensity_in (m, 2) or NULL ((1, 0)).  maps_out (m, 9), intensity_out (m, 2): the best map and (g, b);
 * rigid_out (m, 12) or NULL.  report (m, 7) float64: accepted, mean_first, mean_best, count at the best map, wsum at the best map, lam, flags.
 * trace (iterations, m, 14) float64 or NULL: per evaluation the trial map (9), the trial g, b, then cost, count, wsum.
 * A target that reads black slices only (R = 0 everywhere: SINGULAR) and a target whose weights mask every pixel (NO_OVERLAP) keep their inputs.
 * MSIREN_E_INVALID with a message, before any launch: everything msiren_align_volume_solve refuses; struct_size !=
 * sizeof(msiren_align_volume_solve_w_opts); intensity_mode not 0 or 1; a null intensity_out or report; what msiren_align_volume_w refuses; device
 * weights or intensities not 4-byte aligned.  Under msiren_profile_enable: the prologue's entries once per call; "align_volume_bin_kernels", the
 * jet ragged trunk, "align_volume_reduce_w_kernels" and "align_volume_step_w_kernel" `iterations` times. */
typedef struct {
    uint32_t struct_size;     /* sizeof(msiren_align_volume_solve_w_opts) */
    int32_t mode;             /* 0 affine, 1 rigid */
    int32_t iterations;       /* evaluations, 1 .. 256 */
    int32_t intensity_mode;   /* 0 fixed, 1 estimate */
    double damping, down, up, lam_min, lam_max, spacing;
} msiren_align_volume_solve_w_opts;
MSIREN_API int msiren_align_volume_solve_w(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                           const float* targets_host, int64_t m_targets, int32_t th, int32_t tw,
                                           const msiren_align_volume_solve_w_opts* opts, const float* maps_in /* (m, 9), affine */,
                                           const double* planes /* (m, 12), rigid */, const double* rigid_in /* (m, 12), rigid */,
                                           const float* weights /* (m, th, tw) or NULL */, const float* intensity_in /* (m, 2) or NULL */,
                                           float* maps_out /* (m, 9) */, float* intensity_out /* (m, 2) */, double* rigid_out /* (m, 12) or NULL */,
                                           double* report /* (m, 7) */, double* trace /* (iterations, m, 14) or NULL */);
MSIREN_API int msiren_align_volume_solve_w_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                               const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw,
                                               const msiren_align_volume_solve_w_opts* opts, const float* maps_in_dev /* (m, 9), affine */,
                                               const double* planes_dev /* (m, 12), rigid */, const double* rigid_in_dev /* (m, 12), rigid */,
                                               const float* weights_dev /* (m, th, tw) or NULL */, const float* intensity_in_dev /* (m, 2) or NULL */,
                                               float* maps_out_dev /* (m, 9) */, float* intensity_out_dev /* (m, 2) */,
                                               double* rigid_out_dev /* (m, 12) or NULL */, double* report_dev /* (m, 7) */,
                                               double* trace_dev /* (iterations, m, 14) or NULL */);

/* Build-defined: msiren_align_volume_solve_w's rigid loop for GROUPS of targets that moved together -- the prologue
 * once, then `iterations` x (bin -> jet ragged trunk -> the 80-sum reduce -> the grouped step stage), no host synchronisation.  The m targets are
 * G groups of consecutive targets: group y is targets group_start[y] .. group_start[y + 1] - 1.  group_start (G + 1) int32 is a HOST array in both
 * forms (control data, as opts): first 0, last m, strictly ascending; it is read and checked before the call returns and reaches the device in
 * kernel arguments.  A group carries one rigid state (Rot, u); a target keeps its own plane (e_i, e_j, o, c), weights and intensity (g, b): its
 * trial map is the map of the group's state on its plane.  One PHYSICAL motion per group needs the same centre c in every member's plane; the call
 * does not check it.  Per group behind every evaluation, every sum over the members starting with the first member's term and adding the others in
 * ascending order (mri_inr_amd/align_group.py: lm_step_g restates it in Python floats and gives the same bits):
 *     E, C, W = sum cost, count, wsum;  mean = E / W if C >= P else +inf, P = 6 (intensity_mode 0) or 6 + 2 size (1);  accept / reject, lam:
 *     msiren_align_solve's, per group; on accept every member's best map, (g, b) and sums and the group's best state take the trial's
 *     per member at the best state: t = B^T g, HQ = B^T (H B), msiren_align_volume_solve_w's rigid expressions (6 or 8 columns), undamped
 *     M = sum HQ[0:6, 0:6], tm = sum t[0:6];  A = M damped on its diagonal by lam;  rhs = -0.5 tm
 *     intensity_mode 1: per member D = HQ[6:8, 6:8] damped on its diagonal by lam, X = D^-1 HQ[6:8, 0:6], y = D^-1 (-0.5 t[6:8]) (L D L^T); a member
 *     ELIMINATES iff its count >= 2 and D factorises; A -= C^T X, rhs -= C^T y per eliminating member, ascending, behind the damping
 *     d = A^-1 rhs (L D L^T);  Rot' = Cayley(d[0:3] / 2) Rot, u' = u + d[3:6];  (g, b)' = (float)((double)(g, b) + (y - X d)) where the member
 *     eliminated, (g, b) otherwise
 * A group of one target with intensity_mode 0 gives msiren_align_volume_solve_w's bits (mode 1, intensity_mode 0).
 * planes (m, 12), rigid_in (G, 12), weights (m, th, tw) or NULL, intensity_in (m, 2) or NULL ((1, 0)).  maps_out (m, 9), intensity_out (m, 2): the
 * best map and (g, b) per target; rigid_out (G, 12) or NULL.  report (G, 7) float64: accepted, mean_first, mean_best, C and W at the best state,
 * lam, flags (1 SINGULAR: the last 6 x 6 solve failed; 2 NO_OVERLAP: mean_first is +inf; both keep the inputs).  target_report (m, 3) float64 or
 * NULL: count, wsum, cost of each target at the best state; a member with count 0 contributes zeros and is placed by the others.  trace
 * (iterations, G, 15) float64 or NULL: per evaluation the trial state (12), then E, C, W.
 * MSIREN_E_INVALID with a message, before any launch: everything msiren_align_volume_solve_w refuses in rigid mode; struct_size !=
 * sizeof(msiren_align_volume_solve_group_opts); n_groups < 1; a null group_start; a first offset that is not 0, a last that is not m, offsets not
 * strictly ascending (the message names the index); device pointers not aligned (4 bytes: float arrays, 8: double arrays).  m = 0 or th tw = 0 does
 * nothing.  Under msiren_profile_enable: the prologue's entries once per call; "align_volume_bin_kernels", the jet ragged trunk,
 * "align_volume_reduce_w_kernels" and "align_group_step_kernels" (decide, project, step, apply as one entry) `iterations` times. */
typedef struct {
    uint32_t struct_size;     /* sizeof(msiren_align_volume_solve_group_opts) */
    int32_t iterations;       /* evaluations, 1 .. 256 */
    int32_t intensity_mode;   /* 0 fixed, 1 estimate */
    int32_t reserved;         /* 0 */
    double damping, down, up, lam_min, lam_max, spacing;
} msiren_align_volume_solve_group_opts;
MSIREN_API int msiren_align_volume_solve_group(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                               const float* targets_host, int64_t m_targets, int32_t th, int32_t tw,
                                               const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start /* host, (G + 1) */,
                                               int64_t n_groups, const double* planes /* (m, 12) */, const double* rigid_in /* (G, 12) */,
                                               const float* weights /* (m, th, tw) or NULL */, const float* intensity_in /* (m, 2) or NULL */,
                                               float* maps_out /* (m, 9) */, float* intensity_out /* (m, 2) */, double* rigid_out /* (G, 12) or NULL */,
                                               double* report /* (G, 7) */, double* target_report /* (m, 3) or NULL */,
                                               double* trace /* (iterations, G, 15) or NULL */);
MSIREN_API int msiren_align_volume_solve_group_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                                   const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw,
                                                   const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start /* host, (G + 1) */,
                                                   int64_t n_groups, const double* planes_dev /* (m, 12) */, const double* rigid_in_dev /* (G, 12) */,
                                                   const float* weights_dev /* (m, th, tw) or NULL */, const float* intensity_in_dev /* (m, 2) or NULL */,
                                                   float* maps_out_dev /* (m, 9) */, float* intensity_out_dev /* (m, 2) */,
                                                   double* rigid_out_dev /* (G, 12) or NULL */, double* report_dev /* (G, 7) */,
                                                   double* target_report_dev /* (m, 3) or NULL */, double* trace_dev /* (iterations, G, 15) or NULL */);

/* Build-defined: msiren_align_volume_w under a robust (Geman-McClure) loss rho(r) = r^2 / (1 + r^2 / s), for targets whose
 * bad pixels (dropout, artefacts, anatomy that is not in the stack) come without a mask.  Every argument of msiren_align_volume_w, and
 *     scale (m) float64: s = (c sigma)^2 per target, in SQUARED intensity units;  rweight (m, th, tw) float32 or NULL
 * A pixel is VALID iff msiren_align_volume_w's condition holds and s > 0: a target whose s is NaN, zero or negative has count 0.  s = +inf is
 * allowed.  Per valid pixel, with w, r and J[11] formed exactly as msiren_align_volume_w forms them, in fp64, no fused multiply-add, one rounding
 * per operation, in exactly this association:
 *     u  = (r r) / s        v = 1.0 + u        om = 1.0 / v
 *     wl = w om             wq = wl om
 *     count += 1;  wsum += w;  cost += (wl r) r;  dcost[a] += (2.0 (wq r)) J[a];  jtj[a, b] += (wq J[a]) J[b]  for a <= b
 * sums (m, 80) float64 in msiren_align_volume_w's layout and summation order.  cost is the weighted loss sum w rho(r), dcost its EXACT gradient
 * over the eleven parameters, jtj the Gauss-Newton matrix of the loss's quadratic majoriser (iteratively reweighted least squares), wsum the
 * plain sum of the weights -- cost / wsum cannot be lowered by rejecting pixels.  With s = +inf every term is msiren_align_volume_w's term: the 80
 * sums are its bits.  warped and wgrad as there; rweight = (float)(om om) at a valid pixel (1: an inlier, towards 0: rejected) and NaN elsewhere.
 * mri_inr_amd/align_robust.py: robust_terms restates the five lines in Python floats.
 * MSIREN_E_INVALID before any launch: what msiren_align_volume_w refuses; a null scale; device rweight not 4-byte, scale not 8-byte aligned.
 * Under msiren_profile_enable: "align_volume_bin_kernels", the jet ragged trunk under its name, "align_volume_reduce_r_kernels". */
MSIREN_API int msiren_align_volume_r(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                     const float* targets_host, int64_t m_targets, int32_t th, int32_t tw, const float* maps_host /* (m, 9) */,
                                     const float* weights_host /* (m, th, tw) or NULL */, const float* intensity_host /* (m, 2) or NULL */,
                                     const double* scale_host /* (m) */, double* sums_host /* (m, 80) */, float* warped_host /* or NULL */,
                                     float* wgrad_host /* (3, m, th, tw) or NULL */, float* rweight_host /* (m, th, tw) or NULL */);
MSIREN_API int msiren_align_volume_r_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                         const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw, const float* maps_dev /* (m, 9) */,
                                         const float* weights_dev /* (m, th, tw) or NULL */, const float* intensity_dev /* (m, 2) or NULL */,
                                         const double* scale_dev /* (m) */, double* sums_dev /* (m, 80) */, float* warped_dev /* or NULL */,
                                         float* wgrad_dev /* or NULL */, float* rweight_dev /* or NULL */);

/* Build-defined: msiren_align_volume_solve_group's loop around msiren_align_volume_r -- every evaluation's 80 sums are the
 * robust ones, the grouped step stage, its rule (mri_inr_amd/align_group.py: lm_step_g), the options struct and every output are
 * msiren_align_volume_solve_group's.  scale (m) float64 stands behind intensity_in and is FIXED for the whole call, so every evaluation of one call
 * scores the same objective; mean = sum cost / sum wsum is the mean robust loss per unit weight.  All groups of one target make it the robust
 * rigid solve per target.  With every scale +inf the call returns msiren_align_volume_solve_group's bits.  A first scale from a quadratic pass:
 * mri_inr_amd/align_robust.py: scale_from.
 * MSIREN_E_INVALID before any launch: everything msiren_align_volume_solve_group refuses; a null scale; a device scale not 8-byte aligned.  Under
 * msiren_profile_enable: as msiren_align_volume_solve_group, with "align_volume_reduce_r_kernels" in place of "align_volume_reduce_w_kernels". */
MSIREN_API int msiren_align_volume_solve_group_r(msiren_handle h, const float* images_host, int64_t n_slices, int32_t height, int32_t width,
                                                 const float* targets_host, int64_t m_targets, int32_t th, int32_t tw,
                                                 const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start /* host, (G + 1) */,
                                                 int64_t n_groups, const double* planes /* (m, 12) */, const double* rigid_in /* (G, 12) */,
                                                 const float* weights /* (m, th, tw) or NULL */, const float* intensity_in /* (m, 2) or NULL */,
                                                 const double* scale /* (m) */, float* maps_out /* (m, 9) */, float* intensity_out /* (m, 2) */,
                                                 double* rigid_out /* (G, 12) or NULL */, double* report /* (G, 7) */,
                                                 double* target_report /* (m, 3) or NULL */, double* trace /* (iterations, G, 15) or NULL */);
MSIREN_API int msiren_align_volume_solve_group_r_dev(msiren_handle h, const float* images_dev, int64_t n_slices, int32_t height, int32_t width,
                                                     const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw,
                                                     const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start /* host, (G + 1) */,
                                                     int64_t n_groups, const double* planes_dev /* (m, 12) */, const double* rigid_in_dev /* (G, 12) */,
                                                     const float* weights_dev /* (m, th, tw) or NULL */, const float* intensity_in_dev /* (m, 2) or NULL */,
                                                     const double* scale_dev /* (m) */, float* maps_out_dev /* (m, 9) */,
                                                     float* intensity_out_dev /* (m, 2) */, double* rigid_out_dev /* (G, 12) or NULL */,
                                                     double* report_dev /* (G, 7) */, double* target_report_dev /* (m, 3) or NULL */,
                                                     double* trace_dev /* (iterations, G, 15) or NULL */);

/* Build-defined: msiren_align_volume_r and msiren_align_volume_solve_group_r against a stack that is JUST VOXELS -- what
 * msiren_fuse_targets and the msiren_solve_volume* calls return -- instead of the stack the network reconstructs.  No images, no prologue, no
 * trunk, no committed weights: the handle alone.  This is the registration step of the outer loop reconstruct -> register -> reconstruct.
 *     stack (n, height, width) float32, n, height, width >= 2;  targets (m, th, tw), maps (m, 9), weights, intensity, scale, sums, warped,
 *     wgrad (3, m, th, tw), rweight exactly as in msiren_align_volume_r (the same map convention: Z in slice units, (Y, X) in pixels)
 * The point (Z, Y, X) of pixel (i, j) is msiren_align_volume's, in fp32.  The read is trilinear, in fp64 from the fp32 numbers, + - * only, one
 * rounding per operation, no fused multiply-add, in exactly this association.  A point is INSIDE iff 0 <= Z <= n - 1, 0 <= Y <= height - 1 and
 * 0 <= X <= width - 1, compared in fp32 (the bounds are exact integers; a NaN fails):
 *     z0 = min((int)floorf(Z), n - 2)    fz = (double)Z - z0    az = 1.0 - fz        (y0, fy, ay and x0, fx, ax likewise with height, width)
 *     V[dz][dy][dx] = (double)stack[z0 + dz, y0 + dy, x0 + dx]
 *     c[dz][dy] = (ax V[dz][dy][0]) + (fx V[dz][dy][1])        dx_[dz][dy] = V[dz][dy][1] - V[dz][dy][0]
 *     e[dz] = (ay c[dz][0]) + (fy c[dz][1])    ex[dz] = (ay dx_[dz][0]) + (fy dx_[dz][1])    ey[dz] = c[dz][1] - c[dz][0]
 *     R  = (float)((az e[0]) + (fz e[1]))      gX = (float)((az ex[0]) + (fz ex[1]))
 *     gY = (float)((az ey[0]) + (fz ey[1]))    gZ = (float)(e[1] - e[0])
 * A point outside gives NaN in all four.  A corner that is not finite is NOT special-cased: it makes the values non-finite through the arithmetic
 * (0 x NaN included), so a pixel needs all eight corners finite -- on a stack with NaN holes (outside the support of msiren_solve_volume*) a pixel
 * counts only where its whole cell is known.  At the upper faces the last cell is read with f = 1 (msiren_resample_volume's convention for Z).  The
 * gradient is the derivative of the interpolant inside the cell that was read (gZ per slice, gY, gX per pixel).
 * From (R, gZ, gY, gX) on the rule is msiren_align_volume_r's word for word: validity (s > 0 included), (g, b), J[11], the robust factors, the 80
 * sums, their layout and summation order.  scale = +inf is the weighted square loss.  warped = R, wgrad = (gZ, gY, gX), rweight as there.
 * mri_inr_amd/align_stack.py restates the call in Python floats and gives the same bits.
 * msiren_align_stack_solve_group_r: msiren_align_volume_solve_group_r's loop, options, outputs, report and trace, every evaluation being the call
 * above -- `iterations` x (the reduce -> the grouped step stage), no host synchronisation.
 * MSIREN_E_INVALID with a message that names the argument, before any launch: a negative extent; m th tw >= 2^28; with work to do, n, height or
 * width < 2, n height width >= 2^30 or an extent above 2^24 - 1; a null stack, targets, maps, scale or sums (the solve: what
 * msiren_align_volume_solve_group_r refuses of its options, groups and outputs); device pointers not aligned (4 bytes: float arrays, 8: double
 * arrays).  m = 0 or th tw = 0 does nothing.  Works on a handle whose weights were never committed.  Under msiren_profile_enable:
 * "align_stack_reduce_kernels" (partial and combine as one entry) once per evaluation, "align_group_step_kernels" behind each in the solve;
 * nothing of the prologue or the trunk. */
MSIREN_API int msiren_align_stack_r(msiren_handle h, const float* stack_host /* (n, height, width) */, int64_t n_slices, int32_t height, int32_t width,
                                    const float* targets_host, int64_t m_targets, int32_t th, int32_t tw, const float* maps_host /* (m, 9) */,
                                    const float* weights_host /* (m, th, tw) or NULL */, const float* intensity_host /* (m, 2) or NULL */,
                                    const double* scale_host /* (m) */, double* sums_host /* (m, 80) */, float* warped_host /* or NULL */,
                                    float* wgrad_host /* (3, m, th, tw) or NULL */, float* rweight_host /* (m, th, tw) or NULL */);
MSIREN_API int msiren_align_stack_r_dev(msiren_handle h, const float* stack_dev, int64_t n_slices, int32_t height, int32_t width,
                                        const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw, const float* maps_dev /* (m, 9) */,
                                        const float* weights_dev /* (m, th, tw) or NULL */, const float* intensity_dev /* (m, 2) or NULL */,
                                        const double* scale_dev /* (m) */, double* sums_dev /* (m, 80) */, float* warped_dev /* or NULL */,
                                        float* wgrad_dev /* or NULL */, float* rweight_dev /* or NULL */);
MSIREN_API int msiren_align_stack_solve_group_r(msiren_handle h, const float* stack_host, int64_t n_slices, int32_t height, int32_t width,
                                                const float* targets_host, int64_t m_targets, int32_t th, int32_t tw,
                                                const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start /* host, (G + 1) */,
                                                int64_t n_groups, const double* planes /* (m, 12) */, const double* rigid_in /* (G, 12) */,
                                                const float* weights /* (m, th, tw) or NULL */, const float* intensity_in /* (m, 2) or NULL */,
                                                const double* scale /* (m) */, float* maps_out /* (m, 9) */, float* intensity_out /* (m, 2) */,
                                                double* rigid_out /* (G, 12) or NULL */, double* report /* (G, 7) */,
                                                double* target_report /* (m, 3) or NULL */, double* trace /* (iterations, G, 15) or NULL */);
MSIREN_API int msiren_align_stack_solve_group_r_dev(msiren_handle h, const float* stack_dev, int64_t n_slices, int32_t height, int32_t width,
                                                    const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw,
                                                    const msiren_align_volume_solve_group_opts* opts, const int32_t* group_start /* host, (G + 1) */,
                                                    int64_t n_groups, const double* planes_dev /* (m, 12) */, const double* rigid_in_dev /* (G, 12) */,
                                                    const float* weights_dev /* (m, th, tw) or NULL */, const float* intensity_in_dev /* (m, 2) or NULL */,
                                                    const double* scale_dev /* (m) */, float* maps_out_dev /* (m, 9) */,
                                                    float* intensity_out_dev /* (m, 2) */, double* rigid_out_dev /* (G, 12) or NULL */,
                                                    double* report_dev /* (G, 7) */, double* target_report_dev /* (m, 3) or NULL */,
                                                    double* trace_dev /* (iterations, G, 15) or NULL */);

/* Build-defined: the aligned targets put back onto the stack's voxel grid -- a motion-corrected (n, H, W) stack from what the
 * volume alignment calls return.  No images, no trunk, no committed weights: a gather over the targets per output voxel.
 *     targets (m, th, tw) float32, th, tw >= 2;  maps (m, 9) float32 = (z0, z1, tz, y0, y1, ty, x0, x1, tx), msiren_align_volume's convention (Z in
 *     slice units, (Y, X) in pixels);  weights (m, th, tw) float32 or NULL (all 1);  intensity (m, 2) float32 = (g, b) or NULL ((1, 0)): T ~ g R + b
 *     opts (HOST memory in both forms): spacing (pixels per slice), thickness (half-width of the through-plane window, in pixels), min_coverage
 *     volume (n, H, W) float32;  coverage (n, H, W) float32 or NULL;  flags (m) int32 or NULL
 * All arithmetic is fp64 + - * /, one rounding per operation, no fused multiply-add, in exactly these associations.  Per target q (float32 entries
 * widened first):
 *     a = (z0 spacing, y0, x0)    b = (z1 spacing, y1, x1)    t = (tz spacing, ty, tx)
 *     G11 = ((a0 a0) + (a1 a1)) + (a2 a2)    G12 = ((a0 b0) + (a1 b1)) + (a2 b2)    G22 = ((b0 b0) + (b1 b1)) + (b2 b2)
 *     det = (G11 G22) - (G12 G12)    tt = thickness thickness    dt = det tt
 *     c = ((a1 b2) - (a2 b1), (a2 b0) - (a0 b2), (a0 b1) - (a1 b0))
 *     flags: MSIREN_FUSE_DEGENERATE (1) a map entry not finite, or not (det > 0), or det not finite;  MSIREN_FUSE_BAD_INTENSITY (2) g or b not finite,
 *     or g == 0.  A flagged target contributes nothing.
 * Per output voxel (z, y, x), v = ((double)z spacing, y, x), num = den = 0.0, for q ascending:
 *     p = v - t    pa = ((a0 p0) + (a1 p1)) + (a2 p2), pb with b, cp with c
 *     i = ((G22 pa) - (G12 pb)) / det    j = ((G11 pb) - (G12 pa)) / det    k = 1.0 - ((cp cp) / dt)
 *     q contributes iff flags == 0 and k > 0 and 0 <= i <= th - 1 and 0 <= j <= tw - 1 (a NaN fails every comparison)
 *     i0 = min(floor i, th - 2), fi = i - i0;  j0, fj likewise;  sn = sd = 0.0;  taps (0,0), (0,1), (1,0), (1,1) in this order with
 *     beta = (1 - fi) (1 - fj), (1 - fi) fj, fi (1 - fj), fi fj:  T = target[q, i0 + di, j0 + dj], w the weight there; the tap is valid iff T is finite and
 *     w is finite and > 0;  valid: bw = beta w, sn += bw (((double)T - b) / g), sd += bw
 *     num += k sn;  den += k sd
 *     volume = (float)(num / den) if den > min_coverage, else NaN;  coverage = (float)den
 * k is a quadratic (Welch) window in the distance to the target's plane: no square root, no exp, so mri_inr_amd/fuse.py: fuse_on_host (numpy) gives
 * the same bits.  With thickness = spacing an unmoved target on an integer Z has k = 1 on its own slice and 0 on its neighbours.  m_targets = 0 is
 * valid: every voxel NaN, every coverage 0.
 * MSIREN_E_INVALID before any launch, naming the argument: opts->struct_size; spacing or thickness not finite or not > 0; min_coverage NaN or
 * negative; th or tw < 2 with m > 0; n, height or width < 1; n height width or m th tw at or above 2^30; a null targets, maps, opts or volume with
 * m > 0; a device pointer that is not 4-byte aligned.  The handle need not hold committed weights.
 * Under msiren_profile_enable: one entry per call, "fuse_kernels" (the per-target set-up and the gather). */
#define MSIREN_FUSE_DEGENERATE 1
#define MSIREN_FUSE_BAD_INTENSITY 2
typedef struct {
    int32_t struct_size;      /* sizeof(msiren_fuse_opts) */
    int32_t reserved;         /* 0 */
    double spacing, thickness, min_coverage;
} msiren_fuse_opts;
MSIREN_API int msiren_fuse_targets(msiren_handle h, const float* targets_host, int64_t m_targets, int32_t th, int32_t tw, const float* maps_host /* (m, 9) */,
                                   const float* weights_host /* (m, th, tw) or NULL */, const float* intensity_host /* (m, 2) or NULL */,
                                   const msiren_fuse_opts* opts, int64_t n_slices, int32_t height, int32_t width, float* volume_host /* (n, H, W) */,
                                   float* coverage_host /* (n, H, W) or NULL */, int32_t* flags_host /* (m) or NULL */);
MSIREN_API int msiren_fuse_targets_dev(msiren_handle h, const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw, const float* maps_dev /* (m, 9) */,
                                       const float* weights_dev /* (m, th, tw) or NULL */, const float* intensity_dev /* (m, 2) or NULL */,
                                       const msiren_fuse_opts* opts /* host */, int64_t n_slices, int32_t height, int32_t width,
                                       float* volume_dev /* (n, H, W) */, float* coverage_dev /* (n, H, W) or NULL */, int32_t* flags_dev /* (m) or NULL */);

/* Build-defined: the way back from msiren_fuse_targets -- a stack gathered onto the lattices of m targets under the same maps,
 * with exactly the weights of the fusion: what each target should look like, given the stack.  The forward operator of slice-to-volume
 * reconstruction (msiren_fuse_targets is its normalised adjoint).  No images, no trunk, no committed weights.
 *     volume (n, H, W) float32;  maps (m, 9), intensity (m, 2) or NULL, opts (HOST memory in both forms): msiren_fuse_targets' arguments
 *     targets (m, th, tw) float32 or NULL;  weights (m, th, tw) float32 or NULL (all 1), only with targets
 *     simulated (m, th, tw) float32;  coverage (m, th, tw) float32 or NULL;  residual (m, th, tw) float32 or NULL and stats (m, 4) float64 or NULL,
 *     only with targets;  flags (m) int32 or NULL
 * All arithmetic is fp64 + - * /, one rounding per operation, no fused multiply-add.  The per-target record a, b, t, G11, G12, G22, det, dt, c, g, b,
 * flags is msiren_fuse_targets', unchanged.  For target q and voxel v = ((double)z spacing, y, x) the quantities p, pa, pb, cp, i, j, k, the contribution
 * test (flags == 0, k > 0, 0 <= i <= th - 1, 0 <= j <= tw - 1), i0, j0, fi, fj and the four beta are msiren_fuse_targets' expressions, character for
 * character: the two calls see the same bits.  A voxel is VALID iff volume[z, y, x] is finite.
 * Per target pixel (q, pi, pj): num = den = 0.0; over the voxels in ascending flat index (z, then y, then x), for each valid voxel that contributes to
 * q and has (pi, pj) among its four taps (i0 + di, j0 + dj) (distinct pixels: a voxel adds at most one term to a pixel):
 *     kb = k beta_tap        num += kb (double)V        den += kb
 *     coverage = (float)den        simulated = (float)((g (num / den)) + b) if den > min_coverage, else NaN             (T ~ g R + b)
 * A flagged target has simulated NaN and coverage 0 everywhere.  A volume that is NaN everywhere and m_targets = 0 are valid.
 * With targets:
 *     residual = (float)((double)T - (double)simulated), NaN where either is not finite;  a pixel COUNTS iff residual is finite and w is finite and > 0
 *     stats[q] = (count, sum w, sum w r, sum (w r) r) over the pixels that count, r the float32 residual widened, in this order: per column j the sum
 *     over the rows i ascending starting from 0.0, then the column sums added for j ascending starting from 0.0
 * mri_inr_amd/fuse.py: project_on_host and project_stats_on_host (numpy) give the same bits.
 * MSIREN_E_INVALID before any launch, naming the argument: everything msiren_fuse_targets refuses of opts, th, tw, n, height, width and the two
 * products; a null volume, maps, opts or simulated with m > 0; weights, residual or stats without targets; a device pointer that is not 4-byte
 * aligned, a device stats that is not 8-byte aligned.  Under msiren_profile_enable: one entry per call, "project_kernels". */
MSIREN_API int msiren_project_volume(msiren_handle h, const float* volume_host /* (n, H, W) */, int64_t n_slices, int32_t height, int32_t width,
                                     const float* maps_host /* (m, 9) */, const float* intensity_host /* (m, 2) or NULL */, const msiren_fuse_opts* opts,
                                     int64_t m_targets, int32_t th, int32_t tw, const float* targets_host /* (m, th, tw) or NULL */,
                                     const float* weights_host /* (m, th, tw) or NULL */, float* simulated_host /* (m, th, tw) */,
                                     float* coverage_host /* (m, th, tw) or NULL */, float* residual_host /* (m, th, tw) or NULL */,
                                     double* stats_host /* (m, 4) or NULL */, int32_t* flags_host /* (m) or NULL */);
MSIREN_API int msiren_project_volume_dev(msiren_handle h, const float* volume_dev /* (n, H, W) */, int64_t n_slices, int32_t height, int32_t width,
                                         const float* maps_dev /* (m, 9) */, const float* intensity_dev /* (m, 2) or NULL */, const msiren_fuse_opts* opts /* host */,
                                         int64_t m_targets, int32_t th, int32_t tw, const float* targets_dev /* (m, th, tw) or NULL */,
                                         const float* weights_dev /* (m, th, tw) or NULL */, float* simulated_dev /* (m, th, tw) */,
                                         float* coverage_dev /* (m, th, tw) or NULL */, float* residual_dev /* (m, th, tw) or NULL */,
                                         double* stats_dev /* (m, 4) or NULL */, int32_t* flags_dev /* (m) or NULL */);

/* Build-defined: the stack that best explains all targets at once -- `iterations` steps of conjugate gradients, in one device
 * call without a host synchronisation inside the loop, on the weighted, regularised least-squares problem
 *     F(x) = 1/2 sum over the active pixels of ((w g) g) (tau - (P x))^2  +  1/2 lambda sum over the edges of c_e (x_u - x_v)^2
 * i.e. on the normal equations (Pt Omega P + lambda L) x = Pt Omega tau, with P msiren_project_volume's row-normalised gather, tau = ((double)T - b) / g
 * and the edges the 6-neighbour pairs with both ends in the support, c = 1 in plane and c = 1.0 / (spacing spacing) through plane.  No images, no
 * trunk, no committed weights.
 *     targets, m, th, tw, maps, weights, intensity, n, height, width: msiren_fuse_targets' arguments;  opts (HOST memory in both forms)
 *     start (n, H, W) float32 or NULL: the first iterate; NULL: msiren_fuse_targets' volume of the same arguments (fuse_gather_kernel's bits, widened)
 *     volume (n, H, W) float32;  coverage (n, H, W) float32 or NULL: msiren_fuse_targets' coverage;  history (iterations + 1, 2) float64 or NULL;
 *     flags (m) int32 or NULL;  stopped_at (1) int32 or NULL
 * All arithmetic is fp64 + - * /, one rounding per operation, no fused multiply-add.  Records, flags, p, pa, pb, cp, i, j, k, the contribution test, i0,
 * j0, fi, fj and the four beta are msiren_fuse_targets' expressions, character for character.
 *   The SUPPORT S is the set of voxels where the start is finite; x_0 = (double)start there.  Every vector below is 0.0 outside S.
 *   D[q, pi, pj] = msiren_project_volume's den with "valid" read as "in S".  A pixel is ACTIVE iff its target is unflagged, T is finite, w is finite and
 *   > 0, and D > min_coverage.  Wt = ((double)w g) g.  D and the active pixels are computed once.
 *   FORWARD u = P v: num as msiren_project_volume's with the fp64 entry of v in place of (double)V, over S, in that order; u = num / D on the active
 *   pixels, 0.0 elsewhere.
 *   TRANSPOSE Pt y: per voxel of S, acc = 0.0, for q ascending under the contribution test: sn = 0.0; for the four taps in tap order, if the tap's
 *   pixel is active: sn += beta (y_p / D_p);  acc += k sn.
 *   LAPLACIAN (L v)_u: s = 0.0; for the neighbours u' = z-, z+, y-, y+, x-, x+ in this order that are in the grid and in S: s += c (v_u - v_u').
 *   A v = (Pt (Wt (P v))) + (lambda (L v)).
 *   INNER PRODUCT <a, b>: the products a b on S, 0.0 elsewhere; per slice per column the sum down the rows from 0.0, then the columns ascending from
 *   0.0; then the slices ascending from 0.0.
 *   r = (Pt (Wt tau)) - (A x_0), p = r, rho = <r, r>.  Iteration k = 0 .. iterations - 1: q = A p, gamma = <p, q>.  If the solve has stopped, or
 *   rho == 0, or gamma is not finite, or not gamma > 0: the solve stops (stopped_at = k the first time) and x, r, p, rho stay.  Else alpha = rho / gamma,
 *   x = x + (alpha p), r = r - (alpha q), rho' = <r, r>, p = r + ((rho' / rho) p), rho = rho'.
 *   volume = (float)x on S, NaN elsewhere.  history[k] = (rho_k, gamma_k), gamma NaN in the last row and from the stop on.  stopped_at = -1 if the
 *   solve never stopped.  iterations = 0 with start NULL returns msiren_fuse_targets' bits.
 * mri_inr_amd/solve_volume.py: solve_volume_on_host (numpy) gives the same bits.  m_targets = 0 is valid: with start NULL the support is empty, every
 * voxel NaN and, with iterations > 0, stopped_at = 0.
 * MSIREN_E_INVALID before any launch, naming the argument: a null opts or volume; opts->struct_size; everything msiren_fuse_targets refuses;
 * iterations < 0 or > 1024; lambda NaN, negative or infinite; a device pointer that is not 4-byte aligned, a device history that is not 8-byte
 * aligned.  Under msiren_profile_enable: one entry per call, "solve_volume_kernels". */
typedef struct {
    int32_t struct_size;      /* sizeof(msiren_solve_opts) */
    int32_t iterations;       /* 0 .. 1024 */
    double spacing, thickness, min_coverage, lambda;
} msiren_solve_opts;
MSIREN_API int msiren_solve_volume(msiren_handle h, const float* targets_host, int64_t m_targets, int32_t th, int32_t tw, const float* maps_host /* (m, 9) */,
                                   const float* weights_host /* (m, th, tw) or NULL */, const float* intensity_host /* (m, 2) or NULL */,
                                   const msiren_solve_opts* opts, int64_t n_slices, int32_t height, int32_t width, const float* start_host /* (n, H, W) or NULL */,
                                   float* volume_host /* (n, H, W) */, float* coverage_host /* (n, H, W) or NULL */,
                                   double* history_host /* (iterations + 1, 2) or NULL */, int32_t* flags_host /* (m) or NULL */,
                                   int32_t* stopped_at_host /* (1) or NULL */);
MSIREN_API int msiren_solve_volume_dev(msiren_handle h, const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw, const float* maps_dev /* (m, 9) */,
                                       const float* weights_dev /* (m, th, tw) or NULL */, const float* intensity_dev /* (m, 2) or NULL */,
                                       const msiren_solve_opts* opts /* host */, int64_t n_slices, int32_t height, int32_t width,
                                       const float* start_dev /* (n, H, W) or NULL */, float* volume_dev /* (n, H, W) */, float* coverage_dev /* (n, H, W) or NULL */,
                                       double* history_dev /* (iterations + 1, 2) or NULL */, int32_t* flags_dev /* (m) or NULL */,
                                       int32_t* stopped_at_dev /* (1) or NULL */);

/* Build-defined: msiren_solve_volume with outlier rejection -- `rounds` reweighting rounds in one device call without a host
 * synchronisation.  Each round recomputes every pixel's Geman-McClure weight from the residual of the current iterate and runs `iterations` steps of
 * msiren_solve_volume's conjugate gradients on the reweighted normal equations, warm-started from x in fp64.
 *     targets, m, th, tw, maps, weights, intensity, n, height, width, start, volume, coverage, flags: msiren_solve_volume's arguments
 *     scale (m) float64: per target, (c sigma)^2 in squared target-intensity units as in msiren_align_volume_r; +inf: the quadratic loss
 *     opts (HOST memory in both forms): msiren_solve_opts' fields, rounds (0 .. 64, rounds iterations <= 1024) and anneal (finite, >= 1)
 *     history (rounds, iterations + 1, 2) float64 or NULL;  stopped_at (rounds) int32 or NULL;  rweight (m, th, tw) float32 or NULL;
 *     residual (m, th, tw) float32 or NULL (the _dev form only);  stats (m, 4) float64 or NULL
 * All arithmetic is fp64 + - * /, one rounding per operation, no fused multiply-add.  The records, the flags, the support S, the start, D, the
 * active pixels, tau, FORWARD, TRANSPOSE, LAPLACIAN, the INNER PRODUCT, the loop and its stop rule are msiren_solve_volume's, unchanged; Wt0 = ((double)w g) g
 * is its Wt.
 *   SCHEDULE (on the host, in fp64): c[rounds - 1] = 1.0, c[t] = c[t + 1] anneal.  The scale of target q in round t is s = scale[q] c[t].
 *   REWEIGHTING PASS with the current x and a factor c, per active pixel of an unflagged target, num and D as in FORWARD:
 *     u = num / D        sim = (g u) + b        e = (double)T - sim
 *     a = (e e) / s      v = 1.0 + a            om = 1.0 / v            omega = om om;   if not (s > 0) (a NaN included): omega = +0.0
 *     Wt = Wt0 omega     z = (Wt tau) / D       z' = (Wt u) / D
 *   Wt, z and z' are +0.0 on a pixel that is not active.  s = +inf gives omega = 1.0 and Wt0's bits.  A non-finite omega is not special-cased: it
 *   makes gamma non-finite and the round stops by msiren_solve_volume's rule.
 *   ROUND t = 0 .. rounds - 1: the reweighting pass with c[t]; r = (Pt z) - ((Pt z') + (lambda (L x))), p = r, rho = <r, r>; the stop state is reset;
 *   `iterations` steps of msiren_solve_volume's loop with this round's Wt.  history[t] is the round's (iterations + 1, 2) block, stopped_at[t] the
 *   iteration at which the round stopped, or -1.
 *   AFTER THE LAST ROUND, only if rweight, residual or stats is given: one more reweighting pass with the final x and c = 1.0.
 *     rweight = (float)omega where the pixel is active and s > 0, NaN elsewhere;  residual = (float)e, NaN where the pixel is not active
 *     stats[q] = (count, sum w, sum w omega, sum (((double)w om) e) e) over the active pixels of a target with s > 0, with w omega = (double)w (om om), in
 *     msiren_project_volume's order: per column j the sum over the rows i ascending from 0.0, then the column sums for j ascending from 0.0.  A
 *     flagged target and one whose s is not > 0 have a row of zeros.
 *   volume = (float)x on S, NaN elsewhere.
 * rounds = 1 with every scale +inf returns msiren_solve_volume's volume, history and stopped_at bit for bit; rounds = 0 or iterations = 0 returns the
 * start; m_targets = 0 behaves as in msiren_solve_volume.  mri_inr_amd/solve_volume_robust.py: solve_volume_robust_on_host (numpy) gives the same bits.
 * MSIREN_E_INVALID before any launch, naming the argument: opts->struct_size; everything msiren_solve_volume refuses; rounds < 0 or > 64; rounds
 * iterations > 1024; anneal not finite or < 1; a null scale with m > 0; a device scale, stats or history that is not 8-byte aligned; a device rweight,
 * residual or stopped_at that is not 4-byte aligned.  Under msiren_profile_enable: one entry per call, "solve_volume_r_kernels". */
typedef struct {
    int32_t struct_size;      /* sizeof(msiren_solve_r_opts) */
    int32_t iterations;       /* per round, 0 .. 1024 */
    int32_t rounds;           /* 0 .. 64, rounds iterations <= 1024 */
    int32_t reserved;         /* 0 */
    double spacing, thickness, min_coverage, lambda, anneal;
} msiren_solve_r_opts;
MSIREN_API int msiren_solve_volume_r(msiren_handle h, const float* targets_host, int64_t m_targets, int32_t th, int32_t tw, const float* maps_host /* (m, 9) */,
                                     const float* weights_host /* (m, th, tw) or NULL */, const float* intensity_host /* (m, 2) or NULL */,
                                     const double* scale_host /* (m) */, const msiren_solve_r_opts* opts, int64_t n_slices, int32_t height, int32_t width,
                                     const float* start_host /* (n, H, W) or NULL */, float* volume_host /* (n, H, W) */,
                                     float* coverage_host /* (n, H, W) or NULL */, double* history_host /* (rounds, iterations + 1, 2) or NULL */,
                                     int32_t* flags_host /* (m) or NULL */, int32_t* stopped_at_host /* (rounds) or NULL */,
                                     float* rweight_host /* (m, th, tw) or NULL */, double* stats_host /* (m, 4) or NULL */);
MSIREN_API int msiren_solve_volume_r_dev(msiren_handle h, const float* targets_dev, int64_t m_targets, int32_t th, int32_t tw, const float* maps_dev /* (m, 9) */,
                                         const float* weights_dev /* (m, th, tw) or NULL */, const float* intensity_dev /* (m, 2) or NULL */,
                                         const double* scale_dev /* (m) */, const msiren_solve_r_opts* opts /* host */, int64_t n_slices, int32_t height,
                                         int32_t width, const float* start_dev /* (n, H, W) or NULL */, float* volume_dev /* (n, H, W) */,
                                         float* coverage_dev /* (n, H, W) or NULL */, double* history_dev /* (rounds, iterations + 1, 2) or NULL */,
                                         int32_t* flags_dev /* (m) or NULL */, int32_t* stopped_at_dev /* (rounds) or NULL */,
                                         float* rweight_dev /* (m, th, tw) or NULL */, float* residual_dev /* (m, th, tw) or NULL */,
                                         double* stats_dev /* (m, 4) or NULL */);

/* Build-defined: the `scale` of the robust calls (msiren_align_volume_r, msiren_align_stack_r, the grouped solves,
 * msiren_solve_volume_r) estimated on the device from an exact order statistic of the residuals -- per target, or pooled over groups of consecutive
 * targets -- so that it never has to leave the device.  No images, no trunk: the handle need not hold committed weights.
 *     targets (m, th, tw) float32;  simulated (m, th, tw) float32 or NULL;  weights (m, th, tw) float32 or NULL (all 1);  intensity (m, 2) float32 =
 *     (g, b) per target or NULL;  opts (HOST memory in both forms);  group_start (n_groups + 1) int32, HOST memory in both forms, or NULL with n_groups
 *     = 0;  scale (m) float64 out;  stats (S, 4) float64 out or NULL, S = n_groups, or m without groups
 *   RESIDUAL per pixel, fp64 + - *, one rounding per operation, no fused multiply-add:
 *     simulated and intensity given:   e = (float)((double)T - ((g (double)S) + b))        (pass `warped` of the align calls with their intensity)
 *     simulated alone:                 e = (float)((double)T - (double)S)                  ((g, b) = (1, 0), which are not multiplied in: the product and
 *                                      the sum would turn S = -0.0 into +0.0.  msiren_project_volume's residual bit for bit wherever that one is finite)
 *     simulated NULL:                  e = T                                               (the array already is a residual; intensity must be NULL)
 *   A pixel COUNTS iff e is finite and its weight is finite and > 0 (msiren_project_volume's rule).
 *   SEGMENTS: without group_start one per target.  With it: n_groups >= 1 groups of consecutive targets, group g = targets group_start[g] ..
 *   group_start[g + 1] - 1 (first offset 0, last m, strictly ascending), and one segment covers all pixels of a group.  One group pools everything.
 *   PER SEGMENT with count pixels that count:
 *     k = (int64)floor(quantile (double)(count - 1))                                       (one fp64 multiply; no interpolation between ranks)
 *     centre = 0:  c = +0.0f, d_i = |e_i|
 *     centre = 1:  c = the element of rank k (0-based, ascending) of the e_i in the total order of their bit patterns -- key = bits ^ 0x80000000 where
 *                  the sign bit is clear, ~bits where it is set, compared as uint32: -0 sorts before +0 -- and d_i = fabsf(e_i - c), one fp32 subtraction
 *     d = the element of rank k of the d_i, ordered as their uint32 bits (they are not negative; +inf, from an overflowing subtraction, sorts last)
 *     t = tune (double)d,  s = t t,  scale = s if s > floor, else floor -- written to scale[q] of every target q of the segment
 *     stats[segment] = (count, k, (double)c, (double)d)
 *     count = 0:  scale = +inf (the quadratic loss) and stats = (0, 0, 0, 0)
 *   numpy's quantile(., method="lower") on the same float32 values is the same statistic.  quantile = 0.5, centre = 1, tune = 1.4826 c: (c sigma)^2 from
 *   the median absolute deviation.  mri_inr_amd/residual_scale.py: residual_scale_on_host (numpy) gives the same bits.
 * The _dev form enqueues on the handle's stream rotation without a host synchronisation and reads nothing back: the sequence of launches depends on
 * centre and n_groups alone.  group_start is carried to the device in kernel arguments: the caller may reuse the array as soon as the call returns.
 * m_targets = 0 or th tw = 0 does nothing.  MSIREN_E_INVALID before any launch, naming the argument: opts->struct_size; centre not 0 or 1; quantile
 * outside [0, 1] or NaN; tune not finite or not > 0; floor NaN, negative or infinite; a negative extent; m th tw >= 2^28; with m > 0 a null targets,
 * opts or scale; intensity without simulated; group_start and n_groups not both given or both absent, and a group_start that is not as above; a device
 * targets, simulated, weights or intensity that is not 4-byte aligned, a device scale or stats that is not 8-byte aligned.  Under
 * msiren_profile_enable: one entry per call, "residual_scale_kernels". */
typedef struct {
    int32_t struct_size;      /* sizeof(msiren_scale_opts) */
    int32_t centre;           /* 0: d = |e|;  1: d = |e - c|, c the same order statistic of the e themselves */
    double quantile;          /* 0 .. 1 */
    double tune;              /* finite, > 0 */
    double floor;             /* finite, >= 0: the least scale returned for a segment that has pixels */
} msiren_scale_opts;
MSIREN_API int msiren_residual_scale(msiren_handle h, const float* targets_host /* (m, th, tw) */, const float* simulated_host /* (m, th, tw) or NULL */,
                                     const float* weights_host /* (m, th, tw) or NULL */, const float* intensity_host /* (m, 2) or NULL */, int64_t m_targets,
                                     int32_t th, int32_t tw, const msiren_scale_opts* opts, const int32_t* group_start /* (n_groups + 1), host, or NULL */,
                                     int64_t n_groups, double* scale_host /* (m) */, double* stats_host /* (S, 4) or NULL */);
MSIREN_API int msiren_residual_scale_dev(msiren_handle h, const float* targets_dev /* (m, th, tw) */, const float* simulated_dev /* (m, th, tw) or NULL */,
                                         const float* weights_dev /* (m, th, tw) or NULL */, const float* intensity_dev /* (m, 2) or NULL */, int64_t m_targets,
                                         int32_t th, int32_t tw, const msiren_scale_opts* opts /* host */,
                                         const int32_t* group_start /* (n_groups + 1), host, or NULL */, int64_t n_groups, double* scale_dev /* (m) */,
                                         double* stats_dev /* (S, 4) or NULL */);

/* Build-defined: every target PREDICTED FROM THE OTHERS -- the stack that msiren_fuse_targets builds from all targets outside
 * the target's own group of consecutive targets, read back onto the target's lattice as msiren_project_volume reads a stack -- in one call at about the
 * cost of two projections, instead of one fusion and one projection per group.  The residual against such a prediction is not biased towards zero as
 * the residual against a stack the target helped to build is: the input for msiren_residual_scale, and the score by which thickness and min_coverage
 * can be chosen.  No images, no trunk: the handle need not hold committed weights.
 *     targets (m, th, tw) float32;  maps (m, 9) float32;  weights (m, th, tw) float32 or NULL (all 1);  intensity (m, 2) float32 or NULL ((1, 0));
 *     opts (HOST memory in both forms): msiren_fuse_targets' options;  group_start (n_groups + 1) int32, HOST memory in both forms, or NULL with
 *     n_groups = 0: every target is its own group.  With it: msiren_residual_scale's conventions, group y = targets group_start[y] .. group_start[y + 1] - 1
 *     (first offset 0, last m, strictly ascending);  simulated (m, th, tw) float32 out;  coverage, residual (m, th, tw) float32 out or NULL;  stats (m, 4)
 *     float64 out or NULL;  flags (m) int32 out or NULL;  volume, volume_coverage (n, H, W) float32 out or NULL
 *   fp64 + - * /, one rounding per operation, no fused multiply-add.  The records and flags, p, pa, pb, cp, i, j, k, the contribution test, i0, j0, fi,
 *   fj, the four beta, the validity of a tap and the per-target terms k sn, k sd are msiren_fuse_targets' expressions, character for character.
 *   PASS 1, per voxel v:  num_v, den_v = msiren_fuse_targets' two sums over all targets, q ascending.
 *   PASS 2, per unflagged target q of the group [lo, hi), per target pixel (pi, pj):  N = D = 0.0;  the voxels in ascending flat index;  each voxel v that
 *   contributes to q under msiren_fuse_targets' test and has (pi, pj) among its four taps, with bilinear weight beta_tap:
 *     own_n = own_d = 0.0;  for q' = lo .. hi - 1 ascending, unflagged and contributing at v:  own_n += (k sn)_q',  own_d += (k sd)_q'
 *     numL = num_v - own_n,  denL = den_v - own_d
 *     v takes part iff  denL > min_coverage  and  denL > den_v MSIREN_LEAVE_OUT_FLOOR       (a power of two: the product is exact)
 *     U = numL / denL  (fp64, never rounded to float32),  kb = k_q beta_tap,  N += kb U,  D += kb
 *   coverage = (float)D;  simulated = (float)((g (N / D)) + b) if D > min_coverage, else NaN.  A flagged target: NaN, coverage 0.
 *   residual and stats (m, 4) = (count, sum w, sum w r, sum (w r) r): msiren_project_volume's, from targets, weights and simulated.
 *   volume, volume_coverage: the plain fusion of ALL targets, msiren_fuse_targets' bits ((float)(num_v / den_v) where den_v > min_coverage, else NaN;
 *   (float)den_v).
 *   THE FLOOR: den_v carries up to m roundings; where the group holds all but a sliver of a voxel's weight, denL is rounding noise.  Above
 *   2^-20 den_v its relative error is at most m 2^-33.  Where the group is the voxel's only contributor, num_v and den_v are own_n and own_d exactly (the
 *   same terms in the same order from 0.0), denL = 0 and the voxel is excluded exactly.
 *   mri_inr_amd/leave_out.py: leave_out_on_host (numpy) gives the same bits.
 * The _dev form enqueues on the handle's stream rotation without a host synchronisation and reads nothing back: the sequence of launches depends on
 * m > 0, n_groups and which of residual / stats / volume / volume_coverage are given alone.  group_start is carried to the device in kernel arguments:
 * the caller may reuse the array as soon as the call returns.  m_targets = 0 is valid: nothing that reads a target is launched; volume is NaN and
 * volume_coverage 0 where given.  MSIREN_E_INVALID before any launch, naming the argument: everything msiren_fuse_targets refuses of opts, sizes and
 * limits; with m > 0 a null targets, maps, opts or simulated; group_start and n_groups not both given or both absent, and a group_start that is not as
 * above; a device pointer that is not 4-byte aligned (stats: 8).  Under msiren_profile_enable: one entry per call, "leave_out_kernels". */
#define MSIREN_LEAVE_OUT_FLOOR (1.0 / 1048576.0) /* 2^-20 */
MSIREN_API int msiren_leave_out_targets(msiren_handle h, const float* targets_host /* (m, th, tw) */, int64_t m_targets, int32_t th, int32_t tw,
                                        const float* maps_host /* (m, 9) */, const float* weights_host /* (m, th, tw) or NULL */,
                                        const float* intensity_host /* (m, 2) or NULL */, const msiren_fuse_opts* opts,
                                        const int32_t* group_start /* (n_groups + 1), host, or NULL */, int64_t n_groups, int64_t n_slices, int32_t height,
                                        int32_t width, float* simulated_host /* (m, th, tw) */, float* coverage_host /* (m, th, tw) or NULL */,
                                        float* residual_host /* (m, th, tw) or NULL */, double* stats_host /* (m, 4) or NULL */,
                                        int32_t* flags_host /* (m) or NULL */, float* volume_host /* (n, H, W) or NULL */,
                                        float* volume_coverage_host /* (n, H, W) or NULL */);
MSIREN_API int msiren_leave_out_targets_dev(msiren_handle h, const float* targets_dev /* (m, th, tw) */, int64_t m_targets, int32_t th, int32_t tw,
                                            const float* maps_dev /* (m, 9) */, const float* weights_dev /* (m, th, tw) or NULL */,
                                            const float* intensity_dev /* (m, 2) or NULL */, const msiren_fuse_opts* opts /* host */,
                                            const int32_t* group_start /* (n_groups + 1), host, or NULL */, int64_t n_groups, int64_t n_slices, int32_t height,
                                            int32_t width, float* simulated_dev /* (m, th, tw) */, float* coverage_dev /* (m, th, tw) or NULL */,
                                            float* residual_dev /* (m, th, tw) or NULL */, double* stats_dev /* (m, 4) or NULL */,
                                            int32_t* flags_dev /* (m) or NULL */, float* volume_dev /* (n, H, W) or NULL */,
                                            float* volume_coverage_dev /* (n, H, W) or NULL */);

/* Image-quality scores of the evaluation harness (src/util/error.py:23-84 as mri_inr_amd/metrics.py restates them):
 * n pairs of (H, W) float32 images -> scores (n, 3) float64 = PSNR [dB], SSIM, NRMSE per pair, original first.
 * data range = max - min over both images (subtracted in float32); PSNR = 10 log10(range^2 / mean((o-p)^2));
 * SSIM: 7x7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance, mean over the (H-6)(W-6) windows inside the image;
 * NRMSE = sqrt(mean((o-p)^2)) / sqrt(mean(o^2)).  Sums in fp64 in a fixed order: a pair's scores are the same bits alone or in
 * any batch.  The _dev form enqueues on the handle's current stream (it sees the output of the *_dev call before it without a
 * sync); the host form blocks.  height or width below 7 is MSIREN_E_INVALID; n_images = 0 does nothing. */
MSIREN_API int msiren_score_images_dev(msiren_handle h, const float* original_dev, const float* predicted_dev, int64_t n_images,
                                       int32_t height, int32_t width, double* scores_dev);
MSIREN_API int msiren_score_images(msiren_handle h, const float* original_host, const float* predicted_host, int64_t n_images,
                                   int32_t height, int32_t width, double* scores_host);

/* Pipelining of asynchronous calls.  n = 1 (default): every *_dev call is enqueued on one stream and
 * executes in call order.  n = 2: consecutive *_dev FORWARD calls (forward_mods/latent/tiles_dev,
 * reconstruct_slices_dev) alternate between two streams with private scratch, so independent calls
 * overlap on the device (the under-occupied tail of one call's trunk kernel is filled by the next
 * call's kernels).  n = 3 (round 5): a rotation over three -- call k+2's encoder / Modulator no longer queue behind call k's
 * trunk, which pays where the trunk OWNS its CUs (config 5: +3.7 %; the default model: +0.1 %).  The caller then must not hand the
 * same output buffer to n consecutive calls, nor feed one call's output to the next, without an msiren_sync() in between.
 */
MSIREN_API int msiren_set_streams(msiren_handle h, int32_t n);

/* Blocks until everything enqueued on the handle's streams has finished (the reference's implicit
 * synchronisation at .cpu(), error.py:256-258). */
MSIREN_API int msiren_sync(msiren_handle h);

/* ---- multi-GPU: weights replicated by ONE RCCL broadcast, patches sharded by the caller ------------
 *
 * The reference is single-process, single-GPU (practical_slurm_launcher.sh:8-11, test_mod_siren.py:90-93);
 * patches are independent given the weights, so the forward has no exchange step and the only
 * collective of the scale-out is the broadcast of the state_dict from one rank at load time
 * (load_state_dict, test_mod_siren.py:116-118, executed on one rank instead of all).  librccl is
 * dlopen'ed by the first of these calls: a single-GPU host never loads it.
 *
 * One process per GPU:   rank 0: msiren_comm_unique_id(id) -> ship the 128 bytes to the other ranks
 *                        all:    msiren_comm_init_rank(h, id, 128, nranks, rank)
 *                        all:    msiren_broadcast_weights(h, root)      [collective; commits the weights]
 * One process, n GPUs:   msiren_comm_init_all(handles, n); msiren_broadcast_weights_all(handles, n, root)
 *
 * msiren_broadcast_weights: the root must hold every tensor it wants replicated (msiren_set_tensor);
 * the key set travels with the payload, the other ranks end up with exactly the root's tensors and
 * every rank's weights are committed (as by msiren_commit_weights) when the call returns.
 * msiren_comm_barrier / msiren_comm_allreduce_max_f64 are the two plumbing collectives a benchmark
 * needs (barrier around the timed region, MAX of the per-rank times); both synchronise the host. */
#define MSIREN_COMM_ID_BYTES 128
MSIREN_API int msiren_comm_unique_id(void* id_out, size_t bytes);
MSIREN_API int msiren_comm_init_rank(msiren_handle h, const void* id, size_t bytes, int32_t nranks, int32_t rank);
MSIREN_API int msiren_comm_init_all(msiren_handle* handles, int32_t n);
MSIREN_API int msiren_broadcast_weights(msiren_handle h, int32_t root);
MSIREN_API int msiren_broadcast_weights_all(msiren_handle* handles, int32_t n, int32_t root);
MSIREN_API int msiren_comm_barrier(msiren_handle h);
MSIREN_API int msiren_comm_allreduce_max_f64(msiren_handle h, double* inout, int32_t n);
MSIREN_API int msiren_comm_info(msiren_handle h, int32_t* nranks, int32_t* rank);
MSIREN_API int msiren_comm_destroy(msiren_handle h);

/* ---- device memory + timing helpers (so that a host needs no other GPU runtime) --------------- */

MSIREN_API int msiren_dev_alloc(msiren_handle h, size_t bytes, void** dev_ptr);
MSIREN_API int msiren_dev_free(msiren_handle h, void* dev_ptr);
/* Host buffers of the host-pointer entry points.  Where a caller's buffer is page-locked memory -- from here, or any memory the HIP
 * runtime has page-locked: a torch tensor after .pin_memory(), what the reference's DataLoader delivers with pin_memory=True -- the kernels of
 * a msiren_forward_tiles call of fewer than 2400 tiles work on it IN PLACE (the trunk stores into the output array, the conv kernel reads the
 * tiles), and msiren_reconstruct_slices stores the reconstruction into it; ordinary pageable memory is copied by the runtime.  The Python
 * mirror takes its OUTPUT arrays from a bounded recycling pool of these blocks by default: one 320x320 slice numpy -> numpy 485 (round 4) ->
 * 380 us, 364 with page-locked tiles as well.  Larger calls cut themselves into chunks over the handle's two streams, with copies that run
 * beside the other chunk's kernels.  Same results either way, bit for bit.
 * The library itself never calls hipHostRegister / hipHostUnregister on a caller's memory (round 5 did so per call for a few hours; the
 * path was deleted in round 6 after an unexplained GPU memory fault in processes that used it: profiles/r6/01_*).
 * msiren_host_range_kind: what a host range is to the entry points above -- 0 = pageable (copied by the runtime), 1 = the whole range lies
 * inside ONE page-locked allocation (used in place), 2 = page-locked in part (it begins or ends inside a page-locked allocation that does
 * not hold all of it: goes through a bounce buffer).  No handle: any thread, any time after the first HIP call of the process. */
MSIREN_API int msiren_host_alloc(msiren_handle h, size_t bytes, void** host_ptr);
MSIREN_API int msiren_host_free(msiren_handle h, void* host_ptr);   /* h may be NULL: a block that has outlived its handle */
MSIREN_API int msiren_host_range_kind(const void* host_ptr, size_t bytes, int32_t* kind);
MSIREN_API int msiren_memcpy_h2d(msiren_handle h, void* dst_dev, const void* src_host, size_t bytes);
MSIREN_API int msiren_memcpy_d2h(msiren_handle h, void* dst_host, const void* src_dev, size_t bytes);

/* HIP events on the handle's stream: start .. stop brackets the launches enqueued in between;
 * stop synchronises and returns elapsed milliseconds. */
MSIREN_API int msiren_timer_start(msiren_handle h);
MSIREN_API int msiren_timer_stop(msiren_handle h, float* elapsed_ms);
/* Per-kernel accounting: while enabled, every launch of the fused trunk kernel is bracketed by its
 * own event pair; msiren_profile_read returns launch count and summed milliseconds since enable. */
MSIREN_API int msiren_profile_enable(msiren_handle h, int32_t on);
MSIREN_API int msiren_profile_read(msiren_handle h, int64_t* launches, double* trunk_ms_total);
/* The same, per trunk instance: entry `index` (0-based, in order of first launch since msiren_profile_enable(h, 1)) ->
 * its name as launched (e.g. "siren_trunk_f16x3w_kernel<0,4>"), launch count, summed milliseconds and the coordinates
 * (patches x siren_patch_size^2) its launches evaluated -- a host call of several slices runs two trunk instances, so a roofline figure is per instance: msiren_flops_per_coord x coords_total / ms_total.  MSIREN_E_INVALID past
 * the last entry.  A msiren_sample_* call on a 16-bit handle adds an entry "layer0_table_kernel" (its coordinates: those of the call's set; not
 * part of msiren_profile_read's trunk totals); a gradient call (msiren_sample_grad_*, msiren_reconstruct_slices_grad) adds
 * "siren_trunk_f32_jet_kernel<HP,ACT>" in the same way (coordinates: B x Q).  msiren_last_trunk_kernel: the instance the most recent trunk launch of the handle used. */
MSIREN_API int msiren_profile_read_kernel(msiren_handle h, int32_t index, char* name128, int64_t* launches, double* ms_total,
                                          int64_t* coords_total);
MSIREN_API int msiren_last_trunk_kernel(msiren_handle h, char* name128);
/* The one-launch prologue's counterpart: the instance of the handle's most recent latent_mods launch, e.g.
 * "latent_mods_f16x3_kernel<2,2,8,3>" (<NPH,NPZ,DEPTH,MODE>); empty behind the per-layer exact-fp32 launches (and before any). */
MSIREN_API int msiren_last_prologue_kernel(msiren_handle h, char* name128);

/* name (<=255 chars + NUL), compute units, clock in MHz, total HBM bytes of the handle's device. */
MSIREN_API int msiren_device_info(msiren_handle h, char* name256, int32_t* compute_units, int32_t* clock_mhz,
                       uint64_t* hbm_bytes);
/* PCI bus id of the handle's device, "0000:c1:00.0" (<= 31 chars + NUL): which physical card a rank of a multi-GPU job sits on. */
MSIREN_API int msiren_device_pci(msiren_handle h, char* busid32);
MSIREN_API int msiren_device_count(int32_t* count);
/* Which HIP runtime the library's calls are bound to IN THIS PROCESS: *runtime_version = hipRuntimeGetVersion() (e.g. 70253625),
 * *built_against = the HIP_VERSION libmsiren.so was compiled with, *driver_version = hipDriverGetVersion(), lib_path = the file the
 * dynamic loader mapped for libamdhip64 (dladdr of a HIP entry point).  The library links libamdhip64.so.7 by soname; a PyTorch-ROCm
 * wheel bundles a libamdhip64.so of the same soname, so in a process that imported torch FIRST (the reference's own host program:
 * test_mod_siren.py:1-20 imports torch before anything else) every HIP call of this library runs on torch's bundled runtime, in a
 * torch-free process on the system one.  Any pointer may be NULL.  Needs no handle and no device. */
MSIREN_API int msiren_runtime_info(int32_t* runtime_version, int32_t* built_against, int32_t* driver_version, char* lib_path,
                                   size_t lib_path_bytes);
/* Domain guard of the split-fp16 trunk (MSIREN_PREC_F16X3).  Its fp16 operands carry activation x modulation x the next
 * layer's power-of-two weight scale; the weights are scaled into range at commit, a modulation cannot be known before the
 * call.  Every f16x3 trunk launch checks the scaled modulations it stages; if one exceeds 65504 (or is not finite) it
 * writes its launch number to a word in device memory.  Behind every such launch -- host-pointer and *_dev entry points
 * alike, one stream or two -- the library enqueues the exact-fp32 trunk over the same batch and output buffer as a
 * CONDITIONAL launch on the same stream: its workgroups read the word first and leave (~2 us) unless it holds that number.
 * So the output buffer always ends up holding what the reference's fp32 arithmetic computes (modulated_siren.py:215-233)
 * -- identical semantics, no error to handle, nothing invalidated.  msiren_range_events: synchronising calls that found a
 * conditional launch had run, since msiren_create (informational: such a model is better served by MSIREN_PREC_F32). */
MSIREN_API int msiren_range_events(msiren_handle h, int64_t* count);
/* Diagnostic: the rate the device sustains on nothing but the split-fp16 trunk's MFMA stream (v_mfma_f32_16x16x32_f16, one wave
 * per SIMD on every CU, the trunk's three products per k-step on operands of the trunk's magnitudes), ~10 ms.  *tflops: fp16
 * MFMA TFLOP/s issued chip-wide (divide by 3 for the algorithmic figure of the f16x3 roofline); *mhz_equivalent (optional):
 * the clock at which one MFMA per 16 cycles and SIMD gives that rate.  What the nominal peak becomes under the power limit
 * on real data; bench.py reports it beside the roofline, never as `peak`. */
MSIREN_API int msiren_mfma_sustained_probe(msiren_handle h, double* tflops, double* mhz_equivalent);
/* Algorithmic FLOPs per coordinate for the handle's configuration: 2*2*H + (L-1)*2*H*H + 2*H. */
MSIREN_API int msiren_flops_per_coord(msiren_handle h, double* flops);
MSIREN_API int msiren_abi_version(void);
/* Diagnostic (H=256, sine only): runs a stamped build of the trunk kernel once and returns, per
 * workgroup, 32 uint64: [0] HW_ID, [1] LDS_ALLOC, [2] XCC_ID, [3] s_memrealtime at start,
 * [4..] s_memtime at each phase boundary.  Never used by the forward entry points. */
/* Same for the register-resident f16x3 trunk: per workgroup and pass (first 4), 48 uint64: [0] s_memtime at pass
 * start, [1] after layer 0, [2] after the hidden layers, [6] at pass end, [7] s_memrealtime at pass end, [8..39]
 * s_memtime at the end of each of the 32 hidden-layer tiles.  (H=256, L=5, sine.) */
MSIREN_API int msiren_f16x3_timeline(msiren_handle h, const float* mods_dev, int64_t B, float* out_dev,
                                     uint64_t* stamps_host);
/* Same for the weight-stationary f16x3 trunk: per workgroup and slot (first 96), 8 uint64: [0..2] s_memtime at the top of the
 * slot's bookkeeping, at the start and at the end of its MFMA body, [3] s_memrealtime at the end, [4..6] s_memtime inside the slot
 * boundary (modulation rows staged / pass id handled / end).  (H=256, sine.) */
MSIREN_API int msiren_f16x3w_timeline(msiren_handle h, const float* mods_dev, int64_t B, float* out_dev,
                                      uint64_t* stamps_host);
MSIREN_API int msiren_trunk_timeline(msiren_handle h, const float* mods_dev, int64_t B, float* out_dev,
                                     uint64_t* stamps_host);

#ifdef __cplusplus
}
#endif
#endif /* MSIREN_H */
