"""The cases of the exact-fp32 prologue (the per-layer launches of mri_inr_amd/csrc/encoder_modulator.hip.h), shared by
tests/test_fp32_prologue_reference.py (CPU) and tests/test_gpu_fp32_prologue.py (the kernels).  Not a test module; no GPU, no HIP.

Every fp32 handle runs these launches, and so does every 16-bit handle whose (H, Z) is not (256, 256) or (512, 128)
(weights_pack.hip, pack_prologue_f16x3).  A case is a model (H, Z, L), the handle's precision and a batch; it NAMES the kernel each
stage must run, and tests/test_fp32_prologue_reference.py asserts those names from dispatch.h's functions (modulator_mfma,
encoder_fused_valu, linear_tiled), compiled with g++.  siren_patch_size = 8 everywhere: the trunk costs nothing.

    stage    kernel                              chosen by
    conv12   encoder_kernel (all four stages)    encoder_fused_valu(Z)
             encoder_conv_kernel                 otherwise, followed by
    conv3    Linear(2048, 64)  mfma16 | tile     linear_tiled(B, 64, 2048, 0)
    fc       Linear(64, Z)     mfma16 | tile     linear_tiled(B, Z, 64, 0)
    mod      modulator_layer_kernel (valu)       !modulator_mfma(H, Z)
             mfma16 | tile                       linear_tiled(B, H, Z, Kh)

mfma16 = modulator_layer_mfma_kernel, tile = linear_mfma_tile_kernel<2, 2>, fused = inside encoder_kernel.

Inputs: tiles uniform in [0, 1); every fourth row scaled by 2^-10 and every fifth by 2^4 (exact), so that a row wrong by its own size
is invisible to a whole-array norm and visible to the per-element bound; row 2 all zero (batches of 3 and more).  The Modulator runs on
the device's own latent and on a seeded normal draw.  modulator_bias_center per model so that ReLU leaves every layer visible: the
conditions are asserted on the CPU from the reference alone (tests/test_fp32_prologue_reference.py).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from mri_inr_amd import synthetic as syn

S = 8   # siren_patch_size

MFMA16, TILE, VALU, FUSED = "modulator_layer_mfma_kernel", "linear_mfma_tile_kernel<2,2>", "modulator_layer_kernel", "encoder_kernel"


@dataclass(frozen=True)
class Model:
    H: int
    Z: int
    L: int
    precision: str = "fp32"
    sd_seed: int = 41
    bias_center: float = 0.5

    @property
    def id(self):
        return f"{self.H}-{self.Z}-{self.L}-{self.precision}"


@dataclass(frozen=True)
class Case:
    model: Model
    B: int
    conv3: str     # the kernel of each stage
    fc: str
    mod: str
    why: str

    @property
    def id(self):
        return f"{self.model.id}-B{self.B}"

    @property
    def conv12(self):
        return FUSED if self.conv3 == FUSED else "encoder_conv_kernel"

    @property
    def in_seed(self):
        return 1000 * self.model.H + self.B


M_F16X3 = Model(256, 128, 3, "f16x3")
M_320 = Model(256, 320, 3)
M_64 = Model(64, 16, 2)
M_48 = Model(48, 48, 3)
M_256 = Model(256, 128, 3)
M_512 = Model(512, 512, 2)
M_100 = Model(100, 24, 3)
M_250 = Model(250, 256, 2)
M_20 = Model(20, 3, 2)
MODELS = [M_F16X3, M_320, M_64, M_48, M_256, M_512, M_100, M_250, M_20]

CASES = (
    [Case(M_F16X3, B, MFMA16, MFMA16, MFMA16, "a 16-bit handle off the preset shapes; ragged last row block") for B in (1, 16, 17, 37)]
    + [Case(M_320, 33, MFMA16, MFMA16, MFMA16, "nb = 36: 8 + 1 blocks per wave; the hprev | z switch inside wave 1's batch"),
       Case(M_64, 5, MFMA16, MFMA16, MFMA16, "nb = 1 at layer 0: three waves with an empty k range; Linear(64, 16)"),
       Case(M_48, 33, MFMA16, MFMA16, MFMA16, "H % 32 = 16 on the 16 x 16 kernel"),
       Case(M_48, 1041, TILE, TILE, TILE, "the tile kernel with a half-empty feature tile and 17 rows in its last tile"),
       Case(M_256, 1024, TILE, TILE, TILE, "the tile kernel at its threshold; conv3 and the fc layer on tiles"),
       Case(M_256, 1041, TILE, TILE, TILE, "a ragged second row sub-tile"),
       Case(M_512, 273, MFMA16, TILE, TILE, "the 256-row threshold of 512-wide layers; conv3 (64 outputs) stays 16 x 16")]
    + [Case(M_100, B, FUSED, FUSED, VALU, "both VALU fallbacks; MOD_ROWS full, plus one, ragged; 36 features in the second block; K = 124")
       for B in (1, 8, 9, 50)]
    + [Case(M_250, 9, MFMA16, MFMA16, VALU, "the MFMA encoder in front of the VALU Modulator; K = 506, kper = 127, a short last slice"),
       Case(M_20, 3, FUSED, FUSED, VALU, "K = 3 at layer 0: kper = 1, fourth slice empty; H < 64")]
)
assert len({c.id for c in CASES}) == len(CASES) and {c.model for c in CASES} == set(MODELS)


@functools.lru_cache(maxsize=None)
def state_dict(m: Model) -> dict:
    return syn.make_state_dict(seed=m.sd_seed, dim_hidden=m.H, num_layers=m.L, latent_dim=m.Z, siren_patch_size=S,
                               modulator_bias_center=m.bias_center)


def scale_rows(t: np.ndarray) -> np.ndarray:
    """Every fourth row x 2^-10, every fifth x 2^4 (row 0: both), exact."""
    r = np.arange(t.shape[0])
    e = np.where(r % 4 == 0, -10, 0) + np.where(r % 5 == 0, 4, 0)
    return np.ldexp(t, e.reshape((-1,) + (1,) * (t.ndim - 1))).astype(np.float32)


def make_tiles(B: int, seed: int) -> np.ndarray:
    t = scale_rows(np.random.default_rng(seed).random((B, 32, 32), dtype=np.float32))
    if B >= 3:
        t[2] = 0.0
    return t


@functools.lru_cache(maxsize=4)
def tiles(c: Case) -> np.ndarray:
    t = make_tiles(c.B, c.in_seed)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=4)
def normal_latent(c: Case) -> np.ndarray:
    z = np.random.default_rng(c.in_seed + 7).standard_normal((c.B, c.model.Z)).astype(np.float32)
    z.setflags(write=False)
    return z
