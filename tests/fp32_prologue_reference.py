"""The exact-fp32 prologue (mri_inr_amd/csrc/encoder_modulator.hip.h: encoder_kernel, encoder_conv_kernel + the MFMA Linear kernels,
modulator_layer_kernel) against numpy fp64, PER ELEMENT, with a bound that is derived and not measured.  Built on
oracle/siren_oracle.py; shared by tests/test_fp32_prologue_reference.py (CPU: the conditions the cases must meet, the mutants the
bound must reject) and tests/test_gpu_fp32_prologue.py (the kernels).  Not a test module; no GPU, no HIP.

One Linear layer, out[b, f] = act(bias[f] + sum_k in[b, k] w[f, k]) over K inputs, from the fp32 inputs the device itself read:

    ref   = act(bias_f + sum_k in_k w_fk)                               fp64
    bound = 1.01 (K + 4) 2^-24 (|bias_f| + sum_k |in_k w_fk|)

Any fp32 evaluation -- products rounded or fused, in any order, over four partial sums, with the bias added and the result stored --
passes every term through at most K + 4 roundings of relative size u = 2^-24, so its error is at most ((1 + u)^(K + 4) - 1) times the
sum of the terms' magnitudes; 1.01 covers the second-order part up to K = 2048 ((K + 4) u < 1.3e-4).  ReLU and LeakyReLU(0.2) are
1-Lipschitz, so the bound holds behind them (LeakyReLU's own product is one more rounding of a term that has at most K / 4 + 4 behind
it in these kernels).  Nothing here is taken from a kernel's output, and the same bound holds for all five kernels.

The encoder leaves only the latent on the device, so its reference carries a running bound beside the fp64 values through conv1
(K = 9), conv2 (144), conv3 (2048) and Linear(64, Z):

    e_out = |W| e_in + 1.01 (K + 4) 2^-24 (|b| + |W| |in|),    e = 0 on the tiles.

The mutants of tests/test_fp32_prologue_reference.py are seeded here (`Mutant`): each restates one way in which one of the kernels can
be wrong -- a k-block dropped, an operand boundary off by one block, a clamp read as a value -- in fp64, so that what the bound
rejects is known without a broken kernel.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from oracle import siren_oracle as orc

U = 2.0 ** -24
SLACK = 1.01
LEAKY = float(np.float32(0.2))   # the kernels' (and torch's fp32) slope: 0.2f
ENC = "encoder.encoder.encoder."
SENTINEL = -7.0                  # what rows past a device-side count hold: they are not written


def roundings(K: int) -> float:
    return SLACK * (K + 4) * U


def act(pre, kind: str):
    if kind == "relu":
        return np.where(pre <= 0, 0.0, pre)   # (NaN stays NaN, as the kernels and torch.relu)
    if kind == "leaky":
        return np.where(pre <= 0, pre * LEAKY, pre)
    assert kind == "none"
    return pre


class Ref(NamedTuple):
    out: np.ndarray     # the layer's output, fp64
    bound: np.ndarray   # per element
    pre: np.ndarray     # the pre-activation (what decides where a ReLU's zeros are)


@dataclass(frozen=True)
class Mutant:
    """One seeded error.  stage: conv3 | fc | mod; layer: the Modulator layer (stage mod)."""
    name: str
    stage: str
    layer: int = 0

    @property
    def id(self):
        return f"{self.name}-{self.stage}" + (str(self.layer) if self.stage == "mod" else "")


# what the kernels do with K (encoder_modulator.hip.h): four waves split the nb = K / 16 blocks at nb w / 4 (MFMA kernels); four
# k-slices of (K + 3) / 4 (modulator_layer_kernel; the fused encoder's conv3: 4 x 512)
def wave_blocks(K: int, wave: int):
    nb = K // 16
    return nb * wave // 4, nb * (wave + 1) // 4


def valu_slice(K: int, ks: int):
    kper = (K + 3) // 4
    return min(K, ks * kper), min(K, (ks + 1) * kper)


def dropped_block(K: int) -> int:
    """The k-block the drop_block mutant leaves out: the last of wave 1's range (at nb = 36 the one its remainder loop handles), of
    wave 3's where wave 1 has none (nb = 1)."""
    lo, hi = wave_blocks(K, 1)
    if hi == lo:
        lo, hi = wave_blocks(K, 3)
    assert hi > lo
    return hi - 1


def linear(x, W, b, kind, *, Kh=0, mutant: str | None = None, count=None):
    """x (B, K) fp32 or fp64 inputs [hidden ; latent], W (F, K), b (F) -> Ref, every field (B, F) fp64.
    count: rows from `count` on are not written (SENTINEL, bound 0).  mutant: the seeded error's name, or None."""
    x, W, b = (np.asarray(a, dtype=np.float64) for a in (x, W, b))
    B, K = x.shape
    F = W.shape[0]
    assert W.shape == (F, K) and b.shape == (F,)
    bound = roundings(K) * (np.abs(x) @ np.abs(W).T + np.abs(b))
    if mutant == "clamp_row":      # the last row computed from its neighbour's input: min(row, nrows - 1) taken one too low
        x = x.copy()
        x[B - 1] = x[B - 2]
    elif mutant == "bias16":       # p.bias[f0 + cc] of the next 16-feature tile
        b = np.roll(b, -16)
    elif mutant == "valu_block2":  # blockIdx.y = 1 reading wt[k, fi] instead of wt[k, 64 + fi]
        W = W.copy()
        W[64:128] = W[:min(64, F - 64)] if F < 128 else W[:64]
    pre = x @ W.T + b
    if mutant == "drop_block":
        ks = slice(16 * dropped_block(K), 16 * dropped_block(K) + 16)
        pre = pre - x[:, ks] @ W[:, ks].T
    elif mutant == "kh_shift":     # `k0 < Kh - 16 ? hrow : zrow`: the last hidden block reads the latent's first 16
        assert Kh >= 16 and K - Kh >= 16
        ks = slice(Kh - 16, Kh)
        pre = pre + (x[:, Kh:Kh + 16] - x[:, ks]) @ W[:, ks].T
    elif mutant == "valu_slice4":
        k0, k1 = valu_slice(K, 3)
        pre = pre - x[:, k0:k1] @ W[:, k0:k1].T
    out = act(pre, "relu" if mutant == "conv3_relu" else kind)
    if count is not None and mutant != "count_ignored":
        out[count:] = SENTINEL
    if count is not None:
        bound[count:] = 0.0
    return Ref(out, bound, pre)


# ---- Modulator: one layer in isolation ---------------------------------------------------------------------------------------------
def modulator_weights(sd, l):
    return sd[f"modulator.layers.{l}.0.weight"], sd[f"modulator.layers.{l}.0.bias"]


def modulator_layer(sd, l, hprev, z, *, mutant: str | None = None, count=None):
    """Layer l from the inputs the device read: hprev = its own mods[l - 1] (None at layer 0) and z, both fp32."""
    W, b = modulator_weights(sd, l)
    x = np.asarray(z) if l == 0 else np.concatenate([np.asarray(hprev), np.asarray(z)], axis=1)
    return linear(x, W, b, "relu", Kh=0 if l == 0 else np.asarray(hprev).shape[1], mutant=mutant, count=count)


def modulator_chain(sd, z, L, *, mutant: Mutant | None = None, count=None):
    """What a device without error returns for z, layer by layer, each layer fed the fp32 roundings of the one before -> list of
    (Ref, what the mutant returns instead) per layer; the mutant acts in its own layer only (the layers behind it are compared in isolation)."""
    z = np.asarray(z, dtype=np.float32)
    rows, h = [], None
    for l in range(L):
        ref = modulator_layer(sd, l, h, z, count=count)
        got = ref.out if mutant is None or mutant.layer != l else modulator_layer(sd, l, h, z, mutant=mutant.name, count=count).out
        rows.append((ref, got))
        h = ref.out.astype(np.float32)
    return rows


# ---- encoder: end to end with a running bound --------------------------------------------------------------------------------------
def _conv(x, e, W, b, stride, pad):
    W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
    K = W[0].size
    pre = orc._conv2d(x, W, b, stride, pad)
    e_out = orc._conv2d(e, np.abs(W), np.zeros_like(b), stride, pad) + roundings(K) * orc._conv2d(np.abs(x), np.abs(W), np.abs(b), stride, pad)
    return act(pre, "leaky"), e_out


def encoder(sd, tiles, *, mutant: Mutant | None = None, count=None):
    """tiles (B, 32, 32) fp32 -> (latent, bound), (B, Z) fp64.  A mutant of stage conv3 / fc acts there; what follows runs on its
    output.  (The bound is the unmutated chain's either way.)"""
    g = lambda k: np.asarray(sd[ENC + k], dtype=np.float64)
    x = np.asarray(tiles, dtype=np.float64)[:, None, :, :]
    x, e = _conv(x, np.zeros_like(x), g("0.weight"), g("0.bias"), 2, 1)
    x, e = _conv(x, e, g("2.weight"), g("2.bias"), 2, 1)
    x, e = x.reshape(x.shape[0], -1), e.reshape(e.shape[0], -1)   # (c, y, x): conv3 == Linear(2048, 64)
    pick = lambda stage: mutant.name if mutant is not None and mutant.stage == stage else None
    W3, W7 = g("4.weight").reshape(64, 2048), g("7.weight")
    clean3 = linear(x, W3, g("4.bias"), "leaky")
    a3 = linear(x, W3, g("4.bias"), "leaky", mutant=pick("conv3")).out if pick("conv3") else clean3.out
    e = e @ np.abs(W3).T + clean3.bound
    e = e @ np.abs(W7).T + linear(clean3.out, W7, g("7.bias"), "none").bound
    if count is not None:
        e[count:] = 0.0
    return linear(a3, W7, g("7.bias"), "none", mutant=pick("fc"), count=count).out, e


# ---- the gate ------------------------------------------------------------------------------------------------------------------------
def ratio(got, ref, bound) -> np.ndarray:
    """|got - ref| / bound per element; 0 where both are exactly equal (also at bound 0), inf where got is not finite or differs at
    bound 0."""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - ref)
        r = np.where(d == 0, 0.0, d / bound)
    return np.where(np.isfinite(got), r, np.inf)


def worst(got, ref, bound) -> float:
    return float(ratio(got, ref, bound).max())


def misplaced_zeros(got, ref: Ref) -> int:
    """Behind a ReLU the device's zeros sit where the reference's do: no output is negative, and an element whose pre-activation is
    below -bound (no fp32 evaluation of it is positive) is exactly zero.  Counts the elements that break either."""
    got = np.asarray(got, dtype=np.float64)
    return int((got < 0).sum() + ((ref.pre < -ref.bound) & (got != 0)).sum())
