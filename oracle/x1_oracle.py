"""CPU ORACLE of the single-product 16-bit trunk (H = 512, BASELINE config 5) -- test infrastructure only.

``siren_oracle.siren_forward`` states what the model computes; this file states what the kernels
``siren_trunk_x1w_kernel`` / ``siren_trunk_x1n_kernel`` are DOCUMENTED to compute: the same layer loop with every operand
rounded where the headers and ``weights_pack.hip:pack_trunk_x1`` say it is rounded, one rounding per documented place,
and nothing else.  Comparing a kernel with this restatement takes the number format's own error (1.6e-2 for bf16 with the
residual, 10 x 512) out of the comparison: what is left is the accumulation order and the hardware sine, 2e-4 ... 5e-3.

The restatement is specified by the documentation, never fitted to a kernel's output.  numpy only; only ``tests/`` may
import it.  Files below are under ``mri_inr_amd/csrc/``.

Documented roundings (``roundings=True``), in the order the data meets them:

 1. layer-0 table  ``fp32(sin(w0_initial * pre) [* exp(-pre^2 / 2)])`` in fp64 of an fp32 ``pre = fmaf(g1, W01, fmaf(g0, W00, b0))``
    -- weights_pack.hip:295-304.  (Each ``fmaf`` is formed here as an fp64 sum rounded to fp32; an fp64 sum of an exact
    48-bit product and an fp32 term is itself rounded, which differs from the single rounding in double-rounding ties only.)
 2. modulations    fp32 -> fp16, for BOTH formats -- siren_trunk_x1w.hip.h:484-497 (``X1wLds::mods``),
    siren_trunk_x1n.hip.h:357-368 (``X1nLds::mods``, ``tb_m``).  Beyond 65 504 that is inf.
 3. layer-0 output ``RNE_fmt(fp32(table * m16))`` -- siren_trunk_x1w.hip.h:533-535, siren_trunk_x1n.hip.h:397-399;
    ``x1_pack2`` rounds to nearest even (siren_trunk_x1.hip.h:56-61).
 4. hidden weights ``RNE_fmt(fp32(W * w0/2pi * 2^e))``; fp16: ``e = clamp(floor(log2(16384 / max|W w0/2pi|)), -14, 30)``,
    bf16: ``e = 0`` -- weights_pack.hip:253-260, :270-271 (and :283-284, the weight-stationary order of the same values).
 5. bias           ``fp32(b * w0/2pi * 2^e)``, the accumulator's initial value -- weights_pack.hip:286-287,
    siren_trunk_x1w.hip.h:149-156 (``MSIREN_X1W_MFMA0``), siren_trunk_x1n.hip.h:191-193.
 6. accumulation   products of two 16-bit operands are exact in fp32; the sum is fp32 in the MFMA's own order.  Here:
    ``accumulate`` (fp64 = the order-free value).  ("Exact" is a statement about the products, not about how the MFMA aligns
    them inside its sum: the f16 two-layer instances measure five times the modelled floor, bf16 ones sit at it -- LAB_NOTES.md 14.)
 7. fp16 instances ``r = acc * 2^-e`` behind the accumulation -- siren_trunk_x1w.hip.h:233-234,
    siren_trunk_x1n.hip.h:135-140, weights_pack.hip:260.
 8. activation     in revolutions, every factor an fp32 value: ``sin_rev(r)`` and, for Morlet,
    ``* exp2(cg * r * r)`` with ``cg = fp32(-log2(e)/2 * (2pi/w0)^2)`` -- siren_trunk_f32.hip.h:54-66, weights_pack.hip:115-118.
 9. epilogue       ``fma(s, m16, x)`` in fp32 (one rounding; without the residual ``fp32(s * m16)``), then
    ``RNE_fmt`` between layers -- siren_trunk_x1w.hip.h:243-245, :252-255; siren_trunk_x1n.hip.h:155-175.
10. last hidden layer stays in fp32 and meets ``wout = fp16(fp32(W_last * w0/2pi))`` in an fp32 multiply-add chain --
    siren_trunk_x1w.hip.h:246-247, :563; siren_trunk_x1n.hip.h:171-173; weights_pack.hip:290.  Here: ``accumulate``.
11. output         ``sin_rev(sum + bout)``, ``bout = fp32(b_last * w0/2pi)`` -- siren_trunk_x1w.hip.h:569,
    siren_trunk_x1n.hip.h:436, weights_pack.hip:114.

One place where the x1n kernel's code was not what its header documented (found while writing this file, a 1-ulp-of-fp32
matter far below every gate here): siren_trunk_x1n.hip.h:163-165 forms a layer's LAST tile with the residual as
``fmaf(x, 1, fp32(s * m))`` -- two roundings -- where the header said "ONE v_fma_mix".  The comment was corrected (header
lines 11-13), not the kernel; this restatement keeps the one rounding of tiles 0..14 for all tiles.

Semantics of the residual are this build's own (parity unpinned against the reference), as in siren_oracle.py.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from oracle import siren_oracle as orc

TWO_PI = 6.283185307179586476925286766559  # weights_pack.hip:246
LOG2E = 1.4426950408889634                 # weights_pack.hip:116


# --------------------------------------------------------------------------------------------
# roundings
# --------------------------------------------------------------------------------------------


def rne_bf16(x) -> np.ndarray:
    """fp32 -> bf16 -> fp32, round to nearest even, with integer operations on the fp32 bit pattern
    (weights_pack.hip:229-235 ``f32_to_bf16_rne``; the hardware conversion of ``x1_pack2<1>`` agrees).  NaN stays NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    r = np.where(nan, (u & 0xFFFF0000) | 0x00400000, r)
    return r.astype(np.uint32).view(np.float32)


def trunc_bf16(x) -> np.ndarray:
    """fp32 -> bf16 by dropping the low 16 bits: the WRONG rounding (a seeded error of tests/test_x1_oracle.py)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32)


def rne_f16(x) -> np.ndarray:
    """fp32 -> fp16 -> fp32, round to nearest even; beyond 65 504 (65 520 rounds up) inf."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def trunc_f16(x) -> np.ndarray:
    """fp32 -> fp16 towards zero: the WRONG rounding (a seeded error of tests/test_x1_oracle.py)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16)
        over = np.abs(h.astype(np.float32)) > np.abs(x)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


def _round_fmt(fmt: str):
    if fmt == "bf16":
        return rne_bf16
    if fmt == "f16":
        return rne_f16
    raise ValueError(f"fmt must be 'bf16' or 'f16', got {fmt!r}")


def weight_scale_exponent(W, c: float, fmt: str) -> int:
    """The power-of-two weight scale of ``pack_trunk_x1`` (weights_pack.hip:253-258): fp16 brings max|W c| into
    [8192, 16384); bf16 has fp32's exponent range and takes none."""
    if fmt != "f16":
        return 0
    mx = float(np.max(np.abs(np.asarray(W, dtype=np.float64) * c)))
    if not mx > 0.0:
        return 0
    return max(-14, min(int(math.floor(math.log2(16384.0 / mx))), 30))


# --------------------------------------------------------------------------------------------
# the legitimate variations (what sizes the noise floor)
# --------------------------------------------------------------------------------------------


@dataclass(frozen=True)
class Perturb:
    """Variations a correct kernel is free to show.  ``k_order``: the input features are summed in a seeded permutation
    (with ``accumulate=np.float32`` that is fp32 accumulation in another k order; the MFMA's internal order is not
    documented).  ``sine_eps``: every hardware sine / exp2 result moves by +-sine_eps absolute, sign seeded per element
    (the hardware sine's measured error is 1.25e-7: siren_trunk_f32.hip.h:54-57).  The host-built layer-0 table is an fp64
    sine rounded once and is not perturbed."""
    seed: int = 0
    k_order: bool = True
    sine_eps: float = 2e-7


# --------------------------------------------------------------------------------------------
# the trunk
# --------------------------------------------------------------------------------------------


def x1_forward(sd: dict, mods, *, num_layers: int, fmt: str, residual: bool, activation: str = "sine",
               w0: float = 1.0, w0_initial: float = 30.0, siren_patch_size: int = 24, use_bias: bool = True,
               accumulate=np.float64, perturb: Perturb | None = None, roundings: bool = True, _hook=None) -> np.ndarray:
    """The single-product trunk as documented (module docstring): mods (L, B, 512) -> (B, P) float64.

    ``roundings=False`` turns every rounding off (and takes the pre-activation of layer 0 as the model states it): the
    structure that is left -- scaling by w0/2pi and 2^e, the activation in revolutions, the bias as the accumulator's
    initial value, 2^-e behind the accumulation -- equals ``siren_oracle.siren_forward(dtype=np.float64)`` up to fp64
    rounding, which tests/test_x1_oracle.py checks.

    ``_hook(stage, layer, value)`` is for tests only: it may return a replacement for the value at
    ``"weights"`` (layer l's rounded weight matrix, (512, 512), output feature major), ``"bias"`` (its scaled bias),
    ``"mods"`` (layer l's rounded modulation rows, (B, 512)) and ``"pack"`` (the function that rounds layer l's output to
    the format).  The product path never passes one.
    """
    L = int(num_layers)
    if L < 2:
        raise ValueError("the single-product trunk needs num_layers >= 2 (weights_pack.hip:244)")
    rnd = _round_fmt(fmt)
    f32 = (lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)) if roundings else (lambda a: np.asarray(a, dtype=np.float64))
    hook = _hook or (lambda stage, layer, value: value)
    rng = np.random.default_rng(perturb.seed) if perturb is not None else None
    acc_t = np.dtype(accumulate).type
    morlet = activation == "morlet"

    def wobble(s):  # a hardware transcendental's result, fp32, moved by the perturbation
        s = f32(s)
        if perturb is not None and perturb.sine_eps:
            s = f32(s + perturb.sine_eps * (2.0 * rng.integers(0, 2, size=s.shape, dtype=np.int8) - 1.0))
        return s

    def dot(x, Wq, init):  # init + sum_k x[..., k] * Wq[f, k], summed in `accumulate` (products of 16-bit operands: exact)
        if perturb is not None and perturb.k_order:
            perm = rng.permutation(x.shape[-1])
            x, Wq = x[..., perm], Wq[:, perm]
        if acc_t is np.float64:
            return x @ Wq.T + init
        return ((x.astype(acc_t) @ Wq.astype(acc_t).T) + init.astype(acc_t)).astype(np.float64)

    def activate(r):  # (8) siren_trunk_f32.hip.h:58-66
        s = wobble(np.sin(TWO_PI * r))
        if morlet:
            cg = f32(-0.5 * LOG2E * (TWO_PI / w0) ** 2)  # weights_pack.hip:118
            s = f32(s * wobble(np.exp2(f32(f32(cg * r) * r))))
        return s

    grid = np.asarray(sd["grid"], dtype=np.float32) if "grid" in sd else orc.make_grid(siren_patch_size, np.float32)
    m_all = np.asarray(mods, dtype=np.float32)
    B = m_all.shape[1]
    c = float(w0) / TWO_PI  # weights_pack.hip:247

    def mod_rows(l):  # (2)
        m = rne_f16(m_all[l]).astype(np.float64) if roundings else m_all[l].astype(np.float64)
        return hook("mods", l, m)

    # ---- layer 0 (1), (3) ----
    W0 = np.asarray(sd["net.layers.0.weight"], dtype=np.float32).astype(np.float64)
    b0 = sd.get("net.layers.0.bias") if use_bias else None
    b0 = np.zeros(W0.shape[0]) if b0 is None else np.asarray(b0, dtype=np.float32).astype(np.float64)
    g = grid.astype(np.float64)
    if roundings:
        pre = f32(g[:, 1:2] * W0[None, :, 1] + f32(g[:, 0:1] * W0[None, :, 0] + b0[None, :]))  # (P, 512), two fmaf
    else:
        pre = g @ W0.T + b0
    tab = np.sin(float(w0_initial) * pre)
    if morlet:
        tab = tab * np.exp(-0.5 * pre * pre)
    tab = f32(tab)
    with np.errstate(over="ignore", invalid="ignore"):
        x = f32(tab[None, :, :] * mod_rows(0)[:, None, :])  # (B, P, 512)
        if roundings:
            x = hook("pack", 0, rnd)(x).astype(np.float64)

        # ---- hidden layers (4) .. (10) ----
        for l in range(1, L):
            W = np.asarray(sd[f"net.layers.{l}.weight"], dtype=np.float32).astype(np.float64)
            e = weight_scale_exponent(W, c, fmt)
            sc = math.ldexp(c, e)
            Wq = f32(W * sc)
            if roundings:
                Wq = rnd(Wq).astype(np.float64)
            Wq = hook("weights", l, Wq)
            b = sd.get(f"net.layers.{l}.bias") if use_bias else None
            bias = np.zeros(W.shape[0]) if b is None else f32(np.asarray(b, dtype=np.float32).astype(np.float64) * sc)
            bias = hook("bias", l, bias)
            r = dot(x, Wq, bias) * math.ldexp(1.0, -e)  # (5), (6), (7)
            s = activate(r)
            m = mod_rows(l)[:, None, :]
            v = f32(s * m + x) if residual else f32(s * m)  # (9)
            if l < L - 1 and roundings:
                v = hook("pack", l, rnd)(v).astype(np.float64)
            x = v

        # ---- last_layer (10), (11) ----
        Wo = np.asarray(sd["net.last_layer.weight"], dtype=np.float32).astype(np.float64)
        wout = f32(Wo * c)
        if roundings:
            wout = rne_f16(wout).astype(np.float64)
        bo = sd.get("net.last_layer.bias") if use_bias else None
        bout = np.zeros(1) if bo is None else f32(np.asarray(bo, dtype=np.float32).astype(np.float64) * c)
        out = wobble(np.sin(TWO_PI * dot(x, wout, bout)))
    return out[..., 0]
