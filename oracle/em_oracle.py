"""CPU ORACLE of the split-fp16 prologue (tiles -> latent -> modulations) -- test infrastructure only.

``siren_oracle.encoder_forward`` / ``modulator_forward`` state what the model computes; this file states what
``encoder_conv_f16x3_kernel<1>`` and ``latent_mods_f16x3_kernel<NPH,NPZ,DEPTH,MODE>`` are DOCUMENTED to compute: the same
chain with every operand scaled, split and rounded where ``encoder_modulator_f16x3.hip.h`` and
``weights_pack.hip:pack_prologue_f16x3`` say it is, one rounding per documented place, and nothing else.  Against the fp64
oracle a correct kernel sits at 1-4e-7 (the split's 22 bits, fp32 epilogues); against this restatement what is left is fp32
accumulation in the MFMA's own order, 2-3e-7 per row at most -- and a single wrong ``lo`` fragment is 4e-6.

The restatement is specified by the documentation, never fitted to a kernel's output.  numpy only; only ``tests/`` may
import it.  Files below are under ``mri_inr_amd/csrc/``; ``em:`` is encoder_modulator_f16x3.hip.h, ``wp:`` weights_pack.hip.

Documented roundings (``roundings=True``), in the order the data meets them:

 1. conv1          fp32 FMAs, the bias first, the nine taps in the reference order ky * 3 + kx, over the tile padded in front
                   (stride 2, padding 1: only index -1 is outside); LeakyReLU as ``x >= 0 ? x : 0.2f * x`` -- em:513-530,
                   encoder_params.h:26.  (Each ``fmaf`` is formed here as an fp64 sum rounded to fp32: double rounding in ties only.)
 2. tile scale     ``2^s`` with ``max|a1| 2^s in [2^13, 2^14)`` over the tile's 16 x 16 x 16 conv1 outputs; ``s`` clamped to
                   +-100, ``s = 0`` for a zero tile -- ``em_row_scale``, em:78-84, :537-540.
 3. split          ``hi = f16(v)``, ``lo = f16(v - hi)``, round to nearest even, of the scaled value -- ``em_split8``, em:87-96,
                   :542-543.  The same split at every B operand below, where the row is produced.
 4. conv2 weights  times ``2^a``, ``max|W| 2^a in [2^13, 2^14)`` over the whole layer (``scale_of``, wp:422-430), rounded to
                   fp32, then the same split -- wp:447-468.  A k-step is two taps x 16 channels; the tenth tap has zero weights.
 5. product        ``W_lo x_hi + W_hi x_lo + W_hi x_hi`` per k-step, in this order, on v_mfma_f32_16x16x32_f16 (products of
                   two fp16 values are exact in fp32, the sum is fp32 in the MFMA's own order); ``W_lo x_lo`` is absent --
                   em:564-566, :185-190.  Here: ``accumulate``.
 6. epilogue       ``fma(acc, 2^-(a + s), bias)`` in fp32, one rounding (``2^-a 2^-s`` is an exact fp32 product), then
                   LeakyReLU(0.2) in fp32 -- em:569-574.
 7. feature scale  per tile over its 2048 conv2 features, split: conv3's B images and ``feat_inv`` -- em:576-590.
 8. conv3          == Linear(2048, 64).  Its k order is the order in which the conv kernel's threads hold the features
                   (wp:477-483); the two K halves (k-steps 0..31, 32..63) are accumulated apart and summed in fp32 --
                   em:253-269, :286.  Then (6) with LeakyReLU as ``v <= 0 ? 0.2f * v : v`` -- em:290-291.
 9. Linear(64, Z)  row scale over the 64 features, split, K padded to 128 with a zero image against zero weights
                   (em:273, wp:490), (6) without activation: the latent, fp32 -- em:297-322.
10. latent         row scale over Z, split -- em:344-352.  (With the latent given, MODE 2, the chain starts here: em:330.)
11. Modulator, latent part: for every layer ``Mz_l z + c_l`` with ``Mz_l = W_l[:, Kh:]`` scaled by its OWN power of two
                   (wp:504: the latent part and the hidden part of a layer are scaled separately), rounded to fp32 by (6):
                   layer 0 is ``h_0`` after ReLU; layers 1.. go to the fp32 scratch buffer -- em:359-387.
12. hidden chain   ``h_l = relu(fma(acc, 2^-(a_h + s), scratch_l))``, ``acc = Mh_l h_{l-1}`` with ``Mh_l = W_l[:, :H]`` scaled
                   by its own power of two (wp:517) and ``h_{l-1}`` scaled per row and split -- em:414-456.

ReLU is ``v <= 0 ? 0 : v`` and both activations keep NaN.  Elements more than 2^17 below their row's (layer's) maximum are
fp16 subnormals after the split and keep fewer than 22 bits (em:20-21): numpy's fp16 conversion rounds them as the hardware does.

Code against comments, found while writing this file: the header's arithmetic paragraph and the packer's comment said "weights: per
layer" where the code scales the latent part and the hidden part of every Modulator layer apart (wp:504, :517; em:64) -- both comments
were corrected, not the code.  Everything else above is as the header says; its cited line numbers are those of this commit's
neighbours and are re-checked by hand when those files move (LAB_NOTES.md section 16).
"""

from __future__ import annotations

import numpy as np

SLOPE = 0.2
STAGES = ("conv2", "conv3", "fc", "mod_z", "mod_h")


# --------------------------------------------------------------------------------------------
# roundings and scales
# --------------------------------------------------------------------------------------------


def rne_f16(x) -> np.ndarray:
    """fp32 -> fp16 -> fp32, round to nearest even (subnormals included); beyond 65 504 (65 520 rounds up) inf."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def trunc_f16(x) -> np.ndarray:
    """fp32 -> fp16 towards zero: the WRONG rounding (a seeded error of tests/test_em_oracle.py)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16)
        over = np.abs(h.astype(np.float32)) > np.abs(x)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


def split_f16(v, rnd=rne_f16):
    """``em_split8`` (em:87-96): fp32 v -> (hi, lo) = (f16(v), f16(v - hi)), both returned as fp32 arrays holding fp16 values.
    ``v - hi`` is exact in fp32."""
    v = np.asarray(v, dtype=np.float32)
    hi = rnd(v)
    with np.errstate(invalid="ignore"):
        lo = rnd(v - hi)
    return hi, lo


def row_scale_exponent(m) -> np.ndarray:
    """``em_row_scale`` (em:78-84) on the fp32 bit pattern: s with m 2^s in [2^13, 2^14) for a normal m > 0, 0 for m = 0 (and NaN),
    clamped to +-100 (a subnormal m: 100; inf: -100)."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    e = ((m.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    s = np.where(m > 0, 14 - (e - 126), 0)
    return np.clip(s, -100, 100)


def weight_scale_exponent(W) -> int:
    """``scale_of`` (wp:422-430): a with max|W| 2^a in [2^13, 2^14), clamped to +-100; 0 for a zero or non-finite layer."""
    mx = float(np.max(np.abs(np.asarray(W, dtype=np.float64)))) if np.size(W) else 0.0
    if not (mx > 0.0) or not np.isfinite(mx):
        return 0
    return int(max(-100, min(100, 14 - int(np.frexp(mx)[1]))))


def conv3_ksteps() -> np.ndarray:
    """(64, 32): torch's flattened (channel, position) index of every element of conv3's 64 k-steps -- the order in which
    ``encoder_conv_f16x3_kernel``'s threads hold the features (em:586-589, wp:477-483)."""
    ks = np.empty((64, 32), dtype=np.int64)
    for s2 in range(64):
        for q in range(4):
            for j in range(8):
                cw, cl = s2 >> 4, 4 * (s2 & 15) + q
                ks[s2, 8 * q + j] = (16 * (cw & 1) + 4 * (cl >> 4) + (j & 3)) * 64 + 16 * (2 * (cw >> 1) + (j >> 2)) + (cl & 15)
    return ks


def natural_ksteps(K: int) -> np.ndarray:
    """(K / 32, 32): k-step s of an image in LDS holds inputs 32 s .. 32 s + 31 (em:30-32, ``kin`` of wp:441)."""
    return np.arange(K, dtype=np.int64).reshape(K // 32, 32)


# --------------------------------------------------------------------------------------------
# the chain
# --------------------------------------------------------------------------------------------


def prologue_forward(sd: dict, tiles=None, *, num_layers: int, z_in=None, roundings: bool = True, accumulate: str = "fp64",
                     group_seed=None, modulate: bool = True, return_features: bool = False, _hook=None):
    """The split-fp16 prologue as documented (module docstring): tiles (B, 32, 32) -> latent (B, Z) and modulations (L, B, H),
    float64 [and the conv2 features (B, 2048) in torch's flattened order].  ``z_in`` (B, Z) instead of tiles: the Modulator alone
    (MODE 2); ``modulate=False``: the encoder alone (MODE 1; the modulations are None).

    ``roundings=False`` turns every rounding off; what is left -- the powers of two, the padded k-steps, conv3's k order and
    halves, the hoisted latent part -- equals ``siren_oracle.encoder_forward`` / ``modulator_forward`` in fp64 up to fp64
    rounding, which tests/test_em_oracle.py checks.

    ``accumulate``: "fp64" is the order-free value of every sum of products; "fp32_ksteps" sums in fp32 as the kernels issue
    their MFMAs: k-step by k-step, W_lo x_hi, W_hi x_lo, W_hi x_hi, the accumulator rounded to fp32 behind each MFMA (one
    rounding for its 32 products).  ``group_seed``: each MFMA's 32 products are summed in four seeded groups of eight, rounded
    to fp32 after each -- another legitimate order (the MFMA's internal one is not documented).

    ``_hook(stage, layer, phase, ops)`` is for tests only; it may change the entries of ``ops`` in place.  stage: one of STAGES,
    layer: the Modulator layer (0 for the encoder's stages).  Phases, in order:
      "input"    x (rows, K) fp32 values of the B operand, s (rows,) the rows' scale exponents, split (the rounding function)
      "weights"  W (F, K) as the state dict has it (mod_z / mod_h: the slice of the layer's matrix), a (its scale exponent), split
      "operands" A = [W_lo, W_hi, W_hi] and X = [x_hi, x_lo, x_hi], the three products' operands (F, K) / (rows, K);
                 ksteps (n, 32) input indices per k-step in consumption order; conv3: halves = [first, last k-step) per K half
      "epilogue" acc, s (the exponent undone: the rows'), a, bias (F,) or (rows, F), act (the activation function)
    The product path never passes one.
    """
    if accumulate not in ("fp64", "fp32_ksteps"):
        raise ValueError(f"accumulate must be 'fp64' or 'fp32_ksteps', got {accumulate!r}")
    L = int(num_layers)
    hook = _hook or (lambda stage, layer, phase, ops: None)
    f32 = (lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)) if roundings else (lambda a: np.asarray(a, dtype=np.float64))
    slope = float(np.float32(SLOPE)) if roundings else SLOPE
    rng = np.random.default_rng(group_seed) if group_seed is not None else None
    g = lambda k: np.asarray(sd[k], dtype=np.float32).astype(np.float64)

    def leaky(v):
        return np.where(v >= 0, v, f32(slope * v))

    def leaky_le(v):  # (em:291: the other comparison, the same function)
        return np.where(v <= 0, f32(slope * v), v)

    def relu(v):
        return np.where(v <= 0, 0.0, v)

    def no_split(v):
        v = np.asarray(v, dtype=np.float64)
        return v, np.zeros_like(v)

    def accumulate_products(A, X, ksteps):
        """sum over the k-steps of X[i] A[i]^T, i = 0, 1, 2"""
        if accumulate == "fp64":
            cols = np.asarray(ksteps).ravel()
            return sum(X[i][:, cols] @ A[i][:, cols].T for i in range(3))
        acc = np.zeros((X[0].shape[0], A[0].shape[0]), dtype=np.float32)
        for ks in ksteps:
            for i in range(3):
                groups = [ks] if rng is None else np.split(ks[rng.permutation(len(ks))], 4)
                for c in groups:
                    acc = (acc.astype(np.float64) + X[i][:, c] @ A[i][:, c].T).astype(np.float32)
        return acc.astype(np.float64)

    def stage(name, layer, x, s, W, bias, act, ksteps, halves=None):
        """One scaled, split GEMM with its epilogue: x (rows, K) fp32 values with scale exponents s (rows,), W (F, K)."""
        ops = dict(x=x, s=np.array(s, dtype=np.int64), split=split_f16 if roundings else no_split)
        hook(name, layer, "input", ops)
        s_in = ops["s"]
        with np.errstate(over="ignore", invalid="ignore"):
            x_hi, x_lo = ops["split"](f32(ops["x"] * np.ldexp(1.0, s_in)[:, None]))
        wops = dict(W=W, a=weight_scale_exponent(W), split=split_f16 if roundings else no_split)
        hook(name, layer, "weights", wops)
        a = int(wops["a"])
        w_hi, w_lo = wops["split"](f32(np.ldexp(wops["W"], a)))
        ops = dict(A=[np.array(w_lo, dtype=np.float64), np.array(w_hi, dtype=np.float64), np.array(w_hi, dtype=np.float64)],
                   X=[np.array(x_hi, dtype=np.float64), np.array(x_lo, dtype=np.float64), np.array(x_hi, dtype=np.float64)],
                   ksteps=np.array(ksteps), halves=halves)
        hook(name, layer, "operands", ops)
        with np.errstate(over="ignore", invalid="ignore"):
            if ops["halves"] is None:
                acc = accumulate_products(ops["A"], ops["X"], ops["ksteps"])
            else:  # (8) the K halves apart, then one fp32 addition
                parts = [accumulate_products(ops["A"], ops["X"], ops["ksteps"][lo:hi]) for lo, hi in ops["halves"]]
                acc = parts[0]
                for p in parts[1:]:
                    acc = f32(acc + p)
            eops = dict(acc=acc, s=s_in.copy(), a=a, bias=bias, act=act)
            hook(name, layer, "epilogue", eops)
            u = f32(np.ldexp(1.0, -eops["s"]) * f32(np.ldexp(1.0, -int(eops["a"]))))[:, None]  # 2^-s 2^-a: an fp32 product
            v = f32(eops["acc"] * u + eops["bias"])  # (6)
            return eops["act"](v) if eops["act"] is not None else v

    def row_scale(v):  # (2): per row over all of its features
        with np.errstate(invalid="ignore"):
            return row_scale_exponent(np.max(np.abs(v.reshape(v.shape[0], -1)), axis=1))

    p = "encoder.encoder.encoder."
    feat = None
    if z_in is None:
        t = np.asarray(tiles, dtype=np.float32).astype(np.float64)
        B = t.shape[0]
        if t.shape[1:] != (32, 32):
            raise ValueError(f"tiles must be (B, 32, 32), got {t.shape}")
        with np.errstate(over="ignore", invalid="ignore"):
            # ---- (1) conv1: (B, 16 channels, 16, 16) ----
            t0 = np.zeros((B, 33, 33))
            t0[:, 1:, 1:] = t
            W1, b1 = g(p + "0.weight").reshape(16, 9), g(p + "0.bias")
            a1 = np.broadcast_to(b1[None, :, None, None], (B, 16, 16, 16)).copy()
            for k in range(9):
                ky, kx = divmod(k, 3)
                win = t0[:, ky:ky + 32:2, kx:kx + 32:2]  # t0[2 y + ky][2 x + kx]
                a1 = f32(win[:, None] * W1[None, :, k, None, None] + a1)
            a1 = leaky(a1)
            # ---- (2) .. (6) conv2 as an implicit GEMM: rows = (tile, position), K = 10 taps x 16 channels ----
            s1 = row_scale(a1)
            pad = np.zeros((B, 16, 17, 17))
            pad[:, :, 1:, 1:] = a1
            cols = np.empty((B, 64, 10, 16))
            for tap in range(10):
                ky, kx = divmod(min(tap, 8), 3)  # (the tenth tap: zero weights, any finite operand -- em:556-557)
                cols[:, :, tap, :] = pad[:, :, ky:ky + 16:2, kx:kx + 16:2].reshape(B, 16, 64).transpose(0, 2, 1)
            W2 = np.zeros((32, 10, 16))
            W2[:, :9, :] = g(p + "2.weight").reshape(32, 16, 9).transpose(0, 2, 1)  # [o][tap][ci]
            o2 = stage("conv2", 0, cols.reshape(B * 64, 160), np.repeat(s1, 64), W2.reshape(32, 160), g(p + "2.bias")[None, :], leaky,
                       natural_ksteps(160))
            feat = o2.reshape(B, 64, 32).transpose(0, 2, 1).reshape(B, 2048)  # k = channel * 64 + position
            # ---- (7), (8) conv3 ----
            a3 = stage("conv3", 0, feat, row_scale(feat), g(p + "4.weight").reshape(64, 2048), g(p + "4.bias")[None, :], leaky_le,
                       conv3_ksteps(), halves=[(0, 32), (32, 64)])
            # ---- (9) Linear(64, Z): K padded to 128 ----
            Wf = g(p + "7.weight")
            Z = Wf.shape[0]
            z = stage("fc", 0, np.concatenate([a3, np.zeros((B, 64))], axis=1), row_scale(a3),
                      np.concatenate([Wf, np.zeros((Z, 64))], axis=1), g(p + "7.bias")[None, :], None, natural_ksteps(128))
    else:
        z = f32(np.asarray(z_in, dtype=np.float32))
        B, Z = z.shape
    if not modulate:
        return (z, None, feat) if return_features else (z, None)

    # ---- (10) .. (12) the Modulator ----
    with np.errstate(over="ignore", invalid="ignore"):
        sz = row_scale(z)
        mods = []
        scratch = [None] * L
        H = np.asarray(sd["modulator.layers.0.0.weight"]).shape[0]
        for l in range(L):
            W = g(f"modulator.layers.{l}.0.weight")
            Kh = 0 if l == 0 else H
            v = stage("mod_z", l, z, sz, W[:, Kh:Kh + Z], g(f"modulator.layers.{l}.0.bias")[None, :], relu if l == 0 else None,
                      natural_ksteps(Z))
            if l == 0:
                mods.append(v)
            else:
                scratch[l] = v
        for l in range(1, L):
            W = g(f"modulator.layers.{l}.0.weight")
            h = mods[-1]
            mods.append(stage("mod_h", l, h, row_scale(h), W[:, :H], scratch[l], relu, natural_ksteps(H)))
    mods = np.stack(mods, axis=0)
    return (z, mods, feat) if return_features else (z, mods)
