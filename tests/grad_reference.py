"""Reference for the model's spatial gradient: ``SirenNet.forward(coords, mods)`` (modulated_siren.py:215-233)
and its derivative by ``coords`` as a numpy forward-mode pass in natural units -- what torch.autograd gives the reference.  Not a test
module: tests/test_grad_reference.py checks it on the CPU, tests/test_gpu_grad.py gates the kernels against it.

    layer l        p = x W^T + b            dp = dx W^T                          (no bias in a tangent)
    sine           a = sin(w p)             da = w cos(w p)
    Morlet         a = sin(w p) e^{-p^2/2}  da = (w cos(w p) - p sin(w p)) e^{-p^2/2}
                   x' = a mod               dx' = da dp mod
    last layer     always sine (w0)

``value_and_grad(..., dtype=np.float64)`` is the reference.  ``perturbed=True`` (with ``dtype=np.float32``) is the variant that sizes
the gate, the project's floor convention (tests/x1_cases.py): the same arithmetic in fp32, every sum over k taken in another (random)
order and every sine / cosine moved by +-2e-7 with random sign -- 2e-7 is above the measured error of the hardware sine (1.25e-7,
tools/sin_accuracy.hip).  The gate of a GPU case is 4 x that variant's distance from the fp64 reference, capped at the project's parity
norm (1e-4 / 1e-5): FACTOR and the caps are fixed here and taken from no kernel's output.

``seed`` plants one error of the kinds a forward-mode kernel can make (SEEDS); the CPU test asserts that every one of them lies at
least twice beyond the gate of every GPU case.
"""
import functools
from dataclasses import dataclass

import numpy as np

from mri_inr_amd import synthetic as syn

FACTOR = 4.0
CAP_MAX, CAP_RMS = 1e-4, 1e-5
SINE_EPS = 2e-7

SEEDS = ("const_derivative", "w0_dropped", "mod_missing", "swapped", "bias_in_tangent", "neighbour_cosine", "envelope_dropped",
         "last_cosine_dropped")


def value_and_grad(sd, mods, coords, *, num_layers, w0=1.0, w0_initial=30.0, activation="sine", dtype=np.float64, perturbed=False,
                   seed=None, seed_layer=1, rng_seed=5):
    """mods (L, B, H), coords (Q, 2) -> (value (B, Q), grad (2, B, Q)) of ``dtype``; grad[i] = d value / d coords[:, i]."""
    L = int(num_layers)
    t = np.dtype(dtype).type
    rng = np.random.default_rng(rng_seed) if perturbed else None
    morlet = activation == "morlet"
    grid = np.asarray(coords, dtype=dtype)
    mods_l = [np.asarray(m, dtype=dtype) for m in mods]
    B, P = mods_l[0].shape[0], grid.shape[0]

    def wobble(s):
        if rng is None:
            return s
        return (s + t(SINE_EPS) * (2 * rng.integers(0, 2, size=s.shape, dtype=np.int8) - 1).astype(dtype)).astype(dtype)

    def dot(x, W):
        if rng is not None:
            perm = rng.permutation(x.shape[-1])
            x, W = x[..., perm], W[:, perm]
        return x @ W.T

    def act(p, w, l, last=False):
        """(a, da) of a pre-activation p"""
        s, c = wobble(np.sin(t(w) * p)), wobble(np.cos(t(w) * p))
        if seed == "neighbour_cosine" and l == seed_layer:
            c = np.roll(c, 1, axis=1)  # the cosine of the coordinate next door
        if morlet and not last:
            e = np.exp(t(-0.5) * p * p)
            a = s * e
            da = (t(w) * c - p * s) * e
            if seed == "envelope_dropped" and l == seed_layer:
                da = t(w) * c * e
        else:
            a, da = s, t(w) * c
        if seed == "const_derivative" and l == seed_layer:
            da = np.full_like(da, t(w))
        if seed == "w0_dropped" and l == 0:
            da = da / t(w)  # (layer 0, where the factor is w0_initial: w0 = 1 in the hidden layers would not show)
        if seed == "last_cosine_dropped" and last:
            da = np.full_like(da, t(w))
        return a, da

    x = np.broadcast_to(grid[None], (B, P, grid.shape[1]))
    dx = None  # (2, B, P, H) from layer 0 on
    for l in range(L):
        W = np.asarray(sd[f"net.layers.{l}.weight"], dtype=dtype)
        b = sd.get(f"net.layers.{l}.bias")
        if l == 0:
            p = x @ W.T  # (K = 2: no order to permute; exactly the oracle's expression)
            dp = np.broadcast_to(W.T[:, None, None, :], (2, B, P, W.shape[0]))
        else:
            p = dot(x, W)
            dp = np.stack([dot(dx[0], W), dot(dx[1], W)])
        if b is not None:
            p = p + np.asarray(b, dtype=dtype)
            if seed == "bias_in_tangent" and l == seed_layer:
                dp = dp + np.asarray(b, dtype=dtype)
        a, da = act(p, w0_initial if l == 0 else w0, l)
        m = mods_l[l][:, None, :]
        x = a * m
        dx = (da * dp) * (np.ones_like(m) if seed == "mod_missing" and l == seed_layer else m)
    W = np.asarray(sd["net.last_layer.weight"], dtype=dtype)
    b = sd.get("net.last_layer.bias")
    p = dot(x, W) if rng is not None else x @ W.T
    dp = np.stack([dot(dx[0], W), dot(dx[1], W)])
    if b is not None:
        p = p + np.asarray(b, dtype=dtype)
    out, dout = act(p, w0, L, last=True)
    grad = (dout * dp)[..., 0]
    if seed == "swapped":
        grad = grad[::-1]
    return out[..., 0].astype(dtype), np.ascontiguousarray(grad, dtype=dtype)


# ---- the cases of tests/test_gpu_grad.py (and of the CPU test that keeps their gates honest) ----------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    H: int
    L: int
    act: str
    use_bias: bool = True
    zero_fraction: float = 0.0

    def __str__(self):
        return self.name


# hidden width 256 and 128 (both kernel instances), both activations, no / one / four hidden layers; a padded width (its padded features
# must stay zero in the tangents); a model without biases; modulations with exact zeros (the Modulator ends in ReLU)
CASES = [Case(f"H{H}-{act}-L{L}", H, L, act) for H in (256, 128) for act in ("sine", "morlet") for L in (1, 2, 5)] + [
    Case("H200-sine-L5", 200, 5, "sine"), Case("H256-sine-L5-nobias", 256, 5, "sine", use_bias=False),
    Case("H256-sine-L5-zeros", 256, 5, "sine", zero_fraction=0.3)]
# coordinates per call: one, a chunk of 32 less one / exactly / plus one, three chunks with a ragged last; patches: one and several
SIZES = [(Q, B) for Q in (1, 31, 32, 33, 77) for B in (1, 9)]


@functools.lru_cache(maxsize=None)
def case_state_dict(case):
    sd = syn.make_state_dict(seed=7, dim_hidden=case.H, num_layers=case.L, use_bias=case.use_bias, with_encoder=False)
    return {k: v for k, v in sd.items() if not k.startswith("modulator")}


@functools.lru_cache(maxsize=None)
def case_data(case, Q, B):
    """One call of a case: mods (L, B, H) float32 ~ U(0.5, 1.5), coords (Q, 2) float32 scattered over +-1.2 (beyond the model's grid), the
    fp64 reference (value, grad) and the gate (max, rms) of its gradient.

    The coordinates are the first draw of a fixed sequence of seeds at which the reference ALONE sits inside the caps, i.e. 4 x its own
    perturbed fp32 floor <= (CAP_MAX, CAP_RMS).  Few coordinates make an ill-conditioned draw likely -- one point where the terms of the
    gradient nearly cancel has |grad| ~ 1 where the set's is 10..40, and over two numbers the rms IS the maximum -- and there the caps,
    not the arithmetic, would decide: H256-morlet-L5 at Q = 1, B = 1 draws a point with a floor of 2.9e-5 / 2.2e-5 first.  The rule reads the
    reference only; tests/test_grad_reference.py asserts that every case ends inside the caps."""
    kw = dict(num_layers=case.L, activation=case.act)
    sd = case_state_dict(case)
    mods = syn.make_mods(2, case.L, B, case.H, zero_fraction=case.zero_fraction)
    for draw in range(16):
        coords = np.random.default_rng(200 + Q + 1000 * draw).uniform(-1.2, 1.2, size=(Q, 2)).astype(np.float32)
        val, grad = value_and_grad(sd, mods, coords, **kw)
        _, g32 = value_and_grad(sd, mods, coords, dtype=np.float32, perturbed=True, **kw)
        fm, fr = distances(g32, grad)
        if FACTOR * fm <= CAP_MAX and FACTOR * fr <= CAP_RMS:
            break
    return dict(mods=mods, coords=coords, value=val, grad=grad, floor=(fm, fr), gate=(min(FACTOR * fm, CAP_MAX), min(FACTOR * fr, CAP_RMS)),
                draw=draw)


def case_inputs(case, Q, B):
    d = case_data(case, Q, B)
    return d["mods"], d["coords"]


def distances(a, ref):
    """(max|a - ref| / max|ref|, rms(a - ref) / max|ref|): the two norms of the gate"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    return float(np.abs(a - ref).max() / scale), float(np.sqrt(np.mean((a - ref) ** 2)) / scale)
