"""One reference case for every launched instance of the exact-fp32 and the split-fp16 trunk families (f32, f32_cond, f16x3n,
f16x3h, f16x3w of mri_inr_amd/csrc/trunk_instances.h; the stamped diagnostic builds are not meant), shared by
tests/test_trunk_cases.py (CPU: the manifest is complete, dispatch.h picks each case's instance, the gate means something) and
tests/test_gpu_trunk_cases.py (the kernels against it).  Not a test module; no GPU, no HIP.

A case says which model it is, which inputs it gets, how its instance is reached (precision, environment knobs, streams, the
synchronous or the *_dev entry point) and the exact name msiren_last_trunk_kernel must report afterwards.

Gate of a case -- the suite's existing one (test_trunk_vs_oracle_shapes), against oracle.siren_forward in fp64:
    nerr <= 1e-4 and rms <= 1e-5                       the contract
    nerr <= max(10 e32, 2e-5)                          e32 = nerr(siren_forward in fp32, siren_forward in fp64): the kernel sits at
                                                       the fp32 noise floor of the same model, not merely under the contract
tests/test_trunk_cases.py asserts 10 e32 <= 1e-4 for every case, so the floor term never exceeds the contract.

Guard cases (`guard`): a handful of modulation elements mods[l, b, j] = 1e5, and column j of everything that reads feature j of
layer l's output zeroed in the state dict -- the next hidden layer (last_layer behind the last hidden one); with the residual
skip every later hidden layer and last_layer, since x_l[j] travels down the skip path.  The element then reaches nothing: the
fp64 oracle judges the case like any other, while the 16-bit launch leaves its domain and the conditional exact-fp32 launch
behind it has to redo the batch.  What raises the flag: the split-fp16 trunk (H = 256) compares the SCALED modulation
m * 2^-a_next with 65 504 where it stages the row; a_next is 3 for these weights (weights_pack.hip: rms|W w0/2pi| -> ~0.1), so
1e5 in a middle layer is 12 500 there and is NOT what flags the launch -- the element in the last hidden layer (whose row meets
last_layer unscaled) is.  Both are kept: the middle one must be harmless either way.  The single-product trunks (H = 512) read
an unscaled fp16 table: 1e5 is inf there, 0 * inf is NaN, and a NaN output raises the flag.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace

import numpy as np

from conftest import nerr, rms
from mri_inr_amd import synthetic as syn
from oracle import siren_oracle as orc

TOL, RMS_TOL = 1e-4, 1e-5   # tests/test_gpu_parity.py: check()
FLOOR_FACTOR, ABS_TERM = 10.0, 2e-5
BIG = np.float32(1e5)       # a guard case's out-of-domain modulation


@dataclass(frozen=True)
class Case:
    kernel: str              # msiren_last_trunk_kernel after the case's call
    # model
    H: int = 256
    L: int = 5
    S: int = 24
    act: str = "sine"
    residual: bool = False
    use_bias: bool = True
    w0: float = 1.0
    w0_initial: float = 30.0
    # inputs: modulations U(0.5, 1.5), U(0.1, 0.6) with the residual
    B: int = 3
    sd_seed: int = 3
    mod_seed: int = 5
    # how the instance is reached
    precision: str = "f16x3"
    ws: int | None = None    # MSIREN_F16_WS at msiren_create (None: unset)
    half: int | None = None  # MSIREN_F16_HALF
    streams: int = 1
    dev: bool = False        # msiren_forward_mods_dev + sync instead of the synchronous msiren_forward_mods
    guard: tuple = ()        # ((l, b, j), ...): mods[l, b, j] = 1e5, see the module's docstring

    @property
    def Z(self) -> int:
        return 128 if self.H == 512 else 256

    @property
    def P(self) -> int:
        return self.S * self.S

    @property
    def env(self) -> dict:
        e = {}
        if self.ws is not None:
            e["MSIREN_F16_WS"] = self.ws
        if self.half is not None:
            e["MSIREN_F16_HALF"] = self.half
        return e

    @property
    def numerics(self) -> "Case":
        """The case without how its instance is reached: cases with equal numerics share state dict, inputs and references."""
        return replace(self, kernel="", precision="", ws=None, half=None, streams=1, dev=False)

    @property
    def id(self) -> str:
        k = self.kernel.replace("siren_trunk_", "").replace("_kernel", "")
        s = f"{k}-{self.precision}-H{self.H}-L{self.L}-S{self.S}-B{self.B}-{self.act}"
        s += "-res" if self.residual else ""
        s += "" if self.use_bias else "-nobias"
        s += f"-w{self.w0:g}-{self.w0_initial:g}" if (self.w0 != 1.0 or self.w0_initial != 30.0) else ""
        s += "".join(f"-{k}{v}" for k, v in (("ws", self.ws), ("half", self.half)) if v is not None)
        s += f"-{self.streams}s" + ("-dev" if self.dev else "")
        return s + ("-guard" if self.guard else "")


# ---- state dict, inputs, references (CPU, cached per numerics) -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _state_dict(n: Case):
    sd = syn.make_state_dict(seed=n.sd_seed, dim_hidden=n.H, num_layers=n.L, latent_dim=n.Z, siren_patch_size=n.S, w0=n.w0,
                             use_bias=n.use_bias, with_encoder=False)
    sd = {k: v for k, v in sd.items() if not k.startswith("modulator")}
    for l, _, j in n.guard:
        readers = range(l + 1, n.L if n.residual else min(l + 2, n.L))
        for r in readers:
            sd[f"net.layers.{r}.weight"] = sd[f"net.layers.{r}.weight"].copy()
            sd[f"net.layers.{r}.weight"][:, j] = 0.0
        if n.residual or l == n.L - 1:
            sd["net.last_layer.weight"] = sd["net.last_layer.weight"].copy()
            sd["net.last_layer.weight"][:, j] = 0.0
    return sd


def state_dict(c: Case) -> dict:
    return _state_dict(c.numerics)


@functools.lru_cache(maxsize=None)
def _mods(n: Case):
    lo, hi = (0.1, 0.6) if n.residual else (0.5, 1.5)
    m = syn.make_mods(n.mod_seed, n.L, n.B, n.H, lo=lo, hi=hi)
    for l, b, j in n.guard:
        m[l, b, j] = BIG
    m.setflags(write=False)
    return m


def mods(c: Case) -> np.ndarray:
    return _mods(c.numerics)


@functools.lru_cache(maxsize=None)
def _oracle(n: Case, dtype):
    out = orc.siren_forward(_state_dict(n), _mods(n), num_layers=n.L, w0=n.w0, w0_initial=n.w0_initial, activation=n.act,
                            siren_patch_size=n.S, residual=n.residual, dtype=dtype)
    out.setflags(write=False)
    return out


def ref64(c: Case) -> np.ndarray:
    return _oracle(c.numerics, np.float64)


def e32(c: Case) -> float:
    return nerr(_oracle(c.numerics, np.float32), ref64(c))


def oracle_of_another_model(c: Case, **changed) -> np.ndarray:
    """The fp64 oracle of the case's weights and inputs with a model switch changed (activation, residual, w0)."""
    n = c.numerics
    kw = dict(w0=n.w0, w0_initial=n.w0_initial, activation=n.act, residual=n.residual)
    kw.update(changed)
    return orc.siren_forward(_state_dict(n), _mods(n), num_layers=n.L, siren_patch_size=n.S, dtype=np.float64, **kw)


def distance(c: Case, out):
    r = ref64(c)
    out = np.asarray(out).reshape(r.shape)
    return nerr(out, r), rms(out, r)


def tolerance(c: Case):
    return min(TOL, max(FLOOR_FACTOR * e32(c), ABS_TERM)), RMS_TOL


def passes(c: Case, out) -> bool:
    (e, r), (te, tr) = distance(c, out), tolerance(c)
    return bool(np.isfinite(out).all() and e <= te and r <= tr)


def scaled_modulation_max(c: Case) -> float:
    """Largest |m * 2^-a_next| the split-fp16 trunk stages (weights_pack.hip: pack_trunk_f16x3); for the other trunks max|m|."""
    sd, m = state_dict(c), mods(c)
    worst = 0.0
    for l in range(c.L):
        a = 0
        if c.precision == "f16x3" and l + 1 < c.L:
            w = sd[f"net.layers.{l + 1}.weight"].astype(np.float64) * (c.w0 / (2.0 * np.pi))
            rmsw, mx = float(np.sqrt(np.mean(w * w))), float(np.abs(w).max())
            a = int(np.floor(np.log2(0.1 / rmsw) + 0.5))
            a = max(-14, min(a, int(np.floor(np.log2(32768.0 / mx))), 30))
        worst = max(worst, float(np.abs(m[l]).max()) * 2.0 ** -a)
    return worst


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _k(family, *args):
    return f"siren_trunk_{family}_kernel<{','.join(str(a) for a in args)}>"


ACTS = ("sine", "morlet")

# f32<HP,ACT,RES>, all 16: a padded width and the full one per HP (100 | 128, 200 | 256, 300 | 384, 400 | 512), three or four
# layers, ragged and whole coordinate chunks, B <= 5
_WIDTHS = {128: (100, 128), 256: (200, 256), 384: (300, 384), 512: (400, 512)}
F32 = [Case(kernel=_k("f32", hp, a, r), precision="fp32", H=_WIDTHS[hp][(a + r) % 2], act=ACTS[a], residual=bool(r), L=3 + (a + i) % 2,
            S=(7, 10, 24, 33)[(i + a + 2 * r) % 4], B=5 - (i + r) % 3, sd_seed=3 + i, mod_seed=40 + 4 * i + 2 * a + r)
       for i, hp in enumerate((128, 256, 384, 512)) for a in (0, 1) for r in (0, 1)]

# The groups below share model and inputs over the instances DESIGN.md 5.1 says give the same bits (SAME_BITS).
_L5 = {a: Case(kernel="", L=5, S=24, B=7, act=a, sd_seed=11, mod_seed=61) for a in ACTS}      # 126 units: a half-unit batch
_L5B = {a: Case(kernel="", L=5, S=24, B=29, act=a, sd_seed=11, mod_seed=62) for a in ACTS}    # 522 units > 2 x 256 CUs
_L3 = {a: Case(kernel="", L=3, S=24, B=9, act=a, sd_seed=12, mod_seed=63) for a in ACTS}
_L4 = {a: Case(kernel="", L=4, S=24, B=9, act=a, sd_seed=13, mod_seed=64) for a in ACTS}
_OPT = Case(kernel="", L=4, S=33, B=3, act="morlet", w0=1.5, w0_initial=20.0, use_bias=False, sd_seed=14, mod_seed=65)

F16X3 = []
SAME_BITS = []   # lists of cases whose outputs agree bit for bit
for _i, _a in enumerate(ACTS):
    w, n45, n35, n40, n30 = _k("f16x3w", _i, 4), _k("f16x3n", _i, 4, 5), _k("f16x3n", _i, 3, 5), _k("f16x3n", _i, 4, 0), _k("f16x3n", _i, 3, 0)
    h4, h3 = _k("f16x3h", _i, 4, 5), _k("f16x3h", _i, 3, 5)
    # depth 5: every instance of it.  7 tiles of 18 units fit one round as half-units: the half-unit instance unless it is switched off
    g5 = [replace(_L5[_a], kernel=w, half=0), replace(_L5[_a], kernel=n45, ws=0, half=0), replace(_L5[_a], kernel=h4),
          replace(_L5[_a], kernel=h3, streams=2, dev=True)]
    g5b = [replace(_L5B[_a], kernel=w), replace(_L5B[_a], kernel=n35, streams=2, dev=True), replace(_L5B[_a], kernel=n45, ws=0)]
    # depths 3 and 4: weight-stationary alone; the loop form with the ring of 4 on two streams (L = 3) or with MSIREN_F16_WS=0 (L = 4)
    g3 = [replace(_L3[_a], kernel=w), replace(_L3[_a], kernel=n40, streams=2, dev=True)]
    g4 = [replace(_L4[_a], kernel=w), replace(_L4[_a], kernel=n40, ws=0)]
    F16X3 += g5 + g5b + g3 + g4
    SAME_BITS += [g5, g5b, g3, g4]
    # depth 2: the loop form in every mode; depths 6 and 11: the ring of 4 no longer fits the LDS, the loop form with the ring of 3
    F16X3 += [Case(kernel=n40, L=2, S=(24, 10)[_i], B=5, act=_a, sd_seed=15, mod_seed=66),
              Case(kernel=n30, L=6, S=(24, 7)[_i], B=(3, 5)[_i], act=_a, sd_seed=16, mod_seed=67),
              Case(kernel=n30, L=11, S=(24, 10)[_i], B=(2, 3)[_i], act=_a, sd_seed=17, mod_seed=68, streams=1 + _i, dev=bool(_i))]
# the weight-stationary Morlet instance at other pass shapes: 3 units (one pass of 3), 35 units with a ragged last one, 29 ragged
# one-unit patches, and 57 x 18 = 1026 units (a full round of 4-unit passes and a padded last pass)
F16X3 += [Case(kernel=_k("f16x3w", 1, 4), L=3, S=7, B=3, act="morlet", sd_seed=18, mod_seed=69),
          Case(kernel=_k("f16x3w", 1, 4), L=4, S=33, B=1, act="morlet", sd_seed=19, mod_seed=70),
          Case(kernel=_k("f16x3w", 1, 4), L=5, S=7, B=29, act="morlet", half=0, sd_seed=20, mod_seed=71),
          Case(kernel=_k("f16x3w", 1, 4), L=5, S=24, B=57, act="morlet", sd_seed=11, mod_seed=72)]
# w0 = 1.5 with w0_initial = 20 and use_bias = False, Morlet (the envelope constant and the weights' w0 / 2 pi scale move apart)
_gopt = [replace(_OPT, kernel=_k("f16x3w", 1, 4)), replace(_OPT, kernel=_k("f16x3n", 1, 4, 0), ws=0)]
F16X3 += _gopt
SAME_BITS.append(_gopt)

# Guard cases.  H = 256: siren_trunk_f32_cond_kernel<ACT> behind the split-fp16 launch; H = 512: siren_trunk_f32_kernel<512,ACT,RES>
# as the conditional launch behind the single-product trunks (fp16 and bf16: both read an fp16 modulation table).
GUARD_256 = [Case(kernel=_k("f16x3w", i, 4), L=4, S=10, B=5, act=a, sd_seed=22, mod_seed=73,
                  guard=((1, 0, 17), (3, 2, 200), (3, 4, 3)))
             for i, a in enumerate(ACTS)]
GUARD_512 = [Case(kernel=_k("x1w", int(p == "bf16"), i, int(r)), precision=p, H=512, L=3, S=10, B=5, act=a, residual=r, sd_seed=23,
                  mod_seed=74, guard=((1, 0, 17), (2, 2, 400), (2, 4, 3)))
             for p in ("f16", "bf16") for i, a in enumerate(ACTS) for r in (False, True)]
GUARDS = GUARD_256 + GUARD_512


def conditional_kernel(c: Case) -> str:
    """The instance a guard case's conditional launch runs (dispatch.h: Guard::f32_cond / Guard::f32_512)."""
    a = ACTS.index(c.act)
    return _k("f32_cond", a) if c.H == 256 else _k("f32", 512, a, int(c.residual))


CASES = F32 + F16X3 + GUARDS
assert len({c.id for c in CASES}) == len(CASES)
