"""One reference case for every instance of the trunk families that evaluate the model at caller-chosen coordinates, one set per patch
(f32_ragged, f32_jet_ragged, f16x3n_ragged, f32_ragged_cond of mri_inr_amd/csrc/trunk_instances.h), shared by
tests/test_coordset_cases.py (CPU: the manifest is complete, dispatch.h picks each native case's instance, the gates mean something) and
tests/test_gpu_coordset_cases.py (the kernels against it).  Not a test module; no GPU, no HIP.  The shared-grid trunks have
tests/trunk_cases.py; this file follows it.

A case says which model it is, which call reaches its instance (`form`: model.sample_mods_ragged = value, sample_mods_ragged_grad = grad,
sample_mods_ragged(..., exact=False) = native), the per-patch set sizes and the exact name the profile must show afterwards.

Inputs: coordinates float32, uniform over +-1.2 (beyond the model's grid); modulations syn.make_mods, U(0.5, 1.5), U(0.1, 0.6) with the
residual.

Structure sets, c = the family's chunk (64: f32_ragged and f32_ragged_cond; 32: the jet and the native trunk):
    EDGES(c)  [0, 0, 1, c-1, 0, c, c+1, 0, 0, 2c+2, 0]: empty patches at both ends, single and consecutive ones in the middle (runs of
              equal first[] entries: the tie rule of the binary search decides them), sets one below, at and one above a chunk, and one
              of two chunks and a ragged third
    MANY(c)   300 patches, counts cycling (0, 1, 2, 0, 3), patches 255 / 256 / 299 = c+1 / 1 / c: the item prefix of
              ragged_items_kernel crosses its 256-patch block with work on both sides

References, fp64, patch by patch: grad_reference.value_and_grad (values and gradients); residual cases oracle.siren_forward with
sd["grid"] = the patch's coordinates.

Gates -- none from a kernel's output:
    values     nerr <= min(1e-4, max(10 e32, 2e-5)) and rms <= 1e-5: tests/trunk_cases.py's rule, e32 = nerr(the same
               reference in fp32, the one in fp64)
    gradients  grad_reference's: 4 x the distance of the perturbed-fp32 variant of the same case, capped at 1e-4 / 1e-5; the coordinates
               are the first of 16 fixed draws at which the reference alone sits inside the caps (grad_reference.case_data's rule)
`l0_floor` is the floor the native family falls back on if (and only if) one of its instances meets the contract but misses 10 e32: the
distance of a restatement of its documented arithmetic -- layer 0 as fma(y, w_col, fma(x, w_row, b)) on the fp32 rows
{w_row, w_col, b} w0_initial / 2 pi and its activation in fp32, everything behind in fp64 -- from the fp64 reference; the factor stays 10.
NATIVE_FLOOR names the one in force (LAB_NOTES.md has both numbers per case).

Guard cases (`guard`): tests/trunk_cases.py's dead-end construction -- mods[l, b, j] = 1e5 with column j of the next layer (last_layer
behind the last hidden one) zeroed, in a middle layer and in the last hidden layer, in patches that hold coordinates.  The element reaches
nothing, so the fp64 reference judges the case like any other, while the native launch leaves the fp16 domain (the last hidden layer's
row meets last_layer unscaled: that element raises the flag) and siren_trunk_f32_ragged_cond_kernel<ACT> has to redo the call.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace

import numpy as np

import grad_reference as gr
from conftest import nerr, rms
from mri_inr_amd import synthetic as syn
from oracle import siren_oracle as orc

TOL, RMS_TOL = 1e-4, 1e-5   # the contract (tests/trunk_cases.py)
FLOOR_FACTOR, ABS_TERM = 10.0, 2e-5
BIG = np.float32(1e5)       # a guard case's out-of-domain modulation
ACTS = ("sine", "morlet")
CHUNK = {"f32_ragged": 64, "f32_ragged_cond": 64, "f32_jet_ragged": 32, "f16x3n_ragged": 32}
NATIVE_FLOOR = "e32"        # "e32" | "l0_floor": see the module's docstring
DRAWS = 16


def EDGES(c):
    return (0, 0, 1, c - 1, 0, c, c + 1, 0, 0, 2 * c + 2, 0)


def MANY(c):
    counts = [(0, 1, 2, 0, 3)[t % 5] for t in range(300)]
    counts[255], counts[256], counts[299] = c + 1, 1, c
    return tuple(counts)


MANY_ALONE = (254, 255, 256, 257, 299)  # the patches of a MANY set the GPU file recomputes alone (254 and 257: 3 and 2 coordinates)


@dataclass(frozen=True)
class Case:
    kernel: str              # the instance the case pins, as the profile names it
    # model
    H: int = 256
    L: int = 5
    act: str = "sine"
    residual: bool = False
    use_bias: bool = True
    w0: float = 1.0
    w0_initial: float = 30.0
    # how the instance is reached
    precision: str = "fp32"
    form: str = "value"      # value | grad | native
    # inputs
    counts: tuple = ()
    sd_seed: int = 3
    mod_seed: int = 5
    coord_seed: int = 11     # grad cases: the first of DRAWS seeds coord_seed + 1000 draw, see coords_of()
    zero_fraction: float = 0.0
    guard: tuple = ()        # ((l, b, j), ...): mods[l, b, j] = 1e5, see the module's docstring
    trunk: str = ""          # guard cases: the native instance whose launch the conditional kernel (`kernel`) stands behind

    @property
    def family(self) -> str:
        return self.kernel[len("siren_trunk_"):self.kernel.index("_kernel<")]

    @property
    def chunk(self) -> int:
        return CHUNK[self.family]

    @property
    def NP(self) -> int:
        return len(self.counts)

    @property
    def T(self) -> int:
        return int(sum(self.counts))

    @property
    def Z(self) -> int:
        return 128 if self.H == 512 else 256

    @property
    def many(self) -> bool:
        return self.NP == 300

    @property
    def options(self) -> bool:
        return self.w0 != 1.0 or self.w0_initial != 30.0

    @property
    def launches(self) -> tuple:
        """the profile's kernel names after the case's call"""
        if self.form != "native":
            return (self.kernel,)
        cond = _k("f32_ragged_cond", ACTS.index(self.act))
        return (self.trunk or self.kernel, cond)

    @property
    def model(self) -> "Case":
        """what a handle is built from: cases with equal `model` share one"""
        return replace(self, kernel="", form="", counts=(), mod_seed=0, coord_seed=0, zero_fraction=0.0, trunk="",
                       guard=tuple((l, 0, j) for l, _, j in self.guard))

    @property
    def id(self) -> str:
        k = (self.trunk + "+" if self.trunk else "") + self.kernel
        s = k.replace("siren_trunk_", "").replace("_kernel", "") + f"-{self.precision}-H{self.H}-L{self.L}-{self.act}"
        s += "-res" if self.residual else ""
        s += "" if self.use_bias else "-nobias"
        s += f"-w{self.w0:g}-{self.w0_initial:g}" if self.options else ""
        s += "-zeros" if self.zero_fraction else ""
        s += "-many" if self.many else "-edges"
        return s + ("-guard" if self.guard else "")


# ---- state dict, inputs (CPU, cached) ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _state_dict(m: Case):
    sd = syn.make_state_dict(seed=m.sd_seed, dim_hidden=m.H, num_layers=m.L, latent_dim=m.Z, w0=m.w0, use_bias=m.use_bias, with_encoder=False)
    sd = {k: v for k, v in sd.items() if not k.startswith("modulator")}
    for l, _, j in m.guard:   # (guard cases have no residual: one reader)
        key = f"net.layers.{l + 1}.weight" if l + 1 < m.L else "net.last_layer.weight"
        sd[key] = sd[key].copy()
        sd[key][:, j] = 0.0
    return sd


def state_dict(c: Case) -> dict:
    return _state_dict(c.model)


def with_biases(c: Case) -> dict:
    """the case's weights plus biases of the init's range (synthetic.make_state_dict): `a model with biases` for the no-bias cases"""
    rng = np.random.default_rng(1000 + c.sd_seed)
    sd = dict(state_dict(c))
    for l in range(c.L):
        bound = 0.5 if l == 0 else np.sqrt(6.0 / c.H) / c.w0
        sd[f"net.layers.{l}.bias"] = rng.uniform(-bound, bound, size=c.H).astype(np.float32)
    sd["net.last_layer.bias"] = rng.uniform(-bound, bound, size=1).astype(np.float32)
    return sd


@functools.lru_cache(maxsize=None)
def mods(c: Case) -> np.ndarray:
    lo, hi = (0.1, 0.6) if c.residual else (0.5, 1.5)
    m = syn.make_mods(c.mod_seed, c.L, c.NP, c.H, lo=lo, hi=hi, zero_fraction=c.zero_fraction)
    for l, b, j in c.guard:
        m[l, b, j] = BIG
    m.setflags(write=False)
    return m


def offsets(c: Case) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(c.counts)]).astype(np.int32)


def _draw(c: Case, draw: int) -> np.ndarray:
    xy = np.random.default_rng(c.coord_seed + 1000 * draw).uniform(-1.2, 1.2, size=(c.T, 2)).astype(np.float32)
    xy.setflags(write=False)
    return xy


def patches(c: Case):
    """(b, lo, hi) of every patch that holds coordinates"""
    o = offsets(c)
    return [(b, int(o[b]), int(o[b + 1])) for b in range(c.NP) if o[b + 1] > o[b]]


# ---- the references ------------------------------------------------------------------------------------------------------------------------
def evaluate(c: Case, dtype=np.float64, *, coords=None, sd=None, mods_=None, rows=None, grad=False, **changed):
    """The reference of the case patch by patch -> (value (T,), grad (2, T) or None) of `dtype`.  `changed`: act, residual, w0, w0_initial
    (another model on the same weights), perturbed / seed / seed_layer (grad_reference.value_and_grad).  `rows`: patch -> the patch whose
    modulation rows it is evaluated with."""
    sd = state_dict(c) if sd is None else sd
    m = mods(c) if mods_ is None else mods_
    xy = coords_of(c) if coords is None else coords
    act, res = changed.pop("act", c.act), changed.pop("residual", c.residual)
    kw = dict(num_layers=c.L, w0=changed.pop("w0", c.w0), w0_initial=changed.pop("w0_initial", c.w0_initial), activation=act, dtype=dtype)
    val = np.zeros(c.T, dtype)
    g = np.zeros((2, c.T), dtype) if grad else None
    for b, lo, hi in patches(c):
        r = b if rows is None else rows[b]
        if res:
            assert not grad and not changed
            sdg = dict(sd)
            sdg["grid"] = xy[lo:hi]
            val[lo:hi] = orc.siren_forward(sdg, m[:, r:r + 1], residual=True, **kw)[0]
        else:
            v, d = gr.value_and_grad(sd, m[:, r:r + 1], xy[lo:hi], **kw, **changed)
            val[lo:hi] = v[0]
            if grad:
                g[:, lo:hi] = d[:, 0]
    return val, g


@functools.lru_cache(maxsize=None)
def _grad_draw(c: Case):
    """grad cases: (draw, coords, fp64 value, fp64 grad, floor) at the first draw whose gradient floor x FACTOR sits inside the caps (the
    last draw if none does: tests/test_coordset_cases.py fails then)"""
    for draw in range(DRAWS):
        xy = _draw(c, draw)
        val, g = evaluate(c, coords=xy, grad=True)
        _, g32 = evaluate(c, np.float32, coords=xy, grad=True, perturbed=True)
        fm, fr = gr.distances(g32, g)
        if gr.FACTOR * fm <= gr.CAP_MAX and gr.FACTOR * fr <= gr.CAP_RMS:
            break
    return draw, xy, val, g, (fm, fr)


def coords_of(c: Case) -> np.ndarray:
    return _grad_draw(c)[1] if c.form == "grad" else _draw(c, 0)



@functools.lru_cache(maxsize=None)
def _ref(c: Case, dtype):
    if c.form == "grad" and dtype == np.float64:
        out = _grad_draw(c)[2]
    else:
        out = evaluate(c, dtype)[0]
    out.setflags(write=False)
    return out


def ref64(c: Case) -> np.ndarray:
    return _ref(c, np.float64)


def grad64(c: Case) -> np.ndarray:
    return _grad_draw(c)[3]


def draw_of(c: Case) -> int:
    return _grad_draw(c)[0]


def e32(c: Case) -> float:
    return nerr(_ref(c, np.float32), ref64(c))


@functools.lru_cache(maxsize=None)
def l0_floor(c: Case) -> float:
    """nerr of the native trunk's documented arithmetic restated on the CPU -- layer 0 and its activation in fp32, the rest in fp64 -- from
    the fp64 reference (the module's docstring: the native family's fallback floor)."""
    assert c.form == "native" and not c.residual
    sd, m, xy = state_dict(c), mods(c), coords_of(c)
    f32, f64 = np.float32, np.float64
    c0 = c.w0_initial / (2.0 * np.pi)
    W0 = sd["net.layers.0.weight"].astype(f64)
    w_row, w_col = (W0[:, 0] * c0).astype(f32), (W0[:, 1] * c0).astype(f32)   # weights_pack.hip: the l0 rows
    b0 = (sd["net.layers.0.bias"].astype(f64) * c0).astype(f32) if c.use_bias else np.zeros(c.H, f32)
    cg0 = f32(-0.5 * np.log2(np.e) * (2.0 * np.pi / c.w0_initial) ** 2)
    out = np.zeros(c.T, f64)
    for b, lo, hi in patches(c):
        x, y = xy[lo:hi, 0:1].astype(f64), xy[lo:hi, 1:2].astype(f64)
        # fma in fp32: the product of two fp32 numbers is exact in fp64, the sum is rounded once more there (2^-53: nothing beside 2^-24)
        inner = (x * w_row.astype(f64) + b0.astype(f64)).astype(f32)
        r = (y * w_col.astype(f64) + inner.astype(f64)).astype(f32)
        a = np.sin(2.0 * np.pi * r.astype(f64)).astype(f32)
        if c.act == "morlet":
            a = a * np.exp2((cg0 * r) * r).astype(f32)
        h = a.astype(f64) * m[0, b].astype(f64)
        for l in range(1, c.L):
            p = h @ sd[f"net.layers.{l}.weight"].astype(f64).T
            if c.use_bias:
                p = p + sd[f"net.layers.{l}.bias"].astype(f64)
            a = np.sin(c.w0 * p) * (np.exp(-0.5 * p * p) if c.act == "morlet" else 1.0)
            h = a * m[l, b].astype(f64)
        p = h @ sd["net.last_layer.weight"].astype(f64).T
        if c.use_bias:
            p = p + sd["net.last_layer.bias"].astype(f64)
        out[lo:hi] = np.sin(c.w0 * p)[:, 0]
    return nerr(out, ref64(c))


# ---- the gates ---------------------------------------------------------------------------------------------------------------------------
def distance(c: Case, out):
    """(nerr, rms) as trunk_cases.distance: max|out - ref| / max|ref| and the rms of out - ref"""
    out = np.asarray(out).reshape(c.T)
    return nerr(out, ref64(c)), rms(out, ref64(c))


def floor(c: Case) -> float:
    return l0_floor(c) if (c.form == "native" and NATIVE_FLOOR == "l0_floor") else e32(c)


def tolerance(c: Case, exact=False):
    """exact: the gate of the exact-fp32 kernels on a native case's inputs (always e32)"""
    return min(TOL, max(FLOOR_FACTOR * (e32(c) if exact else floor(c)), ABS_TERM)), RMS_TOL


def passes(c: Case, out) -> bool:
    (e, r), (te, tr) = distance(c, out), tolerance(c)
    return bool(np.isfinite(out).all() and e <= te and r <= tr)


def grad_floor(c: Case):
    return _grad_draw(c)[4]


def grad_tolerance(c: Case):
    fm, fr = grad_floor(c)
    return min(gr.FACTOR * fm, gr.CAP_MAX), min(gr.FACTOR * fr, gr.CAP_RMS)


def grad_distance(c: Case, g):
    return gr.distances(np.asarray(g).reshape(2, c.T), grad64(c))


# ---- mutants built from the reference alone (tests/test_coordset_cases.py: each lies far outside the gate) -------------------------------
def next_patch_rows(c: Case) -> dict:
    """patch -> the next patch that holds coordinates (cyclic): the search picking a neighbour"""
    ps = [b for b, _, _ in patches(c)]
    return {b: ps[(i + 1) % len(ps)] for i, b in enumerate(ps)}


def chunks_rotated(c: Case, ref) -> np.ndarray:
    """every set of more than one chunk with its chunks rotated by one (a wrong chunk offset): output i of the set is the reference's
    output i + chunk"""
    out = np.array(ref)
    for _, lo, hi in patches(c):
        if hi - lo > c.chunk:
            out[..., lo:hi] = np.roll(out[..., lo:hi], -c.chunk, axis=-1)
    return out


def scaled_modulation_max(c: Case) -> float:
    """Largest |m * 2^-a_next| the native trunk stages over the patches that hold coordinates (weights_pack.hip: pack_trunk_f16x3, as
    trunk_cases.scaled_modulation_max states it)."""
    sd, m = state_dict(c), mods(c)
    live = [b for b, _, _ in patches(c)]
    worst = 0.0
    for l in range(c.L):
        a = 0
        if l + 1 < c.L:
            w = sd[f"net.layers.{l + 1}.weight"].astype(np.float64) * (c.w0 / (2.0 * np.pi))
            rmsw, mx = float(np.sqrt(np.mean(w * w))), float(np.abs(w).max())
            a = int(np.floor(np.log2(0.1 / rmsw) + 0.5))
            a = max(-14, min(a, int(np.floor(np.log2(32768.0 / mx))), 30))
        worst = max(worst, float(np.abs(m[l, live]).max()) * 2.0 ** -a)
    return worst


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _k(family, *args):
    return f"siren_trunk_{family}_kernel<{','.join(str(a) for a in args)}>"


_OPT = dict(w0=1.5, w0_initial=20.0)

# f32_ragged<HP,ACT,RES>, all 16: a padded width and the full one per HP alternating as trunk_cases.F32 does, three or four layers;
# instances 1 and 10 without biases, 7 and 12 with w0 = 1.5, w0_initial = 20
_WIDTHS = {128: (100, 128), 256: (200, 256), 384: (300, 384), 512: (400, 512)}
F32_RAGGED = []
for _i, _hp in enumerate((128, 256, 384, 512)):
    for _a in (0, 1):
        for _r in (0, 1):
            _n = 4 * _i + 2 * _a + _r
            F32_RAGGED.append(Case(kernel=_k("f32_ragged", _hp, _a, _r), H=_WIDTHS[_hp][(_a + _r) % 2], L=3 + (_a + _i) % 2, act=ACTS[_a],
                                   residual=bool(_r), use_bias=_n not in (1, 10), **(_OPT if _n in (7, 12) else {}), counts=EDGES(64),
                                   sd_seed=30 + _n, mod_seed=130 + _n, coord_seed=230 + _n))
_F32_256 = next(c for c in F32_RAGGED if c.kernel == _k("f32_ragged", 256, 0, 0))
F32_RAGGED.append(replace(_F32_256, H=256, counts=MANY(64), mod_seed=150, coord_seed=250))  # (the instance's full width: EDGES has 200)

# f32_jet_ragged<HP,ACT>, all 4: widths 100 and 128 at HP 128, 256 and 200 at HP 256; one without biases, one with w0 = 1.5, w0_initial = 20
JET_RAGGED = [
    Case(kernel=_k("f32_jet_ragged", 128, 0), form="grad", H=100, L=3, act="sine", counts=EDGES(32), sd_seed=50, mod_seed=160, coord_seed=260),
    Case(kernel=_k("f32_jet_ragged", 128, 1), form="grad", H=128, L=4, act="morlet", use_bias=False, counts=EDGES(32), sd_seed=51, mod_seed=161,
         coord_seed=261),
    Case(kernel=_k("f32_jet_ragged", 256, 0), form="grad", H=256, L=5, act="sine", counts=EDGES(32), sd_seed=52, mod_seed=162, coord_seed=262),
    Case(kernel=_k("f32_jet_ragged", 256, 1), form="grad", H=200, L=2, act="morlet", **_OPT, counts=EDGES(32), sd_seed=53, mod_seed=163,
         coord_seed=263),
]
JET_RAGGED.append(replace(JET_RAGGED[2], counts=MANY(32), mod_seed=164, coord_seed=264))

# f16x3n_ragged<ACT,R,LFIX>, all 6, at the depth edges of each: <a,3,5> L = 5; <a,4,0> L = 2 and 4; <a,3,0> L = 6 and 11.  Morlet with
# w0 = 1.5, w0_initial = 20 and no biases (the computed layer 0: cg0 against cg, rows without b) on <1,4,0> and <1,3,5>; modulations with
# exact zeros; the MANY set
_N = dict(precision="f16x3", form="native", H=256, counts=EDGES(32))
NATIVE = []
for _a, _act in enumerate(ACTS):
    NATIVE += [Case(kernel=_k("f16x3n_ragged", _a, 3, 5), L=5, act=_act, sd_seed=60, mod_seed=170 + _a, coord_seed=270 + _a, **_N),
               Case(kernel=_k("f16x3n_ragged", _a, 4, 0), L=2, act=_act, sd_seed=61, mod_seed=172 + _a, coord_seed=272 + _a, **_N),
               Case(kernel=_k("f16x3n_ragged", _a, 4, 0), L=4, act=_act, sd_seed=62, mod_seed=174 + _a, coord_seed=274 + _a, **_N),
               Case(kernel=_k("f16x3n_ragged", _a, 3, 0), L=6, act=_act, sd_seed=63, mod_seed=176 + _a, coord_seed=276 + _a, **_N),
               Case(kernel=_k("f16x3n_ragged", _a, 3, 0), L=11, act=_act, sd_seed=64, mod_seed=178 + _a, coord_seed=278 + _a, **_N)]
_SINE_L5 = NATIVE[0]
NATIVE += [Case(kernel=_k("f16x3n_ragged", 1, 4, 0), L=3, act="morlet", use_bias=False, **_OPT, sd_seed=65, mod_seed=180, coord_seed=280, **_N),
           Case(kernel=_k("f16x3n_ragged", 1, 3, 5), L=5, act="morlet", use_bias=False, **_OPT, sd_seed=66, mod_seed=181, coord_seed=281, **_N),
           replace(_SINE_L5, zero_fraction=0.3, mod_seed=182, coord_seed=282),
           replace(_SINE_L5, counts=MANY(32), mod_seed=183, coord_seed=283)]

# f32_ragged_cond<ACT>, both, as guard cases: sine behind <0,3,5>, Morlet behind a loop form (<1,3,0>, L = 7); the sine one on the MANY set
# as well (ragged_items_kernel<32> and then <64> write the same prefix buffer behind one another).  Guard elements sit in patches that
# hold coordinates: EDGES(64) 3, 5, 9; MANY(64) 255, 256, 299
_G = dict(precision="f16x3", form="native", H=256)
GUARDS = [
    Case(kernel=_k("f32_ragged_cond", 0), trunk=_k("f16x3n_ragged", 0, 3, 5), L=5, act="sine", counts=EDGES(64), sd_seed=70, mod_seed=190,
         coord_seed=290, guard=((1, 3, 17), (4, 5, 200), (4, 9, 3)), **_G),
    Case(kernel=_k("f32_ragged_cond", 1), trunk=_k("f16x3n_ragged", 1, 3, 0), L=7, act="morlet", counts=EDGES(64), sd_seed=71, mod_seed=191,
         coord_seed=291, guard=((3, 3, 17), (6, 5, 200), (6, 9, 3)), **_G),
    Case(kernel=_k("f32_ragged_cond", 0), trunk=_k("f16x3n_ragged", 0, 3, 5), L=5, act="sine", counts=MANY(64), sd_seed=70, mod_seed=192,
         coord_seed=292, guard=((1, 255, 17), (4, 256, 200), (4, 299, 3)), **_G),
]

CASES = F32_RAGGED + JET_RAGGED + NATIVE + GUARDS
assert len({c.id for c in CASES}) == len(CASES)
assert all(c.T <= 700 and c.NP <= 300 for c in CASES) and all(c.many or (7 <= c.NP <= 11 and c.T <= 400) for c in CASES)
assert all(c.counts[b] > 0 for c in GUARDS for _, b, _ in c.guard)
