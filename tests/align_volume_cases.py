"""The cases of msiren_align_volume and msiren_align_volume_solve shared by tests/test_align_volume_reference.py (CPU),
tests/test_gpu_align_volume.py and tests/test_gpu_align_volume_solve.py, with their fp64 reference and the gates.  Not a test module; no GPU needed.

The stack is tests/volume_cases.py's: n = 4 slices of 40 x 40 (3 x 3 tiles each, covered over [-4, 51]), slice 1 with its upper row of tiles black,
slice 3 black; the models are tests/align_cases.py's.  m = 7 targets, one kind of map each (m is not n):
    0  a flat plane at Z = 0.37 with a fractional in-plane offset          4  a plane inside the segment 2 .. 3: it reads the black slice
    1  a flat plane at Z = 2                                               5  an anisotropic in-plane map that leaves every cover
    2  a tilted plane, Z from 0.6 to 2.6 (it crosses Z = 1 and Z = 2),      6  a flat plane at Z = 1.5 whose target has a block of NaN pixels
       rotated by 7 degrees in the plane
    3  a tilted plane that leaves the stack: Z from -0.4 to 1.6
Every product a i is zero or a normal fp32 number (no map entry below 1e-3 in magnitude but exact zeros).

The gate of the sums is tests/align_cases.py's: per sum the error against the sum of the magnitudes of its terms; D the largest such error of the
reference's perturbed-fp32 variant over the case; the device within min(4 D, 1e-4) on that scale, the count exact.

The solve cases (SOLVE_*): lattice 19 x 23, slices 4 pixels apart, four targets on nominal planes e_i = (0, 1, 0), e_j = (0, 0, 1), o = (4 z, 10, 8)
with z = 0.6, 1.3, 1.0, 0.4, rotated about c = o + (0, 9, 11).  The truth is a rotation by a vector of 0.25 .. 1.5 degrees and a shift of at most
0.45 pixels; the targets are the reference's warped planes at the truth; every target starts on its nominal plane; 20 evaluations.  What the
normative rule (align_volume.lm_step_v, ldl_solve) reaches on the fp64 reference is recorded in REACHED and GATE_TARGETS below.
"""
import functools

import numpy as np

import align_cases as ac
import align_volume_reference as avr
import volume_cases as vc
from mri_inr_amd import align, align_volume as av

FACTOR, CAP = 4.0, 1e-4
N, HW = vc.N, 40
M = 7
MODELS = ac.MODELS
LATTICES = ac.LATTICES  # (19, 23): one ragged chunk; (47, 45): chunks of 1024, 1024, 67
state_dict, stack_mods, scaled_errors = ac.state_dict, ac.stack_mods, ac.scaled_errors


def maps(shape):
    th, tw = shape
    centre = ((th - 1) / 2, (tw - 1) / 2)
    rot = align.rigid_maps(np.deg2rad(7.0), (19.3 - centre[0], 20.6 - centre[1]), centre)[0]
    return np.array([[0.0, 0.0, 0.37, 1.0, 0.0, 0.37, 0.0, 1.0, 1.61],
                     [0.0, 0.0, 2.0, 1.0, 0.0, 1.25, 0.0, 1.0, 2.5],
                     [1.7 / (th - 1), 0.3 / (tw - 1), 0.6] + rot.tolist(),
                     [1.5 / (th - 1), 0.5 / (tw - 1), -0.4, 1.0, 0.0, 2.25, 0.0, 1.0, 0.75],
                     [0.3 / (th - 1), 0.2 / (tw - 1), 2.35, 0.9, 0.1, 3.3, -0.1, 0.9, 5.2],
                     [0.4 / (th - 1), 0.5 / (tw - 1), 0.8, 1.37, 0.013, -7.3, -0.021, 0.81, 2.2],
                     [0.0, 0.0, 1.5, 1.0, 0.0, 0.61, 0.0, 1.0, 0.43]], np.float32)


def targets(shape):
    """smooth images in [0.1, 0.9]; a block of NaN pixels (a mask) in the last one"""
    th, tw = shape
    i, j = np.mgrid[0:th, 0:tw]
    t = np.stack([0.5 + 0.4 * np.sin(0.21 * i + 0.5 * q) * np.cos(0.17 * j - 0.3 * q) for q in range(M)]).astype(np.float32)
    t[6, 3:6, 4:9] = np.nan
    return t


@functools.lru_cache(maxsize=None)
def _cache(model, dtype_name, perturbed):
    return {}


def reference(model, shape, dtype=np.float64, perturbed=False, seed=None, map_rows=None, target_rows=None):
    mods, black = stack_mods(model, np.dtype(dtype).name)
    return avr.align_volume_of_stack(state_dict(model), mods, black, maps(shape) if map_rows is None else map_rows,
                                     targets(shape) if target_rows is None else target_rows, vc.NV, vc.NH, vc.S, vc.I, num_layers=MODELS[model]["L"],
                                     activation=MODELS[model]["act"], dtype=dtype, perturbed=perturbed, seed=seed,
                                     cache=_cache(model, np.dtype(dtype).name, perturbed))


@functools.lru_cache(maxsize=None)
def data(model, shape):
    """one case: maps, targets, the fp64 reference (sums, magnitudes, planes), the reference's own distance D and the gate"""
    sums, mags, planes = reference(model, shape)
    s32, _, _ = reference(model, shape, np.float32, perturbed=True)
    assert np.array_equal(s32[:, 0], sums[:, 0])  # the same pixels are valid
    D = float(scaled_errors(s32, sums, mags).max())
    return dict(maps=maps(shape), targets=targets(shape), sums=sums, mags=mags, planes=planes, variant=s32, D=D, gate=min(FACTOR * D, CAP))


def accepts(d, sums):
    """the gate of case ``d`` on device sums (m, 56): the count exact, every other sum within the gate on its scale"""
    sums = np.asarray(sums, np.float64)
    return bool(np.array_equal(sums[:, 0], d["sums"][:, 0]) and (scaled_errors(sums, d["sums"], d["mags"]) <= d["gate"]).all())


def mutant_sums(model, shape, seed):
    """the sums of the seeded mutant on the case's own planes (SEEDS), or on the reference with the pair misread (VOLUME_SEEDS)"""
    d = data(model, shape)
    if seed in avr.VOLUME_SEEDS:
        return reference(model, shape, seed=seed)[0]
    pl, out = d["planes"], []
    for q in range(M):
        valid_z = avr.vr.pairs(avr.points(d["maps"][q], shape), N)[0] >= 0
        out.append(avr.sums_of_planes(pl[0, q], pl[1, q], pl[2, q], pl[3, q], d["targets"][q], shape, seed, valid_z)[0])
    return np.stack(out)


# ---- the solve -------------------------------------------------------------------------------------------------------------------------------------
SOLVE_SHAPE = (19, 23)
SPACING = 4.0
SOLVE_M = 4
SOLVE_ITERATIONS = 20
_Z = (0.6, 1.3, 1.0, 0.4)
ROTVECS = 0.5 * np.deg2rad(np.array([[1.5, 2.0, -1.5], [-2.0, -1.0, 2.5], [1.0, 3.0, 1.0], [0.5, 0.5, 0.5]]))
SHIFTS3 = 0.5 * np.array([[0.3, 0.8, -0.6], [-0.3, -0.5, 0.7], [0.3, 0.3, 0.9], [-0.3, 0.2, 0.2]])
MODES = (align.AFFINE, align.RIGID)
# What solve_on_host_v reaches on the fp64 reference after SOLVE_ITERATIONS evaluations (the largest |map - truth| over the nine entries, Z entries
# in slice units), measured with the normative rule; tests/test_align_volume_reference.py asserts it.  sine5 target 2 (its lattice crosses Z = 1
# over slice 1's black tile row) stalls in both modes and is no gate target; morlet3 target 2 crosses Z = 1 and converges.
REACHED = 5e-7  # (half an fp32 ulp of the largest map entries, those between 8 and 16: morlet3 target 0 in affine mode ends there, the others lower)
GATE_TARGETS = {"sine5": (0, 1, 3), "morlet3": (0, 1, 2, 3)}
D_SOLVE_ASSERTED = 1e-6  # what tests/test_align_volume_reference.py asserts of the variant loop's D_solve


def planes():
    """(4, 12) float64 = (e_i, e_j, o, c)"""
    out = np.zeros((SOLVE_M, 12))
    for q, z in enumerate(_Z):
        o = np.array([SPACING * z, 10.0, 8.0])
        out[q] = np.concatenate([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], o, o + np.array([0.0, 9.0, 11.0])])
    return out


def rotation_of(vec):
    """Rodrigues' formula, fp64"""
    vec = np.asarray(vec, np.float64)
    t = np.linalg.norm(vec)
    if t == 0:
        return np.eye(3)
    k = vec / t
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def truth_rotations():
    return np.stack([rotation_of(v) for v in ROTVECS])


def truth():
    return av.rigid_maps3(truth_rotations(), SHIFTS3, planes(), SPACING)


def start_maps():
    return av.rigid_maps3(np.eye(3), np.zeros(3), planes(), SPACING)


def start_rigid():
    """(4, 12) = (Rot, u) of the start: the nominal plane"""
    return np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (SOLVE_M, 1))


def solve_options(mode, iterations=SOLVE_ITERATIONS, **kw):
    return av.SolveOptionsV(mode=mode, iterations=iterations, spacing=SPACING, **kw)


def solve_errors(maps_, rows=slice(None)):
    """the largest |map - truth| per target (maps_: those of ``rows``)"""
    return np.abs(np.asarray(maps_, np.float64) - truth().astype(np.float64)[rows]).max(axis=1)


def crosses_an_integer_z(q):
    z = av.map_points3(truth()[q], SOLVE_SHAPE)[:, 0]
    return bool(np.floor(z.min()) != np.floor(z.max()))


def reference_cost(model, dtype=np.float64, perturbed=False):
    """-> run(maps, targets) -> (sums (m, 56), magnitudes, planes (4, m, th, tw)) of the reference in that arithmetic"""
    def run(maps_, targets_):
        return reference(model, SOLVE_SHAPE, dtype, perturbed, map_rows=np.asarray(maps_, np.float32), target_rows=targets_)

    return run


@functools.lru_cache(maxsize=None)
def reference_targets(model):
    """the fp64 reference's warped planes at the truth as float32 targets (an uncovered pixel stays NaN: masked)"""
    return np.asarray(reference_cost(model)(truth(), np.zeros((SOLVE_M,) + SOLVE_SHAPE, np.float32))[2][0], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def reference_solve(model, mode, variant=False):
    """solve_on_host_v on the fp64 reference (variant: on its perturbed-fp32 variant) -> (SolveResultV with trace, rigid states, the sums of
    every evaluation (iterations, m, 56))"""
    run, tg, seen = reference_cost(model, np.float32 if variant else np.float64, variant), reference_targets(model), []

    def cost_fn(maps_):
        seen.append(run(maps_, tg)[0])
        return seen[-1]

    res, rigid = av.solve_on_host_v(cost_fn, SOLVE_M, maps=start_maps(), rigid=start_rigid(), planes=planes(), options=solve_options(mode), trace=True)
    return res, rigid, np.stack(seen)


@functools.lru_cache(maxsize=None)
def D_solve(model):
    """the variant loop's largest final error over the gate targets and both modes"""
    return float(max(solve_errors(reference_solve(model, mode, True)[0].maps)[list(GATE_TARGETS[model])].max() for mode in MODES))


def solve_gate(model):
    """the convergence gate of the device: 4 D_solve, or the fp32 resolution of the map entries (8 ulp of the largest) where that is larger"""
    return max(4.0 * D_solve(model), 8.0 * 2.0 ** -23 * float(np.abs(truth()).max()))


def device_solve_gate():
    """solve_gate(model) without running the CPU loops: with D_solve <= D_SOLVE_ASSERTED, 4 D_solve is below the fp32 resolution of the map entries,
    so the gate is that resolution for either model (tests/test_align_volume_reference.py asserts the two are equal)"""
    g = 8.0 * 2.0 ** -23 * float(np.abs(truth()).max())
    assert 4.0 * D_SOLVE_ASSERTED <= g
    return g


def replay(trace, sums_of_trial, mode, maps_=None, rigid=None, planes_=None):
    """The host-loop identity on a trace (iterations, m, 11): from the start, ``lm_step_v`` on ``sums_of_trial(k)`` (m, 56), the sums at the traced
    trial maps of evaluation k, has to produce the traced trial map of evaluation k + 1, bit for bit.  -> (the first (k, target) that differs or
    None, the final states)"""
    o, m = solve_options(mode, iterations=len(trace)), trace.shape[1]
    st = [av.lm_init_v(o, None if maps_ is None else maps_[q], None if rigid is None else rigid[q], None if planes_ is None else planes_[q]) for q in range(m)]
    for k in range(len(trace)):
        for q in range(m):
            if not np.array_equal(np.array(st[q]["trial"], np.float32), trace[k, q, :9].astype(np.float32), equal_nan=True):
                return (k, q), st
        sums = sums_of_trial(k)
        for q in range(m):
            av.lm_step_v(st[q], sums[q], k, o)
    return None, st
