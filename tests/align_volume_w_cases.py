"""The cases of msiren_align_volume_w and msiren_align_volume_solve_w shared by tests/test_align_volume_w_reference.py
(CPU), tests/test_gpu_align_volume_w.py and tests/test_gpu_align_volume_solve_w.py.  Not a test module; no GPU needed.

The cost call: tests/align_volume_cases.py's stack, models, lattices, maps and targets (m = 7), with smooth weights in (0, 1] that carry a block
of zeros in three targets and one non-finite weight, and one (g, b) per target.  The gate is section 5.10's construction on the 80 sums: errors
per sum on the scale sum|term|, D the largest error of the reference's own perturbed-fp32 variant, the device within min(4 D, 1e-4), count exact.

The solve: tests/align_volume_cases.py's lattice, planes, start and truth.  The targets are T = g_t W + b_t with W the reference's warped planes at
the true map and four distinct (g_t, b_t) (section 5.12's), the weights smooth in (0, 1] with a zero block, and the target corrupted by + 5
inside that block (what the weights are for).  The loop starts at (g, b) = (1, 0) where the intensity is estimated and at the true (g, b) where it
is fixed.  What the normative rule (align_volume.lm_step_vw, ldl_solve) reaches on the fp64 reference is recorded in REACHED and GATE_TARGETS below.
"""
import functools

import numpy as np

import align_volume_cases as avc
import align_volume_w_reference as avwr
from mri_inr_amd import align, align_volume as av

FACTOR, CAP = avc.FACTOR, avc.CAP
N, HW, M = avc.N, avc.HW, avc.M
MODELS, LATTICES = avc.MODELS, avc.LATTICES
scaled_errors = avc.scaled_errors
INTENSITY = np.array([[1.25, 0.1], [0.8, -0.05], [1.1, 0.03], [0.9, -0.02], [1.05, 0.2], [0.95, -0.1], [1.2, 0.05]], np.float32)
NONFINITE_AT = (0, 2, 3)  # target, row, column of the one weight that is not finite


def weights(shape):
    """smooth in (0, 1], a different bump per target; a block of zeros in targets 1, 2 and 6; one NaN weight in target 0"""
    th, tw = shape
    i, j = np.mgrid[0:th, 0:tw]
    w = np.stack([0.15 + 0.85 * np.exp(-(((i - 0.5 * th - q) / (0.45 * th)) ** 2 + ((j - 0.4 * tw + q) / (0.5 * tw)) ** 2)) for q in range(M)]).astype(np.float32)
    w[1, 7:11, 2:8] = 0.0
    w[2, 2:5, 10:15] = 0.0
    w[6, 12:16, 3:7] = 0.0
    assert w.max() <= 1.0 and w[w != 0].min() > 0.1
    w[NONFINITE_AT] = np.nan
    return w


@functools.lru_cache(maxsize=None)
def variant_planes(model, shape):
    """the planes of the reference's perturbed-fp32 variant (tests/align_volume_cases.py keeps its sums only)"""
    return avc.reference(model, shape, np.float32, perturbed=True)[2]


@functools.lru_cache(maxsize=None)
def data(model, shape):
    """one case: maps, targets, weights, intensity, the fp64 reference (sums, magnitudes, planes), the reference's own distance D and the gate"""
    planes, tg, w = avc.data(model, shape)["planes"], avc.targets(shape), weights(shape)
    sums, mags = avwr.align(planes, tg, w, INTENSITY)
    s32, _ = avwr.align(variant_planes(model, shape), tg, w, INTENSITY)
    assert np.array_equal(s32[:, 0], sums[:, 0])  # the same pixels are valid
    D = float(scaled_errors(s32, sums, mags).max())
    return dict(maps=avc.maps(shape), targets=tg, weights=w, intensity=INTENSITY, sums=sums, mags=mags, planes=planes, variant=s32, D=D, gate=min(FACTOR * D, CAP))


def accepts(d, sums):
    """the gate of case ``d`` on device sums (m, 80): the count exact, every other sum within the gate on its scale"""
    sums = np.asarray(sums, np.float64)
    return bool(np.array_equal(sums[:, 0], d["sums"][:, 0]) and (scaled_errors(sums, d["sums"], d["mags"]) <= d["gate"]).all())


def mutant_sums(model, shape, seed):
    """the sums of the seeded mutant on the case's own planes"""
    d = data(model, shape)
    return avwr.align(d["planes"], d["targets"], d["weights"], d["intensity"], seed)[0]


def packed(res):
    """an AlignResultVW back as (m, 80)"""
    iu = np.triu_indices(11)
    return np.concatenate([res.count[:, None].astype(np.float64), res.wsum[:, None], res.cost[:, None], res.grad, res.jtj[:, iu[0], iu[1]]], axis=1)


# ---- the solve --------------------------------------------------------------------------------------------------------------------------------------
SHAPE, SPACING, SOLVE_M = avc.SOLVE_SHAPE, avc.SPACING, avc.SOLVE_M
ITERATIONS = 12  # the fp64 loop is inside 1e-6 of the truth on every gate target after 7 evaluations at most, from (g, b) = (1, 0) too (measured on the CPU)
MODES = [(mode, est) for mode in avc.MODES for est in (av.FIXED, av.ESTIMATE)]  # (geometry, intensity_mode)
GB_TRUTH = np.array([[1.25, 0.1], [0.8, -0.05], [1.1, 0.03], [0.9, -0.02]], np.float32)
BLOCK = (slice(5, 9), slice(6, 12))  # where the weights are zero and the target is corrupted
CORRUPTION = 5.0
# What solve_on_host_vw reaches on the fp64 reference after ITERATIONS evaluations (the largest |parameter - truth| over the nine map entries and
# (g, b)), measured with the normative rule; tests/test_align_volume_w_reference.py asserts it in estimate mode.  Over the gate targets and all
# four modes the largest is 9.5e-7 (one fp32 ulp of the map entries between 8 and 16) but for sine5 target 2, whose lattice crosses Z = 1 over
# slice 1's black tile row: with the intensity FIXED it stalls near 2e-2 in both geometry modes, as in section 5.13, and is no gate target there;
# with the intensity ESTIMATED the fp64 loop does not stall on it (1.1e-6 affine, 2.0e-6 rigid; the variant loop 6.6e-7 / 2.4e-7), so it stays one.
REACHED = 2.5e-6
GATE_TARGETS = {"sine5": {av.FIXED: (0, 1, 3), av.ESTIMATE: (0, 1, 2, 3)}, "morlet3": {av.FIXED: (0, 1, 2, 3), av.ESTIMATE: (0, 1, 2, 3)}}
D_SOLVE_ASSERTED = 1e-6  # what tests/test_align_volume_w_reference.py asserts of the variant loop's D_solve


def gate_targets(model, est):
    return GATE_TARGETS[model][est]


def options(mode, est, iterations=ITERATIONS, **kw):
    return av.SolveOptionsVW(mode=mode, iterations=iterations, spacing=SPACING, intensity_mode=est, **kw)


def solve_weights():
    th, tw = SHAPE
    i, j = np.mgrid[0:th, 0:tw]
    w = np.stack([0.2 + 0.8 * np.exp(-(((i - 0.5 * th) / (0.6 * th)) ** 2 + ((j - 0.5 * tw - q) / (0.6 * tw)) ** 2)) for q in range(SOLVE_M)]).astype(np.float32)
    w[(slice(None),) + BLOCK] = 0.0
    return w


def targets_of(warped, corrupted=True):
    """planes (m, th, tw) at the truth -> float32 targets g_t W + b_t (an uncovered pixel stays NaN: masked), the block corrupted"""
    W = np.asarray(warped, dtype=np.float64).reshape((SOLVE_M,) + SHAPE)
    t = GB_TRUTH[:, 0].astype(np.float64)[:, None, None] * W + GB_TRUTH[:, 1].astype(np.float64)[:, None, None]
    if corrupted:
        t[(slice(None),) + BLOCK] += CORRUPTION
    return t.astype(np.float32)


def errors(maps, intensity, rows=slice(None)):
    """the largest |parameter - truth| per target over the 11 parameters"""
    got = np.concatenate([np.asarray(maps, np.float64), np.asarray(intensity, np.float64)], axis=1)
    want = np.concatenate([avc.truth().astype(np.float64), GB_TRUTH.astype(np.float64)], axis=1)[rows]
    return np.abs(got - want).max(axis=1)


def reference_cost(model, dtype=np.float64, perturbed=False):
    """-> run(maps, intensity, targets, weights) -> sums (m, 80) of the reference in that arithmetic"""
    base = avc.reference_cost(model, dtype, perturbed)

    def run(maps, intensity, targets, w):
        planes = base(maps, targets)[2]
        return avwr.align(planes, targets, w, intensity)[0]

    return run


@functools.lru_cache(maxsize=None)
def reference_targets(model, corrupted=True):
    return targets_of(avc.reference_cost(model)(avc.truth(), np.zeros((SOLVE_M,) + SHAPE, np.float32))[2][0], corrupted)


def start_intensity(est):
    return None if est == av.ESTIMATE else GB_TRUTH


@functools.lru_cache(maxsize=None)
def reference_solve(model, mode, est, variant=False):
    """solve_on_host_vw on the fp64 reference (variant: on its perturbed-fp32 variant), from (g, b) = (1, 0) in estimate mode and from the true
    (g, b) in fixed mode -> (SolveResultVW with trace, rigid states, the sums of every evaluation (iterations, m, 80))"""
    run, tg, w, seen = reference_cost(model, np.float32 if variant else np.float64, variant), reference_targets(model), solve_weights(), []

    def cost_fn(maps, gb):
        seen.append(run(maps, gb, tg, w))
        return seen[-1]

    res, rigid = av.solve_on_host_vw(cost_fn, SOLVE_M, maps=avc.start_maps(), rigid=avc.start_rigid(), planes=avc.planes(), intensity=start_intensity(est),
                                     options=options(mode, est), trace=True)
    return res, rigid, np.stack(seen)


@functools.lru_cache(maxsize=None)
def D_solve(model):
    """the variant loop's largest final error over the gate targets, both geometry modes, intensity estimated"""
    out = 0.0
    for mode in avc.MODES:
        res = reference_solve(model, mode, av.ESTIMATE, True)[0]
        out = max(out, float(errors(res.maps, res.intensity)[list(gate_targets(model, av.ESTIMATE))].max()))
    return out


def resolution():
    """the fp32 resolution of the 11 parameters: 8 ulp of the largest"""
    return 8.0 * 2.0 ** -23 * float(max(np.abs(avc.truth()).max(), np.abs(GB_TRUTH).max()))


def solve_gate(model):
    return max(4.0 * D_solve(model), resolution())


def device_solve_gate():
    """solve_gate(model) without running the CPU loops: with D_solve <= D_SOLVE_ASSERTED, 4 D_solve is below the fp32 resolution of the parameters"""
    assert 4.0 * D_SOLVE_ASSERTED <= resolution()
    return resolution()


def replay(trace, sums_of_trial, mode, est, maps=None, rigid=None, planes=None, intensity=None, step=av.lm_step_vw):
    """The host-loop identity on a trace (iterations, m, 14): from the start, ``lm_step_vw`` on ``sums_of_trial(k)`` (m, 80), the sums at the traced
    trial (map, g, b) of evaluation k, has to produce the traced trial of evaluation k + 1, bit for bit.  -> (the first (k, target) that differs
    or None, the final states)"""
    o, m = options(mode, est, iterations=len(trace)), trace.shape[1]
    st = [av.lm_init_vw(o, None if maps is None else maps[q], None if rigid is None else rigid[q], None if planes is None else planes[q],
                        None if intensity is None else intensity[q]) for q in range(m)]
    for k in range(len(trace)):
        for q in range(m):
            if not np.array_equal(np.array(st[q]["trial"] + st[q]["gb_trial"], np.float32), trace[k, q, :11].astype(np.float32), equal_nan=True):
                return (k, q), st
        sums = sums_of_trial(k)
        for q in range(m):
            step(st[q], sums[q], k, o)
    return None, st
