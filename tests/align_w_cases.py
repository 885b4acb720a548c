"""The cases of msiren_align_slices_w and msiren_align_solve_w shared by tests/test_align_w_reference.py (CPU),
tests/test_gpu_align_w.py and tests/test_gpu_align_solve_w.py.  Not a test module; no GPU needed.

The cost call: tests/align_cases.py's stack, models, lattices, maps and targets, with smooth weights in (0, 1] that carry a block of zeros, and
one (g, b) per slice.  The gate is section 5.10's construction on the 47 sums: errors per sum on the scale sum|term|, D the largest error of
the reference's own perturbed-fp32 variant, the device within min(4 D, 1e-4), count exact.

The solve: tests/align_solve_cases.py's lattice, start and true maps.  The targets are T = g_t W + b_t with W the warped planes at the true
map, the weights smooth in (0, 1] with a zero block, and the target corrupted by a large constant inside that block (what the weights are
for).  The loop starts at (g, b) = (1, 0).
"""
import functools

import numpy as np

import align_cases as ac
import align_reference as ar
import align_solve_cases as sc
import align_w_reference as awr
import volume_cases as vc
from mri_inr_amd import align

FACTOR, CAP = ac.FACTOR, ac.CAP
N, HW = ac.N, ac.HW
MODELS, LATTICES = ac.MODELS, ac.LATTICES
INTENSITY = np.array([[1.25, 0.1], [0.8, -0.05], [1.1, 0.03], [0.9, -0.02]], np.float32)


def weights(shape):
    """smooth in (0, 1], a different bump per slice; a block of zeros in slices 1 and 2"""
    th, tw = shape
    i, j = np.mgrid[0:th, 0:tw]
    w = np.stack([0.15 + 0.85 * np.exp(-(((i - 0.5 * th - s) / (0.45 * th)) ** 2 + ((j - 0.4 * tw + s) / (0.5 * tw)) ** 2)) for s in range(N)]).astype(np.float32)
    w[1, 7:11, 2:8] = 0.0
    w[2, 2:5, 10:15] = 0.0
    assert w.max() <= 1.0 and w[w != 0].min() > 0.1
    return w


@functools.lru_cache(maxsize=None)
def variant_planes(model, shape):
    """the planes of the reference's perturbed-fp32 variant (tests/align_cases.py keeps its sums only)"""
    return ac.reference(model, shape, np.float32, perturbed=True)[2]


@functools.lru_cache(maxsize=None)
def data(model, shape):
    """one case: maps, targets, weights, intensity, the fp64 reference (sums, magnitudes, planes), the reference's own distance D and the gate"""
    planes, tg, w = ac.data(model, shape)["planes"], ac.targets(shape), weights(shape)
    sums, mags = awr.align(planes, tg, w, INTENSITY)
    s32, _ = awr.align(variant_planes(model, shape), tg, w, INTENSITY)
    assert np.array_equal(s32[:, 0], sums[:, 0])  # the same pixels are valid
    D = float(ac.scaled_errors(s32, sums, mags).max())
    return dict(maps=ac.maps(shape), targets=tg, weights=w, intensity=INTENSITY, sums=sums, mags=mags, planes=planes, variant=s32, D=D, gate=min(FACTOR * D, CAP))


def accepts(d, sums):
    """the gate of case ``d`` on device sums (n, 47): the count exact, every other sum within the gate on its scale"""
    sums = np.asarray(sums, np.float64)
    return bool(np.array_equal(sums[:, 0], d["sums"][:, 0]) and (ac.scaled_errors(sums, d["sums"], d["mags"]) <= d["gate"]).all())


def packed(res):
    """an AlignResultW back as (n, 47)"""
    iu = np.triu_indices(8)
    return np.concatenate([res.count[:, None].astype(np.float64), res.wsum[:, None], res.cost[:, None], res.grad, res.jtj[:, iu[0], iu[1]]], axis=1)


# ---- the solve --------------------------------------------------------------------------------------------------------------------------------------
SHAPE, CENTRE, ITERATIONS, BLACK = sc.SHAPE, sc.CENTRE, 16, sc.BLACK
MODES = [(mode, est) for mode in sc.MODES for est in (align.FIXED, align.ESTIMATE)]  # (geometry, intensity_mode)
GB_TRUTH = np.array([[1.25, 0.1], [0.8, -0.05], [1.1, 0.03], [0.9, -0.02]], np.float32)
BLOCK = (slice(5, 9), slice(6, 12))  # where the weights are zero and the target is corrupted
CORRUPTION = 5.0
GATE_SLICES = {"sine5": (0, 1), "morlet3": (0, 1, 2)}  # chosen on the CPU (tests/test_align_w_reference.py): sine5 slice 2 stalls at a cover edge (section 5.11)
REACHED = 4.1e-8    # what the fp64 loop reaches on the gate slices, over the 8 parameters
D_ASSERTED = 1e-6   # what tests/test_align_w_reference.py asserts of the variant loop's distance


def options(mode, est, iterations=ITERATIONS, **kw):
    return align.SolveOptionsW(mode=mode, iterations=iterations, centre=CENTRE, intensity_mode=est, **kw)


def solve_weights():
    th, tw = SHAPE
    i, j = np.mgrid[0:th, 0:tw]
    w = np.stack([0.2 + 0.8 * np.exp(-(((i - 0.5 * th) / (0.6 * th)) ** 2 + ((j - 0.5 * tw - s) / (0.6 * tw)) ** 2)) for s in range(N)]).astype(np.float32)
    w[(slice(None),) + BLOCK] = 0.0
    return w


def targets_of(warped, corrupted=True):
    """planes (n, th, tw) at the truth -> float32 targets g_t W + b_t (an uncovered pixel stays NaN: masked), the block corrupted"""
    W = np.asarray(warped, dtype=np.float64).reshape((N,) + SHAPE)
    t = GB_TRUTH[:, 0].astype(np.float64)[:, None, None] * W + GB_TRUTH[:, 1].astype(np.float64)[:, None, None]
    if corrupted:
        t[(slice(None),) + BLOCK] += CORRUPTION
    return t.astype(np.float32)


def errors(maps, intensity, slices=slice(None)):
    """the largest |parameter - truth| per slice over the 8 parameters"""
    got = np.concatenate([np.asarray(maps, np.float64), np.asarray(intensity, np.float64)], axis=1)
    want = np.concatenate([sc.truth().astype(np.float64), GB_TRUTH.astype(np.float64)], axis=1)[slices]
    return np.abs(got - want).max(axis=1)


def reference_cost(model, dtype=np.float64, perturbed=False):
    """-> run(maps, intensity, targets, weights, slices) -> sums (n, 47) of the reference in that arithmetic"""
    base = sc.reference_cost(model, dtype, perturbed)

    def run(maps, intensity, targets, w, slices=range(N)):
        planes = base(maps, targets, slices)[2]
        return awr.align(planes, targets, w, intensity)[0]

    return run


@functools.lru_cache(maxsize=None)
def reference_targets(model, corrupted=True):
    return targets_of(sc.reference_cost(model)(sc.truth(), np.zeros((N,) + SHAPE, np.float32))[2][0], corrupted)


@functools.lru_cache(maxsize=None)
def reference_solve(model, mode, est, variant=False):
    """solve_on_host_w on the fp64 reference (variant: on its perturbed-fp32 variant), from (g, b) = (1, 0) in estimate mode and from the true
    (g, b) in fixed mode -> (SolveResultW with trace, rigid states, the sums of every evaluation (iterations, n, 47))"""
    run, tg, w, seen = reference_cost(model, np.float32 if variant else np.float64, variant), reference_targets(model), solve_weights(), []

    def cost_fn(maps, gb):
        seen.append(run(maps, gb, tg, w))
        return seen[-1]

    res, rigid = align.solve_on_host_w(cost_fn, N, maps=sc.start_maps(), rigid=sc.start_rigid(), intensity=start_intensity(est), options=options(mode, est), trace=True)
    return res, rigid, np.stack(seen)


def start_intensity(est):
    return None if est == align.ESTIMATE else GB_TRUTH


@functools.lru_cache(maxsize=None)
def D(model):
    """the variant loop's largest final error over the gate slices, both geometry modes, intensity estimated"""
    out = 0.0
    for mode in sc.MODES:
        res = reference_solve(model, mode, align.ESTIMATE, True)[0]
        out = max(out, float(errors(res.maps, res.intensity)[list(GATE_SLICES[model])].max()))
    return out


def resolution():
    """the fp32 resolution of the 8 parameters: 8 ulp of the largest"""
    return 8.0 * 2.0 ** -23 * float(max(np.abs(sc.truth()).max(), np.abs(GB_TRUTH).max()))


def gate(model):
    return max(4.0 * D(model), resolution())


def device_gate():
    """gate(model) without running the CPU loops: with D <= D_ASSERTED, 4 D is below the fp32 resolution of the parameters"""
    assert 4.0 * D_ASSERTED <= resolution()
    return resolution()


def replay(trace, sums_of_trial, mode, est, maps=None, rigid=None, intensity=None):
    """The host-loop identity on a trace (iterations, n, 11): from the start, ``lm_step_w`` on ``sums_of_trial(k)`` (n, 47), the sums at the traced
    trial (map, g, b) of evaluation k, has to produce the traced trial of evaluation k + 1, bit for bit.  -> (the first (k, slice) that differs or
    None, the final states)"""
    o, n = options(mode, est, iterations=len(trace)), trace.shape[1]
    st = [align.lm_init_w(o, None if maps is None else maps[s], None if rigid is None else rigid[s], None if intensity is None else intensity[s]) for s in range(n)]
    for k in range(len(trace)):
        for s in range(n):
            if not np.array_equal(np.array(st[s]["trial"] + st[s]["gb_trial"], np.float32), trace[k, s, :8].astype(np.float32), equal_nan=True):
                return (k, s), st
        sums = sums_of_trial(k)
        for s in range(n):
            align.lm_step_w(st[s], sums[s], k, o)
    return None, st
