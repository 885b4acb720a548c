"""The cases of msiren_align_volume_r and msiren_align_volume_solve_group_r shared by tests/test_align_robust_reference.py
(CPU) and tests/test_gpu_align_robust.py.  Not a test module; no GPU needed.

The cost call: tests/align_volume_w_cases.py's stack, models, lattices, maps, targets, weights and (g, b) (m = 7), with one scale per target drawn
from {+inf, 0.01, 1.0, 2^-4, 0.0, NaN}: SCALE.  Targets 4 and 5 (scale 0 and NaN) have count 0; target 0 (+inf) has section 5.14's sums.  The gate is
section 5.14's construction on the robust sums: errors per sum on the scale sum|term|, D the largest error of the reference's own perturbed-fp32
variant, the device within min(4 D, 1e-4), count exact.

The solve: tests/align_group_cases.py's planes, groups, truth, corrupted targets and 20 evaluations, its weights with the block set to 1 instead of 0
(the + 5 corruption is NOT masked), scale = 0.01 for every target.  Measured on the CPU with the normative rule (align_group.lm_step_g) on the fp64
reference, the largest |parameter - truth| per group after 20 evaluations (align_group_cases.errors):
                        robust loss, scale 0.01          quadratic loss, the same inputs     the variant's robust loop
    sine5   fixed     3.0e-8  1.2e-7  2.7e-7           0.30   0.68   0.14                 3.0e-8  2.4e-7  7.3e-7
    sine5   estimate  8.9e-8  1.8e-7  7.5e-8           0.38   0.50   0.098                1.7e-7  2.4e-7  9.5e-7
    morlet3 fixed     4.8e-7  6.0e-8  1.5e-7           0.32   0.53   0.58                 8.9e-8  1.8e-7  6.0e-8
    morlet3 estimate  1.2e-7  1.2e-7  2.4e-7           0.38   0.69   0.049                4.8e-7  1.8e-7  1.2e-7
The robust loop reaches align_group_cases.REACHED (5e-7) on EVERY group, so all three are gate groups here (section 5.15 gated 0 and 2); 4.8e-7 is
half an fp32 ulp of a map entry between 8 and 16.  The quadratic loop has to end more than QUADRATIC_AWAY from the truth on every group (0.049 at
least): the case needs the loss.  The variant's robust loop ends within D_solve = 9.5e-7 (sine5) and 4.8e-7 (morlet3) over the gate groups and both
intensity modes.  tests/test_align_robust_reference.py prints all of these; one loop of 20 evaluations on the fp64 reference takes 15 to 30 s.
"""
import functools

import numpy as np

import align_group_cases as gc
import align_robust_reference as arr
import align_volume_cases as avc
import align_volume_w_cases as wc
from mri_inr_amd import align_group as ag, align_robust as ar

FACTOR, CAP = wc.FACTOR, wc.CAP
N, HW, M = wc.N, wc.HW, wc.M
MODELS, LATTICES = wc.MODELS, wc.LATTICES
scaled_errors, packed = wc.scaled_errors, wc.packed
INF = float("inf")
SCALE = np.array([INF, 0.01, 1.0, 2.0 ** -4, 0.0, float("nan"), 0.01], np.float64)  # one per target
UNSCORED = (4, 5)  # the targets whose scale is not > 0


@functools.lru_cache(maxsize=None)
def data(model, shape):
    """one case: section 5.14's inputs and the scales, the fp64 reference (sums, magnitudes, planes, om^2), the reference's own distance D and the gate"""
    d = wc.data(model, shape)
    sums, mags, rw = arr.align(d["planes"], d["targets"], d["weights"], d["intensity"], SCALE, rweight=True)
    s32, _ = arr.align(wc.variant_planes(model, shape), d["targets"], d["weights"], d["intensity"], SCALE)
    assert np.array_equal(s32[:, 0], sums[:, 0])  # the same pixels are valid
    D = float(scaled_errors(s32, sums, mags).max())
    return dict(maps=d["maps"], targets=d["targets"], weights=d["weights"], intensity=d["intensity"], scale=SCALE, sums=sums, mags=mags, planes=d["planes"], rweight=rw,
                variant=s32, D=D, gate=min(FACTOR * D, CAP))


def accepts(d, sums):
    """the gate of case ``d`` on device sums (m, 80): the count exact, every other sum within the gate on its scale"""
    sums = np.asarray(sums, np.float64)
    return bool(np.array_equal(sums[:, 0], d["sums"][:, 0]) and (scaled_errors(sums, d["sums"], d["mags"]) <= d["gate"]).all())


def mutant_sums(model, shape, seed):
    """the sums of the seeded mutant on the case's own planes"""
    d = data(model, shape)
    return arr.align(d["planes"], d["targets"], d["weights"], d["intensity"], SCALE, seed)[0]


# ---- the solve --------------------------------------------------------------------------------------------------------------------------------------
SHAPE, SPACING, SOLVE_M, G = gc.SHAPE, gc.SPACING, gc.M, gc.G
GROUP_START, ITERATIONS, MODES = gc.GROUP_START, gc.ITERATIONS, gc.MODES
SOLVE_SCALE = 0.01
REACHED = gc.REACHED
QUADRATIC_AWAY = 0.01
GATE_GROUPS = (0, 1, 2)
# what tests/test_align_robust_reference.py asserts of the variant loop's D_solve (measured 9.5e-7 at most), chosen as in section 5.15: 4 D_solve stays
# below the fp32 resolution of the parameters (8 ulp of the largest, 1.5e-5), so the device's gate is that resolution
D_SOLVE_ASSERTED = 1e-6


def weights():
    """tests/align_group_cases.py's weights with the block set to 1 instead of 0: nothing masks the corruption"""
    w = gc.weights().copy()
    w[(slice(None),) + wc.BLOCK] = 1.0
    return w


def solve_scale():
    return np.full(SOLVE_M, SOLVE_SCALE, np.float64)


def reference_cost(model, dtype=np.float64, perturbed=False):
    """-> run(maps, intensity, targets, weights, scale) -> sums (m, 80) of the robust reference in that arithmetic, for any number of targets"""
    base = avc.reference_cost(model, dtype, perturbed)

    def run(maps, intensity, targets, w, scale):
        return arr.align(base(maps, targets)[2], targets, w, intensity, scale)[0]

    return run


@functools.lru_cache(maxsize=None)
def reference_solve(model, est, variant=False, robust=True):
    """solve_on_host_r on the fp64 reference (variant: on its perturbed-fp32 variant; robust False: the quadratic loop, solve_on_host_g on section
    5.15's reference with the same unmasked weights) -> (SolveResultG with trace, the final states, the sums of every evaluation (iterations, m, 80))"""
    dtype = np.float32 if variant else np.float64
    tg, w, seen = gc.reference_targets(model), weights(), []
    kw = dict(rigid=gc.start_rigid(), planes=gc.planes(), intensity=gc.start_intensity(est), options=gc.options(est), trace=True)
    if robust:
        run = reference_cost(model, dtype, variant)

        def cost_fn(maps, gb, scale):
            seen.append(run(maps, gb, tg, w, scale))
            return seen[-1]

        res, st = ar.solve_on_host_r(cost_fn, GROUP_START, solve_scale(), **kw)
    else:
        run = gc.reference_cost(model, dtype, variant)

        def cost_fn(maps, gb):
            seen.append(run(maps, gb, tg, w))
            return seen[-1]

        res, st = ag.solve_on_host_g(cost_fn, GROUP_START, **kw)
    return res, st, np.stack(seen)


@functools.lru_cache(maxsize=None)
def D_solve(model):
    """the variant's robust loop's largest final error over the gate groups, both intensity modes"""
    return float(max(gc.errors(reference_solve(model, est, True)[0], est)[list(GATE_GROUPS)].max() for est in MODES))


resolution = gc.resolution


def solve_gate(model):
    return max(4.0 * D_solve(model), resolution())


def device_solve_gate():
    """solve_gate(model) without running the CPU loops: with D_solve <= D_SOLVE_ASSERTED, 4 D_solve is below the fp32 resolution of the parameters"""
    assert 4.0 * D_SOLVE_ASSERTED <= resolution()
    return resolution()
