"""The cases of msiren_solve_volume shared by tests/test_solve_volume_reference.py (CPU) and tests/test_gpu_solve_volume.py.
Not a test module; no GPU and no model needed: pure numpy on top of tests/fuse_cases.py and tests/project_cases.py, small enough that every GPU test
takes seconds.

    planes      fuse_cases.planes(): eight targets (six planes, the DEGENERATE map, the target whose gain is 0) with their weights (a zero block, a
                NaN weight), a NaN pixel and intensities, on both grids, with and without weights and intensity; once at thickness spacing / 4
    graze       fuse_cases.graze(shift) x GRAZE_THICKNESSES: the window's edge and the last row and column on tile-corner voxels, one ulp either side
    identity    flat targets on integer Z with unit maps: P is the identity, the fusion solves the problem, the first residual is exactly 0
    truth       fuse_cases.truth_case(): 24 targets of 44 x 46 that overhang the (4, 40, 40) grid on every side, at both thicknesses
    holes       the planes case with project_cases.holes(grid) given as `start`: a NaN slab, single NaN voxels and an infinity are outside the support
    outside     fuse_cases.outside_target(): no voxel is reached; the support is empty without a start, and with one nothing but the regulariser acts
    none        m = 0, without a start and with one
    flagged     only the DEGENERATE map and the target whose gain is 0
    tiny        five tilted targets of 9 x 11 over (3, 10, 12): small enough for a dense matrix (tests/solve_volume_reference.py)
    tall        (260, 5, 7) from a random start with three small targets: more slices than one workgroup of the inner product's last kernel has
                threads (and than a wave has lanes), a height that is no multiple of its four rows in flight
Every case is solved for ITERATIONS x LAMBDAS.  The expected results of all iteration counts come from ONE run of the restatement with the largest
count: iteration k of a longer run is iteration k of a shorter one (the rule has no look-ahead), so ``expected`` cuts them out of the iterates.

CONSISTENT: the mean |x_k - V| over the support on the truth case with targets = project_on_host(V), V the analytic stack, lambda = 0, k = 0 .. 5, per
thickness, measured from solve_volume_on_host.  POINT_SAMPLES: the same for the point-sample targets of fuse_cases.truth_case() after 0, 1, 5 and 30
iterations (0: fuse_cases.TRUTH_ERRORS; one back-projection step: project_cases.ONE_STEP).  No direction is claimed for the second."""
import functools

import numpy as np

import fuse_cases as fc
import project_cases as pc
from mri_inr_amd import fuse, solve_volume as sv

SPACING, SHAPE, GRIDS, THICKNESSES = fc.SPACING, fc.SHAPE, fc.GRIDS, fc.THICKNESSES
ITERATIONS = (0, 1, 2, 5)
LAMBDAS = (0.0, 0.01)
TINY_GRID, TINY_SHAPE, TINY_M = (3, 10, 12), (9, 11), 5
TALL_GRID, TALL_SHAPE = (260, 5, 7), (4, 6)

# thickness -> mean |x_k - V| over the support, k = 0 .. 5 (measured; tests/test_solve_volume_reference.py compares within 1e-9 and asserts the fall)
CONSISTENT = {
    SPACING: (0.10943863268777618, 0.03249023577137323, 0.017439764479741177, 0.011577158082495495, 0.006972762387707476, 0.003014333508555123),
    SPACING / 4: (0.0018975435836294072, 0.0010324844541239652, 0.0004955598886175073, 0.0003046124806005199, 0.00018930732063593566, 0.00013043032445507762),
}
# thickness -> mean |x_k - V| over the support after k = 0, 1, 5, 30 iterations on the point-sample targets (measured; no direction asserted)
POINT_SAMPLES = {
    SPACING: (0.07665992225660602, 0.058770790860093465, 0.06856077383507293, 0.06877580254259988),
    SPACING / 4: (0.024412606193894286, 0.032181799693131195, 0.036514462637367844, 0.037789835344228036),
}


@functools.lru_cache(maxsize=None)
def tiny():
    rng = np.random.default_rng(19)
    maps = np.zeros((TINY_M, 9), np.float32)
    ci, cj = 0.5 * (TINY_SHAPE[0] - 1), 0.5 * (TINY_SHAPE[1] - 1)
    for q in range(TINY_M):
        ang, z0, z1 = rng.uniform(-0.15, 0.15), rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03)
        c, s = np.cos(ang), np.sin(ang)
        tz = (-0.1 + 0.55 * q) - z0 * ci - z1 * cj
        ty, tx = 4.4 - (c * ci - s * cj), 5.6 - (s * ci + c * cj)
        maps[q] = (z0, z1, tz, c, -s, ty, s, c, tx)
    targets = fc.targets_of(maps, TINY_SHAPE)
    w = (0.5 + rng.random(targets.shape)).astype(np.float32)
    gb = np.stack([rng.uniform(0.8, 1.3, TINY_M), rng.uniform(-0.2, 0.2, TINY_M)], axis=1).astype(np.float32)
    targets = (gb[:, :1, None] * targets + gb[:, 1:, None]).astype(np.float32)
    return dict(targets=targets, maps=maps, weights=w, intensity=gb)


@functools.lru_cache(maxsize=None)
def tall():
    rng = np.random.default_rng(23)
    maps = np.array([[0.02, 0.0, 3.3, 1, 0, 0.5, 0, 1, 0.25], [0.0, -0.03, 100.4, 1, 0, 0.25, 0, 1, 0.5], [0.01, 0.01, 257.8, 1, 0, 0.75, 0, 1, 0.75]], np.float32)
    targets = rng.standard_normal((3,) + TALL_SHAPE).astype(np.float32)
    start = rng.standard_normal(TALL_GRID).astype(np.float32)
    start[130, 2, 3] = np.nan
    return dict(targets=targets, maps=maps, start=start)


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> (args = (targets, maps, grid, spacing), kwargs with the thickness): every case of the bit-for-bit comparison"""
    out = {}
    d = fc.planes()
    for g, grid in enumerate(GRIDS):
        out[f"planes-grid{g}-wgb"] = ((d["targets"], d["maps"], grid, SPACING), dict(thickness=SPACING, weights=d["weights"], intensity=d["intensity"]))
        out[f"planes-grid{g}-plain"] = ((d["targets"], d["maps"], grid, SPACING), dict(thickness=SPACING))
        out[f"holes-grid{g}"] = ((d["targets"], d["maps"], grid, SPACING), dict(thickness=SPACING, weights=d["weights"], intensity=d["intensity"], start=pc.holes(grid)))
    out["planes-grid1-quarter"] = ((d["targets"], d["maps"], GRIDS[1], SPACING), dict(thickness=SPACING / 4, weights=d["weights"], intensity=d["intensity"]))
    out["planes-grid0-mincov"] = ((d["targets"], d["maps"], GRIDS[0], SPACING), dict(thickness=SPACING, weights=d["weights"], intensity=d["intensity"], min_coverage=0.4))
    for shift in fc.GRAZE_SHIFTS:
        for t, thickness in enumerate(fc.GRAZE_THICKNESSES):
            gz = fc.graze(shift)
            out[f"graze{shift:+d}-t{t}"] = ((gz["targets"], gz["maps"], GRIDS[0], SPACING), dict(thickness=thickness))
    i = fc.identity()
    out["identity"] = ((i["targets"], i["maps"], fc.IDENTITY_GRID, SPACING), dict(thickness=SPACING))
    t = fc.truth_case()
    for thickness in THICKNESSES:
        out[f"truth-t{thickness:g}"] = ((t["targets"], t["maps"], fc.TRUTH_GRID, SPACING), dict(thickness=thickness))
    o = fc.outside_target()
    out["outside"] = ((o["targets"], o["maps"], GRIDS[1], SPACING), dict(thickness=SPACING, weights=o["weights"], intensity=o["intensity"]))
    out["outside-start"] = ((o["targets"], o["maps"], GRIDS[1], SPACING), dict(thickness=SPACING, weights=o["weights"], intensity=o["intensity"], start=pc.stack(GRIDS[1])))
    none = (np.zeros((0,) + SHAPE, np.float32), np.zeros((0, 9), np.float32))
    out["none"] = (none + (GRIDS[1], SPACING), dict(thickness=SPACING))
    out["none-start"] = (none + (GRIDS[1], SPACING), dict(thickness=SPACING, start=pc.holes(GRIDS[1])))
    bad = slice(fc.DEGENERATE_AT, fc.M)
    out["flagged"] = ((d["targets"][bad], d["maps"][bad], GRIDS[0], SPACING), dict(thickness=SPACING, intensity=d["intensity"][bad]))
    y = tiny()
    out["tiny"] = ((y["targets"], y["maps"], TINY_GRID, SPACING), dict(thickness=SPACING, weights=y["weights"], intensity=y["intensity"]))
    a = tall()
    out["tall"] = ((a["targets"], a["maps"], TALL_GRID, SPACING), dict(thickness=SPACING, start=a["start"]))
    return out


@functools.lru_cache(maxsize=None)
def longest(name, lam):
    """-> (SolveVolumeResult of max(ITERATIONS) iterations, [geometry, x_0, .., x_K])"""
    args, kw = all_cases()[name]
    its = []
    res = sv.solve_volume_on_host(*args, iterations=max(ITERATIONS), lam=lam, iterates=its, **kw)
    return res, its


def expected(name, lam, iterations):
    """what msiren_solve_volume has to return for ``iterations`` <= max(ITERATIONS), cut out of the longest run"""
    res, its = longest(name, lam)
    geo, xs = its[0], its[1:]
    volume = np.where(geo.support, xs[iterations].astype(np.float32), np.float32(np.nan)).astype(np.float32)
    history = res.history[:iterations + 1].copy()
    history[iterations, 1] = np.nan
    stopped = res.stopped_at if 0 <= res.stopped_at < iterations else -1
    return sv.SolveVolumeResult(volume, res.coverage, history, res.flags, stopped)


@functools.lru_cache(maxsize=None)
def consistent_targets(thickness):
    """the truth case's targets replaced by the projection of the analytic stack: data that the forward model explains exactly (up to float32)"""
    t = fc.truth_case()
    sim = fuse.project_on_host(pc.stack(fc.TRUTH_GRID), t["maps"], fc.TRUTH_SHAPE, SPACING, thickness=thickness).simulated
    sim.setflags(write=False)
    return sim


def mean_errors(targets, thickness, iterations, lam=0.0):
    """mean |x_k - V| over the support for k = 0 .. iterations on the truth case's maps"""
    t = fc.truth_case()
    its = []
    sv.solve_volume_on_host(targets, t["maps"], fc.TRUTH_GRID, SPACING, iterations=iterations, lam=lam, thickness=thickness, iterates=its)
    S = its[0].support
    return [float(np.abs(x - t["volume"])[S].mean()) for x in its[1:]]
