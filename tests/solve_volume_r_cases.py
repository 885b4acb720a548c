"""The cases of msiren_solve_volume_r shared by tests/test_solve_volume_robust_reference.py (CPU) and
tests/test_gpu_solve_volume_robust.py.  Not a test module; no GPU and no model needed: pure numpy on top of tests/solve_volume_cases.py, small enough
that every GPU test takes seconds.

    NAMES       the cases of solve_volume_cases.all_cases() that are solved robustly: tiny, the planes on both grids (with weights and intensity, once
                at thickness spacing / 4), the holes given as the start, one graze case, identity, outside, none, flagged, tall
    scales      every case runs with one scale per target, PATTERN repeated over the targets: a finite value, +inf (the quadratic loss), and the three
                kinds of scale that are not > 0 and switch their target off -- 0, a negative value and NaN
    SETTINGS    rounds x iterations x anneal, each for LAMBDAS
    corrupted   the truth case of tests/fuse_cases.py with targets that the forward model explains (solve_volume_cases.consistent_targets), a 16 x 18 block
                of every fourth target raised by 20 .. 40

The expected results are cut out of one longest run where the rule allows it: with anneal = 1 the schedule is 1.0 throughout, so round t of a longer
run is round t of a shorter one and `expected` cuts rounds 0 .. 3 out of the run of three rounds with the same iterations; rounds <= 1 have the
schedule (1.0) whatever anneal is.  With anneal = 4 the first factor depends on the number of rounds: those runs are made one by one.  The final pass
(rweight, residual, stats) is ``final_pass_on_host`` on the iterate that the cut ends on.

MEASURED: the figures of the corrupted truth case from solve_volume_robust_on_host (tests/test_solve_volume_robust_reference.py compares and asserts
the issue's bounds on them)."""
import collections
import functools
import itertools

import numpy as np

import fuse_cases as fc
import solve_volume_cases as sc
from mri_inr_amd import solve_volume as sv
from mri_inr_amd import solve_volume_robust as svr

SPACING = sc.SPACING
NAMES = ("tiny", "planes-grid0-wgb", "planes-grid1-quarter", "holes-grid1", "graze+1-t0", "identity", "outside", "none", "flagged", "tall")
PATTERN = (0.05, np.inf, 0.0, -1.0, np.nan)
ROUNDS, ITERATIONS, ANNEALS, LAMBDAS = (0, 1, 2, 3), (0, 1, 2), (1.0, 4.0), (0.0, 0.01)
SETTINGS = tuple(itertools.product(ROUNDS, ITERATIONS, ANNEALS))

Expected = collections.namedtuple("Expected", "volume coverage history flags stopped_at rweight stats residual")

# the corrupted truth case: scale 1, 5 rounds x 3 iterations, anneal 4, lambda 0.01 against 15 quadratic iterations (measured from the restatement)
CORRUPT_TARGETS, CORRUPT_ROWS, CORRUPT_COLS = tuple(range(0, 24, 4)), slice(10, 26), slice(12, 30)
CORRUPT_SETTING = dict(rounds=5, iterations=3, anneal=4.0, lam=0.01)
MEASURED = dict(quadratic_mean=1.4328194057504435, quadratic_max=22.774065382715353, robust_mean=0.005022369101628974, robust_max=0.4416925000206424,
                rweight_inside=1.8553756717665237e-06, rweight_outside=0.9999060034751892)
# stats' sum w omega / sum w: 0.829 .. 0.832 on the six corrupted targets (288 of 2024 pixels each), at least 0.9996 on the others


def scales(m):
    """PATTERN repeated over m targets"""
    return np.resize(np.array(PATTERN, np.float64), m)


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> (args = (targets, maps, grid, spacing, scale), kwargs with the thickness)"""
    base = sc.all_cases()
    return {name: (base[name][0] + (scales(len(base[name][0][0])),), base[name][1]) for name in NAMES}


@functools.lru_cache(maxsize=None)
def run(name, lam, anneal, rounds, iterations):
    """-> (SolveVolumeRobustResult, [geometry, x_0, x after every step of every round])"""
    args, kw = all_cases()[name]
    its = []
    res = svr.solve_volume_robust_on_host(*args, rounds=rounds, iterations=iterations, anneal=anneal, lam=lam, iterates=its, **kw)
    return res, its


def expected(name, lam, anneal, rounds, iterations):
    """what msiren_solve_volume_r has to return, cut out of the longest run where the rule allows it"""
    args, kw = all_cases()[name]
    cut = anneal == 1.0 or rounds <= 1
    res, its = run(name, lam, 1.0, max(ROUNDS), iterations) if cut else run(name, lam, anneal, rounds, iterations)
    geo, xs = its[0], its[1:]
    x = xs[rounds * iterations]
    volume = np.where(geo.support, x.astype(np.float32), np.float32(np.nan)).astype(np.float32)
    rw, residual, stats = svr.final_pass_on_host(geo, x, args[0], kw.get("weights"), args[4])
    return Expected(volume, res.coverage, res.history[:rounds].copy(), res.flags, res.stopped_at[:rounds].copy(), rw, stats, residual)


@functools.lru_cache(maxsize=None)
def corrupted():
    """-> dict(targets, clean, maps, inside (24, 44, 46) bool): the truth case with consistent targets and the raised blocks"""
    t = fc.truth_case()
    clean = sc.consistent_targets(SPACING)
    targets = clean.copy()
    q = list(CORRUPT_TARGETS)
    block = (20.0 * (1.0 + np.random.default_rng(5).random((len(q), 16, 18)))).astype(np.float32)
    targets[q, CORRUPT_ROWS, CORRUPT_COLS] += block
    inside = np.zeros(targets.shape, bool)
    inside[q, CORRUPT_ROWS, CORRUPT_COLS] = True
    for a in (targets, inside):
        a.setflags(write=False)
    return dict(targets=targets, clean=clean, maps=t["maps"], inside=inside)


@functools.lru_cache(maxsize=None)
def corrupted_figures():
    """-> dict: the errors against the clean quadratic solve (mean and max |x - x_clean| over the support), the mean rweight inside and outside the
    blocks, and stats' sum w omega / sum w per target"""
    c = corrupted()
    kw = dict(thickness=SPACING)
    its = []
    sv.solve_volume_on_host(c["clean"], c["maps"], fc.TRUTH_GRID, SPACING, iterations=15, lam=CORRUPT_SETTING["lam"], iterates=its, **kw)
    S, x_clean = its[0].support, its[-1]
    its = []
    sv.solve_volume_on_host(c["targets"], c["maps"], fc.TRUTH_GRID, SPACING, iterations=15, lam=CORRUPT_SETTING["lam"], iterates=its, **kw)
    x_quadratic = its[-1]
    its = []
    res = svr.solve_volume_robust_on_host(c["targets"], c["maps"], fc.TRUTH_GRID, SPACING, 1.0, iterates=its, **CORRUPT_SETTING, **kw)
    x_robust = its[-1]
    assert np.array_equal(S, its[0].support)  # (the corruption moves no voxel in or out of the support)
    err = lambda x: np.abs(x - x_clean)[S]
    taking_part = np.isfinite(res.rweight)
    return dict(quadratic_mean=float(err(x_quadratic).mean()), quadratic_max=float(err(x_quadratic).max()), robust_mean=float(err(x_robust).mean()),
                robust_max=float(err(x_robust).max()), rweight_inside=float(res.rweight[c["inside"] & taking_part].mean()),
                rweight_outside=float(res.rweight[~c["inside"] & taking_part].mean()), ratio=res.stats[:, 2] / res.stats[:, 1])
