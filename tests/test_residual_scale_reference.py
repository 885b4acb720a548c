"""The restatement of msiren_residual_scale (mri_inr_amd/residual_scale.py: residual_scale_on_host) on the CPU, no GPU and no library:
against numpy's own order statistic (np.quantile, method="lower", on the same float32 deviations: no interpolation) exactly, on every case of
tests/residual_scale_cases.py; against np.median where the count is odd; the residual against fuse.residual_on_host; pooling against the median of
medians; the efficacy figures of the corrupted truth case under two bounds; and eight seeded mutants of the rule, each rejected."""
import collections

import numpy as np
import pytest

import fuse_cases as fc
import residual_scale_cases as cases
import solve_volume_r_cases as rc
from mri_inr_amd import align_robust as ar
from mri_inr_amd import fuse
from mri_inr_amd import residual_scale as rs
from mri_inr_amd import solve_volume as sv
from mri_inr_amd import solve_volume_robust as svr

bits_equal = cases.bits_equal


def lower_quantile(x, q):
    """np.quantile(x, q, method="lower") on float32 values.  numpy forms its index as n q - q, which rounds 101 x 0.29 - 0.29 up to 29.000000000000004
    where the rule's one multiply 0.29 x 100 = 28.999999999999996 floors to 28: where the rule's product lies that close below an integer, and only
    there, the element of the rule's rank comes from np.partition instead; everywhere else the two are asserted to agree."""
    product = np.float64(q) * np.float64(len(x) - 1)
    k = int(np.floor(product))
    by_rank = np.partition(x, k)[k]
    if np.ceil(product) - product > 1e-9 or np.ceil(product) == product:
        assert np.quantile(x, q, method="lower") == by_rank
    return by_rank


def independent(e, w, *, tune, quantile, centre, groups, floor):
    """the same statistic from numpy's own order statistic on float32 values, segment by segment"""
    m = len(e)
    w = np.ones(e.shape, np.float32) if w is None else w
    offsets = rs.segments(groups, m)
    scale, stats = np.full(m, np.inf), np.zeros((len(offsets) - 1, 4))
    with np.errstate(all="ignore"):
        for s, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
            x = e[lo:hi][np.isfinite(e[lo:hi]) & np.isfinite(w[lo:hi]) & (w[lo:hi] > 0)]
            if not len(x):
                continue
            c = lower_quantile(x, quantile) if centre else np.float32(0)
            d = lower_quantile(np.abs(x - c), quantile)
            assert d.dtype == np.float32
            t = tune * float(d)
            scale[lo:hi] = max(t * t, floor)
            stats[s] = (len(x), 0, c, d)
    return scale, stats


@pytest.mark.parametrize("shape", cases.LATTICES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", cases.KINDS)
def test_the_restatement_is_numpys_lower_quantile_exactly(kind, shape):
    e = cases.residuals(kind, shape)
    for _, w in cases.weights_of(shape):
        for s in cases.SETTINGS:
            got = rs.residual_scale_on_host(e, tune=cases.TUNE, weights=w, **s)
            scale, stats = independent(e, w, tune=cases.TUNE, **s)
            # numpy does not tell -0.0 from +0.0: values are compared, and the rank apart
            assert np.array_equal(got.scale, scale), (s, got.scale, scale)
            assert np.array_equal(got.stats[:, [0, 2, 3]], stats[:, [0, 2, 3]]), (s, got.stats, stats)
            counts = got.stats[:, 0]
            assert np.array_equal(got.stats[:, 1], np.where(counts > 0, np.floor(s["quantile"] * np.maximum(counts - 1, 0)), 0))


def test_the_median_where_the_count_is_odd():
    e = cases.residuals("smooth", cases.LATTICES[0])  # 437 pixels per target, 1311 in three: odd
    got = rs.residual_scale_on_host(e, tune=1.0, centre=True)
    for q in range(cases.M):
        c = np.median(e[q])
        assert got.stats[q, 2] == c and got.stats[q, 3] == np.median(np.abs(e[q] - c)) and got.scale[q] == float(got.stats[q, 3]) ** 2
    pooled = rs.residual_scale_on_host(e[:3], tune=1.0, centre=False, groups=[3])
    assert pooled.stats[0, 3] == np.median(np.abs(e[:3])) and pooled.stats[0, 0] == 1311 and (pooled.scale == pooled.scale[0]).all()


def test_the_rank_of_029_over_101_pixels_is_28():
    assert 0.29 * 100 < 29 and rs.rank(0.29, 101) == 28 and rs.rank(0.5, 101) == 50 and rs.rank(1.0, 101) == 100 and rs.rank(0.0, 101) == 0
    e = cases.residuals("sparse", cases.LATTICES[0])
    got = rs.residual_scale_on_host(e, tune=1.0, quantile=0.29)
    assert got.stats[:4, 0].tolist() == [0, 1, 2, 101] and got.stats[cases.HUNDRED_ONE, 1] == 28
    x = np.sort(np.abs(e[cases.HUNDRED_ONE][np.isfinite(e[cases.HUNDRED_ONE])]))
    assert got.stats[cases.HUNDRED_ONE, 3] == x[28] and x[28] < x[29]
    assert np.isposinf(got.scale[0]) and not got.stats[0].any()  # no pixel: the quadratic loss, a row of zeros


def test_the_key_is_a_total_order_that_tells_the_zeros_apart():
    x = np.array([np.inf, 1.0, 1e-45, 0.0, -0.0, -1e-45, -1.0, -np.inf], np.float32)
    k = rs.sort_key(x)
    assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) < 0).all() and k[3] == 0x80000000 and k[4] == 0x7FFFFFFF
    e = cases.residuals("zeros", cases.LATTICES[0])
    got = rs.residual_scale_on_host(e, tune=1.0, centre=True, quantile=0.0)
    assert np.signbit(got.stats[:, 2]).all() and not np.signbit(rs.residual_scale_on_host(e, tune=1.0, centre=True, quantile=1.0).stats[:, 2]).any()
    assert not got.scale.any()


def test_the_residual_is_projects_where_intensity_is_absent():
    T, S, gb = cases.pair(cases.LATTICES[1])
    e = rs.pixel_residual(T, S, None, None)
    want = fuse.residual_on_host(T, S)
    finite = np.isfinite(want)
    assert finite.sum() > 6000 and bits_equal(e[finite], want[finite]) and not np.isfinite(e[~finite]).any()
    assert (np.signbit(S) & (S == 0) & (T == 0)).any()  # (the -0.0 that a product with g = 1 and a sum with b = 0 would lose)
    # the same counts and the same statistic from either
    a, b = rs.residual_scale_on_host(T, S, tune=2.0, centre=True), rs.residual_scale_on_host(want, tune=2.0, centre=True)
    assert bits_equal(a.scale, b.scale) and bits_equal(a.stats, b.stats)
    # with intensity: the rule's association in fp64, rounded once
    g, bias = gb[:, 0].astype(np.float64).reshape(-1, 1, 1), gb[:, 1].astype(np.float64).reshape(-1, 1, 1)
    with np.errstate(all="ignore"):
        assert bits_equal(rs.pixel_residual(T, S, g, bias), (T.astype(np.float64) - (g * S.astype(np.float64) + bias)).astype(np.float32))
    assert bits_equal(rs.pixel_residual(T, None, None, None), T)
    with pytest.raises(ValueError, match="intensity"):
        rs.residual_scale_on_host(T, None, tune=1.0, intensity=gb)


def test_pooling_is_not_the_median_of_medians():
    e = np.zeros((3, 2, 4), np.float32)
    e[0], e[1], e[2] = 1.0, 2.0, 9.0
    e[2, 0, :3] = np.nan  # 8 + 8 + 5 pixels: the pooled median is 2, the median of the medians 2 as well -- so count them unevenly:
    e[1, 1] = np.nan      # 8 + 4 + 5: ranks 0 .. 7 are 1, 8 .. 11 are 2, 12 .. 16 are 9; the pooled median (rank 8) is 2 ...
    e[0, 0, 0] = 0.5
    per = rs.residual_scale_on_host(e, tune=1.0)
    pooled = rs.residual_scale_on_host(e, tune=1.0, groups=[3])
    assert per.stats[:, 3].tolist() == [1.0, 2.0, 9.0] and pooled.stats.tolist() == [[17.0, 8.0, 0.0, 2.0]]
    e2 = e.copy()
    e2[1] = np.nan        # ... and without target 1's four pixels rank floor(0.5 12) = 6 is 1: not the median 9 of the medians (1, 9), not their mean
    pooled2 = rs.residual_scale_on_host(e2, tune=1.0, groups=[3])
    assert pooled2.stats.tolist() == [[13.0, 6.0, 0.0, 1.0]] and pooled2.scale.tolist() == [1.0, 1.0, 1.0]
    per2 = rs.residual_scale_on_host(e2, tune=1.0)
    assert np.median(per2.stats[[0, 2], 3]) == 5.0 and np.isposinf(per2.scale[1])


Weighted = collections.namedtuple("Weighted", "cost wsum")


def test_the_median_scale_reaches_the_hand_tuned_result_and_the_rms_scale_does_not():
    """The corrupted truth case, fused, projected back, its residual's scale estimated, solved robustly with CORRUPT_SETTING: mean |x - x_clean| over the
    support.  Measured from the restatement: per target 0.00613 (max 0.487), pooled 0.00444 (0.379), against 0.00502 with the hand-picked scale 1 and
    1.43 for the quadratic solve; align_robust.scale_from (a mean of squares) at tune 1: 2.52 (45.8) -- worse than no robust loss at all."""
    c, sp, grid = rc.corrupted(), rc.SPACING, fc.TRUTH_GRID
    tg, maps = c["targets"], c["maps"]
    fused = fuse.fuse_on_host(tg, maps, grid, sp, thickness=sp)
    sim = fuse.project_on_host(fused.volume, maps, tg.shape[1:], sp, thickness=sp).simulated
    res, stats = fuse.project_stats_on_host(tg, sim)
    its = []
    sv.solve_volume_on_host(c["clean"], maps, grid, sp, iterations=15, lam=rc.CORRUPT_SETTING["lam"], iterates=its, thickness=sp)
    S, x_clean = its[0].support, its[-1]

    def error(scale):
        its = []
        svr.solve_volume_robust_on_host(tg, maps, grid, sp, scale, iterates=its, thickness=sp, **rc.CORRUPT_SETTING)
        return float(np.abs(its[-1] - x_clean)[S].mean())

    per = rs.residual_scale_on_host(tg, sim, tune=cases.TUNE)
    assert bits_equal(per.scale, rs.residual_scale_on_host(res, tune=cases.TUNE).scale)
    sigma = np.sqrt(per.scale) / 6.0  # 1.4826 median |e|: 0.04 .. 0.25 on all 24 targets, the corrupted ones among them
    rms = np.sqrt(stats[:, 3] / stats[:, 1])
    bad = np.zeros(len(tg), bool)
    bad[list(rc.CORRUPT_TARGETS)] = True
    print(f"1.4826 median |e|: {sigma.min()} .. {sigma.max()}; rms clean {rms[~bad].min()} .. {rms[~bad].max()}, corrupted {rms[bad].min()} .. {rms[bad].max()}")
    assert 0.04 < sigma.min() and sigma.max() < 0.25 and rms[bad].min() > 2 * rms[~bad].max()
    pooled = rs.residual_scale_on_host(res, tune=cases.TUNE, groups=[len(tg)])
    err_per, err_pooled = error(per.scale), error(pooled.scale)
    err_rms = error(ar.scale_from(Weighted(stats[:, 3], stats[:, 1]), 1.0))
    print(f"mean |x - x_clean|: per target {err_per}, pooled {err_pooled}, scale_from {err_rms}; quadratic {rc.MEASURED['quadratic_mean']}")
    assert err_per < 0.1 * rc.MEASURED["quadratic_mean"] and err_pooled < 0.1 * rc.MEASURED["quadratic_mean"]
    assert err_rms > rc.MEASURED["quadratic_mean"]


def ceil_rank(quantile, count):
    return int(np.ceil(np.float64(quantile) * np.float64(count - 1)))


def rank_over_count(quantile, count):
    return min(int(np.floor(np.float64(quantile) * np.float64(count))), count - 1)


def signed_key(x):
    """the bits compared as signed integers: right for x >= 0, the negatives in reverse"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) + (1 << 31)).astype(np.uint32)


def zero_weight_counts(e, w):
    return np.isfinite(e) & np.isfinite(w) & (w >= 0)


def nan_counts(e, w):
    return ~np.isinf(e) & np.isfinite(w) & (w > 0)


def tune_not_squared(d, tune, floor):
    s = np.float64(tune) * np.float64(d)
    return s if s > floor else np.float64(floor)


def floor_before_squaring(d, tune, floor):
    t = np.float64(tune) * np.float64(d)
    t = t if t > floor else np.float64(floor)
    return t * t


def difference_of_magnitudes(e, c):
    return np.abs(np.abs(e) - np.abs(np.float32(c)))


MUTANTS = [("ceil-for-floor", dict(rank_of=ceil_rank)), ("quantile-times-count", dict(rank_of=rank_over_count)), ("signed-keys", dict(key=signed_key)),
           ("zero-weight-counted", dict(counts=zero_weight_counts)), ("nan-counted", dict(counts=nan_counts)), ("tune-not-squared", dict(scale_from_d=tune_not_squared)),
           ("floor-before-squaring", dict(scale_from_d=floor_before_squaring)), ("magnitudes-subtracted", dict(deviation_of=difference_of_magnitudes))]


def verdicts(**mutant):
    """does the restatement, with one piece replaced, still pass the checks of this file and of the GPU test?  -> the list of (kind, weights, setting)
    on which its scale or stats differ from numpy's own statistic"""
    failed = []
    shape = cases.LATTICES[0]
    for kind in ("smooth", "two", "nonfinite", "sparse", "negatives"):
        e = cases.residuals(kind, shape)
        for wname, w in cases.weights_of(shape):
            for s in cases.SETTINGS:
                with np.errstate(all="ignore"):
                    got = rs.residual_scale_on_host(e, tune=cases.TUNE, weights=w, **s, **mutant)
                scale, stats = independent(e, w, tune=cases.TUNE, **s)
                if not (np.array_equal(got.scale, scale, equal_nan=True) and np.array_equal(got.stats[:, [0, 2, 3]], stats[:, [0, 2, 3]], equal_nan=True)):
                    failed.append((kind, wname, tuple(s.items())))
    return failed


def test_the_checks_pass_the_rule_itself():
    assert verdicts() == []


@pytest.mark.parametrize("name,mutant", MUTANTS, ids=[n for n, _ in MUTANTS])
def test_a_seeded_mutant_is_rejected(name, mutant):
    failed = verdicts(**mutant)
    print(f"{name}: rejected on {len(failed)} settings, first {failed[:1]}")
    assert failed
