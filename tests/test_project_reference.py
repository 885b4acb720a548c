"""msiren_project_volume on the CPU (no GPU needed): the normative restatement mri_inr_amd/fuse.py: project_on_host against the
independent formulation of tests/project_reference.py, the properties the rule promises, adjointness against fuse_on_host, the one-step
back-projection, seeded mutants of the rule, and project_plan.h (the box, what the call refuses, its tiling and scratch) in a stand-alone compiled
host program, built a second time with the address and undefined-behaviour sanitizers.  Cases: tests/project_cases.py.

The bound of the comparison, derived as tests/test_fuse_reference.py derives its own.  Both formulations place a voxel at (i, j, d) on a target; with
kappa the largest condition number of the 3 x 3 systems [a b n] (measured by the reference), s the largest |(i, j, d)| that passed and u = 2^-53,
either one is within delta = 64 kappa^2 u s of the exact coordinates.  Where k > 0, |d| <= thickness, so k = 1 - d^2 / thickness^2 moves by at most
2 delta / thickness; a bilinear weight (a product of two tent functions of slope 1, each at most 1) by at most 2 delta.  One voxel's k beta
therefore moves by at most E = delta (2 / thickness + 2) + 16 u, and with R voxels reaching a pixel and vmax the largest |V|
    |coverage - reference|  <= R E + 2^-24 coverage                                          (the second term: the result is float32)
    |simulated - reference| <= |g| R E (vmax + |ratio|) / coverage + 2^-24 |simulated|       (ratio = num / den of the reference)
Two kinds of pixel are left out and counted: where a voxel is within 1e-9 of the lattice's border without being exactly on it (the two may disagree
about whether it contributes at all), and where the reference's coverage is below R E (NaN or not is undecided)."""
import functools
import math
import os
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

import fuse_cases as fc
import project_cases as pc
import project_reference as pr
from mri_inr_amd import fuse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def ulps32(a, b):
    """the distance of two float32 arrays in units in the last place of the larger"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


REFERENCE_CASES = [f"planes-grid{g}-t{t:g}-{k}" for g in (0, 1) for t in pc.THICKNESSES for k in ("gb", "plain")] + ["holes-grid0", "holes-grid1"]


@functools.lru_cache(maxsize=None)
def reference(name):
    args, kw = pc.all_cases()[name]
    return pr.project(*args, **kw)


def compare(got, ref, args, kw):
    """-> (agrees, the largest error over its bound, pixels left out)"""
    V, thickness = np.asarray(args[0], np.float64), float(kw["thickness"])
    m = len(ref.flags)
    g = np.abs(np.asarray(kw["intensity"], np.float64)[:, 0]) if kw.get("intensity") is not None else np.ones(m)
    vmax = np.abs(V[np.isfinite(V)]).max()
    delta = 64.0 * ref.cond ** 2 * U * ref.scale
    E = delta * (2.0 / thickness + 2.0) + 16.0 * U
    floor = max(ref.reach, 1) * E
    use = ~ref.near_edge & ~((ref.coverage > 0) & (ref.coverage <= floor))
    left = int((~use).sum())
    if not np.array_equal(got.flags, ref.flags) or not np.array_equal(np.isnan(got.simulated)[use], np.isnan(ref.simulated)[use]):
        return False, np.inf, left
    cov_err = np.abs(got.coverage.astype(np.float64) - ref.coverage)
    cov_bound = floor + 2.0 ** -24 * ref.coverage
    seen = use & np.isfinite(ref.simulated)
    with np.errstate(all="ignore"):
        sim_err = np.abs(got.simulated.astype(np.float64) - ref.simulated)[seen]
        sim_bound = (g[:, None, None] * floor * (vmax + np.abs(ref.ratio)) / ref.coverage + 2.0 ** -24 * np.abs(ref.simulated))[seen]
    worst = max(float((cov_err / cov_bound.clip(1e-300))[use].max()), float((sim_err / sim_bound).max()) if seen.any() else 0.0)
    return worst <= 1.0, worst, left


@pytest.mark.parametrize("name", REFERENCE_CASES)
def test_the_host_rule_agrees_with_the_independent_formulation(name):
    args, kw = pc.all_cases()[name]
    got, ref = fuse.project_on_host(*args, **kw), reference(name)
    ok, worst, left_out = compare(got, ref, args, kw)
    print(f"{name}: condition {ref.cond:.9f}, largest coordinate {ref.scale:.2f}, at most {ref.reach} voxels per pixel, largest error / bound {worst:.3f}, "
          f"{left_out} pixels left out, {int(np.isfinite(got.simulated).sum())} covered")
    assert ok and left_out <= 0.01 * got.simulated.size
    assert got.simulated.dtype == np.float32 and got.coverage.dtype == np.float32 and got.flags.dtype == np.int32 and got.residual is None and got.stats is None
    assert got.flags.tolist() == [0] * fc.M_PLANES + [fuse.DEGENERATE, fuse.BAD_INTENSITY if kw["intensity"] is not None else 0]
    covered = np.isfinite(got.simulated).reshape(fc.M, -1)
    assert covered[1].all() and covered[4].all() and not covered[fc.DEGENERATE_AT].any()
    if kw["thickness"] == pc.SPACING / 4:  # the whole-target NaN path
        assert not covered[list(pc.UNCOVERED_AT_QUARTER)].any() and not got.coverage[list(pc.UNCOVERED_AT_QUARTER)].any()
    else:
        assert covered[:fc.M_PLANES].all()


def test_identity_returns_the_stacks_bits():
    d = pc.identity()
    res = fuse.project_on_host(d["volume"], d["maps"], pc.SHAPE, pc.SPACING)
    assert same(res.simulated, d["volume"]) and (res.coverage == 1.0).all() and not res.flags.any()
    assert same(res.simulated, fuse.project_on_host(d["volume"], d["maps"], pc.SHAPE, pc.SPACING, thickness=pc.SPACING, intensity=[[1, 0]] * 3).simulated)


@pytest.mark.parametrize("c", [0.75, -3.1])
def test_a_constant_stack_gives_g_c_plus_b_within_two_ulps(c):
    """num / den is c within one rounding of each of the two sums' relative error; g c + b of that, rounded to float32, is within 2 float32 ulps"""
    for grid in pc.GRIDS:
        args, kw = pc.planes(grid, True, np.full(grid, c, np.float32))
        res = fuse.project_on_host(*args, **kw)
        gb = np.asarray(kw["intensity"], np.float64)
        want = (gb[:, 0] * np.float64(np.float32(c)) + gb[:, 1])[:, None, None] * np.ones(res.simulated.shape)
        covered = np.isfinite(res.simulated)
        assert covered[:fc.M_PLANES].all() and not covered[fc.M_PLANES:].any()
        assert ulps32(res.simulated[covered], want[covered].astype(np.float32)).max() <= 2


@pytest.mark.parametrize("g,b", [(4.0, -2.0), (0.5, 8.0), (-2.0, 0.25)])
def test_gain_and_bias_that_are_powers_of_two_are_applied_exactly(g, b):
    """g x is exact for a power of two.  On the identity case num / den is the voxel itself, and with the voxels on a dyadic grid g V + b is exact in
    fp64 and a float32: the projection has its bits.  On the planes, with b = 0, scaling by g commutes with the rounding to float32"""
    d = pc.identity()
    V = (np.round(d["volume"] * 64) / 64).astype(np.float32)
    got = fuse.project_on_host(V, d["maps"], pc.SHAPE, pc.SPACING, intensity=[[g, b]] * 3)
    exact = g * V.astype(np.float64) + b
    assert same(exact.astype(np.float32).astype(np.float64), exact) and same(got.simulated, exact.astype(np.float32)) and (got.coverage == 1.0).all()
    for grid in pc.GRIDS:
        args, _ = pc.planes(grid, False)
        mp = args[1][:fc.M_PLANES]
        plain = fuse.project_on_host(args[0], mp, pc.SHAPE, pc.SPACING)
        scaled = fuse.project_on_host(args[0], mp, pc.SHAPE, pc.SPACING, intensity=[[g, 0.0]] * fc.M_PLANES)
        assert np.isfinite(plain.simulated).all() and same(scaled.simulated, np.float32(g) * plain.simulated) and same(scaled.coverage, plain.coverage)


def test_a_nan_voxel_only_thins_the_coverage():
    for g, grid in enumerate(pc.GRIDS):
        full = fuse.project_on_host(*pc.planes(grid)[0], **pc.planes(grid)[1])
        args, kw = pc.planes(grid, True, pc.holes(grid))
        thin = fuse.project_on_host(*args, **kw)
        assert np.array_equal(thin.flags, full.flags) and (thin.coverage <= full.coverage).all() and (thin.coverage < full.coverage).sum() > 50
        untouched = thin.coverage == full.coverage
        assert untouched.sum() > 500 and same(thin.simulated[untouched], full.simulated[untouched])
        assert np.isfinite(thin.simulated[thin.coverage > 0]).all()  # the infinity and the NaNs never reach a pixel
    all_nan = fuse.project_on_host(np.full(pc.GRIDS[1], np.nan, np.float32), *pc.planes(pc.GRIDS[1])[0][1:], **pc.planes(pc.GRIDS[1])[1])
    assert np.isnan(all_nan.simulated).all() and not all_nan.coverage.any()


def test_flagged_and_outside_targets_are_nan_with_coverage_zero():
    args, kw = pc.planes(pc.GRIDS[1])
    res = fuse.project_on_host(*args, **kw)
    for q in (fc.DEGENERATE_AT, fc.ZERO_GAIN_AT):
        assert res.flags[q] and np.isnan(res.simulated[q]).all() and not res.coverage[q].any()
    args, kw = pc.all_cases()["outside"]
    res = fuse.project_on_host(*args, **kw)
    assert not res.flags.any() and np.isnan(res.simulated).all() and not res.coverage.any()
    bad = fuse.project_on_host(args[0], np.full((1, 9), np.inf, np.float32), pc.SHAPE, pc.SPACING)
    assert bad.flags.tolist() == [fuse.DEGENERATE] and np.isnan(bad.simulated).all() and not bad.coverage.any()
    none = fuse.project_on_host(args[0], np.zeros((0, 9), np.float32), pc.SHAPE, pc.SPACING)
    assert none.simulated.shape == (0,) + pc.SHAPE and none.flags.shape == (0,)


def test_min_coverage_only_turns_values_into_nan():
    args, kw = pc.planes(pc.GRIDS[0])
    base = fuse.project_on_host(*args, **kw)
    for mc in (1e-3, 0.9, 1.5, 1e9):
        got = fuse.project_on_host(*args, min_coverage=mc, **kw)
        keep = base.coverage.astype(np.float64) > mc
        assert same(got.coverage, base.coverage) and np.array_equal(got.flags, base.flags)
        assert np.array_equal(np.isfinite(got.simulated), keep & np.isfinite(base.simulated)) and same(got.simulated[keep], base.simulated[keep])
        if mc == 1.5:
            assert 0 < np.isfinite(got.simulated).sum() < np.isfinite(base.simulated).sum()


def adjoint_sums(X, Y, maps, grid, shape, thickness):
    p = fuse.project_on_host(X, maps, shape, pc.SPACING, thickness=thickness)
    f = fuse.fuse_on_host(Y, maps, grid, pc.SPACING, thickness=thickness)
    a = p.simulated.astype(np.float64) * p.coverage.astype(np.float64) * Y.astype(np.float64)
    b = f.volume.astype(np.float64) * f.coverage.astype(np.float64) * X.astype(np.float64)
    a, b = a[np.isfinite(a)], b[np.isfinite(b)]
    return math.fsum(a), math.fsum(b), math.fsum(np.abs(a)) + math.fsum(np.abs(b))


@pytest.mark.parametrize("case", ["truth", "planes"])
def test_the_projection_is_the_adjoint_of_the_fusion(case):
    """<project(X) coverage, Y> = <fuse(Y) coverage, X>: either side is the sum of k beta X Y over the (voxel, tap) pairs.  Four float32 roundings of
    outputs at 2^-24 each, with room for the fp64 orders: 2^-21 of the sum of the absolute terms"""
    rng = np.random.default_rng(1)
    if case == "truth":
        maps, grid, shape = fc.truth_case()["maps"], fc.TRUTH_GRID, fc.TRUTH_SHAPE
    else:
        maps, grid, shape = fc.planes()["maps"][:fc.M_PLANES], pc.GRIDS[1], pc.SHAPE
    for thickness in pc.THICKNESSES:
        X, Y = rng.standard_normal(grid).astype(np.float32), rng.standard_normal((len(maps),) + shape).astype(np.float32)
        a, b, scale = adjoint_sums(X, Y, maps, grid, shape, thickness)
        print(f"{case} thickness {thickness}: {a!r} against {b!r}, difference {abs(a - b) / scale:.3g} of the absolute terms, {abs(a - b) / abs(a):.3g} of the sum")
        assert scale > 100 and abs(a - b) <= 2.0 ** -21 * scale


def test_one_back_projection_step_moves_the_fused_stack_towards_the_truth():
    t = fc.truth_case()
    T, maps = t["targets"], t["maps"]
    V0 = fuse.fuse_on_host(T, maps, fc.TRUTH_GRID, pc.SPACING)
    P = fuse.project_on_host(V0.volume, maps, fc.TRUTH_SHAPE, pc.SPACING)
    assert abs(np.isfinite(P.simulated).mean() - pc.TRUTH_COVERED_PIXELS) <= 0.01  # the targets overhang the grid on every side
    res, stats = fuse.project_stats_on_host(T, P.simulated)
    D = fuse.fuse_on_host(res, maps, fc.TRUTH_GRID, pc.SPACING)
    V1 = V0.volume.astype(np.float64) + np.nan_to_num(D.volume.astype(np.float64), nan=0.0)
    covered = np.isfinite(V0.volume)
    before, after = np.abs(V0.volume - t["volume"])[covered].mean(), np.abs(V1 - t["volume"])[covered].mean()
    print(f"mean error over the covered voxels: {before:.6f} before, {after:.6f} after one step (recorded {pc.ONE_STEP})")
    assert abs(before - fc.TRUTH_ERRORS[pc.SPACING][2]) <= 1e-9 and after < fc.TRUTH_ERRORS[pc.SPACING][2]
    assert abs(after - pc.ONE_STEP) <= 0.02 * pc.ONE_STEP and stats[:, 0].sum() == np.isfinite(P.simulated).sum()


# ---- the residual and the sums ------------------------------------------------------------------------------------------------------------------------
def stats_case(grid=pc.GRIDS[1]):
    d = fc.planes()
    args, kw = pc.planes(grid)
    sim = fuse.project_on_host(*args, **kw).simulated
    return d["targets"], sim, d["weights"]


def test_the_sums_agree_with_fsum():
    T, sim, w = stats_case()
    th, tw = pc.SHAPE
    for weights in (w, None):
        res, stats = fuse.project_stats_on_host(T, sim, weights)
        ww = np.ones(T.shape, np.float32) if weights is None else weights
        assert res.dtype == np.float32 and stats.dtype == np.float64 and stats.shape == (fc.M, 4)
        assert np.isnan(res[fc.NAN_PIXEL_AT]) and np.isnan(res[fc.DEGENERATE_AT]).all() and not stats[fc.DEGENERATE_AT].any() and not stats[fc.ZERO_GAIN_AT].any()
        for q in range(fc.M):
            ok = np.isfinite(res[q]) & np.isfinite(ww[q]) & (ww[q] > 0)
            r, x = res[q].astype(np.float64)[ok], ww[q].astype(np.float64)[ok]
            terms = [np.ones(len(r)), x, x * r, (x * r) * r]
            for e in range(4):
                assert abs(stats[q, e] - math.fsum(terms[e])) <= th * tw * U * math.fsum(np.abs(terms[e])), (q, e)
            assert stats[q, 0] == ok.sum()
        if weights is not None:
            assert stats[1, 0] < np.isfinite(res[1]).sum()  # the NaN weight and the zero block count for nothing
            assert same(res, fuse.project_stats_on_host(T, sim, None)[0])
    assert same(fuse.residual_on_host(np.float32([np.inf, 1, np.nan, 2]), np.float32([1, np.inf, 1, 0.5])), np.float32([np.nan, np.nan, np.nan, 1.5]))


# ---- seeded mutants of the rule ------------------------------------------------------------------------------------------------------------------------
def tap_major(acc, pixel, terms):
    for tap in range(4):
        np.add.at(acc, pixel[:, tap], terms[:, tap])


def row_major(terms):
    s = np.float64(0.0)
    for x in terms.ravel():
        s = s + x
    return s


def k_left_out_of_den(k, beta, V):
    return (k * beta) * V, beta + 0.0 * k


MUTANTS = {
    "tap_major_order": ("scatter", tap_major, "bits"),
    "k_left_out_of_den": ("tap_terms", k_left_out_of_den, "reference"),
    "bias_applied_before_gain": ("apply_intensity", lambda ratio, g, bias: g * (ratio + bias), "reference"),
    "window_in_abs_d": ("window", lambda cp, dt: 1.0 - (np.abs(cp) / np.sqrt(dt)), "reference"),
    "an_invalid_voxel_counted": ("voxel_valid", lambda V: np.ones(np.shape(V), bool), "reference"),
    "stats_summed_row_major": ("ordered_sum", row_major, "stats"),
}
MUTANT_CASES = ["planes-grid0-t4-gb", "holes-grid1"]


@functools.lru_cache(maxsize=None)
def rule_bits(name):
    """the two fp64 sums per pixel: an order of summation shows here, and almost never through the rounding to float32"""
    args, kw = pc.all_cases()[name]
    return fuse.project_sums_on_host(*args, **kw)[:2]


@functools.lru_cache(maxsize=None)
def rule_stats():
    return fuse.project_stats_on_host(*stats_case())[1]


def rejected(kind):
    """the checks of this file that the mutant's kind is held against -> it fails at least one"""
    if kind == "stats":
        return not same(fuse.project_stats_on_host(*stats_case())[1], rule_stats())
    for name in MUTANT_CASES:
        args, kw = pc.all_cases()[name]
        got = fuse.project_on_host(*args, **kw)
        if kind == "bits" and not all(same(a, b) for a, b in zip(fuse.project_sums_on_host(*args, **kw)[:2], rule_bits(name))):
            return True
        if kind == "reference" and not compare(got, reference(name), args, kw)[0]:
            return True
    return False


def test_the_checks_accept_the_rule_on_the_mutants_cases():
    rule_bits.cache_clear(), rule_stats.cache_clear()
    assert not any(rejected(kind) for kind in ("bits", "reference", "stats"))


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_checks_reject_every_seeded_mutant(mutant, monkeypatch):
    """the order mutants change bits only, those of the fp64 sums; the others fail the independent formulation"""
    attr, wrong, kind = MUTANTS[mutant]
    for name in MUTANT_CASES:
        rule_bits(name)
    rule_stats()
    monkeypatch.setattr(fuse, attr, wrong)
    assert rejected(kind), mutant


# ---- project_plan.h ------------------------------------------------------------------------------------------------------------------------------------
PROG = textwrap.dedent(r"""
    #include <cmath>
    #include <cstdio>
    #include <cstdlib>
    #include <cstring>
    #include <limits>
    #include <vector>
    #include "project_plan.h"
    using namespace msiren;

    #define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
    static char msg[256];
    static double buf[64];
    static ProjectArgs good(const msiren_fuse_opts* o) {
        return ProjectArgs{buf, 4, 40, 40, buf, nullptr, o, 3, 19, 23, nullptr, nullptr, buf, nullptr, nullptr, nullptr, nullptr, true};
    }
    static bool refused(const ProjectArgs& a, const char* word) {
        msg[0] = 0;
        if (project_check(a, msg, sizeof msg)) return false;
        if (!std::strstr(msg, word)) { std::printf("'%s' does not name '%s'\n", msg, word); return false; }
        return true;
    }

    static void plan() {
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        msiren_fuse_opts o{(int32_t)sizeof(msiren_fuse_opts), 0, 4.0, 4.0, 0.0};
        CHECK(project_check(good(&o), msg, sizeof msg));
        { msiren_fuse_opts b = o; b.struct_size = 24; CHECK(refused(good(&b), "struct_size")); }
        for (double bad : {0.0, -1.0, nan, inf}) {
            msiren_fuse_opts b = o; b.spacing = bad; CHECK(refused(good(&b), "spacing"));
            b = o; b.thickness = bad; CHECK(refused(good(&b), "thickness"));
        }
        for (double bad : {-1e-300, nan}) { msiren_fuse_opts b = o; b.min_coverage = bad; CHECK(refused(good(&b), "min_coverage")); }
        { ProjectArgs a = good(&o); a.th = 1; CHECK(refused(a, "th")); a = good(&o); a.tw = 1; CHECK(refused(a, "tw")); }
        { ProjectArgs a = good(&o); a.n = 0; CHECK(refused(a, "n_slices")); a = good(&o); a.H = 0; CHECK(refused(a, "height")); a = good(&o); a.W = -3; CHECK(refused(a, "width")); }
        { ProjectArgs a = good(&o); a.m = -1; CHECK(refused(a, "m_targets")); }
        { ProjectArgs a = good(&o); a.n = 1 << 10, a.H = 1 << 10, a.W = 1 << 10; CHECK(refused(a, "n_slices height width")); a.W = (1 << 10) - 1; CHECK(project_check(a, msg, sizeof msg)); }
        { ProjectArgs a = good(&o); a.m = 1 << 12, a.th = 1 << 9, a.tw = 1 << 9; CHECK(refused(a, "m_targets th tw")); a.m = (1 << 12) - 1; CHECK(project_check(a, msg, sizeof msg)); }
        { ProjectArgs a = good(&o); a.volume = nullptr; CHECK(refused(a, "volume")); a = good(&o); a.maps = nullptr; CHECK(refused(a, "maps"));
          a = good(&o); a.simulated = nullptr; CHECK(refused(a, "simulated")); a = good(nullptr); CHECK(refused(a, "opts")); }
        { ProjectArgs a = good(&o); a.weights = buf; CHECK(refused(a, "weights")); a = good(&o); a.residual = buf; CHECK(refused(a, "residual"));
          a = good(&o); a.stats = buf; CHECK(refused(a, "stats")); a.targets = buf, a.weights = a.residual = buf; CHECK(project_check(a, msg, sizeof msg)); }
        {
            const char* names[] = {"volume", "maps", "intensity", "targets", "weights", "simulated", "coverage", "residual", "flags"};
            for (int k = 0; k < 9; ++k) {
                ProjectArgs a = good(&o);
                a.targets = buf;
                const void* odd = (const char*)buf + 2;
                const void** slot[] = {&a.volume, &a.maps, &a.intensity, &a.targets, &a.weights, &a.simulated, &a.coverage, &a.residual, &a.flags};
                *slot[k] = odd;
                CHECK(refused(a, names[k]) && std::strstr(msg, "aligned"));
                a.device = false;
                CHECK(project_check(a, msg, sizeof msg));
            }
            ProjectArgs a = good(&o);
            a.targets = buf, a.stats = (const char*)buf + 4;
            CHECK(refused(a, "stats") && std::strstr(msg, "8-byte"));
            a.device = false;
            CHECK(project_check(a, msg, sizeof msg));
        }
        { ProjectArgs a = good(nullptr); a.m = 0, a.volume = a.maps = a.simulated = nullptr, a.th = a.tw = 0; CHECK(project_check(a, msg, sizeof msg)); a.n = 0; CHECK(refused(a, "n_slices")); }
        CHECK(kProjectTile == 16 && project_tiles_y(19) == 2 && project_tiles_x(23) == 2 && project_tiles_x(32) == 2 && project_tiles_x(33) == 3 && project_tiles(24, 44, 46) == 216);
        CHECK(project_layout(0, 23, true).total == 0 && project_layout(8, 23, false).total == 8 * 160 && project_layout(8, 23, true).columns == 8 * 160);
        CHECK(project_layout(8, 23, true).total == 8 * 160 + 8 * 23 * 32 && project_layout(8, 23, true).records == 0);
        // the box: an axis-aligned unit plane; what is not finite, ill conditioned or far away skips nothing
        double r[20] = {0, 1, 0, 0, 0, 1, 8, 0, 0, 1, 0, 1, 1, 16, 1, 0, 0, 1, 0, 0}, R[3];
        CHECK(project_box(r, 4.0, 4.0, 4, 40, 40, R) && R[0] > 1.0 && R[0] < 1.001 && R[1] > 1.0 && R[1] < 1.001 && R[2] > 1.0 && R[2] < 1.001);
        CHECK(project_count(true, R[1], 40) == 4 && project_count(true, R[1], 3) == 3 && project_count(false, R[1], 40) == 40 && project_count(true, nan, 40) == 40);
        CHECK(project_base(10.0, R[1], 40, 4) == 8 && project_base(-7.0, R[1], 40, 4) == 0 && project_base(100.0, R[1], 40, 4) == 36 && project_base(nan, R[1], 40, 4) == 0);
        CHECK(project_base(5.0, R[1], 3, 3) == 0 && project_base(-1e300, R[1], 40, 4) == 0 && project_base(1e300, R[1], 40, 4) == 36 && project_base(inf, R[1], 40, 4) == 36);
        { double b[20]; std::memcpy(b, r, sizeof b); b[FUSE_DET] = nan; CHECK(!project_box(b, 4.0, 4.0, 4, 40, 40, R)); }
        { double b[20]; std::memcpy(b, r, sizeof b); b[FUSE_DET] = 0x1p-11; CHECK(!project_box(b, 4.0, 4.0, 4, 40, 40, R)); }            // G11 G22 > 2^10 det
        { double b[20]; std::memcpy(b, r, sizeof b); b[FUSE_T + 1] = 0x1p25; CHECK(!project_box(b, 4.0, 4.0, 4, 40, 40, R)); b[FUSE_T + 1] = inf; CHECK(!project_box(b, 4.0, 4.0, 4, 40, 40, R)); }
        { double b[20]; std::memcpy(b, r, sizeof b); b[FUSE_A + 2] = inf; CHECK(!project_box(b, 4.0, 4.0, 4, 40, 40, R)); }
        CHECK(!project_box(r, 0x1p40, 4.0, 4, 40, 40, R));                                                                                  // a radius beyond an int
    }

    // mode 0: project_plan.h's box; 1: the radius without the normal term; 2: the span not clipped to the grid
    static bool box_of(int mode, const double* r, double thickness, double spacing, int n, int H, int W, double R[3]) {
        const bool boxed = project_box(r, thickness, spacing, n, H, W, R);
        if (mode == 1) {
            R[0] = ((std::fabs(r[FUSE_A]) + std::fabs(r[FUSE_B])) * (1.0 + 0x1p-20) + 0x1p-10) / spacing;
            for (int e = 1; e < 3; ++e) R[e] = (std::fabs(r[FUSE_A + e]) + std::fabs(r[FUSE_B + e])) * (1.0 + 0x1p-20) + 0x1p-10;
        }
        return boxed;
    }

    int main(int argc, char** argv) {
        CHECK(argc == 3);
        const int mode = std::atoi(argv[2]);
        if (mode == 0) plan();
        std::FILE* f = std::fopen(argv[1], "rb");
        CHECK(f);
        double worst = 0.0, tested = 0.0, pairs_all = 0.0;
        for (;;) {
            double head[8];  // spacing, thickness, n, H, W, th, tw, m
            if (std::fread(head, sizeof(double), 8, f) != 8) break;
            const double spacing = head[0], thickness = head[1];
            const int N[3] = {(int)head[2], (int)head[3], (int)head[4]}, th = (int)head[5], tw = (int)head[6], m = (int)head[7];
            std::vector<double> rec((size_t)m * 20);
            CHECK(std::fread(rec.data(), sizeof(double), rec.size(), f) == rec.size());
            double count;
            CHECK(std::fread(&count, sizeof(double), 1, f) == 1);
            std::vector<double> pairs((size_t)count * 6);  // q, z, y, x, pi, pj
            CHECK(std::fread(pairs.data(), sizeof(double), pairs.size(), f) == pairs.size());
            for (int q = 0; q < m; ++q) {
                const double* r = &rec[(size_t)q * 20];
                if (r[FUSE_FLAGS] != 0.0) continue;
                double R[3];
                const bool boxed = box_of(mode, r, thickness, spacing, N[0], N[1], N[2], R);
                CHECK(boxed);  // every case is well conditioned: the box is what is tested
                tested += (double)th * tw * project_count(boxed, R[0], N[0]) * project_count(boxed, R[1], N[1]) * project_count(boxed, R[2], N[2]);
            }
            for (size_t k = 0; k < (size_t)count; ++k) {
                const double* p = &pairs[6 * k];
                const double* r = &rec[(size_t)p[0] * 20];
                double R[3], G[3];
                const bool boxed = box_of(mode, r, thickness, spacing, N[0], N[1], N[2], R);
                project_radius(r, thickness, spacing, G);
                const double x[3] = {((r[FUSE_T] + r[FUSE_A] * p[4]) + r[FUSE_B] * p[5]) / spacing, (r[FUSE_T + 1] + r[FUSE_A + 1] * p[4]) + r[FUSE_B + 1] * p[5],
                                     (r[FUSE_T + 2] + r[FUSE_A + 2] * p[4]) + r[FUSE_B + 2] * p[5]};
                for (int e = 0; e < 3; ++e) {
                    const int cnt = project_count(boxed, R[e], N[e]);
                    const int base = mode == 2 ? (int)std::floor(x[e] - R[e]) : project_base(x[e], R[e], N[e], cnt);
                    if (base < 0 || base + cnt > N[e]) { std::printf("the span [%d, %d) leaves the axis of %d\n", base, base + cnt, N[e]); return 2; }
                    const int v = (int)p[1 + e];
                    if (v < base || v >= base + cnt) { std::printf("voxel %d outside the span [%d, %d) of axis %d\n", v, base, base + cnt, e); return 3; }
                    const double ratio = std::fabs((double)v - x[e]) / G[e];
                    if (ratio > worst) worst = ratio;
                }
            }
            pairs_all += count;
        }
        std::fclose(f);
        std::printf("ok %.17g %.0f %.0f\n", worst, pairs_all, tested);
        return 0;
    }
""")


def box_input(path):
    """every contributing (voxel, tap) pair of every case, with the records fuse_setup_kernel would write, for the host program"""
    with open(path, "wb") as f:
        for name, (args, kw) in pc.all_cases().items():
            vol, maps, shape, spacing = args
            r = fuse.target_records(maps, kw.get("intensity"), spacing, kw["thickness"])
            m = len(r.flags)
            rec = np.stack(list(r.a) + list(r.b) + list(r.t) + [r.G11, r.G12, r.G22, r.det, r.dt] + list(r.c) + [r.g, r.bias, r.flags.astype(np.float64)], axis=1)
            assert rec.shape == (m, 20)
            rows = []
            for q in range(m):
                taps = None if r.flags[q] else fuse.voxel_taps(r, q, np.isfinite(vol), vol.shape, shape, np.float64(spacing))
                if taps is None:
                    continue
                at, _, pixel, _ = taps
                for tap in range(4):
                    rows.append(np.stack([np.full(len(at[0]), q), at[0], at[1], at[2], pixel[:, tap] // shape[1], pixel[:, tap] % shape[1]], axis=1).astype(np.float64))
            pairs = np.concatenate(rows) if rows else np.zeros((0, 6))
            np.array([spacing, kw["thickness"], *vol.shape, *shape, m], np.float64).tofile(f)
            np.ascontiguousarray(rec, np.float64).tofile(f)
            np.array([len(pairs)], np.float64).tofile(f)
            np.ascontiguousarray(pairs, np.float64).tofile(f)


@pytest.fixture(scope="module")
def box_programs(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    d = tmp_path_factory.mktemp("project_plan")
    src = d / "project_plan.cpp"
    src.write_text(PROG)
    exes = {}
    for name, extra in (("plain", ["-O1"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[name] = d / name
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "mri_inr_amd", "csrc"), str(src), "-o", str(exes[name])], check=True,
                       capture_output=True, text=True)
    box_input(d / "pairs.bin")
    return exes, d / "pairs.bin"


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_every_contributing_pair_lies_inside_the_box(box_programs, build):
    exes, pairs = box_programs
    res = subprocess.run([str(exes[build]), str(pairs), "0"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout + res.stderr
    worst, count, tested = (float(x) for x in res.stdout.split()[1:])
    print(f"{build}: {count:.0f} pairs, worst |v - x| / R = {worst:.6f}, {tested / count:.2f} voxels tested per contributing one")
    assert count > 100000 and 0.99 <= worst <= 1.0 + 1e-9


@pytest.mark.parametrize("mode,code", [(1, 3), (2, 2)])
def test_a_wrong_box_is_rejected(box_programs, mode, code):
    """the radius without the normal term loses a voxel; the span not clipped leaves the grid"""
    exes, pairs = box_programs
    res = subprocess.run([str(exes["plain"]), str(pairs), str(mode)], capture_output=True, text=True, timeout=300)
    assert res.returncode == code, res.stdout + res.stderr
