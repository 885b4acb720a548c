"""msiren_solve_volume's rule on the CPU (no GPU needed): mri_inr_amd/solve_volume.py: solve_volume_on_host, the normative
restatement that tests/test_gpu_solve_volume.py holds the device to bit for bit, is held here against what it has to mean --

    the forward operator is msiren_project_volume's num / den, bit for bit; the transpose is its transpose (the adjointness of the two, within rounding);
    on a case small enough for a dense matrix the iterates converge to the solution of the normal equations built by an independent formulation
    (tests/solve_volume_reference.py), within a bound derived from the measured condition number;
    the objective never increases along the iterates, on every case and lambda;
    no iteration returns the fusion's bits; pixels and targets that take no part change no bit; an empty support stops at iteration 0;
    on data that the forward model explains, the error against the truth falls strictly; on point samples the figures are recorded, no direction claimed;
    seeded mutants of every piece of the rule are rejected by these checks;
    solve_volume_plan.h, stand-alone, also under the address and undefined-behaviour sanitizers."""
import functools
import os
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

import fuse_cases as fc
import project_cases as pc
import solve_volume_cases as sc
import solve_volume_reference as ref
from mri_inr_amd import fuse
from mri_inr_amd import solve_volume as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def geometry_of(name):
    return sc.longest(name, 0.0)[1][0]


# ---- the two operators ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", pc.GRIDS)
@pytest.mark.parametrize("thickness", pc.THICKNESSES)
def test_the_forward_operator_is_the_projections_ratio_bit_for_bit(grid, thickness):
    d = fc.planes()
    vol = pc.holes(grid)
    num, den, r = fuse.project_sums_on_host(vol, d["maps"], pc.SHAPE, pc.SPACING, thickness=thickness, intensity=d["intensity"])
    geo = sv.geometry(d["targets"], d["maps"], np.isfinite(vol), pc.SPACING, thickness=thickness, weights=d["weights"], intensity=d["intensity"])
    v = np.where(geo.support, vol.astype(np.float64), 0.0)
    with np.errstate(all="ignore"):
        want = np.where(geo.active, num / den, 0.0)
    assert same(geo.D, den) and same(sv.forward_sums_on_host(geo, v), num) and same(sv.forward_on_host(geo, v), want)
    assert geo.active.sum() > 300 and not geo.active[fc.DEGENERATE_AT:].any() and not geo.active[2].reshape(pc.SHAPE)[fc.NAN_PIXEL_AT[1:]]


@pytest.mark.parametrize("name", ["truth-t4", "truth-t1", "holes-grid1", "tiny"])
def test_the_transpose_is_the_transpose_of_the_forward_operator(name):
    """<P v, y> = <v, Pt y>: either side is the sum of k beta v y / D over the (voxel, active tap) pairs, in fp64 throughout: some thousand terms in
    two orders, each side with a handful of roundings per term: 2^-40 of the sum of the absolute terms is 2^13 u, far above both"""
    geo = geometry_of(name)
    rng = np.random.default_rng(2)
    v = np.where(geo.support, rng.standard_normal(geo.grid), 0.0)
    y = np.where(geo.active, rng.standard_normal(geo.D.shape), 0.0)
    Pv, Pty = sv.forward_on_host(geo, v), sv.transpose_on_host(geo, y)
    a, b = float(np.sum(Pv * y)), float(np.sum(v * Pty))
    scale = float(np.sum(np.abs(Pv * y)) + np.sum(np.abs(v * Pty)))
    print(f"{name}: <P v, y> = {a!r}, <v, Pt y> = {b!r}, difference {abs(a - b) / scale:.3g} of the absolute terms")
    assert scale > 10 and abs(a - b) <= 2.0 ** -40 * scale  # observed: at most 6e-17 of the absolute terms


def test_the_laplacian_is_symmetric_kills_constants_and_skips_the_holes():
    geo = geometry_of("holes-grid1")
    rng = np.random.default_rng(4)
    S = geo.support
    assert not S.all() and S.sum() > 5000
    ones = np.where(S, 1.0, 0.0)
    assert not sv.laplacian_on_host(geo, ones).any()
    u, v = np.where(S, rng.standard_normal(geo.grid), 0.0), np.where(S, rng.standard_normal(geo.grid), 0.0)
    a, b = float(np.sum(u * sv.laplacian_on_host(geo, v))), float(np.sum(v * sv.laplacian_on_host(geo, u)))
    assert abs(a - b) <= 1e-12 * float(np.sum(np.abs(u * sv.laplacian_on_host(geo, v))))
    assert float(np.sum(v * sv.laplacian_on_host(geo, v))) > 0
    St = np.isfinite(tiny_start())                      # against the matrix built from a list of edges, where that is small
    tiny = geometry_of("tiny")._replace(support=St)
    t = np.where(St, rng.standard_normal(sc.TINY_GRID), 0.0)
    assert not St.all() and np.allclose(sv.laplacian_on_host(tiny, t).ravel(), ref.laplacian_matrix(St, sc.SPACING) @ t.ravel(), rtol=0, atol=1e-12)


def test_the_ordered_dot_is_the_sum_and_its_order_is_the_rules():
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((3, 7, 5)), rng.standard_normal((3, 7, 5))
    S = rng.random((3, 7, 5)) > 0.2
    want = np.float64(0.0)
    for z in range(3):
        cols = []
        for x in range(5):
            s = np.float64(0.0)
            for y in range(7):
                s = s + (a[z, y, x] * b[z, y, x] if S[z, y, x] else 0.0)
            cols.append(s)
        t = np.float64(0.0)
        for c in cols:
            t = t + c
        want = want + t
    assert sv.ordered_dot(a, b, S) == want and abs(want - np.sum((a * b)[S])) < 1e-12


# ---- the dense reference -------------------------------------------------------------------------------------------------------------------------------
TINY_LAMBDA = 0.01
BUDGET = 600


def tiny_start():
    """the tiny case from a start with holes: the support is not the whole grid"""
    y = sc.tiny()
    start = fuse.fuse_on_host(y["targets"], y["maps"], sc.TINY_GRID, sc.SPACING, weights=y["weights"], intensity=y["intensity"]).volume.copy()
    start[1, 3:5, 4:7] = np.nan
    start[0, 8, 2] = np.inf
    return start


@functools.lru_cache(maxsize=None)
def dense():
    y = sc.tiny()
    return ref.solve(y["targets"], y["maps"], np.isfinite(tiny_start()), sc.SPACING, lam=TINY_LAMBDA, thickness=sc.SPACING, weights=y["weights"], intensity=y["intensity"])


def converged(**pieces):
    """the restatement on the tiny case until rho has fallen by 2^-40 -> (x, iterations, rho) or None within the budget"""
    y = sc.tiny()
    its = []
    res = sv.solve_volume_on_host(y["targets"], y["maps"], sc.TINY_GRID, sc.SPACING, iterations=BUDGET, lam=TINY_LAMBDA, weights=y["weights"], intensity=y["intensity"],
                                  start=tiny_start(), iterates=its, **pieces)
    rho = res.history[:, 0]
    below = np.nonzero(rho <= 2.0 ** -40 * rho[0])[0]
    if not len(below) or (0 <= res.stopped_at < below[0]):
        return None
    return its[1 + below[0]], int(below[0]), float(rho[below[0]])


def dense_bound(d, rho):
    """|x_k - x*|_2 <= |A^-1| |r_k| = sqrt(rho_k) / lambda_min for the iteration's own residual; the recurrence's r_k drifts from rhs - A x_k, and
    np.linalg.solve and the two formulations of P differ, by rounding that the condition number amplifies: 2^-36 cond |x*| stands for both (cond u
    |x*| with 2^17 of room for a few hundred iterations' worth of drift)"""
    return np.sqrt(rho) / d.lam_min + 2.0 ** -36 * d.cond * float(np.linalg.norm(d.x))


def agrees_with_the_dense_reference(**pieces):
    d, got = dense(), converged(**pieces)
    if got is None:
        return False, "rho did not fall by 2^-40 within the budget"
    x, k, rho = got
    err, bound = float(np.linalg.norm(x - d.x)), dense_bound(d, rho)
    return err <= bound, f"{k} iterations, cond {d.cond:.4g}, lambda_min {d.lam_min:.4g}: |x - x*| = {err:.3g} against the bound {bound:.3g} (|x*| = {np.linalg.norm(d.x):.4g})"


def test_the_iterates_converge_to_the_dense_solution_of_the_normal_equations():
    d = dense()
    ok, figures = agrees_with_the_dense_reference()
    print(figures)
    assert d.active.sum() > 300 and 1 < d.cond < 1e8 and d.lam_min > 0
    assert ok, figures
    x, k, rho = converged()
    assert k < 150 and dense_bound(d, rho) < 2.0 ** -16 * np.linalg.norm(d.x)  # the bound is not vacuous: far below the solution's own size


# ---- properties of the solve ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", sc.LAMBDAS)
@pytest.mark.parametrize("name", sorted(sc.all_cases()))
def test_the_objective_never_increases_along_the_iterates(name, lam):
    res, its = sc.longest(name, lam)
    geo, xs = its[0], its[1:]
    F = [sv.objective_on_host(geo, x, lam) for x in xs]
    print(f"{name} lambda {lam}: F = {F}, stopped_at {res.stopped_at}")
    assert all(b <= a + 1e-12 * abs(a) for a, b in zip(F, F[1:]))
    if name.startswith(("planes", "truth", "tiny", "holes")):
        assert F[-1] < 0.99 * F[0] and res.stopped_at == -1


@pytest.mark.parametrize("thickness", sc.THICKNESSES)
def test_thirty_iterations_keep_lowering_the_objective(thickness):
    t = fc.truth_case()
    for lam in (0.0, 1e-3, 1e-2, 1e-1):
        its = []
        res = sv.solve_volume_on_host(t["targets"], t["maps"], fc.TRUTH_GRID, sc.SPACING, iterations=30, lam=lam, thickness=thickness, iterates=its)
        F = [sv.objective_on_host(its[0], x, lam) for x in its[1:]]
        assert res.stopped_at == -1 and all(b <= a + 1e-12 * abs(a) for a, b in zip(F, F[1:])) and F[-1] < 0.9 * F[0], (lam, F)


@pytest.mark.parametrize("name", ["planes-grid1-wgb", "planes-grid1-quarter", "truth-t4", "none", "flagged"])
def test_no_iteration_returns_the_fusions_bits(name):
    args, kw = sc.all_cases()[name]
    got = sv.solve_volume_on_host(*args, iterations=0, lam=0.3, **kw)
    f = fuse.fuse_on_host(*args, **kw)
    assert same(got.volume, f.volume) and same(got.coverage, f.coverage) and same(got.flags, f.flags) and got.stopped_at == -1 and got.history.shape == (1, 2)
    assert np.isnan(got.history[0, 1]) and (got.history[0, 0] > 0) == np.isfinite(f.volume).any()


def test_what_takes_no_part_changes_no_bit():
    d = fc.planes()
    grid = sc.GRIDS[1]
    kw = dict(iterations=3, lam=0.01, weights=d["weights"], intensity=d["intensity"])
    base = sv.solve_volume_on_host(d["targets"], d["maps"], grid, sc.SPACING, **kw)
    targets, w = d["targets"].copy(), d["weights"]
    zero = np.argwhere(w == 0)
    assert len(zero) > 10 and np.isnan(w[fc.NAN_WEIGHT_AT]) and np.isnan(targets[fc.NAN_PIXEL_AT])
    targets[tuple(zero.T)] = 1e30                       # the value of a zero-weight pixel
    targets[fc.NAN_WEIGHT_AT] = -1e30                   # of a NaN-weight pixel
    targets[fc.DEGENERATE_AT] = 7.0                     # of a flagged target
    targets[fc.ZERO_GAIN_AT] = np.inf
    w2 = w.copy()
    w2[fc.NAN_PIXEL_AT] = 5.0                           # the weight of a NaN pixel
    w2[fc.DEGENERATE_AT] = 9.0
    moved = sv.solve_volume_on_host(targets, d["maps"], grid, sc.SPACING, **dict(kw, weights=w2))
    assert same(moved.volume, base.volume) and same(moved.history, base.history) and moved.stopped_at == base.stopped_at == -1
    o = fc.outside_target()                             # an outside target behind the others
    more = sv.solve_volume_on_host(np.concatenate([d["targets"], o["targets"]]), np.concatenate([d["maps"], o["maps"]]), grid, sc.SPACING, iterations=3, lam=0.01,
                                   weights=np.concatenate([w, o["weights"]]), intensity=np.concatenate([d["intensity"], o["intensity"]]))
    assert same(more.volume, base.volume) and same(more.history, base.history) and more.flags.tolist() == base.flags.tolist() + [0]
    fewer = sv.solve_volume_on_host(d["targets"][:fc.M_PLANES], d["maps"][:fc.M_PLANES], grid, sc.SPACING, iterations=3, lam=0.01, weights=w[:fc.M_PLANES],
                                    intensity=d["intensity"][:fc.M_PLANES])   # without the flagged targets
    assert same(fewer.volume, base.volume) and same(fewer.history, base.history)


@pytest.mark.parametrize("name", ["none", "flagged", "outside"])
def test_an_empty_support_stops_at_iteration_zero(name):
    args, kw = sc.all_cases()[name]
    res = sv.solve_volume_on_host(*args, iterations=3, lam=0.01, **kw)
    assert res.stopped_at == 0 and np.isnan(res.volume).all() and (res.history[:, 0] == 0).all() and np.isnan(res.history[:, 1]).all() and not res.coverage.any()


def test_identity_is_solved_by_the_fusion_and_stops():
    i = fc.identity()
    res = sv.solve_volume_on_host(i["targets"], i["maps"], fc.IDENTITY_GRID, sc.SPACING, iterations=2)
    assert res.stopped_at == 0 and same(res.volume, i["targets"]) and not res.history[:, 0].any()


@pytest.mark.parametrize("thickness", sc.THICKNESSES)
def test_on_consistent_data_the_error_falls_strictly(thickness):
    errors = sc.mean_errors(sc.consistent_targets(thickness), thickness, 5)
    print(f"thickness {thickness}: mean |x_k - V| over the support, k = 0 .. 5: {errors} (recorded {sc.CONSISTENT[thickness]})")
    assert all(b < a for a, b in zip(errors, errors[1:])) and errors[5] < 0.1 * errors[0]
    assert np.allclose(errors, sc.CONSISTENT[thickness], rtol=1e-9, atol=0)


@pytest.mark.parametrize("thickness", sc.THICKNESSES)
def test_on_point_samples_the_recorded_figures_hold(thickness):
    """no direction is asserted: at thickness = spacing the first iteration improves on the fusion and the solution settles between the fusion and one
    back-projection step; at spacing / 4 the error rises (the model mismatch of section 5.18)"""
    e = sc.mean_errors(fc.truth_case()["targets"], thickness, 30)
    got = (e[0], e[1], e[5], e[30])
    print(f"thickness {thickness}: mean |x_k - V| after 0, 1, 5, 30 iterations: {got} (recorded {sc.POINT_SAMPLES[thickness]}; one back-projection step {pc.ONE_STEP})")
    assert np.allclose(got, sc.POINT_SAMPLES[thickness], rtol=1e-9, atol=0) and abs(got[0] - fc.TRUTH_ERRORS[thickness][2]) <= 1e-9


# ---- seeded mutants of the rule ------------------------------------------------------------------------------------------------------------------------
def laplacian_sign(geo, v):
    return -sv.laplacian_on_host(geo, v)


def gain_once(geo):
    w = geo.omega_gg / np.where(geo.records.g[:, None] == 0, 1.0, geo.records.g[:, None])   # (w g) g -> w g
    return w


def transpose_without_D(geo, y):
    return sv.transpose_on_host(geo._replace(D=np.ones_like(geo.D)), y)


def row_major_dot(a, b, support):
    s = np.float64(0.0)
    for x in np.where(support, a * b, 0.0).ravel():
        s = s + x
    return s


def a_tap_outside_the_support_counted(geo, v):
    """the forward operator over the taps of the whole grid: voxels outside the support count in the row sums"""
    full = sv.geometry(np.zeros((len(geo.records.flags),) + geo.shape, np.float32), TAPS_MAPS, np.ones(geo.grid, bool), sc.SPACING)
    return sv.forward_on_host(geo._replace(taps=full.taps, D=full.D), v)


TAPS_MAPS = sc.tiny()["maps"]
MUTANTS = {
    "laplacian_sign": (dict(laplacian=laplacian_sign), "dense"),
    "g_in_place_of_g_g": (dict(weight=gain_once), "dense"),
    "D_left_out_of_the_transpose": (dict(transpose=transpose_without_D), "dense"),
    "row_major_dot": (dict(dot=row_major_dot), "bits"),
    "rho_over_rho_new": (dict(beta=lambda rho_new, rho: rho / rho_new), "dense"),
    "a_tap_outside_the_support_counted": (dict(forward=a_tap_outside_the_support_counted), "dense"),
}


@functools.lru_cache(maxsize=None)
def rule_history():
    y = sc.tiny()
    return sv.solve_volume_on_host(y["targets"], y["maps"], sc.TINY_GRID, sc.SPACING, iterations=5, lam=TINY_LAMBDA, weights=y["weights"], intensity=y["intensity"],
                                   start=tiny_start()).history


def rejected(kind, pieces):
    """the checks of this file that the mutant's kind is held against -> it fails at least one"""
    if kind == "bits":   # an order of summation shows in the fp64 history, and almost never through the rounding to float32
        y = sc.tiny()
        got = sv.solve_volume_on_host(y["targets"], y["maps"], sc.TINY_GRID, sc.SPACING, iterations=5, lam=TINY_LAMBDA, weights=y["weights"], intensity=y["intensity"],
                                      start=tiny_start(), **pieces)
        return not same(got.history, rule_history())
    return not agrees_with_the_dense_reference(**pieces)[0]


def test_the_checks_accept_the_rule():
    rule_history.cache_clear()
    assert not rejected("bits", {}) and not rejected("dense", {})


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_checks_reject_every_seeded_mutant(mutant):
    pieces, kind = MUTANTS[mutant]
    rule_history()
    assert rejected(kind, pieces), mutant


# ---- solve_volume_plan.h -------------------------------------------------------------------------------------------------------------------------------
PROG = textwrap.dedent(r"""
    #include <cmath>
    #include <cstdio>
    #include <cstring>
    #include <limits>
    #include <vector>

    #include "solve_volume_plan.h"

    using namespace msiren;

    static int failures = 0;
    #define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

    static msiren_solve_opts good() { return msiren_solve_opts{(int32_t)sizeof(msiren_solve_opts), 3, 4.0, 4.0, 0.0, 0.01}; }

    static bool refused(const SolveArgs& a, const char* word) {
        char msg[256] = "";
        const bool ok = solve_check(a, msg, sizeof msg);
        if (ok || !std::strstr(msg, word)) std::printf("wanted a refusal naming '%s', got %s '%s'\n", word, ok ? "accepted" : "refused", msg);
        return !ok && std::strstr(msg, word);
    }

    int main() {
        static_assert(sizeof(msiren_solve_opts) == 40, "40 bytes");
        // ---- the layout: consecutive, 8-byte aligned blocks, sized by the vectors ----
        for (int64_t m : {0, 1, 8}) {
            const int32_t th = 19, tw = 23, H = 37, W = 45;
            const int64_t n = 5;
            const SolveLayout l = solve_layout(m, th, tw, n, H, W);
            const size_t vox = (size_t)n * H * W * 8, pix = (size_t)m * th * tw * 8;
            CHECK(l.records == 0 && l.x == (size_t)m * kFuseRecord * 8);
            CHECK(l.r == l.x + vox && l.p == l.r + vox && l.q == l.p + vox && l.D == l.q + vox);
            CHECK(l.Wt == l.D + pix && l.z == l.Wt + pix && l.columns == l.z + pix);
            CHECK(l.slices == l.columns + (size_t)n * W * 8 && l.state == l.slices + (size_t)n * 8 && l.total == l.state + kSolveState * 8);
            CHECK(l.total % 8 == 0);
            std::vector<char> block(l.total);  // every offset inside the block: written under the sanitizers
            for (size_t off : {l.records, l.x, l.r, l.p, l.q, l.D, l.Wt, l.z, l.columns, l.slices, l.state}) block[off] = 1;
            block[l.total - 1] = 1;
        }
        CHECK(SOLVE_STOPPED_AT < kSolveState);
        // ---- the launch plan ----
        CHECK(solve_launches(8, false, false, 0) == 1 + 1 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 1);
        CHECK(solve_launches(8, true, false, 0) == solve_launches(8, false, false, 0) - 1);
        CHECK(solve_launches(8, true, true, 0) == solve_launches(8, false, true, 0));
        CHECK(solve_launches(8, false, false, 10) == solve_launches(8, false, false, 0) + 10 * 8);
        CHECK(solve_launches(0, false, false, 10) == 1 + 1 + 1 + 1 + 1 + 2 + 10 * 7 + 1);
        CHECK(solve_dot_blocks(16, 320) == 20 && solve_pointwise_blocks(5, 37, 45) == (5 * 37 * 45 + 255) / 256);
        // ---- the refusals ----
        alignas(16) static const char any[16] = {0};
        msiren_solve_opts o = good();
        const SolveArgs base{any, 8, 19, 23, any, nullptr, nullptr, &o, 4, 40, 40, nullptr, any, nullptr, nullptr, nullptr, nullptr, false};
        char msg[256];
        CHECK(solve_check(base, msg, sizeof msg));
        { SolveArgs a = base; a.opts = nullptr; CHECK(refused(a, "opts")); }
        { SolveArgs a = base; a.volume = nullptr; CHECK(refused(a, "volume")); }
        { SolveArgs a = base; a.targets = nullptr; CHECK(refused(a, "targets")); }
        { SolveArgs a = base; a.maps = nullptr; CHECK(refused(a, "maps")); }
        { SolveArgs a = base; a.m = -1; CHECK(refused(a, "m_targets")); }
        { SolveArgs a = base; a.th = 1; CHECK(refused(a, "th")); }
        { SolveArgs a = base; a.n = 0; CHECK(refused(a, "n_slices")); }
        { SolveArgs a = base; a.H = 0; CHECK(refused(a, "height")); }
        { SolveArgs a = base; a.W = 0; CHECK(refused(a, "width")); }
        { SolveArgs a = base; a.n = 1 << 10, a.H = 1 << 10, a.W = 1 << 10; CHECK(refused(a, "n_slices height width")); }
        { SolveArgs a = base; a.m = 1 << 12, a.th = 1 << 9, a.tw = 1 << 9; CHECK(refused(a, "m_targets th tw")); }
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        { msiren_solve_opts b = good(); b.struct_size = 32; SolveArgs a = base; a.opts = &b; CHECK(refused(a, "struct_size")); }
        for (double bad : {0.0, -1.0, nan, inf}) {
            { msiren_solve_opts b = good(); b.spacing = bad; SolveArgs a = base; a.opts = &b; CHECK(refused(a, "spacing")); }
            { msiren_solve_opts b = good(); b.thickness = bad; SolveArgs a = base; a.opts = &b; CHECK(refused(a, "thickness")); }
        }
        for (double bad : {-1.0, nan}) { msiren_solve_opts b = good(); b.min_coverage = bad; SolveArgs a = base; a.opts = &b; CHECK(refused(a, "min_coverage")); }
        for (double bad : {-1e-300, nan, inf, -inf}) { msiren_solve_opts b = good(); b.lambda = bad; SolveArgs a = base; a.opts = &b; CHECK(refused(a, "lambda")); }
        for (int bad : {-1, kSolveMaxIterations + 1}) { msiren_solve_opts b = good(); b.iterations = bad; SolveArgs a = base; a.opts = &b; CHECK(refused(a, "iterations")); }
        for (int okay : {0, kSolveMaxIterations}) { msiren_solve_opts b = good(); b.iterations = okay; SolveArgs a = base; a.opts = &b; CHECK(solve_check(a, msg, sizeof msg)); }
        { SolveArgs a = base; a.m = 0, a.targets = a.maps = nullptr, a.th = a.tw = 0; CHECK(solve_check(a, msg, sizeof msg)); }   // no target is valid
        // alignment: only of device pointers
        alignas(16) static const char buf[64] = {0};
        { SolveArgs a = base; a.start = buf + 2; CHECK(solve_check(a, msg, sizeof msg)); a.device = true; CHECK(refused(a, "start")); }
        { SolveArgs a = base; a.device = true; a.history = buf + 4; CHECK(refused(a, "history")); a.history = buf + 8; CHECK(solve_check(a, msg, sizeof msg)); }
        { SolveArgs a = base; a.device = true; a.stopped_at = buf + 2; CHECK(refused(a, "stopped_at")); }
        { SolveArgs a = base; a.device = true; a.volume = buf + 2; CHECK(refused(a, "volume")); }
        { SolveArgs a = base; a.device = true; a.coverage = buf + 1; CHECK(refused(a, "coverage")); }
        { SolveArgs a = base; a.device = true; a.weights = buf + 3; CHECK(refused(a, "weights")); }
        if (failures) return 1;
        std::puts("ok");
        return 0;
    }
""")


@pytest.fixture(scope="module")
def plan_programs(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    d = tmp_path_factory.mktemp("solve_volume_plan")
    src = d / "solve_volume_plan.cpp"
    src.write_text(PROG)
    exes = {}
    for name, extra in (("plain", ["-O1"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[name] = d / name
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "mri_inr_amd", "csrc"), str(src), "-o", str(exes[name])], check=True,
                       capture_output=True, text=True)
    return exes


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_plan_header_stands_alone(plan_programs, build):
    res = subprocess.run([str(plan_programs[build])], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
