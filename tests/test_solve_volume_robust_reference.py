"""msiren_solve_volume_r's rule on the CPU (no GPU needed): mri_inr_amd/solve_volume_robust.py: solve_volume_robust_on_host, the
normative restatement that tests/test_gpu_solve_volume_robust.py holds the device to bit for bit, is held here against what it has to mean --

    one round under the quadratic loss is solve_volume_on_host, bit for bit; no round and no iteration return the start;
    omega is exactly 1 under the quadratic loss and the schedule ends on exactly 1;
    at a fixed scale the robust objective never rises from round to round (the majorisation property), on every case and lambda;
    on a case small enough for a dense matrix each round converges to the solution of that round's normal equations, with the weights formed by an
    independent formulation (tests/solve_volume_r_reference.py), within section 5.19's bound from the round's measured condition number;
    on the corrupted truth case the annealed solve removes the outliers' error, rejects the corrupted pixels and ranks the corrupted targets lowest;
    seeded mutants of every piece of the rule are rejected by these checks;
    solve_volume_r_plan.h, stand-alone, also under the address and undefined-behaviour sanitizers."""
import functools
import os
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

import fuse_cases as fc
import solve_volume_cases as sc
import solve_volume_r_cases as rc
import solve_volume_r_reference as rr
from mri_inr_amd import fuse
from mri_inr_amd import solve_volume as sv
from mri_inr_amd import solve_volume_robust as svr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- what the rule reduces to --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", rc.LAMBDAS)
@pytest.mark.parametrize("name", rc.NAMES)
def test_one_round_under_the_quadratic_loss_is_the_quadratic_solve_bit_for_bit(name, lam):
    args, kw = sc.all_cases()[name]
    for iterations in (0, 2):
        want = sv.solve_volume_on_host(*args, iterations=iterations, lam=lam, **kw)
        got = svr.solve_volume_robust_on_host(*args, INF, rounds=1, iterations=iterations, anneal=4.0, lam=lam, **kw)
        assert same(got.volume, want.volume) and same(got.coverage, want.coverage) and same(got.flags, want.flags)
        assert got.history.shape == (1, iterations + 1, 2) and same(got.history[0], want.history) and got.stopped_at.tolist() == [want.stopped_at]
        taking_part = np.isfinite(got.rweight)
        assert (got.rweight[taking_part] == 1.0).all() and same(got.stats[:, 1], got.stats[:, 2])  # omega = 1: sum w omega is sum w


@pytest.mark.parametrize("name", ["tiny", "planes-grid1-quarter", "holes-grid1", "none", "flagged"])
def test_no_round_and_no_iteration_return_the_start(name):
    args, kw = rc.all_cases()[name]
    first = kw["start"] if "start" in kw else fuse.fuse_on_host(*args[:4], **kw).volume
    for rounds, iterations in ((0, 0), (0, 2), (1, 0), (3, 0)):
        got = svr.solve_volume_robust_on_host(*args, rounds=rounds, iterations=iterations, anneal=4.0, lam=0.01, **kw)
        assert same(got.volume, np.where(np.isfinite(first), first, np.float32(np.nan))) and got.history.shape == (rounds, iterations + 1, 2)
        assert got.stopped_at.shape == (rounds,) and (got.stopped_at == -1).all()
        assert np.isnan(got.history[:, :, 1]).all() and not np.isnan(got.history[:, :, 0]).any()


def test_omega_is_exactly_one_under_the_quadratic_loss_and_the_schedule_ends_on_one():
    e = np.array([0.0, 1e-300, -3.5, 1e150, -1e154])
    om, omega = svr.robust_weight(e, np.float64(INF))
    assert (om == 1.0).all() and (omega == 1.0).all()
    om, omega = svr.robust_weight(np.float64(3.0), np.float64(9.0))
    assert om == 0.5 and omega == 0.25
    for rounds in (1, 2, 5, 64):
        for anneal in (1.0, 4.0, 1.5, 1e308):
            c = svr.schedule(rounds, anneal)
            with np.errstate(over="ignore"):
                assert c.shape == (rounds,) and c[-1] == 1.0 and all(c[t] == c[t + 1] * anneal for t in range(rounds - 1))
    assert svr.schedule(5, 4.0).tolist() == [256.0, 64.0, 16.0, 4.0, 1.0] and svr.schedule(0, 4.0).shape == (0,)


def test_a_scale_that_is_not_positive_switches_its_target_off():
    args, kw = rc.all_cases()["tiny"]
    got = svr.solve_volume_robust_on_host(*args, rounds=2, iterations=2, anneal=4.0, lam=0.01, **kw)
    assert args[4][1] == INF and not (args[4][2:] > 0).any()
    assert np.isfinite(got.rweight[:2]).sum() > 150 and np.isnan(got.rweight[2:]).all() and not got.stats[2:].any() and (got.stats[:2, 0] > 50).all()
    fewer = svr.solve_volume_robust_on_host(args[0][:2], args[1][:2], args[2], args[3], args[4][:2], rounds=2, iterations=2, anneal=4.0, lam=0.01,
                                            thickness=kw["thickness"], weights=kw["weights"][:2], intensity=kw["intensity"][:2],
                                            start=fuse.fuse_on_host(*args[:4], **kw).volume)  # (the same support)
    with_start = svr.solve_volume_robust_on_host(*args, rounds=2, iterations=2, anneal=4.0, lam=0.01, start=fuse.fuse_on_host(*args[:4], **kw).volume, **kw)
    assert same(fewer.volume, with_start.volume) and same(fewer.history, with_start.history) and same(with_start.volume, got.volume)


# ---- the majorisation property -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", rc.LAMBDAS)
@pytest.mark.parametrize("name", rc.NAMES)
def test_at_a_fixed_scale_the_objective_never_rises_from_round_to_round(name, lam):
    """rho_s is concave in e^2 and omega is its slope there: the reweighted quadratic lies above the robust objective and touches it at the round's
    first iterate, and every step of conjugate gradients lowers that quadratic"""
    args, kw = rc.all_cases()[name]
    rounds, iterations = max(rc.ROUNDS), max(rc.ITERATIONS)
    res, its = rc.run(name, lam, 1.0, rounds, iterations)
    geo, xs = its[0], its[1:]
    F = [svr.robust_objective_on_host(geo, xs[t * iterations], args[0], kw.get("weights"), args[4], lam) for t in range(rounds + 1)]
    print(f"{name} lambda {lam}: F = {F}, stopped_at {res.stopped_at.tolist()}")
    assert all(b <= a + 1e-12 * abs(a) for a, b in zip(F, F[1:]))
    if name.startswith(("planes", "tiny", "holes", "tall")):
        assert F[-1] < 0.99 * F[0] and (res.stopped_at == -1).all()


# ---- the dense reference -------------------------------------------------------------------------------------------------------------------------------
DENSE = dict(scale=0.05, anneal=4.0, lam=0.01, rounds=2, iterations=150)


def tiny_start():
    """the tiny case from a start with holes: the support is not the whole grid"""
    y = sc.tiny()
    start = fuse.fuse_on_host(y["targets"], y["maps"], sc.TINY_GRID, sc.SPACING, weights=y["weights"], intensity=y["intensity"]).volume.copy()
    start[1, 3:5, 4:7] = np.nan
    start[0, 8, 2] = np.inf
    return start


def dense_rounds(**pieces):
    """the restatement's rounds on the tiny case, each run until rho has fallen by 2^-40, against the dense solution of that round's normal equations with
    the weights formed from the iterate that entered it -> [(ok, figures) per round]"""
    y = sc.tiny()
    K, lam = DENSE["iterations"], DENSE["lam"]
    its = []
    res = svr.solve_volume_robust_on_host(y["targets"], y["maps"], sc.TINY_GRID, sc.SPACING, DENSE["scale"], rounds=DENSE["rounds"], iterations=K, anneal=DENSE["anneal"],
                                          lam=lam, weights=y["weights"], intensity=y["intensity"], start=tiny_start(), iterates=its, **pieces)
    geo, xs = its[0], its[1:]
    c = svr.schedule(DENSE["rounds"], DENSE["anneal"])
    out = []
    for t in range(DENSE["rounds"]):
        rho = res.history[t, :, 0]
        below = np.nonzero(rho <= 2.0 ** -40 * rho[0])[0]
        if not len(below) or (0 <= res.stopped_at[t] < below[0]):
            out.append((False, f"round {t}: rho did not fall by 2^-40 within {K} iterations"))
            continue
        k = int(below[0])
        x = xs[t * K + k]
        d = rr.solve_round(y["targets"], y["maps"], geo.support, sc.SPACING, xs[t * K], DENSE["scale"] * c[t], lam=lam, thickness=sc.SPACING, weights=y["weights"],
                           intensity=y["intensity"])
        # section 5.19's bound: |x_k - x*| <= sqrt(rho_k) / lambda_min for the iteration's own residual, and 2^-36 cond |x*| for the rounding that the
        # condition number amplifies (the recurrence's drift, np.linalg.solve, the two formulations of P and of omega)
        err, bound = float(np.linalg.norm(x - d.x)), np.sqrt(rho[k]) / d.lam_min + 2.0 ** -36 * d.cond * float(np.linalg.norm(d.x))
        omega_mean = float(d.omega[d.active].mean())
        out.append((bool(err <= bound and 1 < d.cond < 1e8 and d.lam_min > 0 and bound < 2.0 ** -16 * np.linalg.norm(d.x)),
                    f"round {t}: {k} iterations, cond {d.cond:.4g}, lambda_min {d.lam_min:.4g}, mean omega {omega_mean:.4g}: |x - x*| = {err:.3g} against the bound "
                    f"{bound:.3g} (|x*| = {np.linalg.norm(d.x):.4g})"))
    return out


def test_every_round_converges_to_the_dense_solution_of_its_normal_equations():
    """measured: round 0 (scale 0.2), 41 iterations, cond 91.49, lambda_min 0.03606, mean omega 0.9213: |x - x*| = 4.54e-06 against the bound 3.07e-05;
    round 1 (scale 0.05), 42 iterations, cond 90.29, lambda_min 0.0361, mean omega 0.9061: |x - x*| = 4.98e-07 against the bound 3.18e-06 (|x*| = 39.1).
    The bound is sqrt(rho) / lambda_min almost alone (2^-36 cond |x*| is 5e-08): it is not vacuous, 2^-16 |x*| is 6e-04"""
    got = dense_rounds()
    for ok, figures in got:
        print(figures)
    assert len(got) == DENSE["rounds"] and all(ok for ok, _ in got), got


# ---- efficacy ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_annealed_solve_removes_the_outliers_on_the_corrupted_truth_case():
    f = rc.corrupted_figures()
    print({k: v for k, v in f.items() if k != "ratio"}, "sum w omega / sum w:", f["ratio"].tolist())
    assert f["robust_mean"] < 0.1 * f["quadratic_mean"]
    assert f["rweight_inside"] < 0.01 and f["rweight_outside"] > 0.9
    assert sorted(np.argsort(f["ratio"])[:len(rc.CORRUPT_TARGETS)].tolist()) == list(rc.CORRUPT_TARGETS)
    for key, recorded in rc.MEASURED.items():
        assert np.isclose(f[key], recorded, rtol=1e-6, atol=0), (key, f[key], recorded)


# ---- seeded mutants of the rule ------------------------------------------------------------------------------------------------------------------------
def stops_then_goes_on(**pieces):
    """Two flat targets on one slice with unit maps, T = 1 with weight 3 and T = 5 with weight 1: P is the identity, the fusion x = 2 solves the
    quadratic problem exactly (every operation is exact), so round 0, whose scale 1e308 leaves omega = 1.0, stops at iteration 0 with rho == 0.  Round 1
    has the scale 1: omega = 1 / 4 and 1 / 100, the residual is not 0 and the round takes its step -> the rule holds this"""
    shape, grid = fc.SHAPE, (1,) + fc.SHAPE
    targets = np.stack([np.full(shape, 1.0, np.float32), np.full(shape, 5.0, np.float32)])
    weights = np.stack([np.full(shape, 3.0, np.float32), np.full(shape, 1.0, np.float32)])
    maps = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]] * 2, np.float32)
    res = svr.solve_volume_robust_on_host(targets, maps, grid, sc.SPACING, 1.0, rounds=2, iterations=1, anneal=1e308, weights=weights, **pieces)
    went_on = res.stopped_at.tolist() == [0, -1] and res.history[0, 0, 0] == 0 and res.history[1, 0, 0] > 0 and bool((res.volume < 2.0).all())
    return went_on and bool((np.abs(res.volume - 1.0) < 0.2).all())  # (towards the heavier target)


def stats_are_summed_in_the_rules_order(**pieces):
    args, kw = rc.all_cases()["planes-grid0-wgb"]
    res, its = rc.run("planes-grid0-wgb", 0.01, 4.0, 2, 2)
    geo, x = its[0], its[-1]
    rew = svr.reweight_on_host(geo, x, args[0], args[4])
    th, tw = geo.shape
    w = kw["weights"].astype(np.float64).reshape(len(args[0]), th, tw)
    om, e, counts = (a.reshape(len(args[0]), th, tw) for a in (rew.om, rew.e, rew.counts))
    want = np.zeros((len(args[0]), 4))
    for q in range(len(args[0])):
        for k in range(4):
            total = np.float64(0.0)
            for j in range(tw):
                col = np.float64(0.0)
                for i in range(th):
                    if counts[q, i, j]:
                        col = col + (1.0, w[q, i, j], w[q, i, j] * (om[q, i, j] * om[q, i, j]), ((w[q, i, j] * om[q, i, j]) * e[q, i, j]) * e[q, i, j])[k]
                total = total + col
            want[q, k] = total
    got = svr.robust_stats_on_host(kw["weights"], rew, (th, tw), **pieces)
    return same(got, want) and same(got, res.stats) and bool((want[:2, 0] > 100).all())


def efficacy(**pieces):
    """the corrupted truth case's mean error against the clean solve, as a fraction of the quadratic solve's -> the issue's bound of one tenth holds"""
    f, c = rc.corrupted_figures(), rc.corrupted()
    its = []
    sv.solve_volume_on_host(c["clean"], c["maps"], fc.TRUTH_GRID, sc.SPACING, iterations=15, lam=rc.CORRUPT_SETTING["lam"], thickness=sc.SPACING, iterates=its)
    S, x_clean = its[0].support, its[-1]
    its = []
    svr.solve_volume_robust_on_host(c["targets"], c["maps"], fc.TRUTH_GRID, sc.SPACING, 1.0, thickness=sc.SPACING, iterates=its, **rc.CORRUPT_SETTING, **pieces)
    error = float(np.abs(its[-1] - x_clean)[S].mean())
    print(f"mean error {error:.4g} against the quadratic solve's {f['quadratic_mean']:.4g}")
    return error < 0.1 * f["quadratic_mean"]


def dense(**pieces):
    return all(ok for ok, _ in dense_rounds(**pieces))


def schedule_ends_on_one(schedule_of=svr.schedule):
    return schedule_of(5, 4.0)[-1] == 1.0 and schedule_of(5, 4.0)[0] == 256.0


def om_once(e, s):
    om, _ = svr.robust_weight(e, s)
    return om, om


def frozen_after_round_0(geo, x, s, t, before):
    return before if before is not None else svr.reweight_on_host(geo, x, rc.corrupted()["targets"], s)


MUTANTS = {
    "om_in_place_of_om_om": (dict(weight=om_once), dense),
    "the_residual_without_gain_and_bias": (dict(residual=lambda T, u, g, bias: T - u), dense),
    "the_schedule_reversed": (dict(schedule_of=lambda rounds, anneal: svr.schedule(rounds, anneal)[::-1]), schedule_ends_on_one),
    "weights_frozen_after_round_0": (dict(reweight=frozen_after_round_0), efficacy),
    "the_right_hand_side_on_the_previous_rounds_weights": (dict(rhs_weights=lambda now, before: now.Wt if before is None else before.Wt), dense),
    "the_stop_state_not_reset": (dict(stop_state=lambda stopped: stopped), stops_then_goes_on),
    "each_round_restarted_from_the_fusion": (dict(entering=lambda x, x0, t: x0), efficacy),
    "row_major_stats": (dict(stats_sum=lambda terms: functools.reduce(lambda s, v: s + v, terms.ravel(), np.float64(0.0))), stats_are_summed_in_the_rules_order),
}


def test_the_checks_accept_the_rule():
    assert dense() and schedule_ends_on_one() and efficacy() and stops_then_goes_on() and stats_are_summed_in_the_rules_order()


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_checks_reject_every_seeded_mutant(mutant):
    pieces, check = MUTANTS[mutant]
    assert not check(**pieces), mutant


# ---- solve_volume_r_plan.h -----------------------------------------------------------------------------------------------------------------------------
PROG = textwrap.dedent(r"""
    #include <cmath>
    #include <cstdio>
    #include <cstring>
    #include <limits>
    #include <vector>

    #include "solve_volume_r_plan.h"

    using namespace msiren;

    static int failures = 0;
    #define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

    static msiren_solve_r_opts good() { return msiren_solve_r_opts{(int32_t)sizeof(msiren_solve_r_opts), 3, 2, 0, 4.0, 4.0, 0.0, 0.01, 4.0}; }

    static bool refused(const SolveRArgs& a, const char* word) {
        char msg[256] = "";
        const bool ok = solve_r_check(a, msg, sizeof msg);
        if (ok || !std::strstr(msg, word)) std::printf("wanted a refusal naming '%s', got %s '%s'\n", word, ok ? "accepted" : "refused", msg);
        return !ok && std::strstr(msg, word);
    }

    int main() {
        static_assert(sizeof(msiren_solve_r_opts) == 56, "56 bytes");
        static_assert(sizeof(msiren_solve_opts) == 40, "40 bytes");
        // ---- the layout: section 5.19's block, then two pixel vectors and the columns of the stats ----
        for (int64_t m : {0, 1, 8}) {
            const int32_t th = 19, tw = 23, H = 37, W = 45;
            const int64_t n = 5;
            const SolveRLayout l = solve_r_layout(m, th, tw, n, H, W);
            const SolveLayout b = solve_layout(m, th, tw, n, H, W);
            const size_t pix = (size_t)m * th * tw * 8;
            CHECK(std::memcmp(&l.base, &b, sizeof b) == 0);
            CHECK(l.Wt0 == b.total && l.zp == l.Wt0 + pix && l.stat_columns == l.zp + pix && l.total == l.stat_columns + (size_t)m * tw * kSolveRSums * 8);
            CHECK(l.total % 8 == 0);
            std::vector<char> block(l.total);  // every offset inside the block: written under the sanitizers
            for (size_t off : {b.records, b.x, b.r, b.p, b.q, b.D, b.Wt, b.z, b.columns, b.slices, b.state}) block[off] = 1;
            if (m > 0)
                for (size_t off : {l.Wt0, l.zp, l.stat_columns}) block[off] = 1;
            block[l.total - 1] = 1;
        }
        // ---- the schedule ----
        {
            double c[kSolveRMaxRounds];
            solve_r_schedule(5, 4.0, c);
            CHECK(c[0] == 256.0 && c[1] == 64.0 && c[2] == 16.0 && c[3] == 4.0 && c[4] == 1.0);
            solve_r_schedule(kSolveRMaxRounds, 1.5, c);
            CHECK(c[kSolveRMaxRounds - 1] == 1.0 && c[kSolveRMaxRounds - 2] == 1.5 && c[0] == c[1] * 1.5);
            solve_r_schedule(3, 1e308, c);
            CHECK(std::isinf(c[0]) && c[1] == 1e308 && c[2] == 1.0);
            solve_r_schedule(0, 4.0, c);  // (writes nothing)
        }
        // ---- the launch plan ----
        CHECK(solve_r_launches(8, false, false, 0, 0, false) == 1 + 1 + 1 + 1 + 1);                       // set-up, fusion, start, coverage, store
        CHECK(solve_r_launches(8, true, false, 0, 5, false) == solve_r_launches(8, false, false, 0, 5, false) - 1);
        CHECK(solve_r_launches(8, true, true, 0, 0, false) == solve_r_launches(8, false, true, 0, 0, false));
        CHECK(solve_r_launches(8, false, false, 1, 0, false) == 5 + 7);                                   // reweight, 2 transposes, residual, 2 for <r, r>, stop
        CHECK(solve_r_launches(8, false, false, 3, 2, false) == 5 + 3 * (7 + 2 * 8));
        CHECK(solve_r_launches(8, false, false, 3, 2, true) == solve_r_launches(8, false, false, 3, 2, false) + 2);
        CHECK(solve_r_launches(0, false, false, 3, 2, true) == 1 + 1 + 3 * (6 + 2 * 7) + 1);              // no gather, no set-up, no final pass without targets
        // one round is the plain solve's sequence with the reweighting in place of the second forward gather, and the stop kernel
        CHECK(solve_r_launches(8, false, false, 1, 10, false) == solve_launches(8, false, false, 10) + 1);
        // ---- the refusals ----
        alignas(16) static const char any[16] = {0};
        msiren_solve_r_opts o = good();
        const SolveRArgs base{any, 8, 19, 23, any, nullptr, nullptr, any, &o, 4, 40, 40, nullptr, any, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false};
        char msg[256];
        CHECK(solve_r_check(base, msg, sizeof msg));
        { SolveRArgs a = base; a.opts = nullptr; CHECK(refused(a, "opts")); }
        { SolveRArgs a = base; a.volume = nullptr; CHECK(refused(a, "volume")); }
        { SolveRArgs a = base; a.targets = nullptr; CHECK(refused(a, "targets")); }
        { SolveRArgs a = base; a.maps = nullptr; CHECK(refused(a, "maps")); }
        { SolveRArgs a = base; a.scale = nullptr; CHECK(refused(a, "scale")); }
        { SolveRArgs a = base; a.m = -1; CHECK(refused(a, "m_targets")); }
        { SolveRArgs a = base; a.th = 1; CHECK(refused(a, "th")); }
        { SolveRArgs a = base; a.n = 0; CHECK(refused(a, "n_slices")); }
        { SolveRArgs a = base; a.H = 0; CHECK(refused(a, "height")); }
        { SolveRArgs a = base; a.W = 0; CHECK(refused(a, "width")); }
        { SolveRArgs a = base; a.n = 1 << 10, a.H = 1 << 10, a.W = 1 << 10; CHECK(refused(a, "n_slices height width")); }
        { SolveRArgs a = base; a.m = 1 << 12, a.th = 1 << 9, a.tw = 1 << 9; CHECK(refused(a, "m_targets th tw")); }
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        for (int bad : {40, 48, 64}) { msiren_solve_r_opts b = good(); b.struct_size = bad; SolveRArgs a = base; a.opts = &b; CHECK(refused(a, "struct_size")); }
        for (double bad : {0.0, -1.0, nan, inf}) {
            { msiren_solve_r_opts b = good(); b.spacing = bad; SolveRArgs a = base; a.opts = &b; CHECK(refused(a, "spacing")); }
            { msiren_solve_r_opts b = good(); b.thickness = bad; SolveRArgs a = base; a.opts = &b; CHECK(refused(a, "thickness")); }
        }
        for (double bad : {-1.0, nan}) { msiren_solve_r_opts b = good(); b.min_coverage = bad; SolveRArgs a = base; a.opts = &b; CHECK(refused(a, "min_coverage")); }
        for (double bad : {-1e-300, nan, inf, -inf}) { msiren_solve_r_opts b = good(); b.lambda = bad; SolveRArgs a = base; a.opts = &b; CHECK(refused(a, "lambda")); }
        for (int bad : {-1, kSolveMaxIterations + 1}) { msiren_solve_r_opts b = good(); b.iterations = bad, b.rounds = 1; SolveRArgs a = base; a.opts = &b; CHECK(refused(a, "iterations")); }
        for (int bad : {-1, kSolveRMaxRounds + 1}) { msiren_solve_r_opts b = good(); b.rounds = bad, b.iterations = 1; SolveRArgs a = base; a.opts = &b; CHECK(refused(a, "rounds")); }
        { msiren_solve_r_opts b = good(); b.rounds = 64, b.iterations = 17; SolveRArgs a = base; a.opts = &b; CHECK(refused(a, "rounds x opts->iterations")); }
        { msiren_solve_r_opts b = good(); b.rounds = 2, b.iterations = 513; SolveRArgs a = base; a.opts = &b; CHECK(refused(a, "rounds x opts->iterations")); }
        for (double bad : {0.999, 0.0, -4.0, nan, inf, -inf}) { msiren_solve_r_opts b = good(); b.anneal = bad; SolveRArgs a = base; a.opts = &b; CHECK(refused(a, "anneal")); }
        for (int r : {0, 1, 64}) { msiren_solve_r_opts b = good(); b.rounds = r, b.iterations = 16; SolveRArgs a = base; a.opts = &b; CHECK(solve_r_check(a, msg, sizeof msg)); }
        { msiren_solve_r_opts b = good(); b.rounds = 1, b.iterations = kSolveMaxIterations; SolveRArgs a = base; a.opts = &b; CHECK(solve_r_check(a, msg, sizeof msg)); }
        { msiren_solve_r_opts b = good(); b.rounds = 0, b.iterations = kSolveMaxIterations; SolveRArgs a = base; a.opts = &b; CHECK(solve_r_check(a, msg, sizeof msg)); }
        { msiren_solve_r_opts b = good(); b.anneal = 1.0; SolveRArgs a = base; a.opts = &b; CHECK(solve_r_check(a, msg, sizeof msg)); }
        { SolveRArgs a = base; a.m = 0, a.targets = a.maps = a.scale = nullptr, a.th = a.tw = 0; CHECK(solve_r_check(a, msg, sizeof msg)); }   // no target is valid
        // alignment: only of device pointers
        alignas(16) static const char buf[64] = {0};
        { SolveRArgs a = base; a.start = buf + 2; CHECK(solve_r_check(a, msg, sizeof msg)); a.device = true; CHECK(refused(a, "start")); }
        { SolveRArgs a = base; a.scale = buf + 4; CHECK(solve_r_check(a, msg, sizeof msg)); a.device = true; CHECK(refused(a, "scale")); a.scale = buf + 8; CHECK(solve_r_check(a, msg, sizeof msg)); }
        { SolveRArgs a = base; a.device = true; a.history = buf + 4; CHECK(refused(a, "history")); a.history = buf + 8; CHECK(solve_r_check(a, msg, sizeof msg)); }
        { SolveRArgs a = base; a.device = true; a.stats = buf + 4; CHECK(refused(a, "stats")); a.stats = buf + 8; CHECK(solve_r_check(a, msg, sizeof msg)); }
        { SolveRArgs a = base; a.device = true; a.stopped_at = buf + 2; CHECK(refused(a, "stopped_at")); }
        { SolveRArgs a = base; a.device = true; a.rweight = buf + 2; CHECK(refused(a, "rweight")); a.rweight = buf + 4; CHECK(solve_r_check(a, msg, sizeof msg)); }
        { SolveRArgs a = base; a.device = true; a.residual = buf + 1; CHECK(refused(a, "residual")); a.residual = buf + 4; CHECK(solve_r_check(a, msg, sizeof msg)); }
        { SolveRArgs a = base; a.device = true; a.volume = buf + 2; CHECK(refused(a, "volume")); }
        { SolveRArgs a = base; a.device = true; a.coverage = buf + 1; CHECK(refused(a, "coverage")); }
        { SolveRArgs a = base; a.device = true; a.weights = buf + 3; CHECK(refused(a, "weights")); }
        if (failures) return 1;
        std::puts("ok");
        return 0;
    }
""")


@pytest.fixture(scope="module")
def plan_programs(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    d = tmp_path_factory.mktemp("solve_volume_r_plan")
    src = d / "solve_volume_r_plan.cpp"
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
