"""The grouped rigid solve on the CPU (no GPU needed): the step rule of msiren_align_volume_solve_group as
mri_inr_amd/align_group.py restates it.  All-singleton groups with the intensity fixed replay align_volume.lm_step_vw bit for bit; the Schur
complement step agrees with a dense solve of the damped (6 + 2 size) system to a bound derived from that system's condition number; the validation of
group_start (csrc/align_plan.h) in a stand-alone compiled program; convergence of the loop on the fp64 reference, the variant loop that sizes the
device's gate, the member that never sees the volume, the group that lies wholly outside, and seeded mutants of the rule against convergence and
replay.  Cases: tests/align_group_cases.py."""
import os
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

import align_group_cases as gc
import align_volume_cases as avc
import align_volume_w_cases as wc
from mri_inr_amd import align, align_group as ag, align_volume as av

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def test_the_cases_are_what_the_cases_file_says():
    pl, tr = gc.planes(), gc.truth()
    assert pl.shape == (gc.M, 12) and gc.GROUP_START.tolist() == [0, 3, 4, 6] and gc.SIZES == (3, 1, 2)
    for y in range(gc.G):  # one physical motion per group: the same centre in every member's plane
        assert (pl[gc.GROUP_START[y]:gc.GROUP_START[y + 1], 9:] == pl[gc.GROUP_START[y], 9:]).all()
    z = [av.map_points3(tr[q], gc.SHAPE)[:, 0] for q in range(gc.M)]
    assert np.floor(z[1].min()) != np.floor(z[1].max()) and np.floor(z[1].min()) == 0.0  # the middle plane of group 0 crosses Z = 1
    assert z[gc.OUTSIDE].max() < 0.0 and av.map_points3(gc.start_maps()[gc.OUTSIDE], gc.SHAPE)[:, 0].max() < 0.0  # wholly outside the stack
    assert all(0.0 < z[q].min() and z[q].max() < gc.N - 1 for q in range(gc.M) if q != gc.OUTSIDE)
    assert np.linalg.norm(gc.ROTVECS[0]) == np.linalg.norm(avc.ROTVECS[0]) and 0.0 < abs(gc.SHIFTS3[0][0]) / gc.SPACING < 1.0  # a sub-slice through-plane shift
    tg = gc.reference_targets("morlet3")
    assert np.isnan(tg[gc.OUTSIDE]).all() and np.isfinite(tg[:gc.OUTSIDE]).all() and not (gc.weights()[(slice(None),) + wc.BLOCK]).any()
    assert ag.group_offsets(gc.SIZES, gc.M) == gc.GROUP_START.tolist() == ag.group_offsets(gc.GROUP_START, gc.M)
    for bad in ([0, 3, 3, 6], [1, 3, 6], [0, 3, 5], [], [3, 0, 3], [0, 6, 4, 6]):
        with pytest.raises(ValueError):
            ag.group_offsets(bad, gc.M)


def test_singleton_groups_with_fixed_intensity_replay_lm_step_vw_bit_for_bit():
    """lm_step_g with one group per target beside lm_step_vw (rigid, intensity fixed) on the fp64 reference, over a full trace: every trial map, rigid
    state, lambda, decision and flag is the same"""
    model, rows, iterations = "morlet3", [1, 3, 4], 8
    run, tg, w, gb = gc.reference_cost(model), gc.reference_targets(model)[rows], gc.weights()[rows], gc.GB_TRUTH[rows]
    pl, rigid = gc.planes()[rows], gc.start_rigid(len(rows))
    og, ow = gc.options(av.FIXED, iterations=iterations), wc.options(align.RIGID, av.FIXED, iterations=iterations)
    gs, ts = ag.lm_init_g(og, [0, 1, 2, 3], rigid, pl, gb)
    sw = [av.lm_init_vw(ow, None, rigid[q], pl[q], gb[q]) for q in range(len(rows))]
    for k in range(iterations):
        trial = np.array([t["trial"] for t in ts], np.float32)
        assert np.array_equal(trial, np.array([x["trial"] for x in sw], np.float32))
        sums = run(trial, gb, tg, w)
        ag.lm_step_g(gs, ts, sums, k, og)
        for q in range(len(rows)):
            av.lm_step_vw(sw[q], sums[q], k, ow)
            for key in ("rigid_trial", "rigid_best", "mean_best", "mean_first", "lam", "accepted", "flags"):
                assert gs[q][key] == sw[q][key], (k, q, key)
            for key in ("trial", "best", "gb_trial", "gb_best", "sums"):
                assert ts[q][key] == sw[q][key], (k, q, key)
    assert all(g["accepted"] >= 3 for g in gs)
    rep, trep = ag.report_g(gs, ts)
    assert np.array_equal(rep, av.report_vw(sw)) and np.array_equal(trep, np.array([x["sums"][:3] for x in sw]))


def dense_system(rec, lam):
    """the damped joint system over (w, u, (g, b) of every eliminating member) of one group's records, dense, and its right-hand side"""
    elim = [i for i, r in enumerate(rec) if r[4]]
    n = 6 + 2 * len(elim)
    A, rhs = np.zeros((n, n)), np.zeros(n)
    for tq, HQ, X, y, e in rec:
        H = np.array(HQ)
        H = np.tril(H) + np.tril(H, -1).T
        A[:6, :6] += H[:6, :6]
        rhs[:6] += -0.5 * np.array(tq[:6])
    for j, i in enumerate(elim):
        tq, HQ = rec[i][0], np.array(rec[i][1])
        H = np.tril(HQ) + np.tril(HQ, -1).T
        s = slice(6 + 2 * j, 8 + 2 * j)
        A[s, s], A[s, :6], A[:6, s], rhs[s] = H[6:8, 6:8], H[6:8, :6], H[6:8, :6].T, -0.5 * np.array(tq[6:8])
    return A + lam * np.diag(np.diag(A)), rhs, elim


def records_at(model, rows, rigid_rows, est, lam=1e-3):
    """the records of one group (targets ``rows``) at the state ``rigid_rows`` on the fp64 reference, intensity (1, 0)"""
    run, tg, w, pl = gc.reference_cost(model), gc.reference_targets(model)[rows], gc.weights()[rows], gc.planes()[rows]
    maps = np.array([av.rigid_map3([float(x) for x in rigid_rows], [float(x) for x in p], gc.SPACING) for p in pl], np.float32)
    sums = run(maps, np.tile(np.array([1.0, 0.0], np.float32), (len(rows), 1)), tg, w)
    o = gc.options(est)
    return ag.project_group([[float(x) for x in s] for s in sums], [[float(x) for x in p] for p in pl], [float(x) for x in rigid_rows], lam, o), sums


@pytest.mark.parametrize("rows,lam", [([0, 1, 2], 1e-3), ([0, 1, 2], 1e-7), ([4, 5], 1e-3)])
def test_the_schur_step_is_the_dense_solve_of_the_joint_system(rows, lam):
    """Estimated intensity: d and every (dg, db) of the rule against numpy's solve of the damped (6 + 2 size) system on the same projected records.
    Both are backward stable solves of that system (the elimination of the 2 x 2 blocks is part of a block L D L^T), so each is within about
    n eps cond(A) |x| of the exact solution; the bound asserted is 16 eps cond(A) max|x| with cond(A) measured in the 2-norm and printed."""
    rigid = gc.start_rigid()[0]
    rec, sums = records_at("morlet3", rows, rigid, av.ESTIMATE, lam)
    A, rhs, elim = dense_system(rec, lam)
    assert len(elim) == sum(1 for q in rows if q != gc.OUTSIDE) and A.shape[0] == 6 + 2 * len(elim)
    x = np.linalg.solve(A, rhs)
    d, ok, dgb = ag.solve_group(rec, lam)
    got = np.concatenate([np.array(d)] + [np.array(dgb[i]) for i in elim])
    cond = np.linalg.cond(A)
    bound = 16.0 * EPS * cond * np.abs(x).max()
    print(f"rows {rows} lam {lam:g}: {A.shape[0]} unknowns, cond {cond:.3e}, max|x| {np.abs(x).max():.3e}, largest difference {np.abs(got - x).max():.3e}, bound {bound:.3e}")
    assert ok and np.abs(got - x).max() <= bound
    assert all((dgb[i] is None) == (i not in elim) for i in range(len(rows)))
    if gc.OUTSIDE in rows:  # the member without valid pixels contributes zeros, is no unknown and keeps its (g, b)
        i = rows.index(gc.OUTSIDE)
        assert sums[i][0] == 0 and not np.array(rec[i][1]).any() and not np.array(rec[i][0]).any() and dgb[i] is None


def test_a_singleton_with_estimated_intensity_takes_lm_step_vws_step():
    """one group of one target, intensity estimated: the Schur proposal against lm_step_vw's 8-unknown L D L^T on the same sums, to the bound of the
    test above on the 8 x 8 system (the two eliminate in different orders, so the bits may differ)"""
    model, q = "morlet3", 3
    rec, sums = records_at(model, [q], gc.start_rigid()[1], av.ESTIMATE)
    A, rhs, _ = dense_system(rec, 1e-3)
    cond, x = np.linalg.cond(A), np.linalg.solve(A, rhs)
    bound = 16.0 * EPS * cond * np.abs(x).max()
    og, ow = gc.options(av.ESTIMATE), wc.options(align.RIGID, av.ESTIMATE)
    gs, ts = ag.lm_init_g(og, [0, 1], gc.start_rigid()[1:2], gc.planes()[q:q + 1], None)
    sw = av.lm_init_vw(ow, None, gc.start_rigid()[1], gc.planes()[q], None)
    ag.lm_step_g(gs, ts, sums, 0, og)
    av.lm_step_vw(sw, sums[0], 0, ow)
    diff = np.abs(np.array(gs[0]["rigid_trial"]) - np.array(sw["rigid_trial"])).max()
    print(f"cond {cond:.3e}, max|x| {np.abs(x).max():.3e}, states differ by {diff:.3e}, bound {bound:.3e}; (g, b)' {ts[0]['gb_trial']} / {sw['gb_trial']}")
    assert diff <= bound and gs[0]["flags"] == sw["flags"] == 0 and gs[0]["mean_best"] == sw["mean_best"]
    assert np.abs(np.array(ts[0]["gb_trial"]) - np.array(sw["gb_trial"])).max() <= bound + 2.0 ** -23 * 2.0  # float32 numbers: the bound or one ulp
    assert np.abs(np.array(ts[0]["trial"]) - np.array(sw["trial"])).max() <= 2.0 ** -23 * 16.0  # the maps: one ulp of the largest entry at most


PROG = textwrap.dedent(r"""
    #include <cassert>
    #include <cstdio>
    #include <vector>
    #include "align_plan.h"
    using namespace msiren;

    static GroupStartError check(std::vector<int32_t> v, int64_t G, int64_t m, int64_t want_index) {
        int64_t at = -7;
        const GroupStartError e = group_start_check(v.empty() ? nullptr : v.data(), G, m, &at);
        assert(e == GROUPS_OK || e == GROUPS_NONE || e == GROUPS_NULL || at == want_index);
        return e;
    }

    int main() {
        assert(check({0, 3, 4, 6}, 3, 6, 0) == GROUPS_OK);
        assert(check({0, 6}, 1, 6, 0) == GROUPS_OK);
        assert(check({0, 1, 2, 3, 4, 5, 6}, 6, 6, 0) == GROUPS_OK);
        assert(check({0, 3, 4, 6}, 0, 6, 0) == GROUPS_NONE && check({0, 3, 4, 6}, -1, 6, 0) == GROUPS_NONE);
        assert(check({}, 3, 6, 0) == GROUPS_NULL);
        assert(check({1, 3, 4, 6}, 3, 6, 0) == GROUPS_FIRST && check({-1, 3, 4, 6}, 3, 6, 0) == GROUPS_FIRST);
        assert(check({0, 3, 3, 6}, 3, 6, 2) == GROUPS_ORDER);   // an empty group
        assert(check({0, 4, 3, 6}, 3, 6, 2) == GROUPS_ORDER);   // descending
        assert(check({0, 0, 4, 6}, 3, 6, 1) == GROUPS_ORDER);
        assert(check({0, 3, 4, 4}, 3, 6, 3) == GROUPS_ORDER);
        assert(check({0, 3, 4, 5}, 3, 6, 3) == GROUPS_LAST && check({0, 3, 4, 7}, 3, 6, 3) == GROUPS_LAST);
        assert(check({0, 7}, 1, 6, 1) == GROUPS_LAST);
        assert(check({0, 0}, 1, 0, 1) == GROUPS_ORDER);         // no targets: no valid groups
        {   // 1025 singleton groups: three upload launches
            std::vector<int32_t> v(1026);
            for (int i = 0; i < 1026; ++i) v[i] = i;
            assert(check(v, 1025, 1025, 0) == GROUPS_OK);
            v[700] = 699;
            assert(check(v, 1025, 1025, 700) == GROUPS_ORDER);
        }
        // the layout: doubles first, every section inside [base, total), nothing overlaps
        const GroupSolveLayout s = group_solve_layout(1024, 6, 3, 80, 60, 9, 4);
        assert(s.sums == 1024 && s.sums_best == s.sums + 8 * 6 * 80 && s.rec == s.sums_best + 8 * 6 * 80 && s.rigid_trial == s.rec + 8 * 6 * 60);
        assert(s.rigid_best == s.rigid_trial + 8 * 3 * 12 && s.scal == s.rigid_best + 8 * 3 * 12 && s.trial == s.scal + 8 * 3 * 9 && s.trial % 8 == 0);
        assert(s.best == s.trial + 4 * 6 * 9 && s.gb_trial == s.best + 4 * 6 * 9 && s.gb_best == s.gb_trial + 4 * 6 * 2 && s.group_of == s.gb_best + 4 * 6 * 2);
        assert(s.group_start == s.group_of + 4 * 6 && s.cnt == s.group_start + 4 * 4 && s.total == s.cnt + 4 * 3 * 4);
        assert(group_solve_layout(0, 6, 3, 80, 60, 9, 4).total == s.total - 1024);
        std::puts("ok");
        return 0;
    }
""")


def test_group_start_validation_and_the_state_layout_in_a_compiled_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    src, exe = tmp_path / "groups.cpp", tmp_path / "groups"
    src.write_text(PROG)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mri_inr_amd", "csrc"), str(src), "-o", str(exe)], check=True, capture_output=True,
                   text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr


@pytest.mark.parametrize("model", list(gc.MODELS))
@pytest.mark.parametrize("est", gc.MODES)
def test_the_loop_reaches_the_truth_on_the_gate_groups(model, est):
    res, (gs, ts), seen = gc.reference_solve(model, est)
    err = gc.errors(res, est)
    print(f"{model} intensity {est}: errors per group {np.array2string(err, precision=2)}, accepted {res.accepted.tolist()}, lam {res.damping.tolist()}, "
          f"flags {res.flags.tolist()}, (g, b) {res.intensity.tolist()}")
    assert (err[list(gc.GATE_GROUPS)] <= gc.REACHED).all(), err
    assert not res.flags.any() and (res.mean_best <= res.mean_first).all() and (res.accepted >= 3).all()
    assert res.trace.shape == (gc.ITERATIONS, gc.G, 15) and np.array_equal(res.trace[0, :, :12], gc.start_rigid())
    assert np.array_equal(gc.maps_of(np.concatenate([res.rotation.reshape(gc.G, 9), res.shift], axis=1)), res.maps)  # the best maps are those of the best states
    assert np.abs(res.rotation[list(gc.GATE_GROUPS)] - gc.truth_rotations()[list(gc.GATE_GROUPS)]).max() <= 1e-6
    inside = [q for q in range(gc.M) if q != gc.OUTSIDE]
    assert (res.count[inside] == gc.SHAPE[0] * gc.SHAPE[1] - 24).all() and (res.wsum[inside] < res.count[inside]).all()  # the corrupted block never counts
    # the trace replays with the sums seen: the check tests/test_gpu_align_group.py makes of the device
    differs, st = gc.replay(res.trace, lambda k, maps, gb: seen[k], est, intensity=gc.start_intensity(est))
    rep, trep = ag.report_g(*st)
    assert differs is None and np.array_equal(rep[:, 0], res.accepted.astype(np.float64)) and np.array_equal(trep[:, 2], res.cost)
    if est == av.FIXED:
        assert np.array_equal(res.intensity, gc.GB_TRUTH)


@pytest.mark.parametrize("model", list(gc.MODELS))
@pytest.mark.parametrize("est", gc.MODES)
def test_the_member_that_never_sees_the_volume_ends_on_its_true_map(model, est):
    res, _, seen = gc.reference_solve(model, est)
    q = gc.OUTSIDE
    assert not seen[:, q, :].any() and res.count[q] == 0 and res.wsum[q] == 0 and res.cost[q] == 0  # count 0 in every evaluation: zeros throughout
    err = np.abs(res.maps[q].astype(np.float64) - gc.truth()[q].astype(np.float64)).max()
    moved = np.abs(gc.start_maps()[q].astype(np.float64) - gc.truth()[q].astype(np.float64)).max()
    print(f"{model} intensity {est}: target {q} ends {err:.2e} from its true map (it started {moved:.2e} away)")
    assert err <= gc.REACHED and moved > 0.1
    assert np.array_equal(res.intensity[q], np.array([1.0, 0.0], np.float32) if est == av.ESTIMATE else gc.GB_TRUTH[q])  # nothing to estimate it from


@pytest.mark.parametrize("model", list(gc.MODELS))
def test_the_variant_loop_sizes_the_gate(model):
    D = gc.D_solve(model)
    print(f"{model}: D_solve = {D:.2e} (the perturbed-fp32 variant's largest final error over the gate groups, both intensity modes), gate {gc.solve_gate(model):.2e}")
    assert D <= gc.D_SOLVE_ASSERTED and gc.solve_gate(model) == gc.device_solve_gate()


@pytest.mark.parametrize("est", gc.MODES)
def test_a_group_wholly_outside_keeps_its_inputs_with_both_flags(est):
    pl = gc.planes()[[4, 5]].copy()
    pl[:, 6] = [-1.0 * gc.SPACING, -1.5 * gc.SPACING]
    rot = avc.rotation_of(np.deg2rad([0.5, -0.25, 0.75]))
    rigid = np.concatenate([rot.ravel(), [0.1, -0.2, 0.3]])[None]
    gb = np.array([[1.5, -0.25], [0.75, 0.5]], np.float32)
    run, tg, w = gc.reference_cost("morlet3"), gc.reference_targets("morlet3")[[4, 5]], gc.weights()[[4, 5]]
    res, (gs, ts) = ag.solve_on_host_g(lambda maps, g: run(maps, g, tg, w), [0, 2], rigid=rigid, planes=pl, intensity=gb, options=gc.options(est, iterations=4), trace=True)
    assert res.flags.tolist() == [align.SINGULAR | align.NO_OVERLAP] and res.accepted.tolist() == [0] and res.mean_first[0] == np.inf and res.mean_best[0] == np.inf
    assert np.array_equal(res.rotation[0], rot) and np.array_equal(res.shift[0], rigid[0, 9:]) and np.array_equal(res.intensity, gb)
    assert np.array_equal(res.maps, np.array([av.rigid_map3(rigid[0].tolist(), p.tolist(), gc.SPACING) for p in pl], np.float32))
    assert not res.count.any() and not res.wsum.any() and np.array_equal(res.trace[:, 0, :12], np.tile(rigid, (4, 1))) and not res.trace[:, 0, 12:].any()
    assert res.damping[0] == ((1e-3 * 10.0) * 10.0) * 10.0  # three rejections


# ---- seeded mutants of the step rule --------------------------------------------------------------------------------------------------------------
def mutant(name):
    """(what to patch in mri_inr_amd.align_group, its replacement)"""
    gsum, apply_, params, jac = ag.group_sum, ag.schur_apply, ag.solved_parameters_g, ag.member_jacobian

    def schur_added(A, rhs, HQ, X, y):
        apply_(A, rhs, [[-v for v in row] for row in HQ], X, y)

    def mean_per_member(sums, o):
        mean, E, C, W = 0.0, gsum([s[2] for s in sums]), gsum([s[0] for s in sums]), gsum([s[1] for s in sums])
        for s in sums:  # every member judged on its own mean: their sum decides
            mean = mean + (s[2] / s[1] if s[1] != 0.0 else float("nan"))
        return (mean if C >= float(params(o, len(sums))) else ag.INF), E, C, W

    return {"last_member_left_out": ("group_sum", lambda terms: gsum(terms[:-1] if len(terms) > 1 else terms)),
            "schur_term_added": ("schur_apply", schur_added),
            "back_substitution_dropped": ("back_substitute", lambda X, y, d: [0.0, 0.0]),
            "accept_per_member": ("group_mean", mean_per_member),
            "P_without_the_intensities": ("solved_parameters_g", lambda o, size: 6),
            "first_members_plane_in_B": ("member_jacobian", lambda rb, planes, i, sp, est: jac(rb, planes, 0, sp, est))}[name]


@pytest.mark.parametrize("name", ["last_member_left_out", "schur_term_added", "back_substitution_dropped", "accept_per_member", "P_without_the_intensities",
                                  "first_members_plane_in_B"])
def test_the_checks_reject_every_seeded_mutant_of_the_step_rule(name, monkeypatch):
    """A `device` that runs a mutated rule in estimate mode on morlet3: the convergence check on the gate groups, the replay of its own trace with
    the true rule, or the report against the replayed states has to fail.  The mutant of P only shows where a group has between 6 and 6 + 2 size
    valid pixels: there the singleton's weights leave it seven."""
    model, est = "morlet3", av.ESTIMATE
    run, tg, w, seen = gc.reference_cost(model), gc.reference_targets(model), gc.weights().copy(), []
    if name == "P_without_the_intensities":
        keep = w[3].copy()
        w[3] = 0.0
        w[3, 9, 8:15] = keep[9, 8:15]
        assert (w[3] > 0).sum() == 7

    def cost_fn(maps, gb):
        seen.append(run(maps, gb, tg, w))
        return seen[-1]

    attr, repl = mutant(name)
    true_fn = getattr(ag, attr)
    with monkeypatch.context() as mp:
        mp.setattr(ag, attr, repl)
        res, _ = ag.solve_on_host_g(cost_fn, gc.GROUP_START, rigid=gc.start_rigid(), planes=gc.planes(), intensity=None, options=gc.options(est), trace=True)
    assert getattr(ag, attr) is true_fn
    converged = bool((gc.errors(res, est)[list(gc.GATE_GROUPS)] <= gc.REACHED).all())
    differs, st = gc.replay(res.trace, lambda k, maps, gb: seen[k], est, intensity=None)
    rep, trep = ag.report_g(*st)
    report = np.stack([res.accepted, res.mean_first, res.mean_best, rep[:, 3], rep[:, 4], res.damping, res.flags], axis=1).astype(np.float64)
    report_differs = differs is None and not (np.array_equal(report, rep) and np.array_equal(trep[:, 0], res.count.astype(np.float64)))
    print(f"{name}: errors {np.array2string(gc.errors(res, est), precision=2)}, the replay differs first at (evaluation, group) {differs}, the report differs {report_differs}")
    assert differs is not None or report_differs or not converged
