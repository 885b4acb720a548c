"""msiren_align_solve's step rule on the CPU (mri_inr_amd/align.py: ldl_solve, rigid_jacobian, cayley, lm_step,
solve_on_host) and the cases of tests/align_solve_cases.py on tests/align_reference.py: the loop converges on the gate slices in fp64,
its perturbed-fp32 variant sizes the gate of tests/test_gpu_align_solve.py, and the two checks that file makes of the device -- the
host-loop identity on the trace and the convergence gate -- reject every seeded mutant of the rule."""
import numpy as np
import pytest

import align_solve_cases as sc
from mri_inr_amd import align

CASES = [(m, mode) for m in sc.MODELS for mode in sc.MODES]


@pytest.mark.parametrize("m", [6, 3])
def test_ldl_solve_against_numpy_on_random_spd_systems(m):
    rng = np.random.default_rng(m)
    for _ in range(50):
        J = rng.normal(size=(4 * m, m))
        A, b = J.T @ J, rng.normal(size=m)
        x, ok = align.ldl_solve(A.tolist(), b.tolist(), m)
        want = np.linalg.solve(A, b)
        assert ok and np.abs(np.array(x) - want).max() <= 1e-10 * np.abs(want).max()


def test_ldl_solve_refuses_a_pivot_that_is_not_positive_and_finite():
    for A in ([[0.0] * 3] * 3, [[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0], [0.0, float("nan"), 0.0], [0.0, 0.0, 1.0]],
              [[float("inf"), 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1e-300]]):
        x, ok = align.ldl_solve(A, [1.0, 2.0, 3.0], 3)
        assert not ok and x == [0.0, 0.0, 0.0], A
    # the flag of the step: a black slice (H = 0) proposes nothing
    for mode in sc.MODES:
        o = sc.options(mode)
        st = align.lm_init(o, sc.start_maps()[0], sc.start_rigid()[0])
        before = list(st["trial"])
        align.lm_step(st, [437.0, 3.0] + [0.0] * 27, 0, o)
        assert st["flags"] == align.SINGULAR and st["trial"] == before and st["best"] == before and st["mean_first"] == 3.0 / 437.0


def test_rigid_jacobian_against_central_differences_of_rigid_maps():
    cy, cx = 9.0, 11.25
    for ang, sh in ((0.0, (0.0, 0.0)), (0.3, (1.5, -2.0)), (-1.2, (10.0, 8.0))):
        B = np.array(align.rigid_jacobian(np.cos(ang), np.sin(ang), cy, cx))
        h = 1e-6
        fd = np.zeros((6, 3))
        fd[:, 0] = (align.rigid_maps(ang + h, sh, (cy, cx), np.float64)[0] - align.rigid_maps(ang - h, sh, (cy, cx), np.float64)[0]) / (2 * h)
        for q in (0, 1):
            e = np.zeros(2)
            e[q] = h
            fd[:, 1 + q] = (align.rigid_maps(ang, sh + e, (cy, cx), np.float64)[0] - align.rigid_maps(ang, sh - e, (cy, cx), np.float64)[0]) / (2 * h)
        assert np.abs(B - fd).max() <= 1e-8 * max(1.0, np.abs(B).max()), (ang, B, fd)
    # rigid_map is rigid_maps' formula
    for ang, sh in ((0.0, (10.0, 8.0)), (0.1234567, (1 / 3, 1 / 7))):
        got = align.rigid_map(float(np.cos(ang)), float(np.sin(ang)), sh[0], sh[1], cy, cx)
        assert np.array_equal(np.array(got, np.float32), align.rigid_maps(ang, sh, (cy, cx))[0])


def test_cayley_update_stays_a_rotation():
    rng = np.random.default_rng(0)
    c, s, total = 1.0, 0.0, 0.0
    for u in rng.uniform(-0.05, 0.05, 256):
        cd, sd = align.cayley(float(u))
        c, s = c * cd - s * sd, s * cd + c * sd
        total += 2.0 * np.arctan(u)
        assert abs(c * c + s * s - 1.0) <= 1e-14
    assert abs(np.arctan2(s, c) - total) <= 1e-13
    assert align.cayley(0.0) == (1.0, 0.0)


@pytest.mark.parametrize("model,mode", CASES)
def test_the_loop_converges_on_the_fp64_reference(model, mode):
    res, rigid, seen = sc.reference_solve(model, mode)
    err = sc.errors(res.maps)
    print(f"{model} mode {mode}: errors {np.array2string(err, precision=2)}, accepted {res.accepted.tolist()}, lam {res.damping.tolist()}, flags {res.flags.tolist()}")
    assert (err[list(sc.GATE_SLICES[model])] <= sc.REACHED).all(), err
    # the black slice: SINGULAR, its map the input's; nothing was ever accepted
    assert res.flags[sc.BLACK] == align.SINGULAR and np.array_equal(res.maps[sc.BLACK], sc.start_maps()[sc.BLACK]) and res.accepted[sc.BLACK] == 0
    assert not res.flags[list(sc.GATE_SLICES[model])].any() and (res.mean_best <= res.mean_first).all()
    assert res.trace.shape == (sc.ITERATIONS, sc.N, 8) and np.array_equal(res.trace[0, :, :6], sc.start_maps().astype(np.float64))
    assert np.array_equal(res.trace[:, :, 6], seen[:, :, 1]) and np.array_equal(res.trace[:, :, 7], seen[:, :, 0])
    if mode == align.RIGID:
        assert np.abs(align.rigid_maps(res.angle, res.shift, sc.CENTRE).astype(np.float64) - res.maps).max() <= 4e-6  # (two float32 ulp of the largest entry)
        assert np.abs(rigid[:, 0] ** 2 + rigid[:, 1] ** 2 - 1.0).max() <= 1e-14
        assert np.abs(res.angle[list(sc.GATE_SLICES[model])] - sc.ANGLES[list(sc.GATE_SLICES[model])]).max() <= 1e-7
    else:
        assert res.angle is None and res.shift is None
    # the trace replays: the check tests/test_gpu_align_solve.py makes of the device
    assert sc.replay(res.trace, lambda k: seen[k], mode, sc.start_maps(), sc.start_rigid())[0] is None


@pytest.mark.parametrize("model", list(sc.MODELS))
def test_the_variant_loop_sizes_the_gate(model):
    D = sc.D(model)
    print(f"{model}: D = {D:.2e} (the perturbed-fp32 variant's largest final error over the gate slices, both modes), gate {sc.gate(model):.2e}")
    assert D <= 1e-6 and D <= sc.D_ASSERTED and sc.gate(model) == sc.device_gate()


def mutant(name):
    """(what to patch in mri_inr_amd.align, its replacement, the mode that shows it)"""
    ldl, jac, decide = align.ldl_solve, align.rigid_jacobian, align.lm_decide

    def decide_moves_best(k, mean, mean_best, lam, o):
        accept, counted, lam = decide(k, mean, mean_best, lam, o)
        return True, counted, lam

    def decide_keeps_lam(k, mean, mean_best, lam, o):
        accept, counted, new = decide(k, mean, mean_best, lam, o)
        return accept, counted, (lam if accept else new)

    return {"step_sign_flipped": ("ldl_solve", lambda A, b, m: ([-x for x in ldl(A, b, m)[0]], ldl(A, b, m)[1]), align.AFFINE),
            "half_dropped": ("ldl_solve", lambda A, b, m: ldl(A, [2.0 * x for x in b], m), align.AFFINE),
            "reject_moves_best": ("lm_decide", decide_moves_best, align.AFFINE),
            "lam_never_lowered": ("lm_decide", decide_keeps_lam, align.AFFINE),
            "centre_swapped_in_B": ("rigid_jacobian", lambda c, s, cy, cx: jac(c, s, cx, cy), align.RIGID),
            "sd_without_factor_2": ("cayley", lambda u: ((1.0 - u * u) / (1.0 + u * u), u / (1.0 + u * u)), align.RIGID)}[name]


@pytest.mark.parametrize("name", ["step_sign_flipped", "half_dropped", "reject_moves_best", "lam_never_lowered", "centre_swapped_in_B", "sd_without_factor_2"])
def test_the_checks_reject_every_seeded_mutant(name, monkeypatch):
    """A `device` that runs a mutated rule, on slices 0 and 1 of sine5 (slice 1 rejects steps in the true loop): the convergence check or
    the replay of its trace with the true rule has to fail."""
    model, slices = "sine5", [0, 1]
    attr, repl, mode = mutant(name)
    run, tg, seen = sc.reference_cost(model), sc.reference_targets(model)[slices], []

    def cost_fn(maps):
        seen.append(run(maps, tg, slices)[0])
        return seen[-1]

    true_step = align.lm_step
    start, rigid = sc.start_maps()[slices], sc.start_rigid()[slices]
    with monkeypatch.context() as mp:
        mp.setattr(align, attr, repl)
        res, _ = align.solve_on_host(cost_fn, len(slices), maps=start, rigid=rigid, options=sc.options(mode), trace=True)
    assert align.lm_step is true_step and getattr(align, attr) is not repl
    converged = bool((sc.errors(res.maps, slices) <= sc.REACHED).all())
    differs, _ = sc.replay(res.trace, lambda k: seen[k], mode, start, rigid)
    print(f"{name}: errors {np.array2string(sc.errors(res.maps, slices), precision=2)}, the replay differs first at (evaluation, slice) {differs}")
    assert not converged or differs is not None
