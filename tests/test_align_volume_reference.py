"""tests/align_volume_reference.py, tests/align_volume_cases.py and mri_inr_amd.align_volume on the CPU: the point rule
operation by operation, the chain rule of the 56 sums against central differences, the packing, the gate of tests/test_gpu_align_volume.py (it
accepts the reference's own perturbed-fp32 variant, which sits inside half the cap, and rejects every seeded mutant), and the step rule of
msiren_align_volume_solve: ldl_solve for 9, B against central differences of rigid_maps3, the Cayley update, convergence of the loop on the fp64
reference, the variant loop that sizes the device's gate, and seeded mutants of the rule against convergence and replay."""
import numpy as np
import pytest

import align_cases as ac
import align_reference as ar
import align_volume_cases as avc
import align_volume_reference as avr
import grad_reference as gr
import volume_cases as vc
import volume_reference as vr
from conftest import nerr
from mri_inr_amd import align, align_volume as av
from mri_inr_amd import synthetic as syn

CASES = [(m, s) for m in avc.MODELS for s in avc.LATTICES]
SOLVE_CASES = [(m, mode) for m in avc.MODELS for mode in avc.MODES]


def test_map_points3_is_the_rule_operation_by_operation_in_float32():
    f = np.float32
    for shape in ((5, 7),) + avc.LATTICES:
        for row in avc.maps(shape):
            a = [f(x) for x in row]
            want = np.array([[f(f(f(a[3 * r] * f(i)) + f(a[3 * r + 1] * f(j))) + a[3 * r + 2]) for r in range(3)]
                             for i in range(shape[0]) for j in range(shape[1])], f)
            got = av.map_points3(row, shape)
            assert got.dtype == f and got.shape == (shape[0] * shape[1], 3)
            assert np.array_equal(got, want) and np.array_equal(avr.points(row, shape), want)
            # rows 1 and 2 are the 2-D rule on the in-plane six
            assert np.array_equal(got[:, 1:], align.map_points(row[3:], shape))
    assert av.map_points3(avc.maps((5, 7))[0], (0, 5)).shape == (0, 3)
    # every product a i is zero or a normal fp32 number
    for shape in avc.LATTICES:
        for row in avc.maps(shape):
            prods = np.concatenate([np.outer(row[[0, 3, 6]], np.arange(shape[0])).ravel(), np.outer(row[[1, 4, 7]], np.arange(shape[1])).ravel()]).astype(f)
            assert np.all((prods == 0) | (np.abs(prods) >= np.finfo(f).tiny))
    with pytest.raises(ValueError):
        av.map_points3(np.zeros(6), (2, 2))


def test_the_cases_are_what_the_cases_file_says():
    for shape in avc.LATTICES:
        z = [av.map_points3(row, shape)[:, 0] for row in avc.maps(shape)]
        assert z[0].min() == z[0].max() == np.float32(0.37) and z[1].min() == z[1].max() == 2.0 and z[6].min() == z[6].max() == 1.5
        assert z[2].min() < 1 < 2 < z[2].max() <= 3                      # crosses two integers
        assert z[3].min() < 0 < 1 < z[3].max() and (z[3] < 0).sum() > 20  # leaves the stack below 0
        assert 2 < z[4].min() and z[4].max() < 3                         # inside the segment 2 .. 3: slice 3 is black
        assert 0 < z[5].min() and z[5].max() < 3
        yx = av.map_points3(avc.maps(shape)[5], shape)[:, 1:]
        assert (yx.min() < vc.LO) or (yx.max() > vc.HI)                  # leaves every cover
        assert np.isnan(avc.targets(shape)[6]).sum() == 15 and not np.isnan(avc.targets(shape)[:6]).any()
    assert avc.M != avc.N


def test_unpack_and_gauss_newton_step():
    sums = np.arange(2 * 56, dtype=np.float64).reshape(2, 56)
    r = av.unpack_v(sums)
    assert r.count.dtype == np.int64 and r.count.tolist() == [0, 56] and r.cost.tolist() == [1.0, 57.0] and r.grad[0].tolist() == list(range(2, 11))
    assert np.array_equal(r.jtj, r.jtj.transpose(0, 2, 1)) and r.jtj[0, 0].tolist() == list(range(11, 20)) and r.jtj[0, 1, 1:].tolist() == list(range(20, 28))
    assert r.jtj[0, 8, 8] == 55 and r.jtj[0, 7, 8] == 54 and r.warped is None and r.wgrad is None
    with pytest.raises(ValueError):
        av.unpack_v(np.zeros((2, 29)))
    rng = np.random.default_rng(0)
    J, delta = rng.normal(size=(60, 9)), rng.normal(size=9)
    res = av.AlignResultV(np.array([60, 8]), np.zeros(2), np.stack([2 * J.T @ (-J @ delta)] * 2), np.stack([J.T @ J] * 2), None, None)
    step = av.gauss_newton_step_v(res)
    assert np.abs(step[0] - delta).max() <= 1e-12 and not step[1].any()
    assert np.abs(av.gauss_newton_step_v(res, damping=1.0)[0]).sum() < np.abs(delta).sum()


def test_packing_order_on_a_hand_computed_two_pixel_case():
    # lattice 2 x 3; valid pixels (i, j) = (0, 1): R 0, T 2, gZ 2, gY 1, gX -1 -> r = -2, J = (0, 2, 2, 0, 1, 1, 0, -1, -1)
    #                               and (1, 2): R 1.5, T 1, gZ -1, gY 2, gX 3 -> r = .5, J = (-1, -2, -1, 2, 4, 2, 3, 6, 3)
    T = np.full((2, 3), np.nan, np.float32)
    R, gZ, gY, gX = (np.zeros((2, 3)) for _ in range(4))
    T[0, 1], R[0, 1], gZ[0, 1], gY[0, 1], gX[0, 1] = 2, 0, 2, 1, -1
    T[1, 2], R[1, 2], gZ[1, 2], gY[1, 2], gX[1, 2] = 1, 1.5, -1, 2, 3
    sums, mags = avr.sums_of_planes(R, gZ, gY, gX, T, (2, 3))
    J = np.array([[0, 2, 2, 0, 1, 1, 0, -1, -1], [-1, -2, -1, 2, 4, 2, 3, 6, 3]], np.float64)
    r = np.array([-2.0, 0.5])
    assert sums[:2].tolist() == [2, 4.25] and sums[2:11].tolist() == (2 * r @ J).tolist()
    H = J.T @ J
    assert sums[11:].tolist() == [H[a, b] for a in range(9) for b in range(a, 9)]
    assert np.array_equal(av.unpack_v(sums[None]).jtj[0], H) and mags[11] == 1 and mags[2] == 1
    # the in-plane entries are the 2-D reference's
    s2, _ = ar.sums_of_planes(R, gY, gX, T, (2, 3))
    assert sums[:2].tolist() == s2[:2].tolist() and sums[5:11].tolist() == s2[2:8].tolist()
    assert np.array_equal(av.unpack_v(sums[None]).jtj[0, 3:, 3:], align.unpack(s2[None]).jtj[0])
    R[0, 0] = np.inf  # an invalid plane value behind a NaN target, and behind a finite one: left out either way
    T[1, 0], gZ[1, 0] = 1.0, np.nan
    assert np.array_equal(avr.sums_of_planes(R, gZ, gY, gX, T, (2, 3))[0], sums)


@pytest.mark.parametrize("act", ["sine", "morlet"])
def test_single_tile_dcost_matches_central_differences_of_the_cost(act):
    """Two slices that one tile covers entirely (nV = nH = 1) and a lattice inside the segment 0 .. 1: the value is (1 - f) R0 + f R1 with f = Z,
    smooth in the nine parameters."""
    L, shape = 5, (9, 11)
    sd = syn.make_state_dict(seed=7)
    mods = syn.make_mods(3, L, 2, 256)
    i, j = np.repeat(np.arange(shape[0]), shape[1]).astype(np.float64), np.tile(np.arange(shape[1]), shape[0]).astype(np.float64)
    target = (0.3 * np.sin(0.4 * i) + 0.2 * np.cos(0.3 * j)).reshape(shape)

    def sums_at(a):
        Z, Y, X = a[0] * i + a[1] * j + a[2], a[3] * i + a[4] * j + a[5], a[6] * i + a[7] * j + a[8]
        lo, hi = -vc.PAD, -vc.PAD + vc.S - 1
        assert Y.min() > lo and Y.max() < hi and X.min() > lo and X.max() < hi and Z.min() > 0 and Z.max() < 1  # one cover, one segment
        coords = np.stack([-1.0 + (Y + vc.PAD) * 2.0 / (vc.S - 1), -1.0 + (X + vc.PAD) * 2.0 / (vc.S - 1)], axis=1)
        v, g = gr.value_and_grad(sd, mods, coords, num_layers=L, activation=act)
        g = g * (2.0 / (vc.S - 1))  # per reconstruction pixel
        R = (1 - Z) * v[0] + Z * v[1]
        return avr.sums_of_planes(R, v[1] - v[0], (1 - Z) * g[0, 0] + Z * g[0, 1], (1 - Z) * g[1, 0] + Z * g[1, 1], target, shape)[0]

    a0 = np.array([0.03, -0.02, 0.5, 1.1, -0.15, 1.5, 0.2, 0.9, 0.5])
    ref = sums_at(a0)
    assert ref[0] == shape[0] * shape[1]
    h, fd = 1e-6, np.zeros(9)
    for k in range(9):
        step = np.zeros(9)
        step[k] = h
        fd[k] = (sums_at(a0 + step)[1] - sums_at(a0 - step)[1]) / (2 * h)
    e = nerr(ref[2:11], fd)
    print(f"{act}: cost {ref[1]:.3f} dcost {ref[2:11]} nerr against central differences {e:.2e}")
    assert e <= 1e-7, e  # (tests/test_grad_reference.py's tolerance for its own central differences)


@pytest.mark.parametrize("model,shape", CASES)
def test_reference_sums_are_sane_and_jtj_is_positive_semi_definite(model, shape):
    d = avc.data(model, shape)
    res = av.unpack_v(d["sums"])
    pixels = shape[0] * shape[1]
    z3 = av.map_points3(d["maps"][3], shape)[:, 0]
    assert res.count[0] == res.count[1] == res.count[4] == pixels and res.count[6] == pixels - 15
    assert res.count[3] == (z3 >= 0).sum() < pixels and np.isnan(d["planes"][:, 3].reshape(4, -1)[:, z3 < 0]).all()  # Z < 0: NaN in every plane
    assert 0 < res.count[5] < pixels and np.isnan(d["planes"][0, 5]).any()   # part of target 5's lattice is outside every cover
    assert np.array_equal(d["planes"][1, 1], -d["planes"][0, 1])             # flat at Z = 2: the pair is (2, 3), slice 3 is black, gZ = 0 - R
    assert np.array_equal(res.jtj, res.jtj.transpose(0, 2, 1))
    for q in range(avc.M):
        ev = np.linalg.eigvalsh(res.jtj[q])
        assert ev.min() >= -1e-10 * max(ev.max(), 1.0), (q, ev)
    assert (res.cost > 0).all() and np.abs(res.grad).min() > 0
    # the reference is volume_reference.volume at the rule's points
    mods, black = avc.stack_mods(model, "float64")
    q = 2
    val, grad = vr.volume_of_stack(avc.state_dict(model), mods, black, av.map_points3(d["maps"][q], shape), vc.NV, vc.NH, vc.S, vc.I,
                                   num_layers=avc.MODELS[model]["L"], activation=avc.MODELS[model]["act"])
    assert np.array_equal(d["planes"][0, q].ravel(), val, equal_nan=True) and np.array_equal(d["planes"][1:, q].reshape(3, -1), grad, equal_nan=True)


@pytest.mark.parametrize("model,shape", CASES)
def test_gate_accepts_the_fp32_variant_inside_half_the_cap_and_rejects_the_mutants(model, shape):
    d = avc.data(model, shape)
    print(f"{model} {shape}: distance of the perturbed-fp32 variant {d['D']:.2e}, gate {d['gate']:.2e} (cap {avc.CAP:.0e})")
    assert 0 < d["D"] <= avc.CAP / 2 and d["gate"] == avc.FACTOR * d["D"]
    assert avc.accepts(d, d["variant"]) and avc.accepts(d, d["sums"])
    for seed in avr.SEEDS + avr.VOLUME_SEEDS:
        mutant = avc.mutant_sums(model, shape, seed)
        worst = avc.scaled_errors(mutant, d["sums"], d["mags"])[:, 1:].max()
        print(f"    {seed}: largest scaled error {worst:.2e}, counts {mutant[:, 0].astype(int).tolist()}")
        assert not avc.accepts(d, mutant), seed


# ---- the step rule -----------------------------------------------------------------------------------------------------------------------------------
def test_ldl_solve_for_nine_against_numpy_on_random_spd_systems():
    rng = np.random.default_rng(9)
    for _ in range(50):
        J = rng.normal(size=(36, 9))
        A, b = J.T @ J, rng.normal(size=9)
        x, ok = av.ldl_solve(A.tolist(), b.tolist(), 9)
        want = np.linalg.solve(A, b)
        assert ok and np.abs(np.array(x) - want).max() <= 1e-10 * np.abs(want).max()
    # the flag of the step: a target that reads black slices only (H = 0) proposes nothing
    for mode in avc.MODES:
        o = avc.solve_options(mode)
        st = av.lm_init_v(o, avc.start_maps()[0], avc.start_rigid()[0], avc.planes()[0])
        before = list(st["trial"])
        av.lm_step_v(st, [437.0, 3.0] + [0.0] * 54, 0, o)
        assert st["flags"] == align.SINGULAR and st["trial"] == before and st["best"] == before and st["mean_first"] == 3.0 / 437.0
        # fewer valid pixels than solved parameters: NO_OVERLAP
        st = av.lm_init_v(o, avc.start_maps()[0], avc.start_rigid()[0], avc.planes()[0])
        av.lm_step_v(st, [float(av.solved_parameters_v(o) - 1), 3.0] + [0.0] * 54, 0, o)
        assert st["flags"] == align.SINGULAR | align.NO_OVERLAP and st["mean_first"] == align.INF
    assert av.solved_parameters_v(avc.solve_options(align.AFFINE)) == 9 and av.solved_parameters_v(avc.solve_options(align.RIGID)) == 6


def small_rotation(w):
    return avc.rotation_of(w)


def test_rigid_jacobian3_against_central_differences_of_rigid_maps3():
    pl = avc.planes()[1:2] + np.array([[0.02, 0.0, 0.01, 0.0, 0.03, 0.0, 0, 0, 0, 0, 0, 0]])  # (a lattice that is not axis-aligned)
    for vec, sh in (((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.02, -0.03, 0.05), (0.3, -0.2, 0.7)), ((-0.4, 0.3, 0.2), (1.0, 8.0, -3.0))):
        Rot, sh = avc.rotation_of(vec), np.array(sh)
        state = Rot.ravel().tolist() + sh.tolist()
        B = np.array(av.rigid_jacobian3(state, pl[0].tolist(), avc.SPACING))
        h, fd = 1e-6, np.zeros((9, 6))
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            plus = av.rigid_maps3((small_rotation(e) @ Rot)[None], sh[None], pl, avc.SPACING, np.float64)[0]
            minus = av.rigid_maps3((small_rotation(-e) @ Rot)[None], sh[None], pl, avc.SPACING, np.float64)[0]
            fd[:, k] = (plus - minus) / (2 * h)
            fd[:, 3 + k] = (av.rigid_maps3(Rot[None], (sh + e)[None], pl, avc.SPACING, np.float64)[0]
                            - av.rigid_maps3(Rot[None], (sh - e)[None], pl, avc.SPACING, np.float64)[0]) / (2 * h)
        assert np.abs(B - fd).max() <= 1e-8 * max(1.0, np.abs(B).max()), (vec, B, fd)
        # rigid_map3 is rigid_maps3's formula, rounded once
        assert np.array_equal(np.array(av.rigid_map3(state, pl[0].tolist(), avc.SPACING), np.float32), av.rigid_maps3(Rot[None], sh[None], pl, avc.SPACING)[0])
    # the nominal plane: the identity on (Y, X), Z = z in slice units
    assert np.array_equal(avc.start_maps()[0], np.array([0, 0, 0.6, 1, 0, 10, 0, 1, 8], np.float32))


def test_cayley3_update_stays_a_rotation():
    rng = np.random.default_rng(0)
    Rot = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for a in rng.uniform(-0.05, 0.05, (256, 3)):
        C = av.cayley3([float(x) for x in a])
        Rot = [((C[r][0] * Rot[c]) + (C[r][1] * Rot[3 + c])) + (C[r][2] * Rot[6 + c]) for r in range(3) for c in range(3)]
    R = np.array(Rot).reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 64 * 2.0 ** -52 and abs(np.linalg.det(R) - 1.0) <= 64 * 2.0 ** -52  # (a few ulp after 256 updates)
    assert av.cayley3([0.0, 0.0, 0.0]) == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    # one update is the rotation by 2 atan|a| about a
    a = np.array([0.01, -0.02, 0.03])
    want = avc.rotation_of(2.0 * np.arctan(np.linalg.norm(a)) * a / np.linalg.norm(a))
    assert np.abs(np.array(av.cayley3(a.tolist())) - want).max() <= 1e-15


def test_the_solve_inputs_hold_their_two_conditions():
    crossing = [q for q in range(avc.SOLVE_M) if avc.crosses_an_integer_z(q)]
    for model in avc.MODELS:
        assert len(avc.GATE_TARGETS[model]) >= 3
    assert any(q in avc.GATE_TARGETS[model] for model in avc.MODELS for q in crossing), crossing
    z = [av.map_points3(row, avc.SOLVE_SHAPE)[:, 0] for row in avc.truth()]
    assert all(0 < x.min() and x.max() < avc.N - 1 for x in z)


@pytest.mark.parametrize("model,mode", SOLVE_CASES)
def test_the_loop_converges_on_the_fp64_reference(model, mode):
    res, rigid, seen = avc.reference_solve(model, mode)
    err, gate_targets = avc.solve_errors(res.maps), list(avc.GATE_TARGETS[model])
    print(f"{model} mode {mode}: errors {np.array2string(err, precision=2)}, accepted {res.accepted.tolist()}, lam {res.damping.tolist()}, flags {res.flags.tolist()}")
    assert (err[gate_targets] <= avc.REACHED).all(), err
    assert not res.flags[gate_targets].any() and (res.mean_best <= res.mean_first).all()
    assert res.trace.shape == (avc.SOLVE_ITERATIONS, avc.SOLVE_M, 11) and np.array_equal(res.trace[0, :, :9], avc.start_maps().astype(np.float64))
    assert np.array_equal(res.trace[:, :, 9], seen[:, :, 1]) and np.array_equal(res.trace[:, :, 10], seen[:, :, 0])
    if mode == align.RIGID:
        back = av.rigid_maps3(res.rotation, res.shift, avc.planes(), avc.SPACING)
        assert np.array_equal(back, res.maps)  # the best map is the map of the best state
        assert np.abs(res.rotation @ res.rotation.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14
        assert np.abs(res.rotation[gate_targets] - avc.truth_rotations()[gate_targets]).max() <= 1e-6
        assert np.array_equal(rigid[:, :9].reshape(-1, 3, 3), res.rotation)
    else:
        assert res.rotation is None and res.shift is None
    # the trace replays: the check tests/test_gpu_align_volume_solve.py makes of the device
    assert avc.replay(res.trace, lambda k: seen[k], mode, avc.start_maps(), avc.start_rigid(), avc.planes())[0] is None


@pytest.mark.parametrize("model", list(avc.MODELS))
def test_the_variant_loop_sizes_the_gate(model):
    D = avc.D_solve(model)
    print(f"{model}: D_solve = {D:.2e} (the perturbed-fp32 variant's largest final error over the gate targets, both modes), gate {avc.solve_gate(model):.2e}")
    assert D <= avc.D_SOLVE_ASSERTED and avc.solve_gate(model) == avc.device_solve_gate()


def mutant(name):
    """(what to patch in mri_inr_amd.align_volume, its replacement, the mode that shows it)"""
    ldl, jac, decide, cay = av.ldl_solve, av.rigid_jacobian3, av.lm_decide, av.cayley3

    def decide_moves_best(k, mean, mean_best, lam, o):
        accept, counted, lam = decide(k, mean, mean_best, lam, o)
        return True, counted, lam

    def jac_without_spacing(state, plane, spacing):
        return jac(state, plane, 1.0)

    def jac_transposed_cross(state, plane, spacing):  # v x e_k instead of e_k x v
        B = jac(state, plane, spacing)
        return [[-B[a][k] if k < 3 else B[a][k] for k in range(6)] for a in range(9)]

    def cay_without_factor_2(a):  # the cross-product part taken once: no rotation, and half the angle
        C = cay(a)
        return [[0.5 * (C[r][c] + C[c][r]) + 0.25 * (C[r][c] - C[c][r]) for c in range(3)] for r in range(3)]

    return {"step_sign_flipped": ("ldl_solve", lambda A, b, m: ([-x for x in ldl(A, b, m)[0]], ldl(A, b, m)[1]), align.AFFINE),
            "half_dropped": ("ldl_solve", lambda A, b, m: ldl(A, [2.0 * x for x in b], m), align.RIGID),
            "reject_moves_best": ("lm_decide", decide_moves_best, align.AFFINE),
            "z_rows_of_B_not_over_the_spacing": ("rigid_jacobian3", jac_without_spacing, align.RIGID),
            "cross_product_transposed": ("rigid_jacobian3", jac_transposed_cross, align.RIGID),
            "cayley_cross_part_halved": ("cayley3", cay_without_factor_2, align.RIGID)}[name]


@pytest.mark.parametrize("name", ["step_sign_flipped", "half_dropped", "reject_moves_best", "z_rows_of_B_not_over_the_spacing", "cross_product_transposed",
                                  "cayley_cross_part_halved"])
def test_the_checks_reject_every_seeded_mutant_of_the_step_rule(name, monkeypatch):
    """A `device` that runs a mutated rule, on targets 0 and 1 of morlet3: the convergence check or the replay of its trace with the true rule has
    to fail."""
    model, rows = "morlet3", [0, 1]
    attr, repl, mode = mutant(name)
    run, tg, seen = avc.reference_cost(model), avc.reference_targets(model)[rows], []

    def cost_fn(maps):
        seen.append(run(maps, tg)[0])
        return seen[-1]

    true_step = av.lm_step_v
    start, rigid, pl = avc.start_maps()[rows], avc.start_rigid()[rows], avc.planes()[rows]
    with monkeypatch.context() as mp:
        mp.setattr(av, attr, repl)
        res, _ = av.solve_on_host_v(cost_fn, len(rows), maps=start, rigid=rigid, planes=pl, options=avc.solve_options(mode, iterations=10), trace=True)
    assert av.lm_step_v is true_step and getattr(av, attr) is not repl
    converged = bool((avc.solve_errors(res.maps, rows) <= avc.REACHED).all())
    differs, _ = avc.replay(res.trace, lambda k: seen[k], mode, start, rigid, pl)
    print(f"{name}: errors {np.array2string(avc.solve_errors(res.maps, rows), precision=2)}, the replay differs first at (evaluation, target) {differs}")
    assert not converged or differs is not None
