"""tests/align_w_reference.py, tests/align_w_cases.py and the weighted helpers of mri_inr_amd.align on the CPU: the
47 sums restricted to section 5.10's are section 5.10's, dcost over all 8 parameters against central differences, the gate of
tests/test_gpu_align_w.py (the reference's own perturbed-fp32 variant sits inside half the cap; every seeded mutant is rejected), the step
rule lm_step_w against lm_step, and the convergence of the reference loop with its seeded mutants."""
import numpy as np
import pytest

import align_cases as ac
import align_reference as ar
import align_solve_cases as sc
import align_w_cases as wc
import align_w_reference as awr
import grad_reference as gr
import volume_cases as vc
from conftest import nerr
from mri_inr_amd import align
from mri_inr_amd import synthetic as syn

CASES = [(m, s) for m in ac.MODELS for s in ac.LATTICES]


@pytest.mark.parametrize("model,shape", CASES)
def test_unit_weights_and_identity_intensity_give_section_5_10s_sums(model, shape):
    d = ac.data(model, shape)
    sums, mags = awr.align(d["planes"], d["targets"], None, None)
    assert np.array_equal(sums[:, awr.SHARED], d["sums"]) and np.array_equal(mags[:, awr.SHARED], d["mags"])
    assert np.array_equal(sums[:, 1], sums[:, 0])  # wsum == count
    res = align.unpack_w(sums)
    assert np.array_equal(res.jtj, res.jtj.transpose(0, 2, 1)) and np.array_equal(res.jtj[:, :6, :6], align.unpack(d["sums"]).jtj)
    assert np.array_equal(res.jtj[:, 7, 7], sums[:, 0]) and np.array_equal(res.grad[:, :6], d["sums"][:, 2:8])  # J[7] = 1
    with pytest.raises(ValueError):
        align.unpack_w(np.zeros((2, 29)))


def test_packing_order_and_validity_on_a_hand_computed_case():
    # lattice 1 x 3, g = 2, b = 1; pixel j = 1: R 1, T 2, gY 1, gX -1, w 0.5 -> r = 1, J = (0, 2, 2, 0, -2, -2, 1, 1); the others masked
    R, gY, gX, T = np.array([5.0, 1.0, 7.0]), np.array([3.0, 1.0, 3.0]), np.array([3.0, -1.0, 3.0]), np.array([1.0, 2.0, 1.0])
    for w0, w2 in ((0.0, -1.0), (np.nan, np.inf), (-np.inf, 0.0)):
        sums, mags = awr.sums_of_planes(R, gY, gX, T, np.array([w0, 0.5, w2]), (2.0, 1.0), (1, 3))
        J = [0.0, 2.0, 2.0, 0.0, -2.0, -2.0, 1.0, 1.0]
        assert sums[:3].tolist() == [1.0, 0.5, 0.5] and sums[3:11].tolist() == [1.0 * x for x in J]
        assert sums[11:].tolist() == [0.5 * J[a] * J[b] for a, b in awr.PACK] and np.array_equal(mags, np.abs(sums))
    res = align.unpack_w(sums[None])
    assert res.jtj[0, 1].tolist() == [0.5 * 2.0 * x for x in J] and res.jtj[0, 6, 4] == -1.0 and res.wsum[0] == 0.5 and res.count[0] == 1


@pytest.mark.parametrize("act", ["sine", "morlet"])
def test_single_tile_dcost_matches_central_differences_of_the_cost(act):
    """tests/test_align_reference.py's single-tile slice, step and tolerance, with weights and over all 8 parameters"""
    L, shape = 5, (9, 11)
    sd = syn.make_state_dict(seed=7)
    mods = syn.make_mods(3, L, 1, 256)
    i, j = np.repeat(np.arange(shape[0]), shape[1]).astype(np.float64), np.tile(np.arange(shape[1]), shape[0]).astype(np.float64)
    target = (0.3 * np.sin(0.4 * i) + 0.2 * np.cos(0.3 * j)).reshape(shape)
    weight = 0.2 + 0.8 * np.cos(0.2 * i) ** 2 * np.sin(0.1 + 0.25 * j) ** 2
    weight[7:12] = 0.0

    def sums_at(a):
        Y, X = a[0] * i + a[1] * j + a[2], a[3] * i + a[4] * j + a[5]
        lo, hi = -vc.PAD, -vc.PAD + vc.S - 1
        assert Y.min() > lo and Y.max() < hi and X.min() > lo and X.max() < hi  # every pixel covered, at both ends of a difference too
        coords = np.stack([-1.0 + (Y + vc.PAD) * 2.0 / (vc.S - 1), -1.0 + (X + vc.PAD) * 2.0 / (vc.S - 1)], axis=1)
        v, g = gr.value_and_grad(sd, mods, coords, num_layers=L, activation=act)
        g = g * (2.0 / (vc.S - 1))  # per reconstruction pixel
        return awr.sums_of_planes(v[0], g[0, 0], g[1, 0], target, weight, a[6:8], shape)[0]

    a0 = np.array([1.1, -0.15, 1.5, 0.2, 0.9, 0.5, 1.3, -0.07])
    ref = sums_at(a0)
    assert ref[0] == shape[0] * shape[1] - 5 and abs(ref[1] - weight.sum()) <= 1e-12
    h, fd = 1e-6, np.zeros(8)
    for k in range(8):
        step = np.zeros(8)
        step[k] = h
        fd[k] = (sums_at(a0 + step)[2] - sums_at(a0 - step)[2]) / (2 * h)
    e = nerr(ref[3:11], fd)
    print(f"{act}: cost {ref[2]:.3f} dcost {ref[3:11]} nerr against central differences {e:.2e}")
    assert e <= 1e-7, e


@pytest.mark.parametrize("model,shape", CASES)
def test_gate_accepts_the_fp32_variant_inside_half_the_cap_and_rejects_the_mutants(model, shape):
    d = wc.data(model, shape)
    print(f"{model} {shape}: distance of the perturbed-fp32 variant {d['D']:.2e}, gate {d['gate']:.2e} (cap {wc.CAP:.0e})")
    assert 0 < d["D"] <= wc.CAP / 2 and d["gate"] == wc.FACTOR * d["D"]
    assert wc.accepts(d, d["variant"]) and wc.accepts(d, d["sums"])
    assert (d["weights"] == 0).any() and d["sums"][1, 0] < ac.data(model, shape)["sums"][1, 0]  # the zero block masks pixels
    for seed in awr.SEEDS:
        mutant = awr.align(d["planes"], d["targets"], d["weights"], d["intensity"], seed)[0]
        worst = ac.scaled_errors(mutant, d["sums"], d["mags"])[:, 1:].max()
        print(f"    {seed}: largest scaled error {worst:.2e}, counts {mutant[:, 0].astype(int).tolist()}")
        assert not wc.accepts(d, mutant), seed


@pytest.mark.parametrize("m", [5, 8])
def test_ldl_solve_against_numpy_on_random_spd_systems(m):
    rng = np.random.default_rng(m)
    for _ in range(50):
        J = rng.normal(size=(4 * m, m))
        A, b = J.T @ J, rng.normal(size=m)
        x, ok = align.ldl_solve(A.tolist(), b.tolist(), m)
        want = np.linalg.solve(A, b)
        assert ok and np.abs(np.array(x) - want).max() <= 1e-10 * np.abs(want).max()


def test_rigid_jacobian_w_against_central_differences():
    cy, cx = 9.0, 11.25

    def params(ang, sh, gb):
        return np.concatenate([align.rigid_maps(ang, sh, (cy, cx), np.float64)[0], gb])

    for ang, sh, gb in ((0.0, (0.0, 0.0), (1.0, 0.0)), (0.3, (1.5, -2.0), (1.25, 0.1)), (-1.2, (10.0, 8.0), (0.8, -0.05))):
        B = np.array(align.rigid_jacobian_w(np.cos(ang), np.sin(ang), cy, cx))
        assert B.shape == (8, 5)
        h, x0 = 1e-6, np.array([ang, sh[0], sh[1], gb[0], gb[1]])
        fd = np.zeros((8, 5))
        for q in range(5):
            e = np.zeros(5)
            e[q] = h
            hi, lo = x0 + e, x0 - e
            fd[:, q] = (params(hi[0], hi[1:3], hi[3:]) - params(lo[0], lo[1:3], lo[3:])) / (2 * h)
        assert np.abs(B - fd).max() <= 1e-8 * max(1.0, np.abs(B).max()), (ang, B, fd)
        assert np.array_equal(B[:6, :3], np.array(align.rigid_jacobian(np.cos(ang), np.sin(ang), cy, cx))) and not B[:6, 3:].any() and not B[6:, :3].any()


def test_gauss_newton_step_w_solves_a_linear_model():
    rng = np.random.default_rng(0)
    J, delta = rng.normal(size=(40, 8)), rng.normal(size=8)
    grad, jtj = np.stack([2 * J.T @ (-J @ delta)] * 2), np.stack([J.T @ J] * 2)
    res = align.AlignResultW(np.array([40, 7]), np.array([40.0, 7.0]), np.zeros(2), grad, jtj, None, None)
    step = align.gauss_newton_step_w(res)
    assert np.abs(step[0] - delta).max() <= 1e-12 and not step[1].any()
    six = align.gauss_newton_step_w(res, estimate_intensity=False)
    assert not six[:, 6:].any() and six[1].any() and np.abs(six[0, :6] - np.linalg.solve(jtj[0][:6, :6], -0.5 * grad[0][:6])).max() <= 1e-12


@pytest.mark.parametrize("mode", sc.MODES)
def test_fixed_mode_with_unit_weights_is_lm_step_bit_for_bit_over_a_reference_loop(mode):
    """solve_on_host_w (intensity fixed at (1, 0), no weights) on the 47 sums of the fp64 reference against section 5.11's loop on its 29"""
    model = "sine5"
    old, old_rigid, seen29 = sc.reference_solve(model, mode)
    run, tg, seen = wc.reference_cost(model), sc.reference_targets(model), []

    def cost_fn(maps, gb):
        assert np.array_equal(gb, np.tile(np.array([1.0, 0.0], np.float32), (wc.N, 1)))
        seen.append(run(maps, None, tg, None))
        return seen[-1]

    new, new_rigid = align.solve_on_host_w(cost_fn, wc.N, maps=sc.start_maps(), rigid=sc.start_rigid(), options=wc.options(mode, align.FIXED, iterations=sc.ITERATIONS),
                                           trace=True)
    seen = np.stack(seen)
    assert np.array_equal(seen[:, :, awr.SHARED], seen29) and np.array_equal(seen[:, :, 1], seen[:, :, 0])
    for field in ("maps", "angle", "shift", "accepted", "mean_first", "mean_best", "count", "damping", "flags"):
        a, b = getattr(new, field), getattr(old, field)
        assert (a is None and b is None) or np.array_equal(a, b), field
    assert np.array_equal(new_rigid, old_rigid) and np.array_equal(new.wsum, old.count.astype(np.float64))
    assert np.array_equal(new.trace[:, :, :6], old.trace[:, :, :6]) and np.array_equal(new.trace[:, :, 8:10], old.trace[:, :, 6:8])
    assert np.array_equal(new.intensity, np.tile(np.array([1.0, 0.0], np.float32), (wc.N, 1)))
    # step by step: lm_step_w's state against lm_step's on the same evaluations
    o6, o8 = sc.options(mode), wc.options(mode, align.FIXED, iterations=sc.ITERATIONS)
    for s in range(wc.N):
        a, b = align.lm_init(o6, sc.start_maps()[s], sc.start_rigid()[s]), align.lm_init_w(o8, sc.start_maps()[s], sc.start_rigid()[s])
        for k in range(sc.ITERATIONS):
            align.lm_step(a, seen29[k, s], k, o6)
            align.lm_step_w(b, seen[k, s], k, o8)
            assert all(np.array_equal(a[f], b[f], equal_nan=True) for f in ("trial", "best", "rigid_trial", "rigid_best", "lam", "flags", "accepted", "mean_best", "mean_first")), (s, k)


@pytest.mark.parametrize("model,mode", [(m, mode) for m in wc.MODELS for mode in sc.MODES])
def test_the_estimate_loop_converges_on_the_fp64_reference(model, mode):
    res, rigid, seen = wc.reference_solve(model, mode, align.ESTIMATE)
    err, gates = wc.errors(res.maps, res.intensity), list(wc.GATE_SLICES[model])
    print(f"{model} mode {mode}: errors {np.array2string(err, precision=2)}, accepted {res.accepted.tolist()}, lam {res.damping.tolist()}, flags {res.flags.tolist()}, "
          f"(g, b) {res.intensity.tolist()}")
    assert len(gates) >= 2 and wc.BLACK not in gates
    assert (err[gates] <= wc.REACHED).all(), err
    assert res.flags[wc.BLACK] == align.SINGULAR and np.array_equal(res.maps[wc.BLACK], sc.start_maps()[wc.BLACK]) and res.accepted[wc.BLACK] == 0
    assert res.intensity[wc.BLACK].tolist() == [1.0, 0.0]
    assert not res.flags[gates].any() and (res.mean_best <= res.mean_first).all()
    assert res.trace.shape == (wc.ITERATIONS, wc.N, 11) and np.array_equal(res.trace[0, :, :6], sc.start_maps().astype(np.float64))
    assert np.array_equal(res.trace[:, :, 8], seen[:, :, 2]) and np.array_equal(res.trace[:, :, 9], seen[:, :, 0]) and np.array_equal(res.trace[:, :, 10], seen[:, :, 1])
    assert (res.wsum < res.count).all() and (res.count[gates] <= wc.SHAPE[0] * wc.SHAPE[1] - 24).all()  # the block is masked
    assert wc.replay(res.trace, lambda k: seen[k], mode, align.ESTIMATE, sc.start_maps(), sc.start_rigid())[0] is None
    # the masked, corrupted block does not move the result
    run, clean, w = wc.reference_cost(model), wc.reference_targets(model, False), wc.solve_weights()
    assert np.array_equal(run(res.maps, res.intensity, clean, w), run(res.maps, res.intensity, wc.reference_targets(model), w))


@pytest.mark.parametrize("model", list(wc.MODELS))
def test_the_variant_loop_sizes_the_gate(model):
    D = wc.D(model)
    print(f"{model}: D_solve = {D:.2e} (the perturbed-fp32 variant's largest final error over the gate slices, both geometry modes), gate {wc.gate(model):.2e}")
    assert D <= 1e-6 and D <= wc.D_ASSERTED and wc.gate(model) == wc.device_gate()


def few_pixel_weights(keep):
    """solve_weights with only ``keep`` pixels of slice 0 left"""
    w = wc.solve_weights()
    flat = w[0].reshape(-1)
    idx = np.flatnonzero(flat > 0)[::41][:keep]
    assert len(idx) == keep
    kept = flat[idx].copy()
    flat[:] = 0.0
    flat[idx] = kept
    return w


def mutant(name):
    """(what to patch in mri_inr_amd.align, its replacement, the geometry mode and the weights that show it)"""
    update, jac, mean = align.intensity_update, align.rigid_jacobian_w, align.lm_mean_w

    def jac_without_gain(c, s, cy, cx):
        B = jac(c, s, cy, cx)
        B[6][3] = 0.0
        return B

    return {"d6_d7_swapped": ("intensity_update", lambda gb, dg, db: update(gb, db, dg), align.AFFINE, wc.solve_weights()),
            "d3_d4_swapped_rigid": ("intensity_update", lambda gb, dg, db: update(gb, db, dg), align.RIGID, wc.solve_weights()),
            "P_is_6_in_estimate_mode": ("solved_parameters", lambda o: 3 if o.mode == align.RIGID else 6, align.AFFINE, few_pixel_weights(7)),
            "mean_by_count": ("lm_mean_w", lambda sums, P: mean([sums[0], sums[0], sums[2]], P), align.AFFINE, wc.solve_weights()),
            "B63_omitted": ("rigid_jacobian_w", jac_without_gain, align.RIGID, wc.solve_weights())}[name]


@pytest.mark.parametrize("name", ["d6_d7_swapped", "d3_d4_swapped_rigid", "P_is_6_in_estimate_mode", "mean_by_count", "B63_omitted"])
def test_the_checks_reject_every_seeded_mutant(name, monkeypatch):
    """A `device` that runs a mutated rule in estimate mode on slices 0 and 1 of sine5: the convergence check, the replay of its trace with the
    true rule, or the comparison of its report with the replayed states (the three checks tests/test_gpu_align_solve_w.py makes) has to fail."""
    model, slices = "sine5", [0, 1]
    attr, repl, mode, w = mutant(name)
    run, tg, seen = wc.reference_cost(model), wc.reference_targets(model)[slices], []

    def cost_fn(maps, gb):
        seen.append(run(maps, gb, tg, w[slices], slices))
        return seen[-1]

    true_step = align.lm_step_w
    start, rigid, o = sc.start_maps()[slices], sc.start_rigid()[slices], wc.options(mode, align.ESTIMATE)
    with monkeypatch.context() as mp:
        mp.setattr(align, attr, repl)
        res, _ = align.solve_on_host_w(cost_fn, len(slices), maps=start, rigid=rigid, options=o, trace=True)
    assert align.lm_step_w is true_step and getattr(align, attr) is not repl
    converged = bool((wc.errors(res.maps, res.intensity, slices) <= wc.REACHED).all())
    differs, st = wc.replay(res.trace, lambda k: seen[k], mode, align.ESTIMATE, start, rigid)
    want = align.solve_result_w(np.array([x["best"] for x in st], np.float32), np.array([x["gb_best"] for x in st], np.float32), None, align.report_w(st), None)
    report_same = all(np.array_equal(getattr(res, f), getattr(want, f), equal_nan=True) for f in ("maps", "intensity", "accepted", "mean_first", "mean_best", "count", "wsum",
                                                                                                 "damping", "flags"))
    print(f"{name}: errors {np.array2string(wc.errors(res.maps, res.intensity, slices), precision=2)}, the replay differs first at (evaluation, slice) {differs}, "
          f"report the same {report_same}")
    assert not converged or differs is not None or not report_same
    if name == "P_is_6_in_estimate_mode":  # the case shows the rule at all: 7 valid pixels are fewer than 8 parameters
        assert seen[0][0, 0] == 7.0 and want.flags[0] & align.NO_OVERLAP and want.mean_first[0] == np.inf and (differs is not None or not report_same)
