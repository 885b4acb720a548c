"""tests/align_volume_w_reference.py, tests/align_volume_w_cases.py and the weighted half of mri_inr_amd.align_volume on the CPU (DESIGN.md section
5.14): with unit weights and (g, b) = (1, 0) the 56 shared sums are section 5.13's, the chain rule of the 80 sums over all 11 parameters against
central differences, the packing, the gate of tests/test_gpu_align_volume_w.py (it accepts the reference's own perturbed-fp32 variant and rejects
every seeded mutant), and the step rule of msiren_align_volume_solve_w: lm_step_vw on unit-weight sums is lm_step_v bit for bit, ldl_solve for 8
and 11, the 11 x 8 B against central differences, convergence of the loop on the fp64 reference to the map and (g, b), the variant loop that sizes
the device's gate, and seeded mutants of the rule against convergence and replay."""
import numpy as np
import pytest

import align_volume_cases as avc
import align_volume_reference as avr
import align_volume_w_cases as wc
import align_volume_w_reference as avwr
import grad_reference as gr
import volume_cases as vc
from conftest import nerr
from mri_inr_amd import align, align_volume as av
from mri_inr_amd import synthetic as syn

CASES = [(m, s) for m in wc.MODELS for s in wc.LATTICES]
ESTIMATE_CASES = [(m, mode) for m in wc.MODELS for mode in avc.MODES]


def test_the_cases_are_what_the_cases_file_says():
    for shape in wc.LATTICES:
        w = wc.weights(shape)
        assert w.shape == (wc.M,) + shape and w.dtype == np.float32
        assert np.isnan(w[wc.NONFINITE_AT]) and np.isnan(w).sum() == 1          # one weight that is not finite
        assert [(w[q] == 0).sum() for q in range(wc.M)] == [0, 24, 15, 0, 0, 0, 16]  # a zero block in three targets
        f = w[np.isfinite(w) & (w != 0)]
        assert 0.1 < f.min() and f.max() <= 1.0
    assert wc.INTENSITY.shape == (wc.M, 2) and len({tuple(x) for x in wc.INTENSITY.tolist()}) == wc.M
    assert len({tuple(x) for x in wc.GB_TRUTH.tolist()}) == 4 and wc.GB_TRUTH.shape == (wc.SOLVE_M, 2)
    sw = wc.solve_weights()
    assert (sw[(slice(None),) + wc.BLOCK] == 0).all() and (sw == 0).sum() == wc.SOLVE_M * 24 and sw.max() <= 1.0
    for model in wc.MODELS:
        tg, clean = wc.reference_targets(model), wc.reference_targets(model, corrupted=False)
        diff = tg.astype(np.float64) - clean
        assert np.abs(diff[(slice(None),) + wc.BLOCK] - wc.CORRUPTION).max() < 1e-6 and np.array_equal(np.nan_to_num(diff) != 0, np.broadcast_to(sw == 0, diff.shape))
        for est in (av.FIXED, av.ESTIMATE):
            assert len(wc.gate_targets(model, est)) >= 3
    assert wc.start_intensity(av.ESTIMATE) is None and np.array_equal(wc.start_intensity(av.FIXED), wc.GB_TRUTH)


def test_unpack_and_gauss_newton_step():
    sums = np.arange(2 * 80, dtype=np.float64).reshape(2, 80)
    r = av.unpack_vw(sums)
    assert r.count.dtype == np.int64 and r.count.tolist() == [0, 80] and r.wsum.tolist() == [1.0, 81.0] and r.cost.tolist() == [2.0, 82.0]
    assert r.grad[0].tolist() == list(range(3, 14)) and r.grad.shape == (2, 11)
    assert np.array_equal(r.jtj, r.jtj.transpose(0, 2, 1)) and r.jtj[0, 0].tolist() == list(range(14, 25)) and r.jtj[0, 1, 1:].tolist() == list(range(25, 35))
    assert r.jtj[0, 10, 10] == 79 and r.jtj[0, 9, 10] == 78 and r.warped is None and r.wgrad is None
    assert np.array_equal(wc.packed(r), sums)
    with pytest.raises(ValueError):
        av.unpack_vw(np.zeros((2, 56)))
    rng = np.random.default_rng(0)
    J, delta = rng.normal(size=(60, 11)), rng.normal(size=11)
    res = av.AlignResultVW(np.array([60, 10]), np.array([60.0, 10.0]), np.zeros(2), np.stack([2 * J.T @ (-J @ delta)] * 2), np.stack([J.T @ J] * 2), None, None)
    step = av.gauss_newton_step_vw(res)
    assert np.abs(step[0] - delta).max() <= 1e-12 and not step[1].any()
    nine = av.gauss_newton_step_vw(res, estimate_intensity=False)
    assert not nine[:, 9:].any() and nine[0, :9].any() and nine[1, :9].any()  # (10 valid pixels are enough for nine parameters)
    assert av.SUMS_VW == 80 == avwr.SUMS and len(avwr.SHARED) == av.SUMS_V


def test_packing_order_on_a_hand_computed_two_pixel_case():
    # lattice 2 x 3, (g, b) = (2, 0.5); valid pixels (i, j) = (0, 1): R 0, T 2, gZ 2, gY 1, gX -1, w 0.5 -> r = -1.5, J = (0, 4, 4, 0, 2, 2, 0, -2, -2, 0, 1)
    #                                               and (1, 2): R 1.5, T 1, gZ -1, gY 2, gX 3, w 0.25 -> r = 2.5, J = (-2, -4, -2, 4, 8, 4, 6, 12, 6, 1.5, 1)
    T = np.full((2, 3), np.nan, np.float32)
    R, gZ, gY, gX, w = (np.zeros((2, 3)) for _ in range(5))
    T[0, 1], R[0, 1], gZ[0, 1], gY[0, 1], gX[0, 1], w[0, 1] = 2, 0, 2, 1, -1, 0.5
    T[1, 2], R[1, 2], gZ[1, 2], gY[1, 2], gX[1, 2], w[1, 2] = 1, 1.5, -1, 2, 3, 0.25
    sums, mags = avwr.sums_of_planes(R, gZ, gY, gX, T, w, (2.0, 0.5), (2, 3))
    J = np.array([[0, 4, 4, 0, 2, 2, 0, -2, -2, 0, 1], [-2, -4, -2, 4, 8, 4, 6, 12, 6, 1.5, 1]], np.float64)
    r, ww = np.array([-1.5, 2.5]), np.array([0.5, 0.25])
    assert sums[:3].tolist() == [2, 0.75, 0.5 * 2.25 + 0.25 * 6.25] and sums[3:14].tolist() == (2 * ww * r @ J).tolist()
    H = J.T @ (ww[:, None] * J)
    assert sums[14:].tolist() == [H[a, b] for a in range(11) for b in range(a, 11)]
    assert np.array_equal(av.unpack_vw(sums[None]).jtj[0], H) and sums[79] == 0.75 and mags[1] == 0.75
    # weights that are zero, negative or not finite mask their pixel, whatever is behind them
    T[0, 0], T[1, 0], T[1, 1], T[0, 2] = 1.0, 1.0, 1.0, 1.0
    w[0, 0], w[1, 0], w[1, 1], w[0, 2] = 0.0, -1.0, np.nan, np.inf
    assert np.array_equal(avwr.sums_of_planes(R, gZ, gY, gX, T, w, (2.0, 0.5), (2, 3))[0], sums)


@pytest.mark.parametrize("model,shape", CASES)
def test_unit_weights_and_no_intensity_give_the_56_sums_of_the_plain_reference(model, shape):
    d = avc.data(model, shape)
    sums, mags = avwr.align(d["planes"], d["targets"], None, None)
    assert np.array_equal(sums[:, avwr.SHARED], d["sums"]) and np.array_equal(mags[:, avwr.SHARED], d["mags"])
    assert np.array_equal(sums[:, 1], sums[:, 0]) and np.array_equal(sums[:, 79], sums[:, 0])  # wsum = count = jtj[b, b]
    ones, _ = avwr.align(d["planes"], d["targets"], np.ones((wc.M,) + shape, np.float32), np.tile(np.array([1.0, 0.0], np.float32), (wc.M, 1)))
    assert np.array_equal(ones, sums)
    # the same through the helpers of the package
    r80, r56 = av.unpack_vw(sums), av.unpack_v(d["sums"])
    assert np.array_equal(r80.count, r56.count) and np.array_equal(r80.cost, r56.cost) and np.array_equal(r80.grad[:, :9], r56.grad)
    assert np.array_equal(r80.jtj[:, :9, :9], r56.jtj)


@pytest.mark.parametrize("act", ["sine", "morlet"])
def test_single_tile_dcost_matches_central_differences_of_the_cost_over_all_eleven_parameters(act):
    """tests/test_align_volume_reference.py's construction -- two slices that one tile covers entirely and a lattice inside the segment 0 .. 1 --
    with smooth weights and a gain and a bias: the cost is smooth in the nine map parameters and in (g, b)."""
    L, shape = 5, (9, 11)
    sd = syn.make_state_dict(seed=7)
    mods = syn.make_mods(3, L, 2, 256)
    i, j = np.repeat(np.arange(shape[0]), shape[1]).astype(np.float64), np.tile(np.arange(shape[1]), shape[0]).astype(np.float64)
    target = (0.3 * np.sin(0.4 * i) + 0.2 * np.cos(0.3 * j)).reshape(shape)
    weight = (0.2 + 0.8 * np.exp(-((i - 4) / 5) ** 2 - ((j - 6) / 7) ** 2)).reshape(shape)
    weight[2:4, 3:6] = 0.0

    def sums_at(a):
        Z, Y, X = a[0] * i + a[1] * j + a[2], a[3] * i + a[4] * j + a[5], a[6] * i + a[7] * j + a[8]
        lo, hi = -vc.PAD, -vc.PAD + vc.S - 1
        assert Y.min() > lo and Y.max() < hi and X.min() > lo and X.max() < hi and Z.min() > 0 and Z.max() < 1  # one cover, one segment
        coords = np.stack([-1.0 + (Y + vc.PAD) * 2.0 / (vc.S - 1), -1.0 + (X + vc.PAD) * 2.0 / (vc.S - 1)], axis=1)
        v, g = gr.value_and_grad(sd, mods, coords, num_layers=L, activation=act)
        g = g * (2.0 / (vc.S - 1))  # per reconstruction pixel
        R = (1 - Z) * v[0] + Z * v[1]
        return avwr.sums_of_planes(R, v[1] - v[0], (1 - Z) * g[0, 0] + Z * g[0, 1], (1 - Z) * g[1, 0] + Z * g[1, 1], target, weight, a[9:11], shape)[0]

    a0 = np.array([0.03, -0.02, 0.5, 1.1, -0.15, 1.5, 0.2, 0.9, 0.5, 1.2, -0.07])
    ref = sums_at(a0)
    assert ref[0] == shape[0] * shape[1] - 6 and ref[1] == weight.sum()
    h, fd = 1e-6, np.zeros(11)
    for k in range(11):
        step = np.zeros(11)
        step[k] = h
        fd[k] = (sums_at(a0 + step)[2] - sums_at(a0 - step)[2]) / (2 * h)
    e = nerr(ref[3:14], fd)
    print(f"{act}: cost {ref[2]:.3f} dcost {ref[3:14]} nerr against central differences {e:.2e}")
    assert e <= 1e-7, e  # (tests/test_grad_reference.py's tolerance for its own central differences)


@pytest.mark.parametrize("model,shape", CASES)
def test_gate_accepts_the_fp32_variant_inside_half_the_cap_and_rejects_the_mutants(model, shape):
    d = wc.data(model, shape)
    print(f"{model} {shape}: distance of the perturbed-fp32 variant {d['D']:.2e}, gate {d['gate']:.2e} (cap {wc.CAP:.0e})")
    assert 0 < d["D"] <= wc.CAP / 2 and d["gate"] == wc.FACTOR * d["D"]
    assert wc.accepts(d, d["variant"]) and wc.accepts(d, d["sums"])
    res = av.unpack_vw(d["sums"])
    plain = av.unpack_v(avc.data(model, shape)["sums"])
    assert (res.count <= plain.count).all() and res.count[1] == plain.count[1] - 24 and res.count[0] == plain.count[0] - 1 and (res.wsum < res.count).all()
    for seed in avwr.SEEDS:
        mutant = wc.mutant_sums(model, shape, seed)
        worst = wc.scaled_errors(mutant, d["sums"], d["mags"])[:, 1:].max()
        print(f"    {seed}: largest scaled error {worst:.2e}, counts differ by {np.abs(mutant[:, 0] - d['sums'][:, 0]).astype(int).tolist()}")
        assert not wc.accepts(d, mutant), seed


# ---- the step rule -----------------------------------------------------------------------------------------------------------------------------------
def test_ldl_solve_for_eight_and_eleven_against_numpy_on_random_spd_systems():
    rng = np.random.default_rng(11)
    for n in (8, 11):
        for _ in range(50):
            J = rng.normal(size=(44, n))
            A, b = J.T @ J, rng.normal(size=n)
            x, ok = av.ldl_solve(A.tolist(), b.tolist(), n)
            want = np.linalg.solve(A, b)
            assert ok and np.abs(np.array(x) - want).max() <= 1e-10 * np.abs(want).max()
    expect = {(align.AFFINE, av.FIXED): 9, (align.AFFINE, av.ESTIMATE): 11, (align.RIGID, av.FIXED): 6, (align.RIGID, av.ESTIMATE): 8}
    for (mode, est), P in expect.items():
        o = wc.options(mode, est)
        assert av.solved_parameters_vw(o) == P
        # a target that reads black slices only (R = gZ = gY = gX = 0: only the (b, b) entry of H is left) proposes nothing: SINGULAR, inputs kept
        st = av.lm_init_vw(o, avc.start_maps()[0], avc.start_rigid()[0], avc.planes()[0], wc.GB_TRUTH[0])
        before = list(st["trial"]), list(st["gb_trial"])
        black = [437.0, 300.0, 3.0] + [0.0] * 10 + [-2.0] + [0.0] * 65 + [300.0]
        av.lm_step_vw(st, black, 0, o)
        assert st["flags"] == align.SINGULAR and (st["trial"], st["gb_trial"]) == before and st["best"] == before[0] and st["mean_first"] == 3.0 / 300.0
        # fewer valid pixels than solved parameters (every weight masked: count 0): NO_OVERLAP
        st = av.lm_init_vw(o, avc.start_maps()[0], avc.start_rigid()[0], avc.planes()[0], None)
        av.lm_step_vw(st, [float(P - 1), 3.0, 1.0] + [0.0] * 77, 0, o)
        assert st["flags"] == align.SINGULAR | align.NO_OVERLAP and st["mean_first"] == align.INF and st["gb_trial"] == [1.0, 0.0]
        st = av.lm_init_vw(o, avc.start_maps()[0], avc.start_rigid()[0], avc.planes()[0], None)
        av.lm_step_vw(st, [0.0] * 80, 0, o)
        assert st["flags"] == align.SINGULAR | align.NO_OVERLAP and st["trial"] == before[0]


def test_rigid_jacobian3_w_against_central_differences():
    pl = avc.planes()[1:2] + np.array([[0.02, 0.0, 0.01, 0.0, 0.03, 0.0, 0, 0, 0, 0, 0, 0]])  # (a lattice that is not axis-aligned)
    for vec, sh in (((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.02, -0.03, 0.05), (0.3, -0.2, 0.7)), ((-0.4, 0.3, 0.2), (1.0, 8.0, -3.0))):
        Rot, sh = avc.rotation_of(vec), np.array(sh)
        state = Rot.ravel().tolist() + sh.tolist()
        B = np.array(av.rigid_jacobian3_w(state, pl[0].tolist(), avc.SPACING))
        assert B.shape == (11, 8)

        def params(x):  # (w, u, g, b) -> the 11 parameters: the map of the state moved by (w, u), then (g, b)
            mp = av.rigid_maps3((avc.rotation_of(x[:3]) @ Rot)[None], (sh + x[3:6])[None], pl, avc.SPACING, np.float64)[0]
            return np.concatenate([mp, [1.3 + x[6], -0.2 + x[7]]])

        h, fd = 1e-6, np.zeros((11, 8))
        for k in range(8):
            e = np.zeros(8)
            e[k] = h
            fd[:, k] = (params(e) - params(-e)) / (2 * h)
        assert np.abs(B - fd).max() <= 1e-8 * max(1.0, np.abs(B).max()), (vec, B, fd)
        assert np.array_equal(B[:9, :6], np.array(av.rigid_jacobian3(state, pl[0].tolist(), avc.SPACING)))
        assert B[9, 6] == 1.0 and B[10, 7] == 1.0 and not B[9:, :6].any() and not B[:9, 6:].any() and B[9, 7] == 0.0 and B[10, 6] == 0.0


@pytest.mark.parametrize("mode", avc.MODES)
def test_lm_step_vw_on_unit_weight_sums_is_lm_step_v_bit_for_bit(mode):
    """A plain loop (lm_step_v on the 56 sums) and a weighted loop with the intensity fixed at (1, 0) (lm_step_vw on the 80 sums of the same
    planes with unit weights), side by side on the fp64 reference: every trial map, rigid state, lambda, decision and flag is the same."""
    model, rows, iterations = "morlet3", [0, 3], 8
    run, tg = avc.reference_cost(model), avc.reference_targets(model)[rows]
    o9, o11 = avc.solve_options(mode, iterations=iterations), wc.options(mode, av.FIXED, iterations=iterations)
    start, rigid, pl = avc.start_maps()[rows], avc.start_rigid()[rows], avc.planes()[rows]
    s9 = [av.lm_init_v(o9, start[q], rigid[q], pl[q]) for q in range(2)]
    s11 = [av.lm_init_vw(o11, start[q], rigid[q], pl[q], None) for q in range(2)]
    for k in range(iterations):
        trial = np.array([x["trial"] for x in s9], np.float32)
        assert np.array_equal(trial, np.array([x["trial"] for x in s11], np.float32))
        sums56, _, planes = run(trial, tg)
        sums80 = avwr.align(planes, tg, None, None)[0]
        assert np.array_equal(sums80[:, avwr.SHARED], sums56)
        for q in range(2):
            av.lm_step_v(s9[q], sums56[q], k, o9)
            av.lm_step_vw(s11[q], sums80[q], k, o11)
            for key in ("trial", "best", "rigid_trial", "rigid_best", "mean_best", "mean_first", "lam", "accepted", "flags"):
                assert s9[q][key] == s11[q][key], (k, q, key)
            assert s11[q]["gb_trial"] == [1.0, 0.0] and s11[q]["gb_best"] == [1.0, 0.0]
    assert all(x["accepted"] >= 3 for x in s9)


@pytest.mark.parametrize("model,mode", ESTIMATE_CASES)
def test_the_loop_in_estimate_mode_reaches_map_and_intensity_on_the_fp64_reference(model, mode):
    res, rigid, seen = wc.reference_solve(model, mode, av.ESTIMATE)
    err, gate_targets = wc.errors(res.maps, res.intensity), list(wc.gate_targets(model, av.ESTIMATE))
    print(f"{model} mode {mode}: errors {np.array2string(err, precision=2)}, accepted {res.accepted.tolist()}, lam {res.damping.tolist()}, flags {res.flags.tolist()}, "
          f"(g, b) {res.intensity.tolist()}")
    assert (err[gate_targets] <= wc.REACHED).all(), err
    assert not res.flags[gate_targets].any() and (res.mean_best <= res.mean_first).all()
    assert res.trace.shape == (wc.ITERATIONS, wc.SOLVE_M, 14) and np.array_equal(res.trace[0, :, :9], avc.start_maps().astype(np.float64))
    assert np.array_equal(res.trace[0, :, 9:11], np.tile([1.0, 0.0], (wc.SOLVE_M, 1)))
    assert np.array_equal(res.trace[:, :, 11], seen[:, :, 2]) and np.array_equal(res.trace[:, :, 12], seen[:, :, 0]) and np.array_equal(res.trace[:, :, 13], seen[:, :, 1])
    assert (res.count == wc.SHAPE[0] * wc.SHAPE[1] - 24).all() and (res.wsum < res.count).all()  # the corrupted block never counts
    if mode == align.RIGID:
        assert np.array_equal(av.rigid_maps3(res.rotation, res.shift, avc.planes(), avc.SPACING), res.maps)  # the best map is the map of the best state
        assert np.abs(res.rotation[gate_targets] - avc.truth_rotations()[gate_targets]).max() <= 1e-6
        assert np.array_equal(rigid[:, :9].reshape(-1, 3, 3), res.rotation)
    else:
        assert res.rotation is None and res.shift is None
    # the trace replays: the check tests/test_gpu_align_volume_solve_w.py makes of the device
    differs, st = wc.replay(res.trace, lambda k: seen[k], mode, av.ESTIMATE, avc.start_maps(), avc.start_rigid(), avc.planes(), None)
    assert differs is None and np.array_equal(av.report_vw(st)[:, 0], res.accepted.astype(np.float64))


@pytest.mark.parametrize("model", list(wc.MODELS))
def test_the_variant_loop_sizes_the_gate(model):
    D = wc.D_solve(model)
    print(f"{model}: D_solve = {D:.2e} (the perturbed-fp32 variant's largest final error over the gate targets, both modes, intensity estimated), gate {wc.solve_gate(model):.2e}")
    assert D <= wc.D_SOLVE_ASSERTED and wc.solve_gate(model) == wc.device_solve_gate()


def mutant(name):
    """(what to patch in mri_inr_amd.align_volume, its replacement, the geometry mode that shows it)"""
    ldl, jacw, mean = av.ldl_solve, av.rigid_jacobian3_w, av.lm_mean_vw

    def last_two_swapped(A, b, m):
        d, ok = ldl(A, b, m)
        d[m - 2], d[m - 1] = d[m - 1], d[m - 2]
        return d, ok

    def jac_without_gain_column(state, plane, spacing):
        B = jacw(state, plane, spacing)
        B[9][6] = 0.0
        return B

    return {"dg_db_swapped_affine": ("ldl_solve", last_two_swapped, align.AFFINE),
            "dg_db_swapped_rigid": ("ldl_solve", last_two_swapped, align.RIGID),
            "B_9_6_omitted": ("rigid_jacobian3_w", jac_without_gain_column, align.RIGID),
            "step_sign_flipped": ("ldl_solve", lambda A, b, m: ([-x for x in ldl(A, b, m)[0]], ldl(A, b, m)[1]), align.AFFINE),
            "intensity_not_updated": ("intensity_update_vw", lambda gb, dg, db: list(gb), align.AFFINE),
            "mean_over_count_squared": ("lm_mean_vw", lambda sums, P: mean(sums, P) * sums[1] / sums[0] / sums[0], align.RIGID)}[name]


@pytest.mark.parametrize("name", ["dg_db_swapped_affine", "dg_db_swapped_rigid", "B_9_6_omitted", "step_sign_flipped", "intensity_not_updated",
                                  "mean_over_count_squared"])
def test_the_checks_reject_every_seeded_mutant_of_the_step_rule(name, monkeypatch):
    """A `device` that runs a mutated rule in estimate mode, on targets 0 and 1 of morlet3: the convergence check, the replay of its trace with the
    true rule or the report against the replayed states has to fail."""
    model, rows = "morlet3", [0, 1]
    attr, repl, mode = mutant(name)
    run, tg, w, seen = wc.reference_cost(model), wc.reference_targets(model)[rows], wc.solve_weights()[rows], []

    def cost_fn(maps, gb):
        seen.append(run(maps, gb, tg, w))
        return seen[-1]

    true_step = av.lm_step_vw
    start, rigid, pl = avc.start_maps()[rows], avc.start_rigid()[rows], avc.planes()[rows]
    with monkeypatch.context() as mp:
        mp.setattr(av, attr, repl)
        res, _ = av.solve_on_host_vw(cost_fn, len(rows), maps=start, rigid=rigid, planes=pl, options=wc.options(mode, av.ESTIMATE, iterations=12), trace=True)
    assert av.lm_step_vw is true_step and getattr(av, attr) is not repl
    converged = bool((wc.errors(res.maps, res.intensity, rows) <= wc.REACHED).all())
    differs, st = wc.replay(res.trace, lambda k: seen[k], mode, av.ESTIMATE, start, rigid, pl, None)
    report = np.stack([res.accepted, res.mean_first, res.mean_best, res.count, res.wsum, res.damping, res.flags], axis=1).astype(np.float64)
    report_differs = differs is None and not np.array_equal(report, av.report_vw(st))
    print(f"{name}: errors {np.array2string(wc.errors(res.maps, res.intensity, rows), precision=2)}, the replay differs first at (evaluation, target) {differs}, "
          f"the report differs {report_differs}")
    assert not converged or differs is not None or report_differs
