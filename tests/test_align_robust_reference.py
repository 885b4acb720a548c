"""tests/align_robust_reference.py, tests/align_robust_cases.py and mri_inr_amd.align_robust on the CPU (no GPU needed): with
an infinite scale the robust reference is section 5.14's exactly, dcost is the exact gradient of the robust cost over all 11 parameters (central
differences), robust_terms restates the reference's per-pixel lines, the gate of tests/test_gpu_align_robust.py accepts the reference's own
perturbed-fp32 variant and rejects every seeded mutant; then the solve: on the grouped case with its corruption NOT masked the fp64 loop on the robust
sums reaches the truth, the quadratic loop on the same inputs does not, and the variant loop sizes the device's gate.  The step rule is section
5.15's (tests/test_align_group_reference.py)."""
import numpy as np
import pytest

import align_group_cases as gc
import align_robust_cases as rc
import align_robust_reference as arr
import align_volume_w_reference as avwr
import grad_reference as gr
import volume_cases as vc
from conftest import nerr
from mri_inr_amd import align_group as ag, align_robust as ar, align_volume as av
from mri_inr_amd import synthetic as syn

CASES = [(m, s) for m in rc.MODELS for s in rc.LATTICES]
SOLVES = [(m, est) for m in rc.MODELS for est in rc.MODES]
INF = float("inf")


def test_the_cases_are_what_the_cases_file_says():
    assert rc.SCALE.shape == (rc.M,) and rc.SCALE[0] == INF and np.isnan(rc.SCALE[5]) and rc.SCALE[4] == 0.0
    assert {0.01, 1.0, 2.0 ** -4} <= set(rc.SCALE.tolist()) and [q for q in range(rc.M) if not rc.SCALE[q] > 0] == list(rc.UNSCORED)
    w, old = rc.weights(), gc.weights()
    block = (slice(None),) + gc.wc.BLOCK
    assert (w[block] == 1.0).all() and not old[block].any() and (w > 0).all()  # nothing masks the corruption
    keep = np.ones(w.shape, bool)
    keep[block] = False
    assert np.array_equal(w[keep], old[keep])
    assert np.array_equal(rc.solve_scale(), np.full(gc.M, 0.01)) and rc.ITERATIONS == 20 and rc.GROUP_START.tolist() == [0, 3, 4, 6]
    tg, clean = gc.reference_targets("morlet3"), gc.reference_targets("morlet3", corrupted=False)
    diff = (tg.astype(np.float64) - clean)[:gc.OUTSIDE]
    assert np.abs(diff[block] - gc.wc.CORRUPTION).max() < 1e-6 and not diff[keep[:gc.OUTSIDE]].any()


def test_the_helpers_of_the_package():
    t = ar.robust_terms(3.0, 0.5, 9.0)  # u = 1, v = 2, om = 0.5
    assert t == ar.RobustTerms(0.5, 0.25, 0.125, 2.25, 0.75)
    q = ar.robust_terms(-1.5, 0.75, INF)
    assert q.om == 1.0 and q.wl == q.wq == 0.75 and q.cost == (0.75 * -1.5) * -1.5 and q.dfac == 2.0 * (0.75 * -1.5)
    assert ar.scales(0.01, 3).tolist() == [0.01] * 3 and ar.scales([1.0, 2.0], 2).dtype == np.float64
    for bad in ([1.0, 2.0], np.ones((3, 1))):
        with pytest.raises(ValueError):
            ar.scales(bad, 3)
    res = av.unpack_vw(np.array([[4.0, 2.0, 8.0] + [0.0] * 77, [0.0] * 80]))
    assert ar.scale_from(res, 3.0).tolist() == [9.0 * 8.0 / 2.0, INF]
    r = ar.unpack_r(np.arange(80.0)[None], rweight=np.ones((1, 2, 2), np.float32))
    assert r._fields == av.AlignResultVW._fields + ("rweight",) and r.cost.tolist() == [2.0] and r.warped is None and r.rweight.shape == (1, 2, 2)
    assert np.array_equal(rc.packed(r), np.arange(80.0)[None])


@pytest.mark.parametrize("model,shape", CASES)
def test_an_infinite_scale_gives_the_weighted_reference_exactly(model, shape):
    d = rc.data(model, shape)
    sums, mags, rw = arr.align(d["planes"], d["targets"], d["weights"], d["intensity"], INF, rweight=True)
    want, wmags = avwr.align(d["planes"], d["targets"], d["weights"], d["intensity"])
    assert np.array_equal(sums, want) and np.array_equal(mags, wmags)
    assert (rw[np.isfinite(rw)] == 1.0).all() and np.isfinite(rw).sum() == want[:, 0].sum()
    assert np.array_equal(d["sums"][0], want[0]) and not d["sums"][list(rc.UNSCORED)].any()  # the case: target 0 at +inf, scale 0 and NaN count nothing
    assert np.array_equal(d["sums"][:, :2], np.where(np.isin(np.arange(rc.M), rc.UNSCORED)[:, None], 0.0, want[:, :2]))  # count and wsum stay plain
    assert (d["sums"][[1, 2, 3, 6], 2] < want[[1, 2, 3, 6], 2]).all()  # the loss is below the square


@pytest.mark.parametrize("act", ["sine", "morlet"])
@pytest.mark.parametrize("scale", [0.05, 2.0])
def test_single_tile_dcost_matches_central_differences_of_the_robust_cost_over_all_eleven_parameters(act, scale):
    """tests/test_align_volume_w_reference.py's construction -- two slices that one tile covers entirely, a lattice inside the segment 0 .. 1, smooth
    weights, a gain and a bias -- under the robust loss: dcost is the exact gradient of cost, not that of the majoriser's square."""
    L, shape = 5, (9, 11)
    sd = syn.make_state_dict(seed=7)
    mods = syn.make_mods(3, L, 2, 256)
    i, j = np.repeat(np.arange(shape[0]), shape[1]).astype(np.float64), np.tile(np.arange(shape[1]), shape[0]).astype(np.float64)
    target = (0.3 * np.sin(0.4 * i) + 0.2 * np.cos(0.3 * j)).reshape(shape)
    weight = (0.2 + 0.8 * np.exp(-((i - 4) / 5) ** 2 - ((j - 6) / 7) ** 2)).reshape(shape)
    weight[2:4, 3:6] = 0.0

    def sums_at(a, seed=None):
        Z, Y, X = a[0] * i + a[1] * j + a[2], a[3] * i + a[4] * j + a[5], a[6] * i + a[7] * j + a[8]
        lo, hi = -vc.PAD, -vc.PAD + vc.S - 1
        assert Y.min() > lo and Y.max() < hi and X.min() > lo and X.max() < hi and Z.min() > 0 and Z.max() < 1  # one cover, one segment
        coords = np.stack([-1.0 + (Y + vc.PAD) * 2.0 / (vc.S - 1), -1.0 + (X + vc.PAD) * 2.0 / (vc.S - 1)], axis=1)
        v, g = gr.value_and_grad(sd, mods, coords, num_layers=L, activation=act)
        g = g * (2.0 / (vc.S - 1))  # per reconstruction pixel
        R = (1 - Z) * v[0] + Z * v[1]
        return arr.sums_of_planes(R, v[1] - v[0], (1 - Z) * g[0, 0] + Z * g[0, 1], (1 - Z) * g[1, 0] + Z * g[1, 1], target, weight, a[9:11], scale, shape, seed)

    a0 = np.array([0.03, -0.02, 0.5, 1.1, -0.15, 1.5, 0.2, 0.9, 0.5, 1.2, -0.07])
    ref, _, rw = sums_at(a0)
    assert ref[0] == shape[0] * shape[1] - 6 and ref[1] == weight.sum()
    h, fd = 1e-6, np.zeros(11)
    for k in range(11):
        step = np.zeros(11)
        step[k] = h
        fd[k] = (sums_at(a0 + step)[0][2] - sums_at(a0 - step)[0][2]) / (2 * h)
    e = nerr(ref[3:14], fd)
    wrong = nerr(sums_at(a0, "dcost_with_wl")[0][3:14], fd)
    print(f"{act} scale {scale}: cost {ref[2]:.3f}, om^2 from {np.nanmin(rw):.3f} to {np.nanmax(rw):.3f}, nerr against central differences {e:.2e} (with wl in dcost: {wrong:.2e})")
    assert e <= 1e-7, e  # (section 5.14's bound, tests/test_grad_reference.py's tolerance for its own central differences)
    assert wrong > 1e-3 and np.nanmin(rw) < 0.9  # the loss bends inside the case: the majoriser's gradient is another vector


@pytest.mark.parametrize("model", list(rc.MODELS))
def test_robust_terms_restates_the_reference(model):
    """the five lines in Python floats per pixel against numpy's: om^2 bit for bit, the sums they build (pixels in index order) inside the bound of an
    fp64 sum in any order"""
    shape = (19, 23)
    d = rc.data(model, shape)
    pl, pixels = d["planes"], shape[0] * shape[1]
    for q in (1, 2, 3, 6):
        g, b, s = float(d["intensity"][q, 0]), float(d["intensity"][q, 1]), float(rc.SCALE[q])
        T, w = d["targets"][q].ravel(), d["weights"][q].ravel()
        R, gZ, gY, gX = (np.asarray(pl[c, q], np.float64).ravel() for c in range(4))
        acc, rw = [0.0] * 80, np.full(pixels, np.nan)
        for px in range(pixels):
            if not (np.isfinite([T[px], R[px], gZ[px], gY[px], gX[px], w[px]]).all() and w[px] > 0):
                continue
            i, j = float(px // shape[1]), float(px % shape[1])
            r = ((g * float(R[px])) + b) - float(T[px])
            t = ar.robust_terms(r, w[px], s)
            gz, gy, gx = g * float(gZ[px]), g * float(gY[px]), g * float(gX[px])
            J = [gz * i, gz * j, gz, gy * i, gy * j, gy, gx * i, gx * j, gx, float(R[px]), 1.0]
            rw[px] = t.om * t.om
            acc[0] += 1.0
            acc[1] += float(w[px])
            acc[2] += t.cost
            k = 14
            for a in range(11):
                acc[3 + a] += t.dfac * J[a]
                wj = t.wq * J[a]
                for c in range(a, 11):
                    acc[k] += wj * J[c]
                    k += 1
        assert np.array_equal(rw.reshape(shape), d["rweight"][q], equal_nan=True), q
        assert acc[0] == d["sums"][q, 0] and (np.abs(np.array(acc) - d["sums"][q]) <= pixels * 2.0 ** -52 * d["mags"][q]).all(), q


@pytest.mark.parametrize("model,shape", CASES)
def test_gate_accepts_the_fp32_variant_inside_half_the_cap_and_rejects_the_mutants(model, shape):
    d = rc.data(model, shape)
    print(f"{model} {shape}: distance of the perturbed-fp32 variant {d['D']:.2e}, gate {d['gate']:.2e} (cap {rc.CAP:.0e})")
    assert 0 < d["D"] <= rc.CAP / 2 and d["gate"] == rc.FACTOR * d["D"]
    assert rc.accepts(d, d["variant"]) and rc.accepts(d, d["sums"])
    for seed in arr.SEEDS:
        mutant = rc.mutant_sums(model, shape, seed)
        with np.errstate(invalid="ignore"):
            worst = np.nanmax(rc.scaled_errors(mutant, d["sums"], d["mags"])[:, 1:])
        print(f"    {seed}: largest scaled error {worst:.2e}, counts differ by {np.abs(mutant[:, 0] - d['sums'][:, 0]).astype(int).tolist()}")
        assert not rc.accepts(d, mutant), seed


# ---- the solve --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,est", SOLVES)
def test_the_robust_loop_reaches_the_truth_with_the_corruption_unmasked(model, est):
    res, (gs, ts), seen = rc.reference_solve(model, est)
    err = gc.errors(res, est)
    print(f"{model} intensity {est}: errors per group {np.array2string(err, precision=2)}, accepted {res.accepted.tolist()}, lam {res.damping.tolist()}, "
          f"flags {res.flags.tolist()}, (g, b) {res.intensity.tolist()}")
    assert (err[list(rc.GATE_GROUPS)] <= rc.REACHED).all(), err
    assert not res.flags.any() and (res.mean_best <= res.mean_first).all() and (res.accepted >= 3).all()
    inside = [q for q in range(gc.M) if q != gc.OUTSIDE]
    assert (res.count[inside] == gc.SHAPE[0] * gc.SHAPE[1]).all() and res.count[gc.OUTSIDE] == 0  # the corrupted block counts
    assert np.array_equal(res.wsum[inside], np.array([float(w.astype(np.float64).ravel().sum()) for w in rc.weights()[inside]]))  # the plain sum of the weights
    # the trace replays with the sums seen, under section 5.15's rule unchanged
    differs, st = gc.replay(res.trace, lambda k, maps, gb: seen[k], est, intensity=gc.start_intensity(est))
    rep, trep = ag.report_g(*st)
    assert differs is None and np.array_equal(rep[:, 0], res.accepted.astype(np.float64)) and np.array_equal(trep[:, 2], res.cost)


@pytest.mark.parametrize("model,est", SOLVES)
def test_the_quadratic_loop_on_the_same_inputs_stays_away_from_the_truth(model, est):
    """the proof that the case needs the loss: section 5.15's loop with the block unmasked"""
    res = rc.reference_solve(model, est, robust=False)[0]
    err = gc.errors(res, est)
    print(f"{model} intensity {est}: the quadratic loop's errors per group {np.array2string(err, precision=3)}")
    assert (err > rc.QUADRATIC_AWAY).all(), err


@pytest.mark.parametrize("model", list(rc.MODELS))
def test_the_variant_loop_sizes_the_gate(model):
    D = rc.D_solve(model)
    print(f"{model}: D_solve = {D:.2e} (the perturbed-fp32 variant's largest final error over the gate groups, both intensity modes), gate {rc.solve_gate(model):.2e}")
    assert D <= rc.D_SOLVE_ASSERTED and rc.solve_gate(model) == rc.device_solve_gate()
