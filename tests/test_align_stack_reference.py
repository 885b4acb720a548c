"""msiren_align_stack_r's rule on the CPU: mri_inr_amd/align_stack.py, the bit-for-bit restatement the device is pinned to by
tests/test_gpu_align_stack.py, checked against what it has to mean.  The read against an independent dense trilinear reference within a bound
derived from the terms' magnitudes; exactness on the integer ramp and at integer points; the faces to the ulp; NaN corners propagated; dcost over all
eleven parameters against central differences inside one cell; scale +inf against the same sums with wl = wq = w; the summation order against
math.fsum within its bound; the host loops on the solve cases with the figures tests/align_stack_cases.py records; six seeded mutants rejected."""
import math

import numpy as np
import pytest

import align_stack_cases as sc
import align_stack_reference as asr
from mri_inr_amd import align_stack as ast, align_volume as av

U = 2.0 ** -52


def lattice_points(shape=(19, 23)):
    return np.concatenate([av.map_points3(mp, shape) for mp in sc.maps(shape)])


def extra_points():
    """the faces to the ulp, integer points, the corners of the stack"""
    up, down = sc._up, sc._down
    pts = [(z, y, x) for z in (0.0, 1.0, 3.0) for y in (0.0, 7.0, 20.0) for x in (0.0, 11.0, 26.0)]
    pts += [(1.5, 20.0, 26.0), (1.5, down(20.0), down(26.0)), (1.5, up(20.0), 3.0), (1.5, 3.0, up(26.0)), (up(3.0), 3.0, 3.0), (down(3.0), 3.0, 3.0), (3.0, 20.0, 26.0),
            (down(0.0), 1.0, 1.0), (1.0, down(0.0), 1.0), (1.0, 1.0, down(0.0)), (np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (2.25, 19.5, 25.75)]
    return np.array(pts, np.float32)


@pytest.mark.parametrize("name", sc.STACKS)
def test_the_read_agrees_with_a_dense_trilinear_reference(name):
    """both are a handful of fp64 operations on the same eight corners: they differ by at most 16 x 2^-52 x sum |weight corner|, and the read is rounded
    to float32 once (2^-24 relative)"""
    pts = np.concatenate([lattice_points(), extra_points()])
    got = np.stack(ast.read_stack(sc.stack(name), pts)).astype(np.float64)
    ref, mag = asr.dense(sc.stack(name), pts)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got[0]), np.isnan(ref[0])) or name == "holes"
    assert np.array_equal(np.isfinite(got), fin)  # (holes: a NaN or infinite corner makes both non-finite)
    err = np.abs(got[fin] - ref[fin])
    bound = 2.0 ** -24 * np.abs(ref[fin]) + 16 * U * mag[fin]
    print(name, "points", fin.sum() // 4, "max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert fin[0].sum() > 1500


def test_on_the_ramp_the_value_and_the_gradient_are_exact():
    pts = np.concatenate([lattice_points(), extra_points()])
    R, gZ, gY, gX = ast.read_stack(sc.stack("ramp"), pts)
    ins = np.isfinite(R)
    p = pts[ins].astype(np.float64)
    want = sc.RAMP[0] + sc.RAMP[1] * p[:, 0] + sc.RAMP[2] * p[:, 1] + sc.RAMP[3] * p[:, 2]  # (exact in fp64: small integers times fp32 numbers)
    assert np.array_equal(R[ins], want.astype(np.float32))
    assert (gZ[ins] == sc.RAMP[1]).all() and (gY[ins] == sc.RAMP[2]).all() and (gX[ins] == sc.RAMP[3]).all()


@pytest.mark.parametrize("name", ("smooth", "holes"))
def test_at_integer_points_the_value_has_the_voxels_bits(name):
    v = sc.stack(name)
    z, y, x = np.mgrid[0:sc.N, 0:sc.H, 0:sc.W]
    pts = np.stack([z, y, x], axis=-1).reshape(-1, 3).astype(np.float32)
    R = ast.read_stack(v, pts)[0].reshape(v.shape)
    whole = np.ones(v.shape, bool)  # a voxel whose cell holds a corner that is not finite reads NaN (0 x NaN): the others read their own bits
    for a, b, c in np.argwhere(~np.isfinite(v)):
        whole[max(a - 1, 0):a + 1 + (a == 0), max(b - 1, 0):b + 1 + (b == 0), max(c - 1, 0):c + 1 + (c == 0)] = False
    assert np.array_equal(R[whole].view(np.uint32), v[whole].view(np.uint32)) and whole.sum() > 0.5 * v.size
    assert np.isnan(R[~np.isfinite(v)]).all()


def test_the_faces_to_the_ulp_and_nan_corners():
    up, down = sc._up, sc._down
    v = sc.stack("smooth")
    R = ast.read_stack(v, np.array([(1.0, 20.0, 26.0), (3.0, 20.0, 26.0), (1.0, up(20.0), 26.0), (1.0, 20.0, up(26.0)), (up(3.0), 20.0, 26.0),
                                    (1.0, down(20.0), down(26.0)), (-0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (down(0.0), 0.0, 0.0)], np.float32))[0]
    assert R[0] == v[1, 20, 26] and R[1] == v[3, 20, 26] and np.isnan(R[2:5]).all() and np.isfinite(R[5]) and R[7] == v[0, 0, 0]
    assert R[6] == v[0, 0, 0] and np.isnan(R[8])  # (-0.0 >= 0: inside; the largest negative number: outside)
    h = sc.stack("holes")
    Rh = ast.read_stack(h, np.array([(1.0, 8.0, 12.0), (1.0, 8.5, 12.5), (1.0, 8.0, 11.0), (2.0, 3.5, 19.5), (2.5, 2.0, 2.0), (3.0, 6.0, 2.0)], np.float32))
    # the first point sits on a finite voxel of a cell whose far corner (1, 9, 13) is NaN: weight 0 x NaN is NaN, the pixel is lost on purpose
    assert np.isnan(Rh[0][0]) and np.isnan(Rh[0][1]) and np.isfinite(Rh[0][2]) and not np.isfinite(Rh[0][3]) and np.isnan(Rh[0][4]) and np.isfinite(Rh[0][5])


def test_the_summation_order_is_a_sum():
    rng = np.random.default_rng(5)
    for Mt in (1, 255, 437, 1024, 1221, 2049):
        t = rng.standard_normal((Mt, 7)) * np.exp(rng.uniform(-8, 8, (Mt, 1)))
        got = ast.chunk_sums(t)
        for a in range(7):
            exact, mag = math.fsum(t[:, a]), math.fsum(np.abs(t[:, a]))
            assert abs(got[a] - exact) <= 16 * 2.0 ** -53 * mag  # (at most 4 + 6 + 3 + chunks additions deep)
    assert np.array_equal(ast.chunk_sums(np.zeros((0, 3))), np.zeros(3))
    one = np.zeros((1221, 2))
    one[[0, 255, 256, 1023, 1024, 1220], 0] = [1, 2, 4, 8, 16, 32]
    assert ast.chunk_sums(one)[0] == 63.0


@pytest.mark.parametrize("scale", (sc.INF, 0.01))
def test_dcost_against_central_differences_inside_one_cell(scale):
    """a target whose every pixel stays inside one cell of the stack under every perturbed map: the cost is smooth there (a polynomial over a rational
    function of it), so central differences in fp64 with step h converge as h^2"""
    v = sc.stack("smooth")
    th, tw = 5, 6
    mp = np.array([0.02, 0.015, 1.3, 0.05, 0.02, 7.3, 0.01, 0.06, 11.25], np.float32)
    gb = np.array([1.1, 0.05], np.float32)
    pts = av.map_points3(mp, (th, tw))
    assert (np.floor(pts).min(axis=0) == np.floor(pts).max(axis=0)).all()
    rng = np.random.default_rng(3)
    tg = (ast.read_stack(v, pts)[0].reshape(1, th, tw) * 1.2 + 0.1 * rng.standard_normal((1, th, tw))).astype(np.float32)
    w = rng.uniform(0.3, 1.0, (1, th, tw)).astype(np.float32)

    def cost(par):  # the cost in plain fp64 from fp64 parameters (no fp32 rounding of the map: the derivative of the rule's own polynomial)
        i, j = np.mgrid[0:th, 0:tw].astype(np.float64)
        Z, Y, X = (par[3 * r] * i + par[3 * r + 1] * j + par[3 * r + 2] for r in range(3))
        fz, fy, fx = Z - 1, Y - 7, X - 11
        c = v[1:3, 7:9, 11:13].astype(np.float64)
        R = sum(c[a, b, d] * (fz if a else 1 - fz) * (fy if b else 1 - fy) * (fx if d else 1 - fx) for a in range(2) for b in range(2) for d in range(2))
        r = par[9] * R + par[10] - tg[0]
        return float((w[0] * r * r / (1.0 + r * r / scale)).sum())

    res = ast.result_on_host(v, tg, mp[None], scale, weights=w, intensity=gb[None])
    par = np.concatenate([mp.astype(np.float64), gb.astype(np.float64)])
    assert abs(res.cost[0] - cost(par)) <= 1e-6 * abs(res.cost[0])  # (the rule's points are fp32)
    for a in range(11):
        h = 1e-4 * max(1.0, abs(par[a]))
        lo, hi = par.copy(), par.copy()
        lo[a] -= h
        hi[a] += h
        fd = (cost(hi) - cost(lo)) / (2 * h)
        scale_a = max(abs(fd), np.abs(res.grad[0]).max() * 1e-3)
        assert abs(res.grad[0, a] - fd) <= 2e-5 * scale_a, (a, res.grad[0, a], fd)


@pytest.mark.parametrize("name,shape", [(n, s) for n in sc.STACKS for s in sc.LATTICES])
def test_scale_inf_is_the_weighted_square_loss(name, shape):
    """with s = +inf the sums are the same terms formed with wl = wq = w, added in the same order: bit for bit"""
    d = sc.data(name, shape)
    th, tw = shape
    sums, warped, wgrad, rw = ast.cost_on_host(d["stack"], d["targets"], d["maps"], sc.INF, weights=d["weights"], intensity=d["intensity"])
    for q in range(sc.M):
        R, gZ, gY, gX = (x[q].ravel() for x in (warped, wgrad[0], wgrad[1], wgrad[2]))
        T, w = d["targets"][q].ravel(), d["weights"][q].ravel()
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(T) & np.isfinite(R) & np.isfinite(gZ) & np.isfinite(gY) & np.isfinite(gX) & np.isfinite(w) & (w > 0)
        terms = np.zeros((th * tw, 80))
        px = np.nonzero(ok)[0]
        g, b = (float(x) for x in d["intensity"][q])
        R64, wd = R[ok].astype(np.float64), w[ok].astype(np.float64)
        r = ((g * R64) + b) - T[ok].astype(np.float64)
        gz, gy, gx = (g * x[ok].astype(np.float64) for x in (gZ, gY, gX))
        di, dj = (px // tw).astype(np.float64), (px % tw).astype(np.float64)
        J = [gz * di, gz * dj, gz, gy * di, gy * dj, gy, gx * di, gx * dj, gx, R64, np.ones_like(R64)]
        terms[ok] = np.stack([np.ones_like(r), wd, (wd * r) * r] + [(2.0 * (wd * r)) * J[a] for a in range(11)] + [(wd * J[a]) * J[c] for a, c in ast.PACK], axis=1)
        assert np.array_equal(sums[q], ast.chunk_sums(terms)), q
        assert np.array_equal(rw[q].ravel()[ok], np.ones(ok.sum(), np.float32)) and np.isnan(rw[q].ravel()[~ok]).all()
    assert not sums[list(sc.OUTSIDE)].any() and (sums[[0, 1, 2, 3, 4, 5, 7, 8], 0] > 100).all()


def test_scales_that_are_not_positive_score_nothing_and_every_case_has_its_pixels():
    d = sc.data("holes", (33, 37))
    for s in sc.SCALES[:3]:
        res = ast.result_on_host(d["stack"], d["targets"], d["maps"], s, weights=d["weights"], intensity=d["intensity"])
        dead = ~(s > 0)
        assert not res.count[dead].any() and np.isnan(res.rweight[dead]).all() and np.isfinite(res.warped[dead]).any()
        live = (s > 0) & ~np.isin(np.arange(sc.M), sc.OUTSIDE)
        assert (res.count[live] > 100).all() and np.isfinite(res.cost).all()
    smooth = ast.result_on_host(sc.stack("smooth"), d["targets"], d["maps"], sc.INF)
    holes = ast.result_on_host(d["stack"], d["targets"], d["maps"], sc.INF)
    assert (holes.count <= smooth.count).all() and holes.count.sum() < smooth.count.sum()  # the holes cost pixels, never add any


@pytest.mark.parametrize("est", sc.MODES)
def test_the_host_loop_reaches_the_truth_on_the_gate_groups(est):
    res, _ = sc.reference_solve("masked", est)
    e = sc.errors(res, est)
    print("masked", est, e)
    assert (e[list(sc.GATE_GROUPS)] <= sc.REACHED).all() and e.max() <= sc.SOLVE_FIGURES["masked"] * 1.01
    assert res.count[sc.SOLVE_OUTSIDE] == 0 and (res.flags == 0).all()
    t = sc.truth()
    assert np.abs(res.maps[sc.SOLVE_OUTSIDE].astype(np.float64) - t[sc.SOLVE_OUTSIDE]).max() <= sc.REACHED  # placed by its group


@pytest.mark.parametrize("est", sc.MODES)
def test_the_unmasked_case_needs_the_loss(est):
    rob, quad = sc.reference_solve("robust", est)[0], sc.reference_solve("quadratic", est)[0]
    er, eq = sc.errors(rob, est), sc.errors(quad, est)
    print("robust", est, er, "quadratic", eq)
    assert (er <= sc.ROBUST_REACHED).all() and er.max() <= sc.SOLVE_FIGURES["robust"] * 1.01
    assert (eq - er >= sc.QUADRATIC_MARGIN).all() and eq.min() >= sc.SOLVE_FIGURES["quadratic"] * 0.99


@pytest.mark.parametrize("case", ("masked", "robust"))
def test_d_solve_of_the_perturbed_fp32_variant(case):
    D = max(sc.errors(sc.reference_solve(case, est, True)[0], est)[list(sc.GATE_GROUPS)].max() for est in sc.MODES)
    print(case, "D_solve", D, "recorded", sc.D_SOLVE[case])
    assert D <= sc.D_SOLVE_ASSERTED[case] and abs(D - sc.D_SOLVE[case]) <= 0.1 * sc.D_SOLVE[case]


def test_the_variant_is_another_arithmetic_close_to_the_rule():
    d = sc.data("smooth", (19, 23))
    a = ast.cost_on_host(d["stack"], d["targets"], d["maps"], sc.SCALES[3], weights=d["weights"], intensity=d["intensity"])[0]
    b = sc.variant_cost(d["stack"], d["targets"], d["maps"], sc.SCALES[3], d["weights"], d["intensity"])
    assert np.array_equal(a[:, 0], b[:, 0]) and not np.array_equal(a, b)
    np.testing.assert_allclose(b[:, 2], a[:, 2], rtol=1e-4)


# ---- seeded mutants: each has to be rejected by what the tests above and the device's bit comparison check -------------------------------------------
def _points_for_mutants():
    return np.concatenate([lattice_points(), lattice_points((33, 37)), extra_points()])


def test_mutant_gz_from_the_blended_value():
    pts = _points_for_mutants()
    ref, mag = asr.dense(sc.stack("smooth"), pts)
    got = np.stack(asr.mutant_read(sc.stack("smooth"), pts, "gz_from_blend")).astype(np.float64)
    fin = np.isfinite(ref[1])
    assert (np.abs(got[1][fin] - ref[1][fin]) > 2.0 ** -24 * np.abs(ref[1][fin]) + 16 * U * mag[1][fin]).any()
    assert (asr.mutant_read(sc.stack("ramp"), pts, "gz_from_blend")[1][fin] != sc.RAMP[1]).any()


def test_mutant_fz_without_the_clamp():
    pts = np.array([(3.0, 5.0, 5.0), (3.0, 20.0, 26.0)], np.float32)  # on the upper Z face the fraction has to be 1, not 0
    v = sc.stack("smooth")
    got = asr.mutant_read(v, pts, "fz_without_clamp")[0]
    assert (got != v[3, [5, 20], [5, 26]]).all() and (ast.read_stack(v, pts)[0] == v[3, [5, 20], [5, 26]]).all()


def test_mutant_x_and_y_passes_swapped_is_seen_in_bits_only():
    """The same polynomial in another association: inside the reference's bound, told apart only by the bits of the fp64 stage, in front of the final
    rounding (``rounded=False``).  Behind that rounding the two agreed on every one of these 18 278 x 4 float32 values (asserted, so that it is known):
    the rule fixes the association so that the restatement is one function, but at these cases a float32 output cannot show it."""
    pts = _points_for_mutants()
    v = sc.stack("smooth")
    got, want = np.stack(asr.mutant_read(v, pts, "xy_passes_swapped", rounded=False)), np.stack(ast.read_stack(v, pts, rounded=False))
    ref, mag = asr.dense(v, pts)
    fin = np.isfinite(ref)
    assert (np.abs(got[fin] - ref[fin]) <= 16 * U * mag[fin]).all() and (np.abs(want[fin] - ref[fin]) <= 16 * U * mag[fin]).all()
    differ = (got != want) & fin
    print("fp64 values that differ in bits:", int(differ.sum()), "of", int(fin.sum()))
    assert differ.sum() > 100  # (measured 2 283 of 49 496: many lattice points have a zero fraction on an axis, where the two agree)
    assert np.array_equal(got.astype(np.float32), want.astype(np.float32), equal_nan=True)
    faithful = np.stack(asr.mutant_read(v, pts, "fz_without_clamp", rounded=False))[:, pts[:, 0] < 3]  # (away from its error the copy is the rule, bit for bit)
    assert np.array_equal(faithful, want[:, pts[:, 0] < 3], equal_nan=True)


def test_mutant_a_point_on_the_upper_face_refused():
    pts = np.array([(1.0, 20.0, 3.0), (1.0, 3.0, 26.0), (3.0, 3.0, 3.0)], np.float32)
    assert np.isnan(asr.mutant_read(sc.stack("smooth"), pts, "upper_face_refused")[0]).all() and np.isfinite(ast.read_stack(sc.stack("smooth"), pts)[0]).all()
    d = sc.data("smooth", (19, 23))  # and in the cases: targets 2 (Z = n - 1) and 7 (on both faces) lose every pixel
    assert ast.result_on_host(d["stack"], d["targets"], d["maps"]).count[[2, 7]].min() > 400


def test_mutant_a_nan_corner_skipped():
    pts = np.array([(1.0, 8.0, 12.0), (1.0, 8.5, 12.5), (2.0, 3.5, 19.5)], np.float32)
    h = sc.stack("holes")
    assert np.isfinite(asr.mutant_read(h, pts, "nan_corner_skipped")[0]).all() and not np.isfinite(ast.read_stack(h, pts)[0]).any()


def test_mutant_the_y_and_x_extents_swapped():
    pts = np.array([(1.0, 3.0, 23.5), (1.0, 3.0, 26.0), (1.0, 20.5, 3.0)], np.float32)  # X beyond H - 1 is inside; Y beyond H - 1 is not
    got, want = asr.mutant_read(sc.stack("smooth"), pts, "yx_extents_swapped")[0], ast.read_stack(sc.stack("smooth"), pts)[0]
    assert np.isnan(got[:2]).all() and np.isfinite(want[:2]).all() and np.isnan(want[2])


def test_the_outer_loop_on_the_host_lowers_the_map_error():
    """reconstruct -> register -> reconstruct on the host restatements: the figures tests/align_stack_cases.py records, before any device run"""
    first, reg, second = sc.outer_on_host()
    start, after = sc.outer_error(sc.outer_case()["start"]), sc.outer_error(reg.maps)
    print("map error at the start", start, "behind the alignment", after)
    assert after < start and abs(start - sc.OUTER_START) <= 1e-3 and abs(after - sc.OUTER_AFTER) <= 1e-3
    assert np.isfinite(first.volume).mean() > 0.9 and np.isfinite(second.volume).mean() > 0.9 and reg.count[2:-1].min() > 400
