"""tests/align_reference.py, tests/align_cases.py and mri_inr_amd.align on the CPU: the point rule operation by operation, the chain rule
of the sums against central differences, the packing order, and the gate of tests/test_gpu_align.py -- it accepts the reference's own
perturbed-fp32 variant, which sits inside half the cap, and rejects every seeded mutant."""
import numpy as np
import pytest

import align_cases as ac
import align_reference as ar
import grad_reference as gr
import volume_cases as vc
from conftest import nerr
from mri_inr_amd import align
from mri_inr_amd import synthetic as syn

CASES = [(m, s) for m in ac.MODELS for s in ac.LATTICES]


def test_map_points_is_the_rule_operation_by_operation_in_float32():
    f = np.float32
    for shape in ((5, 7),) + ac.LATTICES:
        for row in ac.maps(shape):
            a = [f(x) for x in row]
            want = np.array([[f(f(f(a[0] * f(i)) + f(a[1] * f(j))) + a[2]), f(f(f(a[3] * f(i)) + f(a[4] * f(j))) + a[5])]
                             for i in range(shape[0]) for j in range(shape[1])], f)
            got = align.map_points(row, shape)
            assert got.dtype == f and got.shape == (shape[0] * shape[1], 2)
            assert np.array_equal(got, want) and np.array_equal(ar.points(row, shape), want)
    # not the fp64 expression rounded once: the two differ somewhere on these lattices
    row, shape = ac.maps((47, 45))[1], (47, 45)
    i, j = np.repeat(np.arange(47.0), 45), np.tile(np.arange(45.0), 47)
    once = (row[0].astype(np.float64) * i + row[1].astype(np.float64) * j + row[2]).astype(f)
    assert not np.array_equal(once, align.map_points(row, shape)[:, 0])
    assert align.map_points(row, (0, 5)).shape == (0, 2)
    # every product a i is zero or a normal fp32 number
    for shape in ac.LATTICES:
        for row in ac.maps(shape):
            prods = np.concatenate([np.outer(row[[0, 3]], np.arange(shape[0])).ravel(), np.outer(row[[1, 4]], np.arange(shape[1])).ravel()]).astype(f)
            assert np.all((prods == 0) | (np.abs(prods) >= np.finfo(f).tiny))
    with pytest.raises(ValueError):
        align.map_points(np.zeros(5), (2, 2))


def test_rigid_maps_unpack_and_gauss_newton_step():
    m = align.rigid_maps([0.0, np.pi / 2], [[0.5, -1.0], [0.0, 0.0]], (10.0, 20.0))
    assert m.dtype == np.float32 and m.shape == (2, 6)
    assert m[0].tolist() == [1.0, 0.0, 0.5, 0.0, 1.0, -1.0]
    p = align.map_points(m[1], (21, 41)).reshape(21, 41, 2)
    assert np.abs(p[10, 20] - [10, 20]).max() <= 1e-5 and np.abs(p[10, 21] - [9, 20]).max() <= 1e-5 and np.abs(p[11, 20] - [10, 21]).max() <= 1e-5
    ang, sh, c = np.array([0.1234567]), np.array([[1 / 3, 1 / 7]]), (9.5, 11.25)
    cs, sn = np.cos(ang[0]), np.sin(ang[0])
    want = np.array([cs, -sn, c[0] - (cs * c[0] - sn * c[1]) + sh[0, 0], sn, cs, c[1] - (sn * c[0] + cs * c[1]) + sh[0, 1]])
    assert np.array_equal(align.rigid_maps(ang, sh, c)[0], want.astype(np.float32))  # formed in fp64, rounded once
    sums = np.arange(2 * 29, dtype=np.float64).reshape(2, 29)
    r = align.unpack(sums)
    assert r.count.dtype == np.int64 and r.count.tolist() == [0, 29] and r.cost.tolist() == [1.0, 30.0] and r.grad[0].tolist() == [2, 3, 4, 5, 6, 7]
    assert np.array_equal(r.jtj, r.jtj.transpose(0, 2, 1)) and r.jtj[0, 0].tolist() == [8, 9, 10, 11, 12, 13] and r.jtj[0, 1, 1:].tolist() == [14, 15, 16, 17, 18]
    assert r.jtj[0, 5, 5] == 28 and r.jtj[0, 4, 5] == 27 and r.warped is None and r.wgrad is None
    with pytest.raises(ValueError):
        align.unpack(np.zeros((2, 28)))
    # a linear model: one step solves it; fewer than six valid pixels: no step
    rng = np.random.default_rng(0)
    J, delta = rng.normal(size=(40, 6)), rng.normal(size=6)
    res = align.AlignResult(np.array([40, 5]), np.zeros(2), np.stack([2 * J.T @ (-J @ delta)] * 2), np.stack([J.T @ J] * 2), None, None)
    step = align.gauss_newton_step(res)
    assert np.abs(step[0] - delta).max() <= 1e-12 and not step[1].any()
    assert np.abs(align.gauss_newton_step(res, damping=1.0)[0]).sum() < np.abs(delta).sum()


def test_packing_order_on_a_hand_computed_two_pixel_case():
    # lattice 2 x 3; valid pixels (i, j) = (0, 1): R 0, T 2, gY 1, gX -1 -> r = -2, J = (0, 1, 1, 0, -1, -1)
    #                               and (1, 2): R 1.5, T 1, gY 2, gX 3  -> r = .5, J = (2, 4, 2, 3, 6, 3)
    T = np.full((2, 3), np.nan, np.float32)
    R, gY, gX = np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3))
    T[0, 1], R[0, 1], gY[0, 1], gX[0, 1] = 2, 0, 1, -1
    T[1, 2], R[1, 2], gY[1, 2], gX[1, 2] = 1, 1.5, 2, 3
    sums, mags = ar.sums_of_planes(R, gY, gX, T, (2, 3))
    assert sums.tolist() == [2, 4.25, 2, 0, -2, 3, 10, 7,
                             4, 8, 4, 6, 12, 6, 17, 9, 12, 23, 11, 5, 6, 11, 5, 9, 18, 9, 37, 19, 10]
    assert mags[:8].tolist() == [2, 4.25, 2, 8, 6, 3, 10, 7] and mags[8] == 4 and mags[17] == 25  # (|6 x 4| + |-1 x 1|)
    res = align.unpack(sums[None])
    assert res.jtj[0, 1].tolist() == [8, 17, 9, 12, 23, 11] and res.jtj[0, 4, 1] == 23 and res.jtj[0, 5].tolist() == [6, 11, 5, 9, 19, 10]
    R[0, 0] = np.inf  # an invalid plane value behind a NaN target, and behind a finite one: left out either way
    T[1, 0], gX[1, 0] = 1.0, np.nan
    assert np.array_equal(ar.sums_of_planes(R, gY, gX, T, (2, 3))[0], sums)


@pytest.mark.parametrize("act", ["sine", "morlet"])
def test_single_tile_dcost_matches_central_differences_of_the_cost(act):
    """A slice that one tile covers entirely (nV = nH = 1): the blend is that tile's value, the cost is smooth in the six parameters."""
    L, shape = 5, (9, 11)
    sd = syn.make_state_dict(seed=7)
    mods = syn.make_mods(3, L, 1, 256)
    i, j = np.repeat(np.arange(shape[0]), shape[1]).astype(np.float64), np.tile(np.arange(shape[1]), shape[0]).astype(np.float64)
    target = (0.3 * np.sin(0.4 * i) + 0.2 * np.cos(0.3 * j)).reshape(shape)

    def sums_at(a):
        Y, X = a[0] * i + a[1] * j + a[2], a[3] * i + a[4] * j + a[5]
        lo, hi = -vc.PAD, -vc.PAD + vc.S - 1
        assert Y.min() > lo and Y.max() < hi and X.min() > lo and X.max() < hi  # every pixel covered, at both ends of a difference too
        coords = np.stack([-1.0 + (Y + vc.PAD) * 2.0 / (vc.S - 1), -1.0 + (X + vc.PAD) * 2.0 / (vc.S - 1)], axis=1)
        v, g = gr.value_and_grad(sd, mods, coords, num_layers=L, activation=act)
        g = g * (2.0 / (vc.S - 1))  # per reconstruction pixel
        return ar.sums_of_planes(v[0], g[0, 0], g[1, 0], target, shape)[0]

    a0 = np.array([1.1, -0.15, 1.5, 0.2, 0.9, 0.5])
    ref = sums_at(a0)
    assert ref[0] == shape[0] * shape[1]
    h, fd = 1e-6, np.zeros(6)
    for k in range(6):
        step = np.zeros(6)
        step[k] = h
        fd[k] = (sums_at(a0 + step)[1] - sums_at(a0 - step)[1]) / (2 * h)
    e = nerr(ref[2:8], fd)
    print(f"{act}: cost {ref[1]:.3f} dcost {ref[2:8]} nerr against central differences {e:.2e}")
    assert e <= 1e-7, e  # (tests/test_grad_reference.py's tolerance for its own central differences)


@pytest.mark.parametrize("model,shape", CASES)
def test_reference_sums_are_sane_and_jtj_is_positive_semi_definite(model, shape):
    d = ac.data(model, shape)
    res = align.unpack(d["sums"])
    pixels = shape[0] * shape[1]
    assert res.count[3] == pixels and res.count[0] == pixels - 15          # the black slice is valid everywhere; the NaN block
    assert 0 < res.count[2] < pixels and np.isnan(d["planes"][0, 2]).any()  # part of slice 2's lattice is outside every cover
    assert not d["sums"][3, 2:].any() and d["sums"][3, 1] > 0               # black: R = gY = gX = 0, the cost is the target's
    assert np.array_equal(res.jtj, res.jtj.transpose(0, 2, 1))
    for s in range(ac.N):
        ev = np.linalg.eigvalsh(res.jtj[s])
        assert ev.min() >= -1e-10 * max(ev.max(), 1.0), (s, ev)
    assert (res.cost > 0).all() and np.abs(res.grad[:3]).min() > 0


@pytest.mark.parametrize("model,shape", CASES)
def test_gate_accepts_the_fp32_variant_inside_half_the_cap_and_rejects_the_mutants(model, shape):
    d = ac.data(model, shape)
    print(f"{model} {shape}: distance of the perturbed-fp32 variant {d['D']:.2e}, gate {d['gate']:.2e} (cap {ac.CAP:.0e})")
    assert 0 < d["D"] <= ac.CAP / 2 and d["gate"] == ac.FACTOR * d["D"]
    assert ac.accepts(d, d["variant"]) and ac.accepts(d, d["sums"])
    for seed in ar.SEEDS:
        mutant = np.stack([ar.sums_of_planes(d["planes"][0, s], d["planes"][1, s], d["planes"][2, s], d["targets"][s], shape, seed)[0] for s in range(ac.N)])
        worst = ac.scaled_errors(mutant, d["sums"], d["mags"])[:, 1:].max()
        print(f"    {seed}: largest scaled error {worst:.2e}, counts {mutant[:, 0].astype(int).tolist()}")
        assert not ac.accepts(d, mutant), seed
