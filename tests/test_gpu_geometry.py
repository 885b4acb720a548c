"""The point and alignment families on the GPU off the 3 x 3 square slice (DESIGN.md sections 5.8 to 5.16): msiren_resample_slices*,
msiren_resample_volume*, msiren_align_slices[_w]*, msiren_align_volume[_w, _r]*, one per-slice and one grouped solve, on the geometries of
tests/geometry_cases.py -- nV != nH everywhere, KA = ceil(S / I) = 1, 2, 3, 4, a black tile column in one slice and a black tile row in another.

Values against the fp64 reference within the project's norm (max <= 1e-4 of max|ref|, rms <= 1e-5), gradients within the case's
gate (4 x the reference's own perturbed-fp32 floor, capped at that norm), NaN exactly where the reference has none; the costs carry the three
assertions of tests/test_gpu_align.py (the planes are resample's bits, the sums lie inside the any-order fp64 bound on the call's own planes and
inside the case's gate against the fp64 reference); the solves equal the host loop around the device's own cost bit for bit.  What a transposed tile
index, an exchanged nV / nH, a transposed black list, truncated slots or a fixed pad would do to these gates: tests/test_geometry_reference.py.  The
distances measured on the MI355X are in LAB_NOTES.md section 40.
"""
import functools

import numpy as np
import pytest

import align_group_cases as gc
import align_reference as ar
import align_robust_reference as arr
import align_solve_cases as sc
import align_volume_reference as avr
import align_volume_w_cases as vwc
import align_volume_w_reference as avwr
import align_w_cases as wc
import align_w_reference as awr
import geometry_cases as gcs
import grad_reference as gr
import volume_reference as vr
from mri_inr_amd import ModulatedSiren, _lib, align, align_group as ag, align_volume as av, synthetic as syn
from test_gpu_align import packed as packed29, profile_off, profile_on, same
from test_gpu_align_group import same as same_group
from test_gpu_align_solve import same as same_solve
from test_gpu_align_volume import packed as packed56

pytestmark = pytest.mark.gpu

GEOS = list(gcs.GEOMETRIES)
N = gcs.N
NORM_MAX, NORM_RMS = 1e-4, 1e-5


def build(sd, I, S, *, L=5, act="sine", prec="fp32"):
    m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=L, latent_dim=256, w0=1.0, w0_initial=30.0, use_bias=True, dropout=0.1, modulate=True,
                       encoder_type="custom", encoder_path=None, outer_patch_size=gcs.O, inner_patch_size=I, siren_patch_size=S, device="cuda", activation=act,
                       precision=prec)
    m.load_state_dict(sd, strict=True)
    m.to("cuda")
    m.eval()
    return m


@functools.lru_cache(maxsize=None)
def model(name, prec="fp32", which="sine5"):
    geo, mo = gcs.GEOMETRIES[name], gcs.MODELS[which]
    return build(gcs.state_dict(name, which), geo.I, geo.S, L=mo["L"], act=mo["act"], prec=prec)


@functools.lru_cache(maxsize=None)
def resampled(name, prec="fp32"):
    val, grad = model(name, prec).resample_with_gradient(gcs.images(name), gcs.data(name)["points"])
    return np.array(val), np.array(grad)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- resample ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", GEOS)
def test_resample_against_the_reference(name, prec):
    d, m, img = gcs.data(name), model(name, prec), gcs.images(name)
    val, grad = resampled(name, prec)
    ok, M = d["finite"], len(d["points"])
    assert val.shape == (N, M) and grad.shape == (2, N, M) and val.dtype == np.float32
    vm, vrms = gr.distances(val[:, ok], d["value"][:, ok])
    gm, grms = gr.distances(grad[:, :, ok], d["grad"][:, :, ok])
    print(f"{name} {prec}: values max {vm:.2e} rms {vrms:.2e} (norm {NORM_MAX:.0e} / {NORM_RMS:.0e}); gradients max {gm:.2e} (gate {d['gate'][0]:.2e}) rms {grms:.2e} "
          f"(gate {d['gate'][1]:.2e})")
    assert vm <= NORM_MAX and vrms <= NORM_RMS
    assert gm <= d["gate"][0] and grms <= d["gate"][1]
    assert np.array_equal(np.isfinite(val), np.broadcast_to(ok, val.shape)) and np.array_equal(np.isfinite(grad), np.broadcast_to(ok, grad.shape))  # NaN exactly there
    assert np.array_equal(bits(m.resample(img, d["points"])), bits(val))                                                              # the value form: the same bits
    assert gcs.outside_the_gate(d, val, grad) is None
    # black tiles: a point under slice 1's black column alone is zero there and nowhere else, and likewise slice 2's black row
    geo, pts = gcs.GEOMETRIES[name], d["points"]
    col0, row0 = ok & (pts[:, 1] < geo.I - geo.pad), ok & (pts[:, 0] < geo.I - geo.pad)
    assert not val[1, col0].any() and not grad[:, 1, col0].any() and val[0, col0].all() and val[2, col0 & ~row0].all()
    assert not val[2, row0].any() and not grad[:, 2, row0].any() and val[0, row0].all() and val[1, row0 & ~col0].all()


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", GEOS)
def test_resample_windows_permutation_and_batch(name, prec):
    d, m, img = gcs.data(name), model(name, prec), gcs.images(name)
    val, grad = resampled(name, prec)
    recon, rgrad = m.reconstruct_with_gradient(img)
    geo = gcs.GEOMETRIES[name]
    assert recon.shape == (N, geo.nV * geo.I, geo.nH * geo.I)
    for key in ("window_y", "window_x"):  # the integer pixels of a window across a seam of each axis: the fp32 reconstruction
        sl = d["parts"][key]
        w = d["points"][sl].astype(int)
        for got, ref, what in ((val[:, sl], recon[:, w[:, 0], w[:, 1]], "values"), (grad[:, :, sl], rgrad[:, :, w[:, 0], w[:, 1]], "gradients")):
            em, er = gr.distances(got, ref)
            print(f"{name} {prec} {key}, {what}: max {em:.2e} rms {er:.2e}")
            assert em <= NORM_MAX and er <= NORM_RMS, (key, what)
    perm = np.random.default_rng(9).permutation(len(d["points"]))
    vp, gp = m.resample_with_gradient(img, d["points"][perm])  # permuted points give permuted bits
    assert np.array_equal(bits(vp), bits(val[:, perm])) and np.array_equal(bits(gp), bits(grad[:, :, perm]))
    for s in range(N):                                         # a slice alone is the slice in the batch
        v1, g1 = m.resample_with_gradient(img[s], d["points"])
        assert np.array_equal(bits(v1), bits(val[s])) and np.array_equal(bits(g1), bits(grad[:, s])), s


# ---- resample_volume --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GEOS)
def test_resample_volume_against_the_reference(name):
    d, m, img = gcs.data3(name), model(name), gcs.images(name)
    pts, ok = d["points"], d["finite"]
    val, grad = (np.array(x) for x in m.resample_volume_with_gradient(img, pts))
    assert val.shape == (len(pts),) and grad.shape == (3, len(pts))
    vm, vrms = gr.distances(val[ok], d["value"][ok])
    gm, grms = gr.distances(grad[1:, ok], d["grad"][1:, ok])
    print(f"{name}: values max {vm:.2e} rms {vrms:.2e}; grad[1:] max {gm:.2e} (gate {d['gate'][0]:.2e}) rms {grms:.2e} (gate {d['gate'][1]:.2e})")
    assert vm <= NORM_MAX and vrms <= NORM_RMS and gm <= d["gate"][0] and grms <= d["gate"][1]
    assert np.array_equal(np.isfinite(val), ok) and np.array_equal(np.isfinite(grad), np.broadcast_to(ok, grad.shape))
    assert np.isnan(val[d["parts"]["invalid_z"]]).all() and np.isnan(grad[:, d["parts"]["invalid_z"]]).all()  # an invalid Z: NaN in every plane
    assert np.array_equal(bits(m.resample_volume(img, pts)), bits(val))                                          # the value form: the same bits
    # the slope along Z is one fp32 subtraction of the two slices' values, and those are resample's bits at (Y, X)
    rows, grows = m.resample_with_gradient(img, pts[:, 1:])
    z0, f = vr.pairs(pts, N)
    idx = np.flatnonzero(ok)
    assert same(grad[0, idx], rows[z0[idx] + 1, idx] - rows[z0[idx], idx])
    whole = idx[f[idx] == 0]
    assert len(whole) >= 200 and same(val[whole], rows[z0[whole], whole]) and same(grad[1:, whole], grows[:, z0[whole], whole])
    err, bound = np.abs(grad[0, ok].astype(np.float64) - d["grad"][0, ok]).max(), 2e-4 * np.abs(d["value"][ok]).max()
    print(f"{name}: grad[0] max abs err {err:.2e} (bound {bound:.2e})")
    assert err <= bound


# ---- the costs: the three assertions of tests/test_gpu_align.py ---------------------------------------------------------------------------------------------
def check_sums(got, planes_of, case, what):
    """``got`` (units, sums) inside the any-order fp64 bound on the call's own planes (``planes_of(u)`` -> (want, mags)) and inside the case's gate"""
    shape = case["targets"].shape[1:]
    pixels = shape[0] * shape[1]
    for u in range(len(got)):
        want, mags = planes_of(u)
        bound = pixels * 2.0 ** -52 * mags  # the worst case of an fp64 sum of N terms in any order (and of the terms' own roundings)
        err = np.abs(got[u] - want)
        assert got[u, 0] == want[0], (what, u)
        assert (err[1:] <= bound[1:]).all(), (what, u, err, bound)
    e = gcs.ac.scaled_errors(got, case["sums"], case["mags"])
    print(f"{what}: counts {got[:, 0].astype(int).tolist()} distance {e.max():.2e}, reference's own {case['D']:.2e}, gate {case['gate']:.2e}")
    assert got[:, 0].tolist() == case["sums"][:, 0].tolist() and gcs.accepts(case, got), (what, e.max(axis=1), case["gate"])


@pytest.mark.parametrize("name,which,shape", gcs.COST_CASES)
def test_slice_costs(name, which, shape):
    d, m, img = gcs.align_data(name, which, shape), model(name, "fp32", which), gcs.images(name)
    p, w = d["plain"], d["w"]
    res = m.align_cost(img, p["targets"], p["maps"], warped=True, gradient=True)
    resw = m.align_cost_w(img, w["targets"], w["maps"], weights=w["weights"], intensity=w["intensity"], warped=True, gradient=True)
    assert res.warped.shape == (N,) + shape and res.wgrad.shape == (2, N) + shape
    for s in range(N):  # the planes are the bits of resample_with_gradient at align.map_points
        val, grad = m.resample_with_gradient(img, align.map_points(p["maps"][s], shape))
        assert same(res.warped[s].ravel(), val[s]) and same(res.wgrad[:, s].reshape(2, -1), grad[:, s]), s
    assert same(resw.warped, res.warped) and same(resw.wgrad, res.wgrad)
    assert np.isfinite(res.warped).any(axis=(1, 2)).all()
    check_sums(packed29(res), lambda s: ar.sums_of_planes(res.warped[s], res.wgrad[0, s], res.wgrad[1, s], p["targets"][s], shape), p, f"{name} {which} {shape} align_cost")
    check_sums(wc.packed(resw), lambda s: awr.sums_of_planes(res.warped[s], res.wgrad[0, s], res.wgrad[1, s], w["targets"][s], w["weights"][s], w["intensity"][s], shape), w,
               f"{name} {which} {shape} align_cost_w")


@pytest.mark.parametrize("name,which,shape", gcs.COST_CASES)
def test_volume_costs(name, which, shape):
    d, m, img = gcs.align_volume_data(name, which, shape), model(name, "fp32", which), gcs.images(name)
    p, w, r = d["plain"], d["w"], d["r"]
    tg, maps = p["targets"], p["maps"]
    res = m.align_volume_cost(img, tg, maps, warped=True, gradient=True)
    resw = m.align_volume_cost_w(img, tg, maps, weights=w["weights"], intensity=w["intensity"], warped=True, gradient=True)
    resr = m.align_volume_cost_r(img, tg, maps, r["scale"], weights=r["weights"], intensity=r["intensity"], warped=True, gradient=True)
    assert res.warped.shape == (gcs.M3,) + shape and res.wgrad.shape == (3, gcs.M3) + shape
    for q in range(gcs.M3):  # the planes are the bits of resample_volume_with_gradient at align_volume.map_points3
        val, grad = m.resample_volume_with_gradient(img, av.map_points3(maps[q], shape))
        assert same(res.warped[q].ravel(), val) and same(res.wgrad[:, q].reshape(3, -1), grad), q
    for other in (resw, resr):
        assert same(other.warped, res.warped) and same(other.wgrad, res.wgrad)
    assert np.isnan(res.warped[:2]).any() and np.isfinite(res.warped).any(axis=(1, 2)).all()  # targets 0 and 1 leave 0 <= Z <= n - 1
    W, G = res.warped, res.wgrad
    what = f"{name} {which} {shape}"
    check_sums(packed56(res), lambda q: avr.sums_of_planes(W[q], G[0, q], G[1, q], G[2, q], tg[q], shape), p, what + " align_volume_cost")
    check_sums(vwc.packed(resw), lambda q: avwr.sums_of_planes(W[q], G[0, q], G[1, q], G[2, q], tg[q], w["weights"][q], w["intensity"][q], shape), w, what + " align_volume_cost_w")
    check_sums(vwc.packed(resr), lambda q: arr.sums_of_planes(W[q], G[0, q], G[1, q], G[2, q], tg[q], r["weights"][q], r["intensity"][q], r["scale"][q], shape)[:2], r,
               what + " align_volume_cost_r")


# ---- the solves on rect: the host loop around the device's own cost, bit for bit ------------------------------------------------------------------------------
def test_align_solve_is_the_host_loop_on_rect():
    name, it = "rect", 4
    m, img, move = model(name), gcs.images(name), np.float32(gcs.GEOMETRIES[name].shift)
    truth, start = sc.truth()[:N].copy(), sc.start_maps()[:N].copy()
    truth[:, 5] += move
    start[:, 5] += move
    tg = m.align_cost(img, np.zeros((N,) + sc.SHAPE, np.float32), truth, warped=True).warped  # zero residual at the truth; an uncovered pixel stays NaN: masked
    res = m.align_solve(img, tg, start, iterations=it, trace=True)
    host, _ = align.solve_on_host(lambda maps: packed29(m.align_cost(img, tg, maps)), N, maps=start, options=sc.options(align.AFFINE, iterations=it), trace=True)
    assert res.trace.shape == (it, N, 8) and np.array_equal(res.trace, host.trace, equal_nan=True)
    assert same_solve(res, host), (res[:9], host[:9])
    assert res.accepted.sum() >= N and (res.mean_best < res.mean_first).all() and not np.array_equal(res.maps, start)


def test_align_volume_solve_group_is_the_host_loop_on_rect():
    name, it, est = "rect", 4, av.ESTIMATE
    m, img, move = model(name), gcs.images(name), gcs.GEOMETRIES[name].shift
    planes = gc.planes()
    planes[:, 8] += move   # o and c of every plane along X
    planes[:, 11] += move
    truth = np.array([av.rigid_map3([float(x) for x in gc.truth_rigid()[y]], [float(x) for x in p], gc.SPACING) for p, y in zip(planes, gc.GROUP_OF)], np.float32)
    tg = gc.targets_of(m.align_volume_cost(img, np.zeros((gc.M,) + gc.SHAPE, np.float32), truth, warped=True).warped)
    w = gc.weights()
    res = m.align_volume_solve_group(img, tg, planes, gc.SPACING, gc.GROUP_START, weights=w, estimate_intensity=True, iterations=it, trace=True)
    host, _ = ag.solve_on_host_g(lambda maps, gb: vwc.packed(m.align_volume_cost_w(img, tg, maps, weights=w, intensity=gb)), gc.GROUP_START, rigid=gc.start_rigid(),
                                 planes=planes, intensity=gc.start_intensity(est), options=gc.options(est, iterations=it), trace=True)
    assert res.trace.shape == (it, gc.G, 15) and np.array_equal(res.trace, host.trace)
    assert same_group(res, host), (res[:12], host[:12])
    assert (res.accepted >= 1).all() and res.count[:gc.OUTSIDE].all() and res.count[gc.OUTSIDE] == 0


# ---- a _dev form with (height, width) = (40, 72) -----------------------------------------------------------------------------------------------------------------
def test_dev_form_on_rect_gives_the_bits_of_the_host_form():
    name = "rect"
    m, img, pts = model(name), gcs.images(name), gcs.data(name)["points"]
    val, grad = resampled(name)
    n, height, width = img.shape
    assert (height, width) == (40, 72)
    M = len(pts)
    d_i, d_p = m.device_array(img.shape).copy_from(img), m.device_array(pts.shape).copy_from(pts)
    d_v, d_g, d_v2 = m.device_array((n, M)), m.device_array((2, n, M)), m.device_array((n, M))
    _lib.check(m._lib.msiren_resample_slices_grad_dev(m._h, d_i.ptr, n, height, width, d_p.ptr, M, d_v.ptr, d_g.ptr))
    _lib.check(m._lib.msiren_resample_slices_dev(m._h, d_i.ptr, n, height, width, d_p.ptr, M, d_v2.ptr))
    m.sync()
    assert np.array_equal(bits(d_v.numpy()), bits(val)) and np.array_equal(bits(d_g.numpy()), bits(grad)) and np.array_equal(bits(d_v2.numpy()), bits(val))


# ---- KA > 4 is refused -------------------------------------------------------------------------------------------------------------------------------------------
def test_more_than_four_covering_tiles_per_axis_are_refused():
    I, S = 4, 20  # KA = 5
    sd = syn.make_state_dict(seed=7, num_layers=5, siren_patch_size=S, trained_like=True)
    m = build(sd, I, S)
    img = np.stack([syn.make_slice(3 + s, 40, 40) for s in range(2)])
    recon = m.reconstruct(img)  # the fold has no such limit
    assert recon.shape == (2, 40, 40) and np.isfinite(recon).all() and recon.any()
    shape = (5, 6)
    pts = np.array([[3.5, 4.25], [20.0, 20.0]], np.float32)
    pts3 = np.array([[0.5, 3.5, 4.25]], np.float32)
    tg2, maps2 = np.full((2,) + shape, 0.5, np.float32), np.tile(np.array([1, 0, 5, 0, 1, 5], np.float32), (2, 1))
    maps3 = np.tile(np.array([0, 0, 0.5, 1, 0, 5, 0, 1, 5], np.float32), (2, 1))
    calls = [lambda: m.resample(img, pts), lambda: m.resample_with_gradient(img, pts), lambda: m.resample_volume(img, pts3),
             lambda: m.resample_volume_with_gradient(img, pts3), lambda: m.align_cost(img, tg2, maps2), lambda: m.align_cost_w(img, tg2, maps2),
             lambda: m.align_volume_cost(img, tg2, maps3), lambda: m.align_volume_cost_r(img, tg2, maps3, 1.0), lambda: m.align_solve(img, tg2, maps2, iterations=2)]
    m.sync()
    profile_on(m)
    try:
        for k, call in enumerate(calls):
            with pytest.raises(ValueError, match="siren_patch_size"):
                call()
            assert "more than 4 tiles per axis" in _lib.last_error(), k
        d = m.device_array(img.shape).copy_from(img)
        m.sync()
        assert m.profile_kernels() == []
        assert m._lib.msiren_resample_slices_dev(m._h, d.ptr, 2, 40, 40, d.ptr, 2, d.ptr) == _lib.E_INVALID and "siren_patch_size" in _lib.last_error()
        m.sync()
        assert m.profile_kernels() == [] and np.array_equal(d.numpy(), img)
    finally:
        profile_off(m)
    assert np.array_equal(m.reconstruct(img), recon)  # the handle stays usable
