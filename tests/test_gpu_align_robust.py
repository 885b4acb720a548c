"""Robust alignment of target slices to the stack read as a volume on the GPU: model.align_volume_cost_r, i.e.
msiren_align_volume_r* -- section 5.14's pipeline with the Geman-McClure reduce -- and model.align_volume_solve_group_robust, i.e.
msiren_align_volume_solve_group_r* -- section 5.15's loop on those sums.  Cases, reference and gates: tests/align_robust_cases.py.

With scale +inf both calls have to return the weighted calls' bits; the sums are compared with numpy on the call's own planes inside the worst-case
bound of an fp64 sum in any order (N 2^-52 sum|term|, N the pixels of a target: the five roundings of a term's factors are far inside it) and with
the fp64 reference inside section 5.14's gate; rweight is the float32 of align_robust.robust_terms' om^2 on the call's own planes, bit for bit.  The
device loop is pinned bit for bit against the host loop (align_robust.solve_on_host_r around model.align_volume_cost_r), trace included; the solve
case leaves its + 5 corruption unmasked and converges where the quadratic loop ends 0.049 away or more (tests/test_align_robust_reference.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import align_group_cases as gc
import align_robust_cases as rc
import align_robust_reference as arr
import align_volume_cases as avc
import volume_cases as vc
from mri_inr_amd import _lib, align_group as ag, align_robust as ar, align_volume as av
from test_gpu_align import model, profile_off, profile_on, same

pytestmark = pytest.mark.gpu

N, M, HW = rc.N, rc.M, rc.HW
CASES = [(m, s) for m in rc.MODELS for s in rc.LATTICES]
PRECS = ["fp32", "f16x3"]
SUMS = av.SUMS_VW
INF = float("inf")
packed = rc.packed
SHAPE, SM, G, IT = rc.SHAPE, rc.SOLVE_M, rc.G, rc.ITERATIONS
ALL = [(prec, name, est) for prec in PRECS for name in rc.MODELS for est in rc.MODES]


def f64_dev(m, x):
    """a float64 array on the device, as pairs of floats"""
    x = np.ascontiguousarray(x, np.float64)
    return m.device_array(x.shape + (2,)).copy_from(x.view(np.float32).reshape(x.shape + (2,)))


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_result_r(name, shape, prec="fp32"):
    d = rc.data(name, shape)
    return model(name, prec).align_volume_cost_r(vc.images(), d["targets"], d["maps"], rc.SCALE, weights=d["weights"], intensity=d["intensity"], warped=True, gradient=True,
                                                 rweight=True)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,shape", CASES)
def test_with_an_infinite_scale_the_sums_and_planes_are_align_volume_cost_ws_bits(name, shape, prec):
    m, d = model(name, prec), rc.data(name, shape)
    old = m.align_volume_cost_w(vc.images(), d["targets"], d["maps"], weights=d["weights"], intensity=d["intensity"], warped=True, gradient=True)
    for scale in (INF, np.full(M, INF)):
        new = m.align_volume_cost_r(vc.images(), d["targets"], d["maps"], scale, weights=d["weights"], intensity=d["intensity"], warped=True, gradient=True, rweight=True)
        assert np.array_equal(packed(new), packed(old)) and same(new.warped, old.warped) and same(new.wgrad, old.wgrad)
        assert (new.rweight[np.isfinite(new.rweight)] == 1.0).all() and np.isfinite(new.rweight).sum() == old.count.sum()
    plain = m.align_volume_cost_r(vc.images(), d["targets"], d["maps"], INF)  # without weights and intensity too
    assert np.array_equal(packed(plain), packed(m.align_volume_cost_w(vc.images(), d["targets"], d["maps"])))
    res = gpu_result_r(name, shape, prec)  # finite scales: the planes are untouched, target 0 (scale +inf) keeps section 5.14's sums
    assert same(res.warped, old.warped) and same(res.wgrad, old.wgrad) and np.array_equal(packed(res)[0], packed(old)[0])
    assert not np.array_equal(packed(res)[1, 2:], packed(old)[1, 2:]) and np.array_equal(packed(res)[1, :2], packed(old)[1, :2])  # count and wsum stay plain


@pytest.mark.parametrize("name,shape", CASES)
def test_sums_against_the_calls_own_planes(name, shape):
    res, d = gpu_result_r(name, shape), rc.data(name, shape)
    got, pixels = packed(res), shape[0] * shape[1]
    for q in range(M):
        want, mags, _ = arr.sums_of_planes(res.warped[q], res.wgrad[0, q], res.wgrad[1, q], res.wgrad[2, q], d["targets"][q], d["weights"][q], d["intensity"][q], rc.SCALE[q], shape)
        bound = pixels * 2.0 ** -52 * mags  # the worst case of an fp64 sum of N terms in any order (and of the terms' own roundings)
        err = np.abs(got[q] - want)
        print(f"{name} {shape} target {q}: scale {rc.SCALE[q]}, count {int(got[q, 0])}, largest error / bound {np.max(err[1:] / np.maximum(bound[1:], 1e-300)):.3f}")
        assert got[q, 0] == want[0], q
        assert (err[1:] <= bound[1:]).all(), (q, err, bound)
    assert res.count.tolist() == d["sums"][:, 0].astype(int).tolist()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,shape", CASES)
def test_sums_against_the_fp64_reference(name, shape, prec):
    d = rc.data(name, shape)
    got = packed(gpu_result_r(name, shape, prec))
    e = rc.scaled_errors(got, d["sums"], d["mags"])
    print(f"{prec} {name} {shape}: distance {e.max():.2e} (per target {np.array2string(e.max(axis=1), precision=2)}), reference's own {d['D']:.2e}, gate {d['gate']:.2e}")
    assert rc.accepts(d, got), (e.max(axis=1), d["gate"])


@pytest.mark.parametrize("name,shape", CASES)
def test_rweight_is_the_float32_of_robust_terms_on_the_calls_own_planes(name, shape):
    res, d = gpu_result_r(name, shape), rc.data(name, shape)
    want = np.full((M,) + shape, np.nan, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d["targets"]) & np.isfinite(res.warped) & np.isfinite(res.wgrad).all(axis=0) & np.isfinite(d["weights"]) & (d["weights"] > 0)
    for q in range(M):
        if not rc.SCALE[q] > 0:
            continue
        g, b = float(d["intensity"][q, 0]), float(d["intensity"][q, 1])
        for i, j in zip(*np.nonzero(ok[q])):
            r = ((g * float(res.warped[q, i, j])) + b) - float(d["targets"][q, i, j])
            om = ar.robust_terms(r, d["weights"][q, i, j], rc.SCALE[q]).om
            want[q, i, j] = np.float32(om * om)
    assert res.rweight.dtype == np.float32 and same(res.rweight, want)
    assert np.isnan(res.rweight[list(rc.UNSCORED)]).all() and np.isfinite(res.rweight).sum() == res.count.sum()
    inside = res.rweight[1][np.isfinite(res.rweight[1])]
    assert inside.min() < 0.5 and 0.0 < inside.max() <= 1.0  # scale 0.01: pixels are rejected


@pytest.mark.parametrize("prec", PRECS)
def test_a_scale_that_is_not_positive_gives_count_zero(prec):
    name, shape = "morlet3", (19, 23)
    m, d = model(name, prec), rc.data(name, shape)
    res = m.align_volume_cost_r(vc.images(), d["targets"], d["maps"], np.array([0.0, float("nan"), -1.0, -0.0, -INF, 1.0, INF]), weights=d["weights"], intensity=d["intensity"],
                                rweight=True)
    assert not packed(res)[:5].any() and (res.count[5:] > 0).all() and np.isnan(res.rweight[:5]).all()
    full = gpu_result_r(name, shape, prec)
    assert not packed(full)[list(rc.UNSCORED)].any()


def test_determinism_and_independence_of_the_sums():
    name, shape = "sine5", (47, 45)
    d = rc.data(name, shape)
    m, img, tg, maps, w, gb, sc = model(name), vc.images(), d["targets"], d["maps"], d["weights"], d["intensity"], rc.SCALE
    res = gpu_result_r(name, shape)
    again = m.align_volume_cost_r(img, tg, maps, sc, weights=w, intensity=gb, warped=True, gradient=True, rweight=True)
    assert np.array_equal(packed(again), packed(res)) and same(again.warped, res.warped) and same(again.wgrad, res.wgrad) and same(again.rweight, res.rweight)  # two runs
    for q in range(M):                                                                                                     # a target alone
        one = m.align_volume_cost_r(img, tg[q:q + 1], maps[q:q + 1], sc[q:q + 1], weights=w[q:q + 1], intensity=gb[q:q + 1], rweight=True)
        assert np.array_equal(packed(one)[0], packed(res)[q]) and same(one.rweight[0], res.rweight[q]), q
    sub = [5, 2, 2, 0, 1]                                                                                                  # any batch: rows in another order, one twice
    part = m.align_volume_cost_r(img, tg[sub], maps[sub], sc[sub], weights=w[sub], intensity=gb[sub])
    assert np.array_equal(packed(part), packed(res)[sub])
    for kw in (dict(), dict(warped=True), dict(gradient=True), dict(rweight=True)):                                        # optional outputs omitted
        part = m.align_volume_cost_r(img, tg, maps, sc, weights=w, intensity=gb, **kw)
        assert np.array_equal(packed(part), packed(res))
        assert (part.warped is None) == ("warped" not in kw) and (part.wgrad is None) == ("gradient" not in kw) and (part.rweight is None) == ("rweight" not in kw)
    # the _dev form against the host form, on one stream and on two alternating, calls back to back without a sync; sums as pairs of floats
    th, tw = shape
    d_i, d_t, d_m = m.device_array(img.shape).copy_from(img), m.device_array(tg.shape).copy_from(tg), m.device_array(maps.shape).copy_from(maps)
    d_w, d_gb, d_sc = m.device_array(w.shape).copy_from(w), m.device_array(gb.shape).copy_from(gb), f64_dev(m, sc)
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array((M, 2 * SUMS)),) + tuple(m.device_array(s) if k != 1 else None for s in ((M, th, tw), (3, M, th, tw), (M, th, tw))) for k in range(streams + 1)]
            for d_s, d_wp, d_g, d_rw in outs:
                _lib.check(m._lib.msiren_align_volume_r_dev(m._h, d_i.ptr, N, HW, HW, d_t.ptr, M, th, tw, d_m.ptr, d_w.ptr, d_gb.ptr, d_sc.ptr, d_s.ptr, d_wp.ptr if d_wp else None,
                                                            d_g.ptr if d_g else None, d_rw.ptr if d_rw else None))
            m.sync()
            for d_s, d_wp, d_g, d_rw in outs:
                assert np.array_equal(d_s.numpy().view(np.float64), packed(res)), streams
                assert d_wp is None or (same(d_wp.numpy(), res.warped) and same(d_g.numpy(), res.wgrad) and same(d_rw.numpy(), res.rweight)), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


# ---- the solve --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def targets(name, prec="fp32"):
    warped = model(name, prec).align_volume_cost(vc.images(), np.zeros((SM,) + SHAPE, np.float32), gc.truth(), warped=True).warped
    return gc.targets_of(warped, True)


def solve(m, tg, est, scale=rc.SOLVE_SCALE, rows=slice(None), groups=None, weights=None, **kw):
    kw.setdefault("iterations", IT)
    w, gb = rc.weights() if weights is None else weights, gc.start_intensity(est)
    sc = scale if np.ndim(scale) == 0 else np.asarray(scale)[rows]
    return m.align_volume_solve_group_robust(vc.images(), tg[rows], gc.planes()[rows], gc.SPACING, gc.GROUP_START if groups is None else groups, sc, weights=w[rows],
                                             intensity=None if gb is None else gb[rows], estimate_intensity=est == av.ESTIMATE, **kw)


@functools.lru_cache(maxsize=None)
def solved(prec, name, est):
    return solve(model(name, prec), targets(name, prec), est, trace=True)


def same_solve(a, b, targets_=slice(None), groups=slice(None), other_targets=slice(None), other_groups=slice(None)):
    """two SolveResultGs, bit for bit (trace aside); with rows: those targets / groups of ``a`` against those of ``b``"""
    return (all(np.array_equal(x[targets_], y[other_targets], equal_nan=True) for x, y in zip(a[:5], b[:5])) and
            all(np.array_equal(x[groups], y[other_groups], equal_nan=True) for x, y in zip(a[5:12], b[5:12])))


def opts(iterations=4, est=1, *, struct_size=None, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, spacing=gc.SPACING):
    return _lib.AlignVolumeSolveGroupOpts(C.sizeof(_lib.AlignVolumeSolveGroupOpts) if struct_size is None else struct_size, iterations, est, 0, damping, down, up, lam_min,
                                          lam_max, spacing)


@pytest.mark.parametrize("prec,name,est", ALL)
def test_the_device_loop_is_the_host_loop_bit_for_bit(prec, name, est):
    m, tg, w, res = model(name, prec), targets(name, prec), rc.weights(), solved(prec, name, est)
    assert res.trace.shape == (IT, G, 15)
    host, _ = ar.solve_on_host_r(lambda maps, gb, s: packed(m.align_volume_cost_r(vc.images(), tg, maps, s, weights=w, intensity=gb)), gc.GROUP_START, rc.SOLVE_SCALE,
                                 rigid=gc.start_rigid(), planes=gc.planes(), intensity=gc.start_intensity(est), options=gc.options(est), trace=True)
    assert same_solve(res, host), (res[:12], host[:12])
    assert np.array_equal(res.trace, host.trace)
    assert (res.accepted >= 3).all() and (res.trace[1:, :, :12] != res.trace[:1, :, :12]).any()


@pytest.mark.parametrize("prec,name,est", ALL)
def test_with_an_infinite_scale_the_solve_returns_align_volume_solve_groups_bits(prec, name, est):
    m, tg, w, gb = model(name, prec), targets(name, prec), rc.weights(), gc.start_intensity(est)
    new = solve(m, tg, est, INF, iterations=6, trace=True)
    old = m.align_volume_solve_group(vc.images(), tg, gc.planes(), gc.SPACING, gc.GROUP_START, weights=w, intensity=gb, estimate_intensity=est == av.ESTIMATE, iterations=6,
                                     trace=True)
    assert same_solve(new, old) and np.array_equal(new.trace, old.trace) and (old.accepted >= 1).all()
    assert not same_solve(solve(m, tg, est, iterations=6), old)  # (the finite scale is another objective)


@pytest.mark.parametrize("prec,name,est", ALL)
def test_convergence_on_the_gate_groups_with_the_corruption_unmasked(prec, name, est):
    res, gate, rows = solved(prec, name, est), rc.device_solve_gate(), list(rc.GATE_GROUPS)
    err = gc.errors(res, est)
    print(f"{prec} {name} intensity {est}: errors per group {np.array2string(err, precision=2)} gate {gate:.2e}; accepted {res.accepted.tolist()}, lam {res.damping.tolist()}, "
          f"flags {res.flags.tolist()}, (g, b) {res.intensity.tolist()}")
    assert (err[rows] <= gate).all(), (err, gate)
    assert (res.mean_best <= res.mean_first).all() and not res.flags.any()
    inside = [t for t in range(SM) if t != gc.OUTSIDE]
    assert (res.count[inside] == SHAPE[0] * SHAPE[1]).all() and res.count[gc.OUTSIDE] == 0  # the corrupted block counts: nothing masks it
    # the outlier map at the solution: the block is rejected, the rest is not
    rw = model(name, prec).align_volume_cost_r(vc.images(), targets(name, prec), res.maps, rc.SOLVE_SCALE, weights=rc.weights(), intensity=res.intensity, rweight=True).rweight
    block = rw[(slice(None),) + gc.wc.BLOCK][inside]
    rest = rw.copy()
    rest[(slice(None),) + gc.wc.BLOCK] = np.nan
    print(f"    rweight inside the block at most {block.max():.2e}, outside at least {np.nanmin(rest[inside]):.6f}")
    assert block.max() < 1e-5 and np.nanmin(rest[inside]) > 0.99


@pytest.mark.parametrize("est", rc.MODES)
def test_determinism_and_independence_of_the_solve(est):
    prec, name = "fp32", "morlet3"
    m, tg, res = model(name, prec), targets(name, prec), solved(prec, name, est)
    again = solve(m, tg, est, trace=True)
    assert same_solve(again, res) and np.array_equal(again.trace, res.trace)  # two runs
    assert same_solve(solve(m, tg, est), res)                                 # without the trace
    assert same_solve(solve(m, tg, est, rc.solve_scale()), res)              # the scale as an array
    for y in range(G):                                                        # a group alone
        lo, hi = gc.GROUP_START[y], gc.GROUP_START[y + 1]
        one = solve(m, tg, est, rows=slice(lo, hi), groups=[0, hi - lo], trace=True)
        assert same_solve(one, res, other_targets=slice(lo, hi), other_groups=slice(y, y + 1)), y
        assert np.array_equal(one.trace[:, 0], res.trace[:, y]), y
    # the _dev form against the host form, on one stream and on two alternating, calls back to back without a sync, with and without the optional outputs
    o = opts(IT, est)
    img, rigid, pl, w, gb = vc.images(), gc.start_rigid(), gc.planes(), rc.weights(), gc.start_intensity(est)
    d = dict(images=m.device_array(img.shape).copy_from(img), targets=m.device_array(tg.shape).copy_from(tg), planes=f64_dev(m, pl), rigid=f64_dev(m, rigid),
             weights=m.device_array(w.shape).copy_from(w), gb=None if gb is None else m.device_array(gb.shape).copy_from(gb), scale=f64_dev(m, rc.solve_scale()))
    gs = np.ascontiguousarray(gc.GROUP_START, np.int32)
    p = lambda x: None if x is None else x.ptr  # noqa: E731
    f64 = lambda x: x.numpy().view(np.float64).reshape(x.numpy().shape[:-1])  # noqa: E731
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [dict(out=m.device_array((SM, 9)), gout=m.device_array((SM, 2)), rep=m.device_array((G, 7, 2)), rout=m.device_array((G, 12, 2)) if k != 1 else None,
                         trep=m.device_array((SM, 3, 2)) if k != 1 else None, trace=m.device_array((IT, G, 15, 2)) if k != 1 else None) for k in range(streams + 1)]
            for x in outs:
                _lib.check(m._lib.msiren_align_volume_solve_group_r_dev(m._h, d["images"].ptr, N, HW, HW, d["targets"].ptr, SM, SHAPE[0], SHAPE[1], C.byref(o), gs.ctypes.data, G,
                                                                        d["planes"].ptr, d["rigid"].ptr, d["weights"].ptr, p(d["gb"]), d["scale"].ptr, x["out"].ptr, x["gout"].ptr,
                                                                        p(x["rout"]), x["rep"].ptr, p(x["trep"]), p(x["trace"])))
            m.sync()
            for x in outs:
                rep = f64(x["rep"])
                assert np.array_equal(x["out"].numpy(), res.maps) and np.array_equal(x["gout"].numpy(), res.intensity), streams
                assert np.array_equal(rep[:, [0, 1, 2, 5, 6]], np.stack([res.accepted, res.mean_first, res.mean_best, res.damping, res.flags], axis=1).astype(np.float64)), streams
                if x["rout"] is not None:
                    rout = f64(x["rout"])
                    assert np.array_equal(rout[:, :9].reshape(G, 3, 3), res.rotation) and np.array_equal(rout[:, 9:], res.shift), streams
                    assert np.array_equal(f64(x["trep"]), np.stack([res.count.astype(np.float64), res.wsum, res.cost], axis=1)), streams
                    assert np.array_equal(f64(x["trace"]), res.trace), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


def test_refusals_launch_nothing():
    shape = (19, 23)
    d = rc.data("sine5", shape)
    m, img, tg, maps, w, gb = model("sine5"), vc.images(), d["targets"], d["maps"], d["weights"], d["intensity"]
    sc = np.full(M, 0.01)
    sums, rwt = np.full((M, SUMS), -7.0), np.full((M,) + shape, -7.0, np.float32)
    stg, pl, rigid, sw, ssc = targets("sine5"), gc.planes(), gc.start_rigid(), rc.weights(), rc.solve_scale()
    out, gout, rout, rep, trep = np.full((SM, 9), -7.0, np.float32), np.full((SM, 2), -7.0, np.float32), np.full((G, 12), -7.0), np.full((G, 7), -7.0), np.full((SM, 3), -7.0)
    dimg = m.device_array(img.shape).copy_from(img)
    gs = np.ascontiguousarray(gc.GROUP_START, np.int32)
    m.sync()
    profile_on(m)
    try:
        # the cost call: images, targets, maps, scale, sums
        args = (img.ctypes.data, N, HW, HW, tg.ctypes.data, M, shape[0], shape[1], maps.ctypes.data, w.ctypes.data, gb.ctypes.data, sc.ctypes.data, sums.ctypes.data, None, None,
                rwt.ctypes.data)
        for k in (0, 4, 8, 11, 12):
            bad = list(args)
            bad[k] = None
            assert m._lib.msiren_align_volume_r(m._h, *bad) == _lib.E_INVALID and "null" in _lib.last_error(), k
            dev = [dimg.ptr, N, HW, HW, dimg.ptr, 2, 4, 4, dimg.ptr, dimg.ptr, dimg.ptr, dimg.ptr, dimg.ptr, None, None, None]
            dev[k] = None
            assert m._lib.msiren_align_volume_r_dev(m._h, *dev) == _lib.E_INVALID, k
        for k, off in ((9, 2), (10, 2), (11, 4), (13, 2), (14, 2), (15, 2)):  # misaligned device weights, intensity, scale, warped, wgrad, rweight
            dev = [dimg.ptr, N, HW, HW, dimg.ptr, 2, 4, 4, dimg.ptr, dimg.ptr, dimg.ptr, dimg.ptr, dimg.ptr, None, None, None]
            dev[k] = dimg.ptr + off
            assert m._lib.msiren_align_volume_r_dev(m._h, *dev) == _lib.E_INVALID and "aligned" in _lib.last_error(), k
        # what msiren_align_volume_w refuses: an oversize product, the weighted form's own limit, n < 2
        for mm, th, tw in ((M, 1 << 12, 1 << 12), (1 << 20, 64, 64), (-1, 4, 4)):
            assert m._lib.msiren_align_volume_r(m._h, *args[:5], mm, th, tw, *args[8:]) == _lib.E_INVALID
            assert m._lib.msiren_align_volume_r_dev(m._h, dimg.ptr, N, HW, HW, dimg.ptr, mm, th, tw, dimg.ptr, None, None, dimg.ptr, dimg.ptr, None, None, None) == _lib.E_INVALID
        assert m._lib.msiren_align_volume_r_dev(m._h, dimg.ptr, N, HW, HW, dimg.ptr, 7680, 32, 32, None, None, None, None, None, None, None, None) == _lib.E_INVALID
        assert "640 bytes per chunk" in _lib.last_error()
        assert m._lib.msiren_align_volume_r(m._h, args[0], 1, *args[2:]) == _lib.E_INVALID
        for kw in (dict(weights=w[:2]), dict(intensity=gb[:3])):
            with pytest.raises(ValueError):
                m.align_volume_cost_r(img, tg, maps, 0.01, **kw)
        for n_bad in ((M - 1,), (M, 2)):
            with pytest.raises(ValueError):
                m.align_volume_cost_r(img, tg, maps, np.full(n_bad, 0.01))
        for n_bad in ((SM + 1,), (SM, 2)):
            with pytest.raises(ValueError):
                m.align_volume_solve_group_robust(img, stg, pl, gc.SPACING, gc.GROUP_START, np.full(n_bad, 0.01))
        # nothing to do
        assert m._lib.msiren_align_volume_r(m._h, img.ctypes.data, N, HW, HW, None, 0, shape[0], shape[1], None, None, None, None, sums.ctypes.data, None, None, None) == 0
        assert m._lib.msiren_align_volume_r_dev(m._h, dimg.ptr, N, HW, HW, dimg.ptr, 2, 0, 4, dimg.ptr, None, None, None, dimg.ptr, None, None, None) == 0

        # the solve
        def host(o, ng=G, **kw):
            a = dict(images=img.ctypes.data, n=N, targets=stg.ctypes.data, m=SM, th=SHAPE[0], tw=SHAPE[1], gs=gs.ctypes.data, planes=pl.ctypes.data, rigid=rigid.ctypes.data,
                     weights=sw.ctypes.data, gb=None, scale=ssc.ctypes.data, out=out.ctypes.data, gout=gout.ctypes.data, rep=rep.ctypes.data)
            a.update(kw)
            return m._lib.msiren_align_volume_solve_group_r(m._h, a["images"], a["n"], HW, HW, a["targets"], a["m"], a["th"], a["tw"], C.byref(o) if o is not None else None, a["gs"],
                                                            ng, a["planes"], a["rigid"], a["weights"], a["gb"], a["scale"], a["out"], a["gout"], rout.ctypes.data, a["rep"],
                                                            trep.ctypes.data, None)

        two = np.array([0, 1, 2], np.int32)

        def dev(o, ng=2, **kw):
            a = dict(images=dimg.ptr, n=N, targets=dimg.ptr, m=2, th=4, tw=4, gs=two.ctypes.data, planes=dimg.ptr, rigid=dimg.ptr, weights=dimg.ptr, gb=dimg.ptr, scale=dimg.ptr,
                     out=dimg.ptr, gout=dimg.ptr, rout=dimg.ptr, rep=dimg.ptr, trep=dimg.ptr, trace=None)
            a.update(kw)
            return m._lib.msiren_align_volume_solve_group_r_dev(m._h, a["images"], a["n"], HW, HW, a["targets"], a["m"], a["th"], a["tw"], C.byref(o) if o is not None else None,
                                                                a["gs"], ng, a["planes"], a["rigid"], a["weights"], a["gb"], a["scale"], a["out"], a["gout"], a["rout"], a["rep"],
                                                                a["trep"], a["trace"])

        inf, nan = float("inf"), float("nan")
        for o in (opts(struct_size=72), opts(struct_size=0), opts(est=2), opts(iterations=0), opts(iterations=257), opts(lam_min=0.0), opts(lam_max=inf), opts(damping=nan),
                  opts(down=0.0), opts(up=0.5), opts(spacing=0.0), opts(spacing=nan), None):
            assert host(o) == _lib.E_INVALID and _lib.last_error()
            assert dev(o) == _lib.E_INVALID
        assert host(opts(struct_size=72)) == _lib.E_INVALID and "struct_size" in _lib.last_error()
        assert host(opts(), scale=None) == _lib.E_INVALID and "null" in _lib.last_error()  # a null scale is refused
        assert dev(opts(), scale=None) == _lib.E_INVALID and "scale" in _lib.last_error()
        assert dev(opts(), scale=dimg.ptr + 4) == _lib.E_INVALID and "aligned" in _lib.last_error()
        for bad_gs, ng, word in ((np.array([0, 3, 4, 6], np.int32), 0, "n_groups"), (None, G, "null"), (np.array([1, 3, 4, 6], np.int32), G, "group_start[0]"),
                                 (np.array([0, 3, 3, 6], np.int32), G, "group_start[2]"), (np.array([0, 3, 4, 5], np.int32), G, "group_start[3]")):
            assert host(opts(), ng, gs=None if bad_gs is None else bad_gs.ctypes.data) == _lib.E_INVALID and word in _lib.last_error(), word
        for key in ("rigid", "planes", "out", "gout", "rep", "images", "targets"):
            assert host(opts(), **{key: None}) == _lib.E_INVALID and "null" in _lib.last_error(), key
            assert dev(opts(), **{key: None}) == _lib.E_INVALID, key
        for key, off in (("targets", 2), ("out", 2), ("weights", 2), ("gb", 2), ("gout", 2), ("rigid", 4), ("planes", 4), ("rout", 4), ("rep", 4), ("trep", 4), ("trace", 4)):
            assert dev(opts(), **{key: dimg.ptr + off}) == _lib.E_INVALID and "aligned" in _lib.last_error(), key
        for kw in (dict(th=1 << 12, tw=1 << 12), dict(m=-1), dict(n=1)):
            assert host(opts(), **kw) == _lib.E_INVALID and dev(opts(), **kw) == _lib.E_INVALID, kw
        assert host(opts(), m=0) == 0 and host(opts(), th=0) == 0 and dev(opts(), tw=0) == 0 and dev(opts(), m=0) == 0
        m.sync()
        assert (sums == -7.0).all() and (rwt == -7.0).all() and (out == -7.0).all() and (gout == -7.0).all() and (rout == -7.0).all() and (rep == -7.0).all() and (trep == -7.0).all()
        assert np.array_equal(dimg.numpy(), img) and m.profile_kernels() == []
    finally:
        profile_off(m)
    assert np.array_equal(packed(m.align_volume_cost_r(img, tg, maps, rc.SCALE, weights=w, intensity=gb)), packed(gpu_result_r("sine5", shape)))  # the handle stays usable


@pytest.mark.parametrize("name,act", [("sine5", 0), ("morlet3", 1)])
def test_profile_counts(name, act):
    m, tg, w = model(name), targets(name), rc.weights()
    trunk = f"siren_trunk_f32_jet_ragged_kernel<256,{act}>"
    per_eval = ("align_volume_bin_kernels", trunk, "align_volume_reduce_r_kernels")
    profile_on(m)
    try:
        m.align_volume_cost_r(vc.images(), tg, gc.start_maps(), rc.SOLVE_SCALE, weights=w)
        m.sync()
        one = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
    finally:
        profile_off(m)
    assert all(one[k] == 1 for k in per_eval) and "align_volume_reduce_w_kernels" not in one and not [k for k in one if "step" in k], one
    for est in rc.MODES:
        profile_on(m)
        try:
            solve(m, tg, est, iterations=5)
            m.sync()
            got = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
        finally:
            profile_off(m)
        assert got["align_group_step_kernels"] == 5 and all(got[k] == 5 for k in per_eval), got
        assert "align_volume_reduce_w_kernels" not in got and "align_volume_step_w_kernel" not in got, got
        assert {k: v for k, v in got.items() if k not in per_eval + ("align_group_step_kernels",)} == {k: v for k, v in one.items() if k not in per_eval}, (got, one)
    profile_on(m)  # the weighted grouped solve: its step stage runs as often, on the weighted reduce
    try:
        m.align_volume_solve_group(vc.images(), tg, gc.planes(), gc.SPACING, gc.GROUP_START, weights=w, iterations=5)
        m.sync()
        old = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
    finally:
        profile_off(m)
    assert old["align_group_step_kernels"] == 5 and old["align_volume_reduce_w_kernels"] == 5 and "align_volume_reduce_r_kernels" not in old, old


def test_a_robust_call_leaves_the_other_calls_alone():
    name = "sine5"
    m, tg, img, w = model(name), targets(name), vc.images(), gc.weights()
    pts = av.map_points3(gc.truth()[1], SHAPE)

    def others():
        s = m.align_volume_solve_group(img, tg, gc.planes(), gc.SPACING, gc.GROUP_START, weights=w, iterations=3, trace=True)
        c = m.align_volume_cost_w(img, tg, gc.truth(), weights=w, intensity=gc.GB_TRUTH, warped=True, gradient=True)
        val, grad = m.resample_volume_with_gradient(img, pts)
        return tuple(s[:12]) + (s.trace, packed(c), c.warped, c.wgrad, val, grad)

    before = others()
    m.align_volume_cost_r(img, tg, gc.truth(), rc.SOLVE_SCALE, weights=rc.weights(), rweight=True)
    for est in rc.MODES:
        solve(m, tg, est, iterations=3)
    after = others()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, after))
