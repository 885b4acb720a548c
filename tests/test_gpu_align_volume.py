"""Target slices scored against the stack read as a volume on the GPU: model.align_volume_cost, i.e. msiren_align_volume*
-- slice prologue, the pixels of the m target lattices placed by their target's 3 x 3 map in the kernel and binned by (slice, tile) with two slices
each, the jet ragged trunk, blend across tiles and the pair, and the 56 fp64 sums per target.  Stack, models, lattices, maps, targets and
reference: tests/align_volume_cases.py.

The planes have to be the bits of model.resample_volume_with_gradient at align_volume.map_points3; with flat Z rows the shared entries are the
bits of model.align_cost; the sums are compared with numpy on the call's own planes inside the worst-case bound of an fp64 sum in any order
(N 2^-52 sum|term|), and with the fp64 reference inside the gate of the cases file (4 x the reference's own perturbed-fp32 distance, capped at
1e-4 of sum|term|); the distances measured on the MI355X are in LAB_NOTES.md section 25.
"""
import functools

import numpy as np
import pytest

import align_cases as ac
import align_volume_cases as avc
import align_volume_reference as avr
import volume_cases as vc
from mri_inr_amd import _lib, align_volume as av, synthetic as syn
from test_gpu_align import build, model, packed as packed2, profile_off, profile_on, same

pytestmark = pytest.mark.gpu

N, M, HW = avc.N, avc.M, avc.HW
CASES = [(m, s) for m in avc.MODELS for s in avc.LATTICES]
SUMS = av.SUMS_V


@functools.lru_cache(maxsize=None)
def gpu_result(name, shape, prec="fp32"):
    return model(name, prec).align_volume_cost(vc.images(), avc.targets(shape), avc.maps(shape), warped=True, gradient=True)


def packed(res):
    """an AlignResultV back as (m, 56)"""
    iu = np.triu_indices(9)
    return np.concatenate([res.count[:, None].astype(np.float64), res.cost[:, None], res.grad, res.jtj[:, iu[0], iu[1]]], axis=1)


def same_result(a, b):
    return np.array_equal(packed(a), packed(b))


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name,shape", CASES)
def test_planes_are_the_bits_of_resample_volume(name, shape, prec):
    res = gpu_result(name, shape, prec)
    m, maps = model(name, prec), avc.maps(shape)
    assert res.warped.shape == (M,) + shape and res.wgrad.shape == (3, M) + shape and res.warped.dtype == np.float32
    for q in range(M):
        val, grad = m.resample_volume_with_gradient(vc.images(), av.map_points3(maps[q], shape))
        assert same(res.warped[q].ravel(), val) and same(res.wgrad[:, q].reshape(3, -1), grad), (prec, q)
    assert np.isnan(res.warped[3]).any() and np.isfinite(res.warped[3]).any() and np.isnan(res.warped[5]).any() and np.isfinite(res.warped[[0, 1, 4, 6]]).all()
    z3 = av.map_points3(maps[3], shape)[:, 0]
    assert np.isnan(res.wgrad[:, 3].reshape(3, -1)[:, z3 < 0]).all() and np.isnan(res.warped[3].ravel()[z3 < 0]).all()  # an invalid Z: NaN in every plane


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name,shape", CASES)
def test_flat_z_rows_give_the_bits_of_the_2d_call(name, shape, prec):
    """m = n targets, target s on slice s (Z rows (0, 0, s)): count, cost, dcost[3:9] and the in-plane block of jtj are align_cost's of slice s under
    the in-plane six -- also for s = n - 1, where the pair is (n - 2, n - 1) with f' = 1"""
    m, maps2, tg = model(name, prec), ac.maps(shape), ac.targets(shape)
    maps3 = np.zeros((N, 9), np.float32)
    maps3[:, 2] = np.arange(N)
    maps3[:, 3:] = maps2
    two = m.align_cost(vc.images(), tg, maps2, warped=True, gradient=True)
    three = m.align_volume_cost(vc.images(), tg, maps3, warped=True, gradient=True)
    assert np.array_equal(three.count, two.count) and np.array_equal(three.cost, two.cost) and np.array_equal(three.grad[:, 3:], two.grad)
    assert np.array_equal(three.jtj[:, 3:, 3:], two.jtj)
    assert same(three.warped, two.warped) and same(three.wgrad[1:], two.wgrad)
    assert two.count[N - 1] == shape[0] * shape[1] and three.jtj[:3, :3, :3].any()


@pytest.mark.parametrize("name,shape", CASES)
def test_sums_against_the_calls_own_planes(name, shape):
    res = gpu_result(name, shape)
    got, targets = packed(res), avc.targets(shape)
    pixels = shape[0] * shape[1]
    for q in range(M):
        want, mags = avr.sums_of_planes(res.warped[q], res.wgrad[0, q], res.wgrad[1, q], res.wgrad[2, q], targets[q], shape)
        bound = pixels * 2.0 ** -52 * mags  # the worst case of an fp64 sum of N terms in any order (and of the terms' own roundings)
        err = np.abs(got[q] - want)
        print(f"{name} {shape} target {q}: count {int(got[q, 0])}, largest error / bound {np.max(err[1:] / np.maximum(bound[1:], 1e-300)):.3f}")
        assert got[q, 0] == want[0], q
        assert (err[1:] <= bound[1:]).all(), (q, err, bound)
    assert res.count.tolist() == avc.data(name, shape)["sums"][:, 0].astype(int).tolist()


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name,shape", CASES)
def test_sums_against_the_fp64_reference(name, shape, prec):
    d = avc.data(name, shape)
    got = packed(gpu_result(name, shape, prec))
    e = avc.scaled_errors(got, d["sums"], d["mags"])
    print(f"{prec} {name} {shape}: distance {e.max():.2e} (per target {np.array2string(e.max(axis=1), precision=2)}), reference's own {d['D']:.2e}, gate {d['gate']:.2e}")
    assert avc.accepts(d, got), (e.max(axis=1), d["gate"])


def test_determinism_and_independence():
    name, shape = "sine5", (47, 45)
    m, img, tg, maps = model(name), vc.images(), avc.targets(shape), avc.maps(shape)
    res = gpu_result(name, shape)
    again = m.align_volume_cost(img, tg, maps, warped=True, gradient=True)
    assert same_result(again, res) and same(again.warped, res.warped) and same(again.wgrad, res.wgrad)  # two runs
    for q in range(M):                                                                                   # a target alone
        one = m.align_volume_cost(img, tg[q:q + 1], maps[q:q + 1], warped=True)
        assert np.array_equal(packed(one)[0], packed(res)[q]) and same(one.warped[0], res.warped[q]), q
    sub = [5, 2, 2, 0]                                                                                   # any batch: rows in another order, one twice
    part = m.align_volume_cost(img, tg[sub], maps[sub])
    assert np.array_equal(packed(part), packed(res)[sub])
    for kw in (dict(), dict(warped=True), dict(gradient=True)):                                          # optional outputs omitted
        part = m.align_volume_cost(img, tg, maps, **kw)
        assert same_result(part, res) and (part.warped is None) == ("warped" not in kw) and (part.wgrad is None) == ("gradient" not in kw)
    # the _dev form, on one stream and on two alternating, calls back to back without a sync; sums as pairs of floats on the device
    th, tw = shape
    d_i, d_t, d_m = m.device_array(img.shape).copy_from(img), m.device_array(tg.shape).copy_from(tg), m.device_array(maps.shape).copy_from(maps)
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array((M, 2 * SUMS)), m.device_array((M, th, tw)) if k != 1 else None, m.device_array((3, M, th, tw)) if k != 1 else None)
                    for k in range(streams + 1)]
            for d_s, d_w, d_g in outs:
                _lib.check(m._lib.msiren_align_volume_dev(m._h, d_i.ptr, N, HW, HW, d_t.ptr, M, th, tw, d_m.ptr, d_s.ptr, d_w.ptr if d_w else None,
                                                          d_g.ptr if d_g else None))
            m.sync()
            for d_s, d_w, d_g in outs:
                assert np.array_equal(d_s.numpy().view(np.float64), packed(res)), streams
                assert d_w is None or (same(d_w.numpy(), res.warped) and same(d_g.numpy(), res.wgrad)), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


def test_zero_residual():
    name, shape = "morlet3", (47, 45)
    m, maps = model(name), avc.maps(shape)
    first = gpu_result(name, shape)
    zero = m.align_volume_cost(vc.images(), first.warped, maps)  # (NaN where the first call's pixel was invalid: the mask)
    assert not zero.cost.any() and not zero.grad.any()
    valid = np.isfinite(first.warped) & np.isfinite(first.wgrad).all(axis=0)
    assert zero.count.tolist() == valid.reshape(M, -1).sum(axis=1).tolist()
    masked = np.where(np.isnan(avc.targets(shape)), np.nan, first.warped)  # with the first call's mask: count and jtj of every target are its bits
    zero = m.align_volume_cost(vc.images(), masked, maps)
    assert not zero.cost.any() and not zero.grad.any() and np.array_equal(zero.count, first.count) and np.array_equal(zero.jtj, first.jtj)
    assert first.cost.all() and first.jtj.any(axis=(1, 2)).all()


def test_refusals_launch_nothing():
    shape = (19, 23)
    img, tg, maps = vc.images(), avc.targets(shape), avc.maps(shape)
    sums = np.full((M, SUMS), -7.0)
    wide = build(syn.make_state_dict(seed=3, dim_hidden=512, num_layers=3), H=512, L=3)
    res = build(syn.make_state_dict(seed=7, num_layers=2), L=2, residual=True)
    for m, word in ((wide, "256"), (res, "residual")):
        profile_on(m)
        try:
            with pytest.raises(ValueError, match=word):
                m.align_volume_cost(img, tg, maps)
            d = m.device_array(img.shape).copy_from(img)
            assert m._lib.msiren_align_volume_dev(m._h, d.ptr, N, HW, HW, d.ptr, 2, 4, 4, d.ptr, d.ptr, None, None) == _lib.E_INVALID
            m.sync()
            assert m.profile_kernels() == []
        finally:
            profile_off(m)
    m = model()
    profile_on(m)
    try:
        d = m.device_array(img.shape).copy_from(img)
        m.sync()
        args = (img.ctypes.data, N, HW, HW, tg.ctypes.data, M, shape[0], shape[1], maps.ctypes.data, sums.ctypes.data, None, None)
        for k in (0, 4, 8, 9):  # images, targets, maps, sums
            bad = list(args)
            bad[k] = None
            assert m._lib.msiren_align_volume(m._h, *bad) == _lib.E_INVALID and "null" in _lib.last_error()
            dev = [d.ptr, N, HW, HW, d.ptr, 2, 4, 4, d.ptr, d.ptr, None, None]
            dev[k] = None
            assert m._lib.msiren_align_volume_dev(m._h, *dev) == _lib.E_INVALID
        # an oversize product: 32 m th tw K + 8 m th tw >= 2^30, or m th tw >= 2^28
        for mm, th, tw in ((M, 1 << 12, 1 << 12), (1 << 20, 64, 64), (M, 1 << 30, 1 << 30), (1 << 40, 1 << 20, 1 << 20)):
            assert m._lib.msiren_align_volume(m._h, img.ctypes.data, N, HW, HW, tg.ctypes.data, mm, th, tw, maps.ctypes.data, sums.ctypes.data, None, None) == _lib.E_INVALID
            assert "too many pixels" in _lib.last_error() and "32 m th tw K" in _lib.last_error()
            assert m._lib.msiren_align_volume_dev(m._h, d.ptr, N, HW, HW, d.ptr, mm, th, tw, d.ptr, d.ptr, None, None) == _lib.E_INVALID
        assert m._lib.msiren_align_volume(m._h, *args[:1], 1 << 25, *args[2:]) == _lib.E_INVALID and "too many slices" in _lib.last_error()
        for n in (1, 0, -1):  # a volume needs two slices
            assert m._lib.msiren_align_volume(m._h, *args[:1], n, *args[2:]) == _lib.E_INVALID
            assert m._lib.msiren_align_volume_dev(m._h, d.ptr, n, HW, HW, d.ptr, 2, 4, 4, d.ptr, d.ptr, None, None) == _lib.E_INVALID
        assert m._lib.msiren_align_volume(m._h, *args[:5], -1, *args[6:]) == _lib.E_INVALID
        assert m._lib.msiren_align_volume_dev(m._h, d.ptr, N, HW, HW, d.ptr + 2, 2, 4, 4, d.ptr, d.ptr, None, None) == _lib.E_INVALID and "aligned" in _lib.last_error()
        for bad_tg, bad_maps in ((tg, maps[:2]), (tg, maps[:, :6]), (tg[0], maps)):
            with pytest.raises(ValueError):
                m.align_volume_cost(img, bad_tg, bad_maps)
        with pytest.raises(ValueError):
            m.align_volume_cost(img[:1], tg, maps)
        # nothing to do: 0 is returned, nothing written
        assert m._lib.msiren_align_volume(m._h, img.ctypes.data, N, HW, HW, None, 0, shape[0], shape[1], None, sums.ctypes.data, None, None) == 0
        assert m._lib.msiren_align_volume(m._h, *args[:6], 0, shape[1], *args[8:]) == 0
        assert m._lib.msiren_align_volume(m._h, *args[:7], 0, *args[8:]) == 0
        assert m._lib.msiren_align_volume_dev(m._h, d.ptr, N, HW, HW, d.ptr, 2, 0, 4, d.ptr, d.ptr, None, None) == 0
        empty = m.align_volume_cost(img, tg[:0], maps[:0], warped=True)
        assert empty.count.shape == (0,) and empty.jtj.shape == (0, 9, 9) and empty.warped.shape == (0,) + shape
        m.sync()
        assert (sums == -7.0).all() and np.array_equal(d.numpy(), img) and m.profile_kernels() == []
    finally:
        profile_off(m)
    assert same_result(m.align_volume_cost(img, tg, maps), gpu_result("sine5", shape))  # the handle stays usable


@pytest.mark.parametrize("name,act", [("sine5", 0), ("morlet3", 1)])
def test_profile_names_the_steps(name, act):
    m, shape = model(name), (19, 23)
    profile_on(m)
    try:
        m.align_volume_cost(vc.images(), avc.targets(shape), avc.maps(shape))
        names = [e["kernel"] for e in m.profile_kernels()]
        assert names.count("align_volume_bin_kernels") == 1 and names.count("align_volume_reduce_kernels") == 1, names
        assert f"siren_trunk_f32_jet_ragged_kernel<256,{act}>" in names, names
        assert not [k for k in names if "resample" in k or k in ("align_bin_kernels", "align_reduce_kernels")], names
        assert len([k for k in names if "align" in k or "ragged" in k]) == 3, names
    finally:
        profile_off(m)


def test_the_other_calls_return_the_same_bits_before_and_after():
    name, shape = "sine5", (19, 23)
    m, img = model(name), vc.images()
    pts = av.map_points3(avc.maps(shape)[2], shape)

    def others():
        two = m.align_cost(img, ac.targets(shape), ac.maps(shape), warped=True, gradient=True)
        val, grad = m.resample_volume_with_gradient(img, pts)
        return packed2(two), two.warped, two.wgrad, val, grad

    before = others()
    m.align_volume_cost(img, avc.targets(shape), avc.maps(shape), warped=True, gradient=True)
    after = others()
    assert all(same(x, y) for x, y in zip(before, after))
