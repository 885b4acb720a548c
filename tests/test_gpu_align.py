"""Slices scored under affine maps against targets on the GPU: model.align_cost, i.e. msiren_align_slices* -- slice
prologue, the pixels of the target lattices placed by their slice's map in the kernel and binned by (slice, tile), the jet ragged trunk,
blend and the 29 fp64 sums per slice.  Stack, models, lattices, maps, targets and reference: tests/align_cases.py.

The planes have to be the bits of model.resample_with_gradient at align.map_points; the sums are compared with numpy on the call's own
planes inside the worst-case bound of an fp64 sum in any order (N 2^-52 sum|term|), and with the fp64 reference inside section 5.7's gate
on the sums (4 x the reference's own perturbed-fp32 distance, capped at 1e-4 of sum|term|); the distances measured on the MI355X are in
LAB_NOTES.md section 22.
"""
import functools

import numpy as np
import pytest

import align_cases as ac
import align_reference as ar
import volume_cases as vc
from mri_inr_amd import ModulatedSiren, _lib, align, synthetic as syn

pytestmark = pytest.mark.gpu

N, HW = ac.N, ac.HW
CASES = [(m, s) for m in ac.MODELS for s in ac.LATTICES]


def build(sd, *, H=256, L=5, act="sine", prec="fp32", **kw):
    m = ModulatedSiren(dim_in=2, dim_hidden=H, dim_out=1, num_layers=L, latent_dim=256, w0=1.0, w0_initial=30.0, use_bias=True,
                       dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None, outer_patch_size=vc.O, inner_patch_size=vc.I,
                       siren_patch_size=vc.S, device="cuda", activation=act, precision=prec, **kw)
    m.load_state_dict(sd, strict=True)
    m.to("cuda")
    m.eval()
    return m


@functools.lru_cache(maxsize=None)
def model(name="sine5", prec="fp32"):
    return build(ac.state_dict(name), L=ac.MODELS[name]["L"], act=ac.MODELS[name]["act"], prec=prec)


@functools.lru_cache(maxsize=None)
def gpu_result(name, shape, prec="fp32"):
    return model(name, prec).align_cost(vc.images(), ac.targets(shape), ac.maps(shape), warped=True, gradient=True)


def packed(res):
    """an AlignResult back as (n, 29)"""
    iu = np.triu_indices(6)
    return np.concatenate([res.count[:, None].astype(np.float64), res.cost[:, None], res.grad, res.jtj[:, iu[0], iu[1]]], axis=1)


def same(a, b):
    """np.array_equal with NaNs in the same places"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def same_result(a, b):
    return np.array_equal(packed(a), packed(b))


def profile_on(m):
    _lib.check(m._lib.msiren_profile_enable(m._h, 1))


def profile_off(m):
    _lib.check(m._lib.msiren_profile_enable(m._h, 0))


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name,shape", CASES)
def test_planes_are_the_bits_of_resample(name, shape, prec):
    res = gpu_result(name, shape, prec)
    m, maps = model(name, prec), ac.maps(shape)
    assert res.warped.shape == (N,) + shape and res.wgrad.shape == (2, N) + shape and res.warped.dtype == np.float32
    for s in range(N):
        val, grad = m.resample_with_gradient(vc.images(), align.map_points(maps[s], shape))  # (every slice at slice s's points; row s)
        assert same(res.warped[s].ravel(), val[s]) and same(res.wgrad[:, s].reshape(2, -1), grad[:, s]), (prec, s)
    assert np.isnan(res.warped[2]).any() and np.isfinite(res.warped[2]).any() and not res.warped[3].any() and np.isfinite(res.warped[[0, 1, 3]]).sum() > 0


@pytest.mark.parametrize("name,shape", CASES)
def test_sums_against_the_calls_own_planes(name, shape):
    res = gpu_result(name, shape)
    got, targets = packed(res), ac.targets(shape)
    pixels = shape[0] * shape[1]
    for s in range(N):
        want, mags = ar.sums_of_planes(res.warped[s], res.wgrad[0, s], res.wgrad[1, s], targets[s], shape)
        bound = pixels * 2.0 ** -52 * mags  # the worst case of an fp64 sum of N terms in any order (and of the terms' own roundings)
        err = np.abs(got[s] - want)
        print(f"{name} {shape} slice {s}: count {int(got[s, 0])}, largest error / bound {np.max(err[1:] / np.maximum(bound[1:], 1e-300)):.3f}")
        assert got[s, 0] == want[0], s
        assert (err[1:] <= bound[1:]).all(), (s, err, bound)
    assert res.count.tolist() == ac.data(name, shape)["sums"][:, 0].astype(int).tolist()


@pytest.mark.parametrize("name,shape", CASES)
def test_sums_against_the_fp64_reference(name, shape):
    d = ac.data(name, shape)
    got = packed(gpu_result(name, shape))
    e = ac.scaled_errors(got, d["sums"], d["mags"])
    print(f"{name} {shape}: distance {e.max():.2e} (per slice {np.array2string(e.max(axis=1), precision=2)}), reference's own {d['D']:.2e}, gate {d['gate']:.2e}")
    assert ac.accepts(d, got), (e.max(axis=1), d["gate"])


def test_determinism_and_independence():
    name, shape = "sine5", (47, 45)
    m, img, tg, maps = model(name), vc.images(), ac.targets(shape), ac.maps(shape)
    res = gpu_result(name, shape)
    again = m.align_cost(img, tg, maps, warped=True, gradient=True)
    assert same_result(again, res) and same(again.warped, res.warped) and same(again.wgrad, res.wgrad)  # two runs
    for s in range(N):                                                                                   # a slice alone
        one = m.align_cost(img[s:s + 1], tg[s:s + 1], maps[s:s + 1], warped=True)
        assert np.array_equal(packed(one)[0], packed(res)[s]) and same(one.warped[0], res.warped[s]), s
    for kw in (dict(), dict(warped=True), dict(gradient=True)):                                          # optional outputs omitted
        part = m.align_cost(img, tg, maps, **kw)
        assert same_result(part, res) and (part.warped is None) == ("warped" not in kw) and (part.wgrad is None) == ("gradient" not in kw)
    # the _dev form, on one stream and on two alternating, calls back to back without a sync; sums as pairs of floats on the device
    th, tw = shape
    d_i, d_t, d_m = m.device_array(img.shape).copy_from(img), m.device_array(tg.shape).copy_from(tg), m.device_array(maps.shape).copy_from(maps)
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array((N, 2 * align.SUMS)), m.device_array((N, th, tw)) if k != 1 else None, m.device_array((2, N, th, tw)) if k != 1 else None)
                    for k in range(streams + 1)]
            for d_s, d_w, d_g in outs:
                _lib.check(m._lib.msiren_align_slices_dev(m._h, d_i.ptr, N, HW, HW, d_t.ptr, th, tw, d_m.ptr, d_s.ptr, d_w.ptr if d_w else None,
                                                          d_g.ptr if d_g else None))
            m.sync()
            for d_s, d_w, d_g in outs:
                assert np.array_equal(d_s.numpy().view(np.float64), packed(res)), streams
                assert d_w is None or (same(d_w.numpy(), res.warped) and same(d_g.numpy(), res.wgrad)), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


def test_zero_residual():
    name, shape = "morlet3", (47, 45)
    m, maps = model(name), ac.maps(shape)
    first = gpu_result(name, shape)
    zero = m.align_cost(vc.images(), first.warped, maps)  # (NaN where the first call's pixel was uncovered: the mask)
    assert not zero.cost.any() and not zero.grad.any()
    valid = np.isfinite(first.warped) & np.isfinite(first.wgrad).all(axis=0)
    assert zero.count.tolist() == valid.reshape(N, -1).sum(axis=1).tolist()
    nanfree = [s for s in range(N) if not np.isnan(ac.targets(shape)[s]).any()]  # the first call's target of slice 0 masks 15 pixels more
    assert nanfree == [1, 2, 3] and np.array_equal(zero.count[nanfree], first.count[nanfree]) and np.array_equal(zero.jtj[nanfree], first.jtj[nanfree])
    tg = ac.targets(shape)
    masked = np.where(np.isnan(tg), np.nan, first.warped)  # with the first call's mask: count and jtj of every slice are its bits
    zero = m.align_cost(vc.images(), masked, maps)
    assert not zero.cost.any() and not zero.grad.any() and np.array_equal(zero.count, first.count) and np.array_equal(zero.jtj, first.jtj)
    assert first.cost.all() and first.jtj[:3].any()


def test_refusals_launch_nothing():
    shape = (19, 23)
    img, tg, maps = vc.images(), ac.targets(shape), ac.maps(shape)
    sums = np.full((N, align.SUMS), -7.0)
    wide = build(syn.make_state_dict(seed=3, dim_hidden=512, num_layers=3), H=512, L=3)
    res = build(syn.make_state_dict(seed=7, num_layers=2), L=2, residual=True)
    for m, word, H, L in ((wide, "256", 512, 3), (res, "residual", 256, 2)):
        profile_on(m)
        try:
            with pytest.raises(ValueError, match=word):
                m.align_cost(img, tg, maps)
            d = m.device_array(img.shape).copy_from(img)
            assert m._lib.msiren_align_slices_dev(m._h, d.ptr, N, HW, HW, d.ptr, 4, 4, d.ptr, d.ptr, None, None) == _lib.E_INVALID
            m.sync()
            assert m.profile_kernels() == []
            assert m.sample_mods(syn.make_mods(2, L, 2, H), align.map_points(maps[0], (2, 5)) / 8).shape == (2, 10)  # the handle stays usable
        finally:
            profile_off(m)
    m = model()
    profile_on(m)
    try:
        d = m.device_array(img.shape).copy_from(img)
        m.sync()
        args = (img.ctypes.data, N, HW, HW, tg.ctypes.data, shape[0], shape[1], maps.ctypes.data, sums.ctypes.data, None, None)
        for k in (0, 4, 7, 8):  # images, targets, maps, sums
            bad = list(args)
            bad[k] = None
            assert m._lib.msiren_align_slices(m._h, *bad) == _lib.E_INVALID and "null" in _lib.last_error()
            dev = [d.ptr, N, HW, HW, d.ptr, 4, 4, d.ptr, d.ptr, None, None]
            dev[k] = None
            assert m._lib.msiren_align_slices_dev(m._h, *dev) == _lib.E_INVALID
        # an oversize product: 20 n th tw K >= 2^30
        for n, th, tw in ((N, 1 << 12, 1 << 12), (1 << 20, 64, 64), (N, 1 << 30, 1 << 30)):
            assert m._lib.msiren_align_slices(m._h, img.ctypes.data, n, HW, HW, tg.ctypes.data, th, tw, maps.ctypes.data, sums.ctypes.data, None, None) == _lib.E_INVALID
            assert "too many pixels" in _lib.last_error() and "20 n th tw K" in _lib.last_error()
            assert m._lib.msiren_align_slices_dev(m._h, d.ptr, n, HW, HW, d.ptr, th, tw, d.ptr, d.ptr, None, None) == _lib.E_INVALID
        assert m._lib.msiren_align_slices(m._h, *args[:1], 1 << 25, *args[2:]) == _lib.E_INVALID
        assert m._lib.msiren_align_slices(m._h, *args[:1], -1, *args[2:]) == _lib.E_INVALID
        for bad_tg, bad_maps in ((tg[:2], maps), (tg, maps[:, :5]), (tg[0], maps)):
            with pytest.raises(ValueError):
                m.align_cost(img, bad_tg, bad_maps)
        # nothing to do: 0 is returned, nothing written
        assert m._lib.msiren_align_slices(m._h, None, 0, HW, HW, None, shape[0], shape[1], None, sums.ctypes.data, None, None) == 0
        assert m._lib.msiren_align_slices(m._h, *args[:5], 0, shape[1], *args[7:]) == 0
        assert m._lib.msiren_align_slices(m._h, *args[:6], 0, *args[7:]) == 0
        assert m._lib.msiren_align_slices_dev(m._h, d.ptr, N, HW, HW, d.ptr, 0, 4, d.ptr, d.ptr, None, None) == 0
        empty = m.align_cost(img[:0], tg[:0], maps[:0], warped=True)
        assert empty.count.shape == (0,) and empty.jtj.shape == (0, 6, 6) and empty.warped.shape == (0,) + shape
        m.sync()
        assert (sums == -7.0).all() and np.array_equal(d.numpy(), img) and m.profile_kernels() == []
    finally:
        profile_off(m)
    assert same_result(m.align_cost(img, tg, maps), gpu_result("sine5", shape))  # the handle stays usable


@pytest.mark.parametrize("name,act", [("sine5", 0), ("morlet3", 1)])
def test_profile_names_the_steps(name, act):
    m, shape = model(name), (19, 23)
    profile_on(m)
    try:
        m.align_cost(vc.images(), ac.targets(shape), ac.maps(shape))
        names = [e["kernel"] for e in m.profile_kernels()]
        assert names.count("align_bin_kernels") == 1 and names.count("align_reduce_kernels") == 1, names
        assert f"siren_trunk_f32_jet_ragged_kernel<256,{act}>" in names, names
        assert not [k for k in names if "resample" in k], names
        assert len([k for k in names if "align" in k or "ragged" in k]) == 3, names
    finally:
        profile_off(m)
