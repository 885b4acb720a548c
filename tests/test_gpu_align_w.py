"""Weighted, gain/bias-compensated slice scoring on the GPU: model.align_cost_w, i.e. msiren_align_slices_w* --
section 5.10's pipeline with the 47-sum reduce.  Stack, models, lattices, maps, targets: tests/align_cases.py; weights, intensities,
reference and gate: tests/align_w_cases.py.

Without weights and intensity the shared entries have to be the bits of model.align_cost; weights in {0, 1} those of NaN-masked targets; a
weight halved scales exactly.  The sums are compared with numpy on the call's own planes inside the worst-case bound of an fp64 sum in any
order (N 2^-52 sum|term|), and with the fp64 reference inside the gate (4 x the reference's own perturbed-fp32 distance, capped at 1e-4 of
sum|term|); the distances measured on the MI355X are in LAB_NOTES.md section 24.
"""
import functools

import numpy as np
import pytest

import align_cases as ac
import align_w_cases as wc
import align_w_reference as awr
import volume_cases as vc
from mri_inr_amd import _lib, align, synthetic as syn
from test_gpu_align import build, gpu_result, model, packed as packed29, profile_off, profile_on, same

pytestmark = pytest.mark.gpu

N, HW = ac.N, ac.HW
CASES = [(m, s) for m in ac.MODELS for s in ac.LATTICES]
PRECS = ["fp32", "f16x3"]
packed = wc.packed


@functools.lru_cache(maxsize=None)
def gpu_result_w(name, shape, prec="fp32"):
    return model(name, prec).align_cost_w(vc.images(), ac.targets(shape), ac.maps(shape), weights=wc.weights(shape), intensity=wc.INTENSITY, warped=True, gradient=True)


def shared(res):
    """the entries an AlignResultW shares with an AlignResult, as (n, 29)"""
    return packed(res)[:, awr.SHARED]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,shape", CASES)
def test_without_weights_and_intensity_the_shared_entries_are_align_costs_bits(name, shape, prec):
    old = gpu_result(name, shape, prec)
    new = model(name, prec).align_cost_w(vc.images(), ac.targets(shape), ac.maps(shape), warped=True, gradient=True)
    assert np.array_equal(new.count, old.count) and np.array_equal(new.cost, old.cost) and np.array_equal(new.grad[:, :6], old.grad)
    assert np.array_equal(new.jtj[:, :6, :6], old.jtj) and same(new.warped, old.warped) and same(new.wgrad, old.wgrad)
    assert np.array_equal(shared(new), packed29(old)) and np.array_equal(new.wsum, new.count.astype(np.float64))
    assert np.array_equal(new.jtj[:, 7, 7], new.wsum) and new.grad.shape == (N, 8) and new.jtj.shape == (N, 8, 8)
    ones = model(name, prec).align_cost_w(vc.images(), ac.targets(shape), ac.maps(shape), weights=np.ones((N,) + shape, np.float32),
                                          intensity=np.tile(np.array([1.0, 0.0], np.float32), (N, 1)))
    assert np.array_equal(packed(ones), packed(new))  # the defaults are w = 1, (g, b) = (1, 0)
    # warped / wgrad stay the planes before gain and bias
    got = gpu_result_w(name, shape, prec)
    assert same(got.warped, old.warped) and same(got.wgrad, old.wgrad)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,shape", CASES)
def test_mask_and_scale_identities(name, shape, prec):
    m, img, tg, maps = model(name, prec), vc.images(), ac.targets(shape), ac.maps(shape)
    keep = (wc.weights(shape) > 0.5).astype(np.float32)
    assert 0 < keep.sum() < keep.size
    masked = m.align_cost(img, np.where(keep > 0, tg, np.nan).astype(np.float32), maps)
    binary = m.align_cost_w(img, tg, maps, weights=keep)
    assert np.array_equal(shared(binary), packed29(masked)) and np.array_equal(binary.wsum, binary.count.astype(np.float64))
    full = gpu_result_w(name, shape, prec)
    half = m.align_cost_w(img, tg, maps, weights=0.5 * wc.weights(shape), intensity=wc.INTENSITY)
    assert np.array_equal(half.count, full.count) and np.array_equal(packed(half)[:, 1:], 0.5 * packed(full)[:, 1:])
    w = wc.weights(shape)
    bad = w.copy()
    zero = w == 0
    assert zero.sum() >= 4
    bad[zero] = np.resize(np.array([-1.0, np.nan, np.inf, -np.inf, -0.0], np.float32), int(zero.sum()))
    extra = np.zeros_like(zero)
    extra[0, 1, 1:5] = True
    bad[extra], w[extra] = np.array([-2.5, np.nan, np.inf, -np.inf], np.float32), 0.0
    assert np.array_equal(packed(m.align_cost_w(img, tg, maps, weights=bad, intensity=wc.INTENSITY)), packed(m.align_cost_w(img, tg, maps, weights=w, intensity=wc.INTENSITY)))


@pytest.mark.parametrize("name,shape", CASES)
def test_sums_against_the_calls_own_planes(name, shape):
    res = gpu_result_w(name, shape)
    got, targets, w = packed(res), ac.targets(shape), wc.weights(shape)
    pixels = shape[0] * shape[1]
    for s in range(N):
        want, mags = awr.sums_of_planes(res.warped[s], res.wgrad[0, s], res.wgrad[1, s], targets[s], w[s], wc.INTENSITY[s], shape)
        bound = pixels * 2.0 ** -52 * mags  # the worst case of an fp64 sum of N terms in any order (and of the terms' own roundings)
        err = np.abs(got[s] - want)
        print(f"{name} {shape} slice {s}: count {int(got[s, 0])}, largest error / bound {np.max(err[1:] / np.maximum(bound[1:], 1e-300)):.3f}")
        assert got[s, 0] == want[0], s
        assert (err[1:] <= bound[1:]).all(), (s, err, bound)
    assert res.count.tolist() == wc.data(name, shape)["sums"][:, 0].astype(int).tolist()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,shape", CASES)
def test_sums_against_the_fp64_reference(name, shape, prec):
    d = wc.data(name, shape)
    got = packed(gpu_result_w(name, shape, prec))
    e = ac.scaled_errors(got, d["sums"], d["mags"])
    print(f"{prec} {name} {shape}: distance {e.max():.2e} (per slice {np.array2string(e.max(axis=1), precision=2)}), reference's own {d['D']:.2e}, gate {d['gate']:.2e}")
    assert wc.accepts(d, got), (e.max(axis=1), d["gate"])


def test_determinism_and_independence():
    name, shape = "sine5", (47, 45)
    m, img, tg, maps, w, gb = model(name), vc.images(), ac.targets(shape), ac.maps(shape), wc.weights(shape), wc.INTENSITY
    res = gpu_result_w(name, shape)
    again = m.align_cost_w(img, tg, maps, weights=w, intensity=gb, warped=True, gradient=True)
    assert np.array_equal(packed(again), packed(res)) and same(again.warped, res.warped) and same(again.wgrad, res.wgrad)  # two runs
    for s in range(N):                                                                                                     # a slice alone
        one = m.align_cost_w(img[s:s + 1], tg[s:s + 1], maps[s:s + 1], weights=w[s:s + 1], intensity=gb[s:s + 1], warped=True)
        assert np.array_equal(packed(one)[0], packed(res)[s]) and same(one.warped[0], res.warped[s]), s
    for kw in (dict(), dict(warped=True), dict(gradient=True)):                                                            # optional outputs omitted
        part = m.align_cost_w(img, tg, maps, weights=w, intensity=gb, **kw)
        assert np.array_equal(packed(part), packed(res)) and (part.warped is None) == ("warped" not in kw) and (part.wgrad is None) == ("gradient" not in kw)
    # the _dev form, on one stream and on two alternating, calls back to back without a sync; sums as pairs of floats on the device
    th, tw = shape
    d_i, d_t, d_m = m.device_array(img.shape).copy_from(img), m.device_array(tg.shape).copy_from(tg), m.device_array(maps.shape).copy_from(maps)
    d_w, d_gb = m.device_array(w.shape).copy_from(w), m.device_array(gb.shape).copy_from(gb)
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array((N, 2 * align.SUMS_W)), m.device_array((N, th, tw)) if k != 1 else None, m.device_array((2, N, th, tw)) if k != 1 else None)
                    for k in range(streams + 1)]
            for d_s, d_wp, d_g in outs:
                _lib.check(m._lib.msiren_align_slices_w_dev(m._h, d_i.ptr, N, HW, HW, d_t.ptr, th, tw, d_m.ptr, d_w.ptr, d_gb.ptr, d_s.ptr, d_wp.ptr if d_wp else None,
                                                            d_g.ptr if d_g else None))
            m.sync()
            for d_s, d_wp, d_g in outs:
                assert np.array_equal(d_s.numpy().view(np.float64), packed(res)), streams
                assert d_wp is None or (same(d_wp.numpy(), res.warped) and same(d_g.numpy(), res.wgrad)), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


def test_gauss_newton_step_w_lowers_the_cost():
    name, shape = "morlet3", (19, 23)
    m, img, tg, maps, w = model(name), vc.images(), ac.targets(shape), ac.maps(shape), wc.weights(shape)
    first = m.align_cost_w(img, tg, maps, weights=w)
    step = align.gauss_newton_step_w(first, damping=1e-2)
    moved = m.align_cost_w(img, tg, (maps.astype(np.float64) + step[:, :6]).astype(np.float32), weights=w,
                           intensity=(np.array([1.0, 0.0]) + step[:, 6:]).astype(np.float32))
    assert step[:2].any() and (moved.cost[:2] / moved.wsum[:2] < first.cost[:2] / first.wsum[:2]).all()


def test_refusals_launch_nothing_and_the_plain_call_is_left_alone():
    shape = (19, 23)
    img, tg, maps, w, gb = vc.images(), ac.targets(shape), ac.maps(shape), wc.weights(shape), wc.INTENSITY
    sums = np.full((N, align.SUMS_W), -7.0)
    wide = build(syn.make_state_dict(seed=3, dim_hidden=512, num_layers=3), H=512, L=3)
    profile_on(wide)
    try:
        with pytest.raises(ValueError, match="256"):
            wide.align_cost_w(img, tg, maps, weights=w)
        wide.sync()
        assert wide.profile_kernels() == []
    finally:
        profile_off(wide)
    m = model()
    before = m.align_cost(img, tg, maps, warped=True, gradient=True)
    profile_on(m)
    try:
        d = m.device_array(img.shape).copy_from(img)
        m.sync()
        args = (img.ctypes.data, N, HW, HW, tg.ctypes.data, shape[0], shape[1], maps.ctypes.data, w.ctypes.data, gb.ctypes.data, sums.ctypes.data, None, None)
        for k in (0, 4, 7, 10):  # images, targets, maps, sums
            bad = list(args)
            bad[k] = None
            assert m._lib.msiren_align_slices_w(m._h, *bad) == _lib.E_INVALID and "null" in _lib.last_error()
            dev = [d.ptr, N, HW, HW, d.ptr, 4, 4, d.ptr, d.ptr, d.ptr, d.ptr, None, None]
            dev[k] = None
            assert m._lib.msiren_align_slices_w_dev(m._h, *dev) == _lib.E_INVALID
        for k in (8, 9):  # misaligned device weights, intensity
            dev = [d.ptr, N, HW, HW, d.ptr, 4, 4, d.ptr, d.ptr, d.ptr, d.ptr, None, None]
            dev[k] = d.ptr + 2
            assert m._lib.msiren_align_slices_w_dev(m._h, *dev) == _lib.E_INVALID and "aligned" in _lib.last_error()
        for n, th, tw in ((N, 1 << 12, 1 << 12), (1 << 20, 64, 64), (N, 1 << 30, 1 << 30), (-1, 4, 4)):
            assert m._lib.msiren_align_slices_w(m._h, img.ctypes.data, n, HW, HW, tg.ctypes.data, th, tw, maps.ctypes.data, None, None, sums.ctypes.data, None, None) == _lib.E_INVALID
            assert m._lib.msiren_align_slices_w_dev(m._h, d.ptr, n, HW, HW, d.ptr, th, tw, d.ptr, None, None, d.ptr, None, None) == _lib.E_INVALID
        for kw in (dict(weights=w[:2]), dict(weights=w[:, :5]), dict(intensity=gb[:, :1]), dict(intensity=gb[:3])):
            with pytest.raises(ValueError):
                m.align_cost_w(img, tg, maps, **kw)
        with pytest.raises(ValueError):
            m.align_cost_w(img, tg, maps[:, :5])
        # nothing to do: 0 is returned, nothing written
        assert m._lib.msiren_align_slices_w(m._h, None, 0, HW, HW, None, shape[0], shape[1], None, None, None, sums.ctypes.data, None, None) == 0
        assert m._lib.msiren_align_slices_w_dev(m._h, d.ptr, N, HW, HW, d.ptr, 0, 4, d.ptr, None, None, d.ptr, None, None) == 0
        empty = m.align_cost_w(img[:0], tg[:0], maps[:0], warped=True)
        assert empty.count.shape == (0,) and empty.jtj.shape == (0, 8, 8) and empty.warped.shape == (0,) + shape
        m.sync()
        assert (sums == -7.0).all() and np.array_equal(d.numpy(), img) and m.profile_kernels() == []
        # the profile names the steps of one call
        m.align_cost_w(img, tg, maps, weights=w, intensity=gb)
        names = [e["kernel"] for e in m.profile_kernels()]
        assert names.count("align_bin_kernels") == 1 and names.count("align_reduce_w_kernels") == 1 and "align_reduce_kernels" not in names, names
        assert "siren_trunk_f32_jet_ragged_kernel<256,0>" in names and len([k for k in names if "align" in k or "ragged" in k]) == 3, names
    finally:
        profile_off(m)
    after = m.align_cost(img, tg, maps, warped=True, gradient=True)  # the plain call before and after weighted calls: the same bits
    assert np.array_equal(packed29(before), packed29(after)) and same(before.warped, after.warped) and same(before.wgrad, after.wgrad)
    assert np.array_equal(packed29(after), packed29(gpu_result("sine5", shape)))
