"""Weighted, gain/bias-compensated scoring of target slices against the stack read as a volume on the GPU:
model.align_volume_cost_w, i.e. msiren_align_volume_w* -- section 5.13's pipeline with the 80-sum reduce.  Stack, models, lattices, maps, targets:
tests/align_volume_cases.py; weights, intensities, reference and gate: tests/align_volume_w_cases.py.

Without weights and intensity the 56 shared entries have to be the bits of model.align_volume_cost; with flat Z rows the 47 entries of
model.align_cost_w of every slice stand in their places; weights in {0, 1} give the bits of NaN-masked targets; a weight halved scales exactly;
warped / wgrad stay the bits of model.resample_volume_with_gradient.  The sums are compared with numpy on the call's own planes inside the
worst-case bound of an fp64 sum in any order (N 2^-52 sum|term|), and with the fp64 reference inside the gate (4 x the reference's own
perturbed-fp32 distance, capped at 1e-4 of sum|term|); the distances measured on the MI355X are in LAB_NOTES.md section 27.
"""
import functools

import numpy as np
import pytest

import align_cases as ac
import align_volume_cases as avc
import align_volume_w_cases as wc
import align_volume_w_reference as avwr
import align_w_cases as w2
import align_w_reference as awr
import volume_cases as vc
from mri_inr_amd import _lib, align_volume as av, synthetic as syn
from test_gpu_align import build, model, profile_off, profile_on, same
from test_gpu_align_volume import gpu_result, packed as packed56

pytestmark = pytest.mark.gpu

N, M, HW = wc.N, wc.M, wc.HW
CASES = [(m, s) for m in wc.MODELS for s in wc.LATTICES]
PRECS = ["fp32", "f16x3"]
SUMS = av.SUMS_VW
packed = wc.packed
# where align_cost_w's 47 entries (count, wsum, cost, dcost over (a00 .. t1, g, b), jtj over the same eight) stand among the 80: the in-plane six
# are parameters 3 .. 8 of the eleven, (g, b) 9 and 10
IN_PLANE = [3, 4, 5, 6, 7, 8, 9, 10]
AS_47 = [0, 1, 2] + [3 + a for a in IN_PLANE] + [14 + avwr.PACK.index((IN_PLANE[a], IN_PLANE[b])) for a, b in awr.PACK]


@functools.lru_cache(maxsize=None)
def gpu_result_w(name, shape, prec="fp32"):
    return model(name, prec).align_volume_cost_w(vc.images(), avc.targets(shape), avc.maps(shape), weights=wc.weights(shape), intensity=wc.INTENSITY, warped=True,
                                                 gradient=True)


def shared(res):
    """the entries an AlignResultVW shares with an AlignResultV, as (m, 56)"""
    return packed(res)[:, avwr.SHARED]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,shape", CASES)
def test_without_weights_and_intensity_the_shared_entries_are_align_volume_costs_bits(name, shape, prec):
    old = gpu_result(name, shape, prec)
    m = model(name, prec)
    new = m.align_volume_cost_w(vc.images(), avc.targets(shape), avc.maps(shape), warped=True, gradient=True)
    assert np.array_equal(shared(new), packed56(old)) and np.array_equal(new.wsum, new.count.astype(np.float64))
    assert np.array_equal(new.count, old.count) and np.array_equal(new.cost, old.cost) and np.array_equal(new.grad[:, :9], old.grad) and np.array_equal(new.jtj[:, :9, :9], old.jtj)
    assert same(new.warped, old.warped) and same(new.wgrad, old.wgrad)
    assert np.array_equal(new.jtj[:, 10, 10], new.wsum) and new.grad.shape == (M, 11) and new.jtj.shape == (M, 11, 11)
    ones = m.align_volume_cost_w(vc.images(), avc.targets(shape), avc.maps(shape), weights=np.ones((M,) + shape, np.float32),
                                 intensity=np.tile(np.array([1.0, 0.0], np.float32), (M, 1)))
    assert np.array_equal(packed(ones), packed(new))  # the defaults are w = 1, (g, b) = (1, 0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,shape", CASES)
def test_planes_stay_the_bits_of_resample_volume_before_gain_and_bias(name, shape, prec):
    res, old = gpu_result_w(name, shape, prec), gpu_result(name, shape, prec)
    assert same(res.warped, old.warped) and same(res.wgrad, old.wgrad) and res.warped.dtype == np.float32 and res.wgrad.shape == (3, M) + shape
    m, maps = model(name, prec), avc.maps(shape)
    for q in (2, 3):  # (tests/test_gpu_align_volume.py pins every target of the plain call to resample_volume_with_gradient)
        val, grad = m.resample_volume_with_gradient(vc.images(), av.map_points3(maps[q], shape))
        assert same(res.warped[q].ravel(), val) and same(res.wgrad[:, q].reshape(3, -1), grad), (prec, q)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,shape", CASES)
def test_flat_z_rows_give_the_bits_of_the_weighted_2d_call(name, shape, prec):
    """m = n targets, target s on slice s (Z rows (0, 0, s)): the 47 entries of align_cost_w of slice s stand in their places among the 80"""
    m, maps2, tg, w, gb = model(name, prec), ac.maps(shape), ac.targets(shape), w2.weights(shape), w2.INTENSITY
    maps3 = np.zeros((N, 9), np.float32)
    maps3[:, 2] = np.arange(N)
    maps3[:, 3:] = maps2
    two = m.align_cost_w(vc.images(), tg, maps2, weights=w, intensity=gb, warped=True, gradient=True)
    three = m.align_volume_cost_w(vc.images(), tg, maps3, weights=w, intensity=gb, warped=True, gradient=True)
    assert np.array_equal(packed(three)[:, AS_47], w2.packed(two))
    assert same(three.warped, two.warped) and same(three.wgrad[1:], two.wgrad)
    assert three.jtj[:3, :3, :3].any() and three.grad[:3, :3].any()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,shape", CASES)
def test_mask_and_scale_identities(name, shape, prec):
    m, img, tg, maps = model(name, prec), vc.images(), avc.targets(shape), avc.maps(shape)
    with np.errstate(invalid="ignore"):
        keep = (wc.weights(shape) > 0.5).astype(np.float32)
    assert 0 < keep.sum() < keep.size
    masked = m.align_volume_cost(img, np.where(keep > 0, tg, np.nan).astype(np.float32), maps)
    binary = m.align_volume_cost_w(img, tg, maps, weights=keep)
    assert np.array_equal(shared(binary), packed56(masked)) and np.array_equal(binary.wsum, binary.count.astype(np.float64))  # weights in {0, 1}: NaN-masked targets
    full = gpu_result_w(name, shape, prec)
    for scale in (0.5, 4.0):  # a power of two scales exactly
        scaled = m.align_volume_cost_w(img, tg, maps, weights=np.float32(scale) * wc.weights(shape), intensity=wc.INTENSITY)
        assert np.array_equal(scaled.count, full.count) and np.array_equal(packed(scaled)[:, 1:], scale * packed(full)[:, 1:]), scale
    w = wc.weights(shape)
    bad = w.copy()
    with np.errstate(invalid="ignore"):
        zero = ~(w > 0)  # the zero blocks and the one NaN
    assert zero.sum() >= 4
    bad[zero] = np.resize(np.array([-1.0, np.nan, np.inf, -np.inf, -0.0], np.float32), int(zero.sum()))
    w[zero] = 0.0
    extra = np.zeros_like(zero)
    extra[4, 1, 1:5] = True
    bad[extra], w[extra] = np.array([-2.5, np.nan, np.inf, -np.inf], np.float32), 0.0
    assert np.array_equal(packed(m.align_volume_cost_w(img, tg, maps, weights=bad, intensity=wc.INTENSITY)),
                          packed(m.align_volume_cost_w(img, tg, maps, weights=w, intensity=wc.INTENSITY)))


@pytest.mark.parametrize("name,shape", CASES)
def test_sums_against_the_calls_own_planes(name, shape):
    res = gpu_result_w(name, shape)
    got, targets, w = packed(res), avc.targets(shape), wc.weights(shape)
    pixels = shape[0] * shape[1]
    for q in range(M):
        want, mags = avwr.sums_of_planes(res.warped[q], res.wgrad[0, q], res.wgrad[1, q], res.wgrad[2, q], targets[q], w[q], wc.INTENSITY[q], shape)
        bound = pixels * 2.0 ** -52 * mags  # the worst case of an fp64 sum of N terms in any order (and of the terms' own roundings)
        err = np.abs(got[q] - want)
        print(f"{name} {shape} target {q}: count {int(got[q, 0])}, largest error / bound {np.max(err[1:] / np.maximum(bound[1:], 1e-300)):.3f}")
        assert got[q, 0] == want[0], q
        assert (err[1:] <= bound[1:]).all(), (q, err, bound)
    assert res.count.tolist() == wc.data(name, shape)["sums"][:, 0].astype(int).tolist()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,shape", CASES)
def test_sums_against_the_fp64_reference(name, shape, prec):
    d = wc.data(name, shape)
    got = packed(gpu_result_w(name, shape, prec))
    e = wc.scaled_errors(got, d["sums"], d["mags"])
    print(f"{prec} {name} {shape}: distance {e.max():.2e} (per target {np.array2string(e.max(axis=1), precision=2)}), reference's own {d['D']:.2e}, gate {d['gate']:.2e}")
    assert wc.accepts(d, got), (e.max(axis=1), d["gate"])


def test_determinism_and_independence():
    name, shape = "sine5", (47, 45)
    m, img, tg, maps, w, gb = model(name), vc.images(), avc.targets(shape), avc.maps(shape), wc.weights(shape), wc.INTENSITY
    res = gpu_result_w(name, shape)
    again = m.align_volume_cost_w(img, tg, maps, weights=w, intensity=gb, warped=True, gradient=True)
    assert np.array_equal(packed(again), packed(res)) and same(again.warped, res.warped) and same(again.wgrad, res.wgrad)  # two runs
    for q in range(M):                                                                                                     # a target alone
        one = m.align_volume_cost_w(img, tg[q:q + 1], maps[q:q + 1], weights=w[q:q + 1], intensity=gb[q:q + 1], warped=True)
        assert np.array_equal(packed(one)[0], packed(res)[q]) and same(one.warped[0], res.warped[q]), q
    sub = [5, 2, 2, 0]                                                                                                     # any batch: rows in another order, one twice
    part = m.align_volume_cost_w(img, tg[sub], maps[sub], weights=w[sub], intensity=gb[sub])
    assert np.array_equal(packed(part), packed(res)[sub])
    for kw in (dict(), dict(warped=True), dict(gradient=True)):                                                            # optional outputs omitted
        part = m.align_volume_cost_w(img, tg, maps, weights=w, intensity=gb, **kw)
        assert np.array_equal(packed(part), packed(res)) and (part.warped is None) == ("warped" not in kw) and (part.wgrad is None) == ("gradient" not in kw)
    # the _dev form against the host form, on one stream and on two alternating, calls back to back without a sync; sums as pairs of floats
    th, tw = shape
    d_i, d_t, d_m = m.device_array(img.shape).copy_from(img), m.device_array(tg.shape).copy_from(tg), m.device_array(maps.shape).copy_from(maps)
    d_w, d_gb = m.device_array(w.shape).copy_from(w), m.device_array(gb.shape).copy_from(gb)
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array((M, 2 * SUMS)), m.device_array((M, th, tw)) if k != 1 else None, m.device_array((3, M, th, tw)) if k != 1 else None)
                    for k in range(streams + 1)]
            for d_s, d_wp, d_g in outs:
                _lib.check(m._lib.msiren_align_volume_w_dev(m._h, d_i.ptr, N, HW, HW, d_t.ptr, M, th, tw, d_m.ptr, d_w.ptr, d_gb.ptr, d_s.ptr, d_wp.ptr if d_wp else None,
                                                            d_g.ptr if d_g else None))
            m.sync()
            for d_s, d_wp, d_g in outs:
                assert np.array_equal(d_s.numpy().view(np.float64), packed(res)), streams
                assert d_wp is None or (same(d_wp.numpy(), res.warped) and same(d_g.numpy(), res.wgrad)), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


def test_gauss_newton_step_vw_lowers_the_cost():
    name, shape = "morlet3", (19, 23)
    m, img, tg, maps, w = model(name), vc.images(), avc.targets(shape), avc.maps(shape), wc.weights(shape)
    first = m.align_volume_cost_w(img, tg, maps, weights=w)
    step = av.gauss_newton_step_vw(first, damping=1e-2)
    moved = m.align_volume_cost_w(img, tg, (maps.astype(np.float64) + step[:, :9]).astype(np.float32), weights=w,
                                  intensity=(np.array([1.0, 0.0]) + step[:, 9:]).astype(np.float32))
    assert step[[0, 1]].any() and (moved.cost[[0, 1]] / moved.wsum[[0, 1]] < first.cost[[0, 1]] / first.wsum[[0, 1]]).all()


def test_refusals_launch_nothing_and_the_other_calls_are_left_alone():
    shape = (19, 23)
    img, tg, maps, w, gb = vc.images(), avc.targets(shape), avc.maps(shape), wc.weights(shape), wc.INTENSITY
    sums = np.full((M, SUMS), -7.0)
    wide = build(syn.make_state_dict(seed=3, dim_hidden=512, num_layers=3), H=512, L=3)
    profile_on(wide)
    try:
        with pytest.raises(ValueError, match="256"):
            wide.align_volume_cost_w(img, tg, maps, weights=w)
        wide.sync()
        assert wide.profile_kernels() == []
    finally:
        profile_off(wide)
    m = model()

    def others():
        plain = m.align_volume_cost(img, tg, maps, warped=True, gradient=True)
        two = m.align_cost_w(img, ac.targets(shape), ac.maps(shape), weights=w2.weights(shape), intensity=w2.INTENSITY, warped=True, gradient=True)
        return packed56(plain), plain.warped, plain.wgrad, w2.packed(two), two.warped, two.wgrad

    before = others()
    profile_on(m)
    try:
        d = m.device_array(img.shape).copy_from(img)
        m.sync()
        args = (img.ctypes.data, N, HW, HW, tg.ctypes.data, M, shape[0], shape[1], maps.ctypes.data, w.ctypes.data, gb.ctypes.data, sums.ctypes.data, None, None)
        for k in (0, 4, 8, 11):  # images, targets, maps, sums
            bad = list(args)
            bad[k] = None
            assert m._lib.msiren_align_volume_w(m._h, *bad) == _lib.E_INVALID and "null" in _lib.last_error()
            dev = [d.ptr, N, HW, HW, d.ptr, 2, 4, 4, d.ptr, d.ptr, d.ptr, d.ptr, None, None]
            dev[k] = None
            assert m._lib.msiren_align_volume_w_dev(m._h, *dev) == _lib.E_INVALID
        for k in (9, 10, 12, 13):  # misaligned device weights, intensity, warped, wgrad
            dev = [d.ptr, N, HW, HW, d.ptr, 2, 4, 4, d.ptr, d.ptr, d.ptr, d.ptr, None, None]
            dev[k] = d.ptr + 2
            assert m._lib.msiren_align_volume_w_dev(m._h, *dev) == _lib.E_INVALID and "aligned" in _lib.last_error()
        # an oversize product: 32 m th tw K + 8 m th tw with 640 bytes per chunk >= 2^30, or m th tw >= 2^28; n < 2
        for mm, th, tw in ((M, 1 << 12, 1 << 12), (1 << 20, 64, 64), (M, 1 << 30, 1 << 30), (-1, 4, 4)):
            assert m._lib.msiren_align_volume_w(m._h, img.ctypes.data, N, HW, HW, tg.ctypes.data, mm, th, tw, maps.ctypes.data, None, None, sums.ctypes.data, None, None) == _lib.E_INVALID
            assert m._lib.msiren_align_volume_w_dev(m._h, d.ptr, N, HW, HW, d.ptr, mm, th, tw, d.ptr, None, None, d.ptr, None, None) == _lib.E_INVALID
        # the weighted form's own limit, K = 4 and one chunk per target: 7680 (136 x 1024 + 448) < 2^30 <= 7680 (136 x 1024 + 640)
        mm, th, tw = 7680, 32, 32
        assert (vc.S + vc.I - 1) // vc.I == 2
        assert m._lib.msiren_align_volume_dev(m._h, d.ptr, N, HW, HW, d.ptr, mm, th, tw, None, None, None, None) == _lib.E_INVALID and "null" in _lib.last_error()
        assert m._lib.msiren_align_volume_w_dev(m._h, d.ptr, N, HW, HW, d.ptr, mm, th, tw, None, None, None, None, None, None) == _lib.E_INVALID
        assert "too many pixels" in _lib.last_error() and "640 bytes per chunk" in _lib.last_error() and "32 m th tw K" in _lib.last_error()
        for n in (1, 0):
            assert m._lib.msiren_align_volume_w(m._h, *args[:1], n, *args[2:]) == _lib.E_INVALID
        for kw in (dict(weights=w[:2]), dict(weights=w[:, :5]), dict(intensity=gb[:, :1]), dict(intensity=gb[:3])):
            with pytest.raises(ValueError):
                m.align_volume_cost_w(img, tg, maps, **kw)
        with pytest.raises(ValueError):
            m.align_volume_cost_w(img, tg, maps[:, :6])
        # nothing to do: 0 is returned, nothing written
        assert m._lib.msiren_align_volume_w(m._h, img.ctypes.data, N, HW, HW, None, 0, shape[0], shape[1], None, None, None, sums.ctypes.data, None, None) == 0
        assert m._lib.msiren_align_volume_w_dev(m._h, d.ptr, N, HW, HW, d.ptr, 2, 0, 4, d.ptr, None, None, d.ptr, None, None) == 0
        empty = m.align_volume_cost_w(img, tg[:0], maps[:0], warped=True)
        assert empty.count.shape == (0,) and empty.jtj.shape == (0, 11, 11) and empty.warped.shape == (0,) + shape
        m.sync()
        assert (sums == -7.0).all() and np.array_equal(d.numpy(), img) and m.profile_kernels() == []
        # the profile names the steps of one call
        m.align_volume_cost_w(img, tg, maps, weights=w, intensity=gb)
        names = [e["kernel"] for e in m.profile_kernels()]
        assert names.count("align_volume_bin_kernels") == 1 and names.count("align_volume_reduce_w_kernels") == 1 and "align_volume_reduce_kernels" not in names, names
        assert "siren_trunk_f32_jet_ragged_kernel<256,0>" in names and len([k for k in names if "align" in k or "ragged" in k]) == 3, names
    finally:
        profile_off(m)
    after = others()  # the plain volume call and the weighted 2-D call before and after: the same bits
    assert all(same(x, y) for x, y in zip(before, after))
    assert np.array_equal(packed(m.align_volume_cost_w(img, tg, maps, weights=w, intensity=gb)), packed(gpu_result_w("sine5", shape)))  # the handle stays usable
