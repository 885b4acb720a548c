"""Weighted, gain/bias-compensated alignment of target slices to the stack read as a volume on the GPU:
model.align_volume_solve_w / align_volume_solve_rigid_w, i.e. msiren_align_volume_solve_w* -- msiren_align_volume_w's prologue once, then per
evaluation bin -> jet ragged trunk -> the 80-sum reduce -> align_volume_step_w_kernel of the (geometry, intensity) mode, on one stream.  Cases:
tests/align_volume_w_cases.py (the targets here are g_t W + b_t of the device's own warped planes W at the truth, corrupted inside the block the
weights mask).

The device loop is pinned bit for bit against the host loop in all four modes: every traced evaluation has the (cost, count, wsum) of
model.align_volume_cost_w at the traced trial (map, g, b), mri_inr_amd.align_volume.lm_step_vw produces the next traced trial from that call's
sums, and the report is that of the replayed states.  With the intensity fixed at (1, 0) and no weights the call returns
model.align_volume_solve's bits.  Convergence is gated by the CPU variant's distance (tests/test_align_volume_w_reference.py asserts D_solve <=
1e-6, so the gate is the fp32 resolution of the parameters); the errors measured on the MI355X are in LAB_NOTES.md section 27.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import align_cases as ac
import align_volume_cases as avc
import align_volume_w_cases as wc
import align_w_cases as w2
import volume_cases as vc
from mri_inr_amd import _lib, align, align_volume as av
from test_gpu_align import model, profile_off, profile_on
from test_gpu_align_volume import packed as packed56
from test_gpu_align_volume_solve import solve as solve_plain, targets as plain_targets

pytestmark = pytest.mark.gpu

N, HW, SHAPE, M, IT = wc.N, wc.HW, wc.SHAPE, wc.SOLVE_M, wc.ITERATIONS
ALL = [(prec, name, mode, est) for prec in ("fp32", "f16x3") for name in wc.MODELS for mode, est in wc.MODES]
packed = wc.packed


@functools.lru_cache(maxsize=None)
def targets(name, prec="fp32", corrupted=True):
    return wc.targets_of(plain_targets(name, prec), corrupted)


def solve(m, tg, mode, est, images=None, sub=slice(None), planes=None, start=None, weights="case", intensity="case", **kw):
    images = vc.images() if images is None else images
    kw.setdefault("iterations", IT)
    w = wc.solve_weights() if isinstance(weights, str) else weights
    gb = wc.start_intensity(est) if isinstance(intensity, str) else intensity
    kw.update(weights=None if w is None else w[sub], intensity=None if gb is None else gb[sub], estimate_intensity=est == av.ESTIMATE)
    if mode == align.RIGID:
        return m.align_volume_solve_rigid_w(images, tg[sub], (avc.planes() if planes is None else planes)[sub], avc.SPACING, **kw)
    return m.align_volume_solve_w(images, tg[sub], (avc.start_maps() if start is None else start)[sub], **kw)


@functools.lru_cache(maxsize=None)
def solved(prec, name, mode, est):
    return solve(model(name, prec), targets(name, prec), mode, est, trace=True)


def same(a, b):
    """two SolveResultVWs, bit for bit (trace aside)"""
    return all(np.array_equal(x, y, equal_nan=True) if x is not None else y is None for x, y in zip(a[:9] + a[10:], b[:9] + b[10:]))


def opts(mode=0, iterations=4, est=1, *, struct_size=None, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, spacing=avc.SPACING):
    return _lib.AlignVolumeSolveWOpts(C.sizeof(_lib.AlignVolumeSolveWOpts) if struct_size is None else struct_size, mode, iterations, est, damping, down, up, lam_min,
                                      lam_max, spacing)


@pytest.mark.parametrize("prec,name,mode,est", ALL)
def test_the_device_loop_is_the_host_loop_bit_for_bit(prec, name, mode, est):
    m, tg, w, res = model(name, prec), targets(name, prec), wc.solve_weights(), solved(prec, name, mode, est)
    assert res.trace.shape == (IT, M, 14)
    sums = []
    for k in range(IT):  # every evaluation: the bits of align_volume_cost_w at the traced trial (map, g, b)
        trial = res.trace[k, :, :11].astype(np.float32)
        assert np.array_equal(trial.astype(np.float64), res.trace[k, :, :11], equal_nan=True)
        sums.append(packed(m.align_volume_cost_w(vc.images(), tg, trial[:, :9], weights=w, intensity=trial[:, 9:])))
        assert np.array_equal(res.trace[k, :, 11], sums[k][:, 2]) and np.array_equal(res.trace[k, :, 12], sums[k][:, 0]) and np.array_equal(res.trace[k, :, 13], sums[k][:, 1]), k
    differs, st = wc.replay(res.trace, lambda k: sums[k], mode, est, avc.start_maps(), avc.start_rigid(), avc.planes(), wc.start_intensity(est))  # every step: lm_step_vw's bits
    assert differs is None, differs
    # hence the outputs are those of solve_on_host_vw(model.align_volume_cost_w)
    rigid = np.array([x["rigid_best"] for x in st]) if mode == align.RIGID else None
    want = av.solve_result_vw(np.array([x["best"] for x in st], np.float32), np.array([x["gb_best"] for x in st], np.float32), rigid, av.report_vw(st), None)
    assert same(res, want), (res[:9], want[:9])
    if est == av.FIXED:
        assert np.array_equal(res.intensity, wc.GB_TRUTH) and np.array_equal(res.trace[:, :, 9:11], np.broadcast_to(wc.GB_TRUTH.astype(np.float64), (IT, M, 2)))
    else:
        assert np.array_equal(res.trace[0, :, 9:11], np.tile([1.0, 0.0], (M, 1))) and (res.trace[1:, :, 9:11] != res.trace[:1, :, 9:11]).any()


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("mode", avc.MODES)
def test_the_host_loop_around_the_cost_call_gives_the_calls_bits(prec, mode):
    name, est = "morlet3", av.ESTIMATE
    m, tg, w, res = model(name, prec), targets(name, prec), wc.solve_weights(), solved(prec, name, mode, est)
    host, _ = av.solve_on_host_vw(lambda maps, gb: packed(m.align_volume_cost_w(vc.images(), tg, maps, weights=w, intensity=gb)), M, maps=avc.start_maps(),
                                  rigid=avc.start_rigid(), planes=avc.planes(), intensity=None, options=wc.options(mode, est), trace=True)
    assert same(res, host) and np.array_equal(res.trace, host.trace)


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", list(wc.MODELS))
@pytest.mark.parametrize("mode", avc.MODES)
def test_fixed_unit_intensity_without_weights_is_align_volume_solve(prec, name, mode):
    m, tg = model(name, prec), plain_targets(name, prec)
    old = solve_plain(m, tg, mode, iterations=IT, trace=True)
    new = solve(m, tg, mode, av.FIXED, weights=None, intensity=None, trace=True)
    assert np.array_equal(new.maps, old.maps) and np.array_equal(new.accepted, old.accepted) and np.array_equal(new.mean_first, old.mean_first)
    assert np.array_equal(new.mean_best, old.mean_best) and np.array_equal(new.count, old.count) and np.array_equal(new.damping, old.damping) and np.array_equal(new.flags, old.flags)
    assert np.array_equal(new.wsum, new.count.astype(np.float64)) and np.array_equal(new.intensity, np.tile(np.array([1.0, 0.0], np.float32), (M, 1)))
    if mode == align.RIGID:
        assert np.array_equal(new.rotation, old.rotation) and np.array_equal(new.shift, old.shift)
    else:
        assert new.rotation is None and new.shift is None
    assert np.array_equal(new.trace[:, :, :9], old.trace[:, :, :9]) and np.array_equal(new.trace[:, :, 11:13], old.trace[:, :, 9:11])  # trial map, cost, count
    assert np.array_equal(new.trace[:, :, 13], new.trace[:, :, 12]) and np.array_equal(new.trace[:, :, 9:11], np.broadcast_to([1.0, 0.0], (IT, M, 2)))
    assert old.accepted.sum() >= 3 * M
    ones = solve(m, tg, mode, av.FIXED, weights=np.ones((M,) + SHAPE, np.float32), intensity=np.tile(np.array([1.0, 0.0], np.float32), (M, 1)), trace=True)
    assert same(ones, new) and np.array_equal(ones.trace, new.trace)


@pytest.mark.parametrize("mode,est", wc.MODES)
def test_one_iteration_returns_the_input(mode, est):
    m, tg, w = model("sine5"), targets("sine5"), wc.solve_weights()
    gb = np.array([[1.5, -0.25], [0.75, 0.5], [1.0, 0.0], [2.0, 1.0]], np.float32)
    res = solve(m, tg, mode, est, intensity=gb, iterations=1)
    first = m.align_volume_cost_w(vc.images(), tg, avc.start_maps(), weights=w, intensity=gb)
    assert np.array_equal(res.maps, avc.start_maps()) and np.array_equal(res.intensity, gb) and not res.accepted.any()
    assert np.array_equal(res.mean_first, first.cost / first.wsum) and np.array_equal(res.mean_best, res.mean_first)
    assert np.array_equal(res.count, first.count) and np.array_equal(res.wsum, first.wsum)
    assert np.array_equal(res.damping, np.full(M, 1e-3)) and not res.flags.any()
    if mode == align.RIGID:
        assert np.array_equal(res.rotation, np.tile(np.eye(3), (M, 1, 1))) and not res.shift.any()


@pytest.mark.parametrize("prec,name,mode,est", ALL)
def test_convergence_on_the_gate_targets(prec, name, mode, est):
    res, gate, rows = solved(prec, name, mode, est), wc.device_solve_gate(), list(wc.gate_targets(name, est))
    err = wc.errors(res.maps, res.intensity)
    print(f"{prec} {name} mode {mode} intensity {est}: errors {np.array2string(err, precision=2)} gate {gate:.2e}; accepted {res.accepted.tolist()}, "
          f"lam {res.damping.tolist()}, flags {res.flags.tolist()}, (g, b) {res.intensity.tolist()}")
    assert (err[rows] <= gate).all(), (err, gate)
    assert (res.mean_best <= res.mean_first).all() and not res.flags[rows].any()
    assert (res.count == SHAPE[0] * SHAPE[1] - 24).all() and (res.wsum < res.count).all()  # the corrupted block never counts


@pytest.mark.parametrize("prec,name,mode,est", ALL)
def test_the_corruption_behind_the_mask_reaches_no_bit(prec, name, mode, est):
    res = solved(prec, name, mode, est)
    clean = solve(model(name, prec), targets(name, prec, False), mode, est, trace=True)
    assert same(clean, res) and np.array_equal(clean.trace, res.trace)
    assert not np.array_equal(targets(name, prec, False), targets(name, prec), equal_nan=True)


@pytest.mark.parametrize("mode,est", wc.MODES)
def test_determinism_and_independence(mode, est):
    prec, name = "fp32", "morlet3"
    m, tg, res = model(name, prec), targets(name, prec), solved(prec, name, mode, est)
    again = solve(m, tg, mode, est, trace=True)
    assert same(again, res) and np.array_equal(again.trace, res.trace)  # two runs
    assert same(solve(m, tg, mode, est), res)                           # without the trace
    for q in range(M):                                                  # a target alone
        one = solve(m, tg, mode, est, sub=slice(q, q + 1), trace=True)
        assert all(np.array_equal(x[0], y[q], equal_nan=True) for x, y in zip(one[:9] + one[10:], res[:9] + res[10:]) if x is not None), q
        assert np.array_equal(one.trace[:, 0], res.trace[:, q]), q
    # the _dev form against the host form, on one stream and on two alternating, calls back to back without a sync; doubles as pairs of floats
    img, start, rigid, pl, w, gb = vc.images(), avc.start_maps(), avc.start_rigid(), avc.planes(), wc.solve_weights(), wc.start_intensity(est)
    d_i, d_t, d_m = m.device_array(img.shape).copy_from(img), m.device_array(tg.shape).copy_from(tg), m.device_array(start.shape).copy_from(start)
    d_r, d_p = m.device_array((M, 24)).copy_from(rigid.view(np.float32)), m.device_array((M, 24)).copy_from(pl.view(np.float32))
    d_w, d_gb = m.device_array(w.shape).copy_from(w), None if gb is None else m.device_array(gb.shape).copy_from(gb)
    o = opts(mode, IT, est)
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array((M, 9)), m.device_array((M, 2)), m.device_array((M, 24)), m.device_array((M, 14)), m.device_array((IT, M, 28)) if k != 1 else None)
                    for k in range(streams + 1)]
            for d_o, d_go, d_ro, d_rep, d_tr in outs:
                _lib.check(m._lib.msiren_align_volume_solve_w_dev(m._h, d_i.ptr, N, HW, HW, d_t.ptr, M, SHAPE[0], SHAPE[1], C.byref(o), d_m.ptr, d_p.ptr, d_r.ptr, d_w.ptr,
                                                                  d_gb.ptr if d_gb else None, d_o.ptr, d_go.ptr, d_ro.ptr, d_rep.ptr, d_tr.ptr if d_tr else None))
            m.sync()
            for d_o, d_go, d_ro, d_rep, d_tr in outs:
                got = av.solve_result_vw(d_o.numpy(), d_go.numpy(), d_ro.numpy().view(np.float64) if mode == align.RIGID else None, d_rep.numpy().view(np.float64), None)
                assert same(got, res), streams
                assert d_tr is None or np.array_equal(d_tr.numpy().view(np.float64), res.trace), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


@pytest.mark.parametrize("mode,est", wc.MODES)
def test_masked_and_black_targets_keep_their_inputs(mode, est):
    """target 0's weights mask every pixel (no valid pixel: NO_OVERLAP), target 1 moved onto a plane between two black slices (R = 0 everywhere:
    SINGULAR); both keep their map and their (g, b); the others are untouched by them"""
    name = "sine5"
    m = model(name)
    img = vc.images().copy()
    img[2] = 0.0  # slices 2 and 3 black
    pl = avc.planes().copy()
    pl[1, [6, 9]] = avc.SPACING * 2.5   # o and c of target 1: Z = 2.5
    start = av.rigid_maps3(np.eye(3), np.zeros(3), pl, avc.SPACING)
    tg, w = targets(name), wc.solve_weights()
    gb = np.array([[1.5, -0.25], [0.75, 0.5], [1.0, 0.0], [0.9, 0.1]], np.float32)
    ref = solve(m, tg, mode, est, images=img, intensity=gb, trace=True)  # targets 2 and 3 on this stack, in their usual places
    w0 = w.copy()
    w0[0] = np.resize(np.array([0.0, -1.0, np.nan, -np.inf], np.float32), SHAPE)
    got = solve(m, tg, mode, est, images=img, planes=pl, start=start, weights=w0, intensity=gb)
    assert got.flags[0] == (align.SINGULAR | align.NO_OVERLAP) and np.array_equal(got.maps[0], start[0]) and np.array_equal(got.intensity[0], gb[0]) and got.accepted[0] == 0
    assert got.mean_first[0] == np.inf and got.mean_best[0] == np.inf and got.count[0] == 0 and got.wsum[0] == 0
    assert got.flags[1] == align.SINGULAR and np.array_equal(got.maps[1], start[1]) and np.array_equal(got.intensity[1], gb[1]) and got.accepted[1] == 0
    assert np.isfinite(got.mean_first[1]) and got.count[1] == SHAPE[0] * SHAPE[1] - 24
    if mode == align.RIGID:
        assert np.array_equal(got.rotation[:2], np.tile(np.eye(3), (2, 1, 1))) and not got.shift[:2].any()
    assert all(np.array_equal(x[2:], y[2:]) for x, y in zip(got[:9] + got[10:], ref[:9] + ref[10:]) if x is not None)


def test_refusals_launch_nothing():
    m, img, tg, start, rigid, pl, w = model("sine5"), vc.images(), targets("sine5"), avc.start_maps(), avc.start_rigid(), avc.planes(), wc.solve_weights()
    out, gout, rout, rep = np.full((M, 9), -7.0, np.float32), np.full((M, 2), -7.0, np.float32), np.full((M, 12), -7.0), np.full((M, 7), -7.0)
    d = m.device_array(img.shape).copy_from(img)
    m.sync()
    profile_on(m)
    try:
        def host(o, **kw):
            a = dict(images=img.ctypes.data, n=N, targets=tg.ctypes.data, m=M, th=SHAPE[0], tw=SHAPE[1], maps=start.ctypes.data, planes=pl.ctypes.data,
                     rigid=rigid.ctypes.data, weights=w.ctypes.data, gb=None, out=out.ctypes.data, gout=gout.ctypes.data, rep=rep.ctypes.data)
            a.update(kw)
            return m._lib.msiren_align_volume_solve_w(m._h, a["images"], a["n"], HW, HW, a["targets"], a["m"], a["th"], a["tw"], C.byref(o) if o is not None else None,
                                                      a["maps"], a["planes"], a["rigid"], a["weights"], a["gb"], a["out"], a["gout"], rout.ctypes.data, a["rep"], None)

        def dev(o, **kw):
            a = dict(images=d.ptr, n=N, targets=d.ptr, m=2, th=4, tw=4, maps=d.ptr, planes=d.ptr, rigid=d.ptr, weights=d.ptr, gb=d.ptr, out=d.ptr, gout=d.ptr, rout=d.ptr,
                     rep=d.ptr, trace=None)
            a.update(kw)
            return m._lib.msiren_align_volume_solve_w_dev(m._h, a["images"], a["n"], HW, HW, a["targets"], a["m"], a["th"], a["tw"], C.byref(o) if o is not None else None,
                                                          a["maps"], a["planes"], a["rigid"], a["weights"], a["gb"], a["out"], a["gout"], a["rout"], a["rep"], a["trace"])

        inf, nan = float("inf"), float("nan")
        bad_opts = [opts(struct_size=72), opts(struct_size=0), opts(est=2), opts(est=-1), opts(mode=2), opts(mode=-1), opts(iterations=0), opts(iterations=257),
                    opts(lam_min=0.0), opts(lam_min=1e-2), opts(lam_max=1e-4), opts(lam_max=inf), opts(damping=nan), opts(down=0.0), opts(down=1.5), opts(down=nan),
                    opts(up=0.5), opts(up=inf), opts(up=nan), opts(mode=1, spacing=0.0), opts(mode=1, spacing=-1.0), opts(mode=1, spacing=inf), opts(mode=1, spacing=nan)]
        for o in bad_opts:
            assert host(o) == _lib.E_INVALID and _lib.last_error(), (o.mode, o.iterations)
            assert dev(o) == _lib.E_INVALID
        assert host(opts(est=2)) == _lib.E_INVALID and "intensity_mode" in _lib.last_error()
        assert host(opts(struct_size=72)) == _lib.E_INVALID and "struct_size" in _lib.last_error()
        assert host(None) == _lib.E_INVALID and dev(None) == _lib.E_INVALID
        for mode, missing in ((0, ("maps",)), (1, ("rigid", "planes"))):  # a missing input of the mode, outputs, images, targets
            for key in missing + ("out", "gout", "rep", "images", "targets"):
                assert host(opts(mode), **{key: None}) == _lib.E_INVALID and "null" in _lib.last_error(), (mode, key)
                assert dev(opts(mode), **{key: None}) == _lib.E_INVALID, (mode, key)
        for key, off in (("targets", 2), ("maps", 2), ("out", 2), ("weights", 2), ("gb", 2), ("gout", 2), ("rigid", 4), ("planes", 4), ("rout", 4), ("rep", 4),
                         ("trace", 4)):  # misaligned device pointers
            assert dev(opts(1 if key in ("rigid", "planes") else 0), **{key: d.ptr + off}) == _lib.E_INVALID and "aligned" in _lib.last_error(), key
        # everything msiren_align_volume_solve refuses, and the weighted form's own size limit (tests/test_gpu_align_volume_w.py)
        for kw in (dict(th=1 << 12, tw=1 << 12), dict(m=1 << 20, th=64, tw=64), dict(m=-1), dict(n=1), dict(n=1 << 25), dict(m=7680, th=32, tw=32)):
            assert host(opts(), **kw) == _lib.E_INVALID and dev(opts(), **kw) == _lib.E_INVALID, kw
        assert "640 bytes per chunk" in _lib.last_error()
        # nothing to do
        assert host(opts(), m=0) == 0 and host(opts(), th=0) == 0 and dev(opts(), tw=0) == 0 and dev(opts(), m=0) == 0
        for kw in (dict(iterations=0), dict(damping=0.0), dict(up=0.9)):
            with pytest.raises(ValueError):
                solve(m, tg, 0, av.ESTIMATE, **kw)
        with pytest.raises(ValueError):
            m.align_volume_solve_w(img, tg, start[:, :6])
        with pytest.raises(ValueError):
            m.align_volume_solve_w(img, tg, start, weights=w[:2])
        with pytest.raises(ValueError):
            m.align_volume_solve_w(img, tg, start, intensity=wc.GB_TRUTH[:, :1])
        with pytest.raises(ValueError):
            m.align_volume_solve_rigid_w(img, tg, pl, 0.0)
        with pytest.raises(ValueError):
            m.align_volume_solve_rigid_w(img, tg, pl[:2], avc.SPACING)
        m.sync()
        assert (out == -7.0).all() and (gout == -7.0).all() and (rout == -7.0).all() and (rep == -7.0).all() and np.array_equal(d.numpy(), img) and m.profile_kernels() == []
    finally:
        profile_off(m)
    assert same(solve(m, tg, 0, av.ESTIMATE), solved("fp32", "sine5", 0, av.ESTIMATE))  # the handle stays usable


@pytest.mark.parametrize("name,act", [("sine5", 0), ("morlet3", 1)])
def test_profile_counts(name, act):
    m, tg, w = model(name), targets(name), wc.solve_weights()
    trunk = f"siren_trunk_f32_jet_ragged_kernel<256,{act}>"
    per_eval = ("align_volume_bin_kernels", trunk, "align_volume_reduce_w_kernels")
    profile_on(m)
    try:
        m.align_volume_cost_w(vc.images(), tg, avc.start_maps(), weights=w)
        m.sync()
        one = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
    finally:
        profile_off(m)
    assert all(one[k] == 1 for k in per_eval) and not [k for k in one if "step" in k or k == "align_volume_reduce_kernels"], one
    for mode, est in wc.MODES:
        profile_on(m)
        try:
            solve(m, tg, mode, est, iterations=5)
            m.sync()
            got = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
        finally:
            profile_off(m)
        assert got["align_volume_step_w_kernel"] == 5 and all(got[k] == 5 for k in per_eval), got
        assert "align_volume_step_kernel" not in got and "align_volume_reduce_kernels" not in got, got
        prologue = {k: v for k, v in one.items() if k not in per_eval}
        assert {k: v for k, v in got.items() if k not in per_eval + ("align_volume_step_w_kernel",)} == prologue, (got, one)


def test_a_weighted_volume_solve_leaves_the_other_calls_alone():
    name, shape = "sine5", (19, 23)
    m, tg, img = model(name), targets(name), vc.images()

    def others():
        three = m.align_volume_cost(img, plain_targets(name), avc.truth(), warped=True, gradient=True)
        s3 = solve_plain(m, plain_targets(name), align.RIGID, iterations=3, trace=True)
        two = m.align_cost_w(img, ac.targets(shape), ac.maps(shape), weights=w2.weights(shape), intensity=w2.INTENSITY, warped=True, gradient=True)
        return packed56(three), three.warped, three.wgrad, s3.maps, s3.mean_best, s3.trace, s3.rotation, w2.packed(two), two.warped, two.wgrad

    before = others()
    for mode, est in wc.MODES:
        solve(m, tg, mode, est)
    after = others()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, after))
