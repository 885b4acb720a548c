"""Weighted, gain/bias-compensated alignment on the GPU: model.align_solve_w / align_solve_rigid_w, i.e.
msiren_align_solve_w* -- section 5.11's loop on the 47 sums, in the four modes (affine / rigid) x (intensity fixed / estimated).  Cases:
tests/align_w_cases.py (the targets are g_t W + b_t with W the device's own warped planes at the true map, corrupted inside the block the
weights mask).

The device loop is pinned bit for bit against the host loop: every traced evaluation has the (cost, count, wsum) of model.align_cost_w at
the traced trial (map, g, b), and mri_inr_amd.align.lm_step_w produces the next traced trial from that call's sums.  Without weights and with
the intensity fixed the call returns model.align_solve's bits.  Convergence over the 8 parameters is gated by the CPU variant's distance
(tests/test_align_w_reference.py asserts D <= 1e-6, so the gate is the fp32 resolution of the parameters); the errors measured on the
MI355X are in LAB_NOTES.md section 24.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import align_solve_cases as sc
import align_w_cases as wc
import volume_cases as vc
from mri_inr_amd import _lib, align
from test_gpu_align import model, packed as packed29, profile_off, profile_on
from test_gpu_align_solve import solve as plain_solve, solved as plain_solved, targets as plain_targets

pytestmark = pytest.mark.gpu

N, HW, SHAPE = sc.N, sc.HW, sc.SHAPE
ALL = [(prec, name, mode, est) for prec in ("fp32", "f16x3") for name in sc.MODELS for mode, est in wc.MODES]
FIELDS = ("maps", "angle", "shift", "accepted", "mean_first", "mean_best", "count", "damping", "flags", "intensity", "wsum")
packed = wc.packed


@functools.lru_cache(maxsize=None)
def targets(name, prec="fp32", corrupted=True):
    return wc.targets_of(model(name, prec).align_cost(vc.images(), np.zeros((N,) + SHAPE, np.float32), sc.truth(), warped=True).warped, corrupted)


def solve(m, tg, mode, est, images=None, sub=slice(None), weights="case", **kw):
    images = vc.images() if images is None else images
    kw.setdefault("iterations", wc.ITERATIONS)
    w = wc.solve_weights() if isinstance(weights, str) else weights
    gb = wc.start_intensity(est)
    kw.update(weights=None if w is None else w[sub], intensity=None if gb is None else gb[sub], estimate_intensity=est == align.ESTIMATE)
    if mode == align.RIGID:
        return m.align_solve_rigid_w(images[sub], tg[sub], np.zeros(N)[sub], np.tile(sc.START_SHIFT, (N, 1))[sub], sc.CENTRE, **kw)
    return m.align_solve_w(images[sub], tg[sub], sc.start_maps()[sub], **kw)


@functools.lru_cache(maxsize=None)
def solved(prec, name, mode, est):
    return solve(model(name, prec), targets(name, prec), mode, est, trace=True)


def same(a, b):
    """two SolveResultWs, bit for bit (trace aside)"""
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) if getattr(a, f) is not None else getattr(b, f) is None for f in FIELDS)


def opts(mode=0, est=1, iterations=4, *, struct_size=None, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, centre_y=sc.CENTRE[0], centre_x=sc.CENTRE[1]):
    return _lib.AlignSolveWOpts(C.sizeof(_lib.AlignSolveWOpts) if struct_size is None else struct_size, mode, iterations, est, damping, down, up, lam_min, lam_max,
                                centre_y, centre_x)


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("prec,name", [("fp32", "sine5"), ("f16x3", "morlet3")])
def test_fixed_intensity_without_weights_is_align_solve_bit_for_bit(prec, name, mode):
    m, tg, old = model(name, prec), plain_targets(name, prec), plain_solved(prec, name, mode)
    kw = dict(estimate_intensity=False, iterations=sc.ITERATIONS, trace=True)
    if mode == align.RIGID:
        new = m.align_solve_rigid_w(vc.images(), tg, np.zeros(N), np.tile(sc.START_SHIFT, (N, 1)), sc.CENTRE, **kw)
    else:
        new = m.align_solve_w(vc.images(), tg, sc.start_maps(), **kw)
    for f in ("maps", "angle", "shift", "accepted", "mean_first", "mean_best", "count", "damping", "flags"):
        a, b = getattr(new, f), getattr(old, f)
        assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True), f
    assert np.array_equal(new.trace[:, :, :6], old.trace[:, :, :6], equal_nan=True) and np.array_equal(new.trace[:, :, 8:10], old.trace[:, :, 6:8])
    assert np.array_equal(new.trace[:, :, 10], new.trace[:, :, 9]) and np.array_equal(new.wsum, new.count.astype(np.float64))
    assert np.array_equal(new.intensity, np.tile(np.array([1.0, 0.0], np.float32), (N, 1))) and np.array_equal(new.trace[:, :, 6:8], np.tile([1.0, 0.0], (sc.ITERATIONS, N, 1)))


@pytest.mark.parametrize("prec,name,mode,est", ALL)
def test_the_device_loop_is_the_host_loop_bit_for_bit(prec, name, mode, est):
    m, tg, res, w = model(name, prec), targets(name, prec), solved(prec, name, mode, est), wc.solve_weights()
    assert res.trace.shape == (wc.ITERATIONS, N, 11)
    sums = []
    for k in range(wc.ITERATIONS):  # every evaluation: the bits of align_cost_w at the traced trial (map, g, b)
        trial = res.trace[k, :, :8].astype(np.float32)
        assert np.array_equal(trial.astype(np.float64), res.trace[k, :, :8], equal_nan=True)
        sums.append(packed(m.align_cost_w(vc.images(), tg, trial[:, :6], weights=w, intensity=trial[:, 6:])))
        assert np.array_equal(res.trace[k, :, 8], sums[k][:, 2]) and np.array_equal(res.trace[k, :, 9], sums[k][:, 0]) and np.array_equal(res.trace[k, :, 10], sums[k][:, 1]), k
    gb0 = wc.start_intensity(est)
    differs, st = wc.replay(res.trace, lambda k: sums[k], mode, est, sc.start_maps(), sc.start_rigid(), gb0)  # every step: lm_step_w's bits
    assert differs is None, differs
    # hence the outputs are those of solve_on_host_w(model.align_cost_w)
    rigid = np.array([x["rigid_best"] for x in st]) if mode == align.RIGID else None
    want = align.solve_result_w(np.array([x["best"] for x in st], np.float32), np.array([x["gb_best"] for x in st], np.float32), rigid, align.report_w(st), None)
    assert same(res, want), (res[:9], want[:9])
    if prec == "fp32" and name == "morlet3":  # (the whole host loop again: once per mode is enough, the replay above is the same statement)
        host, _ = align.solve_on_host_w(lambda maps, gb: packed(m.align_cost_w(vc.images(), tg, maps, weights=w, intensity=gb)), N, maps=sc.start_maps(),
                                        rigid=sc.start_rigid(), intensity=gb0, options=wc.options(mode, est))
        assert same(res, host)


@pytest.mark.parametrize("mode,est", wc.MODES)
def test_one_iteration_returns_the_input(mode, est):
    m, tg, w = model("sine5"), targets("sine5"), wc.solve_weights()
    res = solve(m, tg, mode, est, iterations=1)
    gb = np.tile(np.array([1.0, 0.0], np.float32), (N, 1)) if est == align.ESTIMATE else wc.GB_TRUTH
    first = m.align_cost_w(vc.images(), tg, sc.start_maps(), weights=w, intensity=gb)
    assert np.array_equal(res.maps, sc.start_maps()) and np.array_equal(res.intensity, gb) and not res.accepted.any()
    assert np.array_equal(res.mean_first, first.cost / first.wsum) and np.array_equal(res.mean_best, res.mean_first)
    assert np.array_equal(res.count, first.count) and np.array_equal(res.wsum, first.wsum)
    assert np.array_equal(res.damping, np.full(N, 1e-3)) and res.flags.tolist() == [0, 0, 0, align.SINGULAR]


@pytest.mark.parametrize("prec,name,mode,est", [c for c in ALL if c[3] == align.ESTIMATE])
def test_convergence_on_the_gate_slices(prec, name, mode, est):
    res, gate, gates = solved(prec, name, mode, est), wc.device_gate(), list(wc.GATE_SLICES[name])
    err = wc.errors(res.maps, res.intensity)
    print(f"{prec} {name} mode {mode}: errors over (map, g, b) {np.array2string(err, precision=2)} gate {gate:.2e}; accepted {res.accepted.tolist()}, lam {res.damping.tolist()}, "
          f"flags {res.flags.tolist()}, (g, b) {res.intensity.tolist()}")
    assert (err[gates] <= gate).all(), (err, gate)
    assert (res.mean_best <= res.mean_first).all() and not res.flags[gates].any()
    # the masked, corrupted block does not move the result: the same call on uncorrupted targets gives the same bits
    clean = solve(model(name, prec), targets(name, prec, False), mode, est, trace=True)
    assert same(clean, res) and np.array_equal(clean.trace, res.trace, equal_nan=True)


@pytest.mark.parametrize("mode,est", wc.MODES)
def test_determinism_and_independence(mode, est):
    prec, name = "fp32", "morlet3"
    m, tg, res, w = model(name, prec), targets(name, prec), solved(prec, name, mode, est), wc.solve_weights()
    again = solve(m, tg, mode, est, trace=True)
    assert same(again, res) and np.array_equal(again.trace, res.trace)  # two runs
    assert same(solve(m, tg, mode, est), res)                           # without the trace
    for s in (0, 3):                                                    # a slice alone
        one = solve(m, tg, mode, est, sub=slice(s, s + 1), trace=True)
        assert all(np.array_equal(getattr(one, f)[0], getattr(res, f)[s], equal_nan=True) for f in FIELDS if getattr(one, f) is not None), s
        assert np.array_equal(one.trace[:, 0], res.trace[:, s]), s
    # the _dev form, on one stream and on two alternating, calls back to back without a sync; doubles as pairs of floats on the device
    img, start, rigid, gb = vc.images(), sc.start_maps(), sc.start_rigid(), wc.start_intensity(est)
    d_i, d_t, d_m = m.device_array(img.shape).copy_from(img), m.device_array(tg.shape).copy_from(tg), m.device_array(start.shape).copy_from(start)
    d_r, d_w = m.device_array((N, 8)).copy_from(rigid.view(np.float32)), m.device_array(w.shape).copy_from(w)
    d_gb = m.device_array((N, 2)).copy_from(gb) if gb is not None else None
    o = opts(mode, est, wc.ITERATIONS)
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array((N, 6)), m.device_array((N, 2)), m.device_array((N, 8)), m.device_array((N, 14)), m.device_array((wc.ITERATIONS, N, 22)) if k != 1 else None)
                    for k in range(streams + 1)]
            for d_o, d_go, d_ro, d_rep, d_tr in outs:
                _lib.check(m._lib.msiren_align_solve_w_dev(m._h, d_i.ptr, N, HW, HW, d_t.ptr, SHAPE[0], SHAPE[1], C.byref(o), d_m.ptr, d_r.ptr, d_w.ptr,
                                                           d_gb.ptr if d_gb else None, d_o.ptr, d_go.ptr, d_ro.ptr, d_rep.ptr, d_tr.ptr if d_tr else None))
            m.sync()
            for d_o, d_go, d_ro, d_rep, d_tr in outs:
                got = align.solve_result_w(d_o.numpy(), d_go.numpy(), d_ro.numpy().view(np.float64) if mode == align.RIGID else None, d_rep.numpy().view(np.float64), None)
                assert same(got, res), streams
                assert d_tr is None or np.array_equal(d_tr.numpy().view(np.float64), res.trace), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


@pytest.mark.parametrize("mode,est", wc.MODES)
def test_degenerate_slices_keep_their_inputs(mode, est):
    name = "sine5"
    m, res, gb = model(name), solved("fp32", name, mode, est), wc.start_intensity(est)
    gb = np.tile(np.array([1.0, 0.0], np.float32), (N, 1)) if gb is None else gb
    assert res.flags[sc.BLACK] == align.SINGULAR and np.array_equal(res.maps[sc.BLACK], sc.start_maps()[sc.BLACK]) and res.accepted[sc.BLACK] == 0
    assert np.array_equal(res.intensity[sc.BLACK], gb[sc.BLACK])
    w = wc.solve_weights()
    w[0] = np.resize(np.array([0.0, -1.0, np.nan, np.inf], np.float32), SHAPE)  # every pixel of slice 0 masked
    got = solve(m, targets(name), mode, est, weights=w)
    assert got.flags[0] == (align.SINGULAR | align.NO_OVERLAP) and np.array_equal(got.maps[0], sc.start_maps()[0]) and got.accepted[0] == 0
    assert np.array_equal(got.intensity[0], gb[0]) and got.mean_first[0] == np.inf and got.mean_best[0] == np.inf and got.count[0] == 0 and got.wsum[0] == 0
    assert all(np.array_equal(getattr(got, f)[1:], getattr(res, f)[1:]) for f in FIELDS if getattr(got, f) is not None)  # the other slices: untouched by it
    if est == align.ESTIMATE and mode == align.AFFINE:  # 7 valid pixels are fewer than 8 parameters: NO_OVERLAP; 6 parameters would have a mean
        w = wc.solve_weights()
        keep = np.flatnonzero(w[0].reshape(-1) > 0)[::41][:7]
        few = np.zeros(SHAPE[0] * SHAPE[1], np.float32)
        few[keep] = w[0].reshape(-1)[keep]
        w[0] = few.reshape(SHAPE)
        got = solve(m, targets(name), mode, est, weights=w)
        assert got.count[0] == 7 and got.flags[0] & align.NO_OVERLAP and got.mean_first[0] == np.inf and np.array_equal(got.maps[0], sc.start_maps()[0])
        fixed = solve(m, targets(name), mode, align.FIXED, weights=w, iterations=1)
        assert fixed.count[0] == 7 and np.isfinite(fixed.mean_first[0]) and not fixed.flags[0] & align.NO_OVERLAP


def test_refusals_launch_nothing():
    m, img, tg, start, rigid, w = model("sine5"), vc.images(), targets("sine5"), sc.start_maps(), sc.start_rigid(), wc.solve_weights()
    out, gout, rout, rep = np.full((N, 6), -7.0, np.float32), np.full((N, 2), -7.0, np.float32), np.full((N, 4), -7.0), np.full((N, 7), -7.0)
    d = m.device_array(img.shape).copy_from(img)
    m.sync()
    profile_on(m)
    try:
        def host(o, **kw):
            a = dict(images=img.ctypes.data, n=N, targets=tg.ctypes.data, th=SHAPE[0], tw=SHAPE[1], maps=start.ctypes.data, rigid=rigid.ctypes.data, w=w.ctypes.data, gb=None,
                     out=out.ctypes.data, gout=gout.ctypes.data, rep=rep.ctypes.data)
            a.update(kw)
            return m._lib.msiren_align_solve_w(m._h, a["images"], a["n"], HW, HW, a["targets"], a["th"], a["tw"], C.byref(o) if o is not None else None, a["maps"], a["rigid"],
                                               a["w"], a["gb"], a["out"], a["gout"], rout.ctypes.data, a["rep"], None)

        def dev(o, **kw):
            a = dict(images=d.ptr, n=N, targets=d.ptr, th=4, tw=4, maps=d.ptr, rigid=d.ptr, w=d.ptr, gb=d.ptr, out=d.ptr, gout=d.ptr, rout=d.ptr, rep=d.ptr, trace=None)
            a.update(kw)
            return m._lib.msiren_align_solve_w_dev(m._h, a["images"], a["n"], HW, HW, a["targets"], a["th"], a["tw"], C.byref(o) if o is not None else None, a["maps"],
                                                   a["rigid"], a["w"], a["gb"], a["out"], a["gout"], a["rout"], a["rep"], a["trace"])

        inf, nan = float("inf"), float("nan")
        bad_opts = [opts(struct_size=64), opts(struct_size=0), opts(est=2), opts(est=-1), opts(mode=2), opts(mode=-1), opts(iterations=0), opts(iterations=257),
                    opts(lam_min=0.0), opts(lam_min=1e-2), opts(lam_max=1e-4), opts(lam_max=inf), opts(damping=nan), opts(down=0.0), opts(down=1.5), opts(down=nan),
                    opts(up=0.5), opts(up=inf), opts(up=nan), opts(mode=1, centre_y=nan), opts(mode=1, centre_x=inf)]
        for o in bad_opts:
            assert host(o) == _lib.E_INVALID and _lib.last_error(), (o.mode, o.iterations, o.intensity_mode)
            assert dev(o) == _lib.E_INVALID
        assert host(opts(est=3)) == _lib.E_INVALID and "intensity_mode" in _lib.last_error()
        assert host(None) == _lib.E_INVALID and dev(None) == _lib.E_INVALID
        for mode, missing in ((0, "maps"), (1, "rigid")):  # a missing input of the mode, outputs, images, targets
            for key in (missing, "out", "gout", "rep", "images", "targets"):
                assert host(opts(mode), **{key: None}) == _lib.E_INVALID and "null" in _lib.last_error(), (mode, key)
                assert dev(opts(mode), **{key: None}) == _lib.E_INVALID, (mode, key)
        for key, off in (("targets", 2), ("maps", 2), ("out", 2), ("w", 2), ("gb", 2), ("gout", 2), ("rigid", 4), ("rout", 4), ("rep", 4), ("trace", 4)):  # misaligned
            assert dev(opts(1 if key == "rigid" else 0), **{key: d.ptr + off}) == _lib.E_INVALID and "aligned" in _lib.last_error(), key
        for n, th, tw in ((N, 1 << 12, 1 << 12), (1 << 20, 64, 64), (-1, 4, 4)):  # everything align_check refuses
            assert host(opts(), n=n, th=th, tw=tw) == _lib.E_INVALID and dev(opts(), n=n, th=th, tw=tw) == _lib.E_INVALID
        assert host(opts(), n=0) == 0 and host(opts(), th=0) == 0 and dev(opts(), tw=0) == 0 and dev(opts(), n=0) == 0  # nothing to do
        for kw in (dict(iterations=0), dict(damping=0.0), dict(up=0.9)):
            with pytest.raises(ValueError):
                solve(m, tg, 0, 1, **kw)
        with pytest.raises(ValueError):
            m.align_solve_w(img, tg, start, weights=w[:, :4])
        with pytest.raises(ValueError):
            m.align_solve_rigid_w(img, tg, np.zeros(N), np.zeros((N, 2)), (np.nan, 0.0))
        m.sync()
        assert (out == -7.0).all() and (gout == -7.0).all() and (rout == -7.0).all() and (rep == -7.0).all() and np.array_equal(d.numpy(), img) and m.profile_kernels() == []
    finally:
        profile_off(m)
    assert same(solve(m, tg, 0, 1), solved("fp32", "sine5", 0, 1))  # the handle stays usable


@pytest.mark.parametrize("name,act", [("sine5", 0), ("morlet3", 1)])
def test_profile_counts_and_the_plain_calls_are_left_alone(name, act):
    m, tg = model(name), targets(name)
    before_cost = m.align_cost(vc.images(), tg, sc.truth(), warped=True, gradient=True)
    before_solve = plain_solve(m, plain_targets(name), align.AFFINE)
    trunk = f"siren_trunk_f32_jet_ragged_kernel<256,{act}>"
    per_eval = ("align_bin_kernels", trunk, "align_reduce_w_kernels")
    profile_on(m)
    try:
        m.align_cost_w(vc.images(), tg, sc.start_maps(), weights=wc.solve_weights())
        m.sync()
        one = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
    finally:
        profile_off(m)
    assert all(one[k] == 1 for k in per_eval) and "align_step_w_kernel" not in one and "align_reduce_kernels" not in one, one
    profile_on(m)
    try:
        solve(m, tg, align.RIGID, align.ESTIMATE, iterations=5)
        m.sync()
        got = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
    finally:
        profile_off(m)
    assert got["align_step_w_kernel"] == 5 and all(got[k] == 5 for k in per_eval) and "align_step_kernel" not in got and "align_reduce_kernels" not in got, got
    prologue = {k: v for k, v in one.items() if k not in per_eval}
    assert {k: v for k, v in got.items() if k not in per_eval + ("align_step_w_kernel",)} == prologue, (got, one)
    after_cost = m.align_cost(vc.images(), tg, sc.truth(), warped=True, gradient=True)
    assert np.array_equal(packed29(before_cost), packed29(after_cost)) and np.array_equal(before_cost.warped, after_cost.warped, equal_nan=True)
    after_solve = plain_solve(m, plain_targets(name), align.AFFINE)
    assert all(np.array_equal(x, y, equal_nan=True) if x is not None else y is None for x, y in zip(before_solve[:9], after_solve[:9]))
