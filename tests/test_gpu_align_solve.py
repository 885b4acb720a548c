"""Slices aligned to their targets on the GPU: model.align_solve / align_solve_rigid, i.e. msiren_align_solve* --
msiren_align_slices' prologue once, then per evaluation bin -> jet ragged trunk -> reduce -> align_step_kernel, on one stream.  Cases:
tests/align_solve_cases.py (the targets here are the device's own warped planes at the truth: zero residual there).

The device loop is pinned bit for bit against the host loop: every traced evaluation has the (cost, count) of model.align_cost at the traced
trial map, and mri_inr_amd.align.lm_step produces the next traced trial map from that call's sums.  Convergence is gated by the CPU
variant's distance (tests/test_align_solve_reference.py asserts D <= 1e-6, so the gate is the fp32 resolution of the map entries); the
errors measured on the MI355X are in LAB_NOTES.md section 23.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import align_solve_cases as sc
import volume_cases as vc
from mri_inr_amd import _lib, align
from test_gpu_align import model, packed, profile_off, profile_on

pytestmark = pytest.mark.gpu

N, HW, SHAPE = sc.N, sc.HW, sc.SHAPE
ALL = [(prec, name, mode) for prec in ("fp32", "f16x3") for name in sc.MODELS for mode in sc.MODES]


@functools.lru_cache(maxsize=None)
def targets(name, prec="fp32"):
    return sc.targets_of(model(name, prec).align_cost(vc.images(), np.zeros((N,) + SHAPE, np.float32), sc.truth(), warped=True).warped)


def solve(m, tg, mode, images=None, sub=slice(None), **kw):
    images = vc.images() if images is None else images
    kw.setdefault("iterations", sc.ITERATIONS)
    if mode == align.RIGID:
        return m.align_solve_rigid(images[sub], tg[sub], np.zeros(N)[sub], np.tile(sc.START_SHIFT, (N, 1))[sub], sc.CENTRE, **kw)
    return m.align_solve(images[sub], tg[sub], sc.start_maps()[sub], **kw)


@functools.lru_cache(maxsize=None)
def solved(prec, name, mode):
    return solve(model(name, prec), targets(name, prec), mode, trace=True)


def same(a, b):
    """two SolveResults, bit for bit (trace aside)"""
    return all(np.array_equal(x, y, equal_nan=True) if x is not None else y is None for x, y in zip(a[:9], b[:9]))


def opts(mode=0, iterations=4, *, struct_size=None, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, centre_y=sc.CENTRE[0], centre_x=sc.CENTRE[1]):
    return _lib.AlignSolveOpts(C.sizeof(_lib.AlignSolveOpts) if struct_size is None else struct_size, mode, iterations, 0, damping, down, up, lam_min, lam_max,
                               centre_y, centre_x)


@pytest.mark.parametrize("prec,name,mode", ALL)
def test_the_device_loop_is_the_host_loop_bit_for_bit(prec, name, mode):
    m, tg, res = model(name, prec), targets(name, prec), solved(prec, name, mode)
    assert res.trace.shape == (sc.ITERATIONS, N, 8)
    sums = []
    for k in range(sc.ITERATIONS):  # every evaluation: the bits of align_cost at the traced trial map
        trial = res.trace[k, :, :6].astype(np.float32)
        assert np.array_equal(trial.astype(np.float64), res.trace[k, :, :6], equal_nan=True)
        sums.append(packed(m.align_cost(vc.images(), tg, trial)))
        assert np.array_equal(res.trace[k, :, 6], sums[k][:, 1]) and np.array_equal(res.trace[k, :, 7], sums[k][:, 0]), k
    differs, st = sc.replay(res.trace, lambda k: sums[k], mode, sc.start_maps(), sc.start_rigid())  # every step: lm_step's bits
    assert differs is None, differs
    # hence the outputs are those of solve_on_host(model.align_cost)
    rigid = np.array([x["rigid_best"] for x in st]) if mode == align.RIGID else None
    want = align.solve_result(np.array([x["best"] for x in st], np.float32), rigid,
                              np.array([[x["accepted"], x["mean_first"], x["mean_best"], x["sums"][0], x["lam"], x["flags"]] for x in st], np.float64), None)
    assert same(res, want), (res[:9], want[:9])
    host, _ = align.solve_on_host(lambda maps: packed(m.align_cost(vc.images(), tg, maps)), N, maps=sc.start_maps(), rigid=sc.start_rigid(), options=sc.options(mode))
    assert same(res, host)


@pytest.mark.parametrize("mode", sc.MODES)
def test_one_iteration_returns_the_input(mode):
    m, tg = model("sine5"), targets("sine5")
    res = solve(m, tg, mode, iterations=1)
    first = m.align_cost(vc.images(), tg, sc.start_maps())
    assert np.array_equal(res.maps, sc.start_maps()) and not res.accepted.any()
    assert np.array_equal(res.mean_first, first.cost / first.count) and np.array_equal(res.mean_best, res.mean_first) and np.array_equal(res.count, first.count)
    assert np.array_equal(res.damping, np.full(N, 1e-3)) and res.flags.tolist() == [0, 0, 0, align.SINGULAR]
    if mode == align.RIGID:
        assert np.array_equal(res.angle, np.zeros(N)) and np.array_equal(res.shift, np.tile(sc.START_SHIFT, (N, 1)))


@pytest.mark.parametrize("prec,name,mode", ALL)
def test_convergence_on_the_gate_slices(prec, name, mode):
    res, gate = solved(prec, name, mode), sc.device_gate()
    err = sc.errors(res.maps)
    print(f"{prec} {name} mode {mode}: errors {np.array2string(err, precision=2)} gate {gate:.2e}; accepted {res.accepted.tolist()}, lam {res.damping.tolist()}, "
          f"flags {res.flags.tolist()}")
    assert (err[list(sc.GATE_SLICES[name])] <= gate).all(), (err, gate)
    assert (res.mean_best <= res.mean_first).all() and not res.flags[list(sc.GATE_SLICES[name])].any()


@pytest.mark.parametrize("mode", sc.MODES)
def test_determinism_and_independence(mode):
    prec, name = "fp32", "morlet3"
    m, tg, res = model(name, prec), targets(name, prec), solved(prec, name, mode)
    again = solve(m, tg, mode, trace=True)
    assert same(again, res) and np.array_equal(again.trace, res.trace)  # two runs
    assert same(solve(m, tg, mode), res)                                # without the trace
    for s in range(N):                                                  # a slice alone
        one = solve(m, tg, mode, sub=slice(s, s + 1), trace=True)
        assert all(np.array_equal(x[0], y[s], equal_nan=True) for x, y in zip(one[:9], res[:9]) if x is not None) and np.array_equal(one.trace[:, 0], res.trace[:, s]), s
    # the _dev form, on one stream and on two alternating, calls back to back without a sync; doubles as pairs of floats on the device
    img, start, rigid = vc.images(), sc.start_maps(), sc.start_rigid()
    d_i, d_t, d_m = m.device_array(img.shape).copy_from(img), m.device_array(tg.shape).copy_from(tg), m.device_array(start.shape).copy_from(start)
    d_r = m.device_array((N, 8)).copy_from(rigid.view(np.float32))
    o = opts(mode, sc.ITERATIONS)
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array((N, 6)), m.device_array((N, 8)), m.device_array((N, 12)), m.device_array((sc.ITERATIONS, N, 16)) if k != 1 else None)
                    for k in range(streams + 1)]
            for d_o, d_ro, d_rep, d_tr in outs:
                _lib.check(m._lib.msiren_align_solve_dev(m._h, d_i.ptr, N, HW, HW, d_t.ptr, SHAPE[0], SHAPE[1], C.byref(o), d_m.ptr, d_r.ptr, d_o.ptr, d_ro.ptr, d_rep.ptr,
                                                         d_tr.ptr if d_tr else None))
            m.sync()
            for d_o, d_ro, d_rep, d_tr in outs:
                got = align.solve_result(d_o.numpy(), d_ro.numpy().view(np.float64) if mode == align.RIGID else None, d_rep.numpy().view(np.float64), None)
                assert same(got, res), streams
                assert d_tr is None or np.array_equal(d_tr.numpy().view(np.float64), res.trace), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


@pytest.mark.parametrize("mode", sc.MODES)
def test_invalid_slices_keep_their_map(mode):
    name = "sine5"
    m, res = model(name), solved("fp32", name, mode)
    assert res.flags[sc.BLACK] == align.SINGULAR and np.array_equal(res.maps[sc.BLACK], sc.start_maps()[sc.BLACK]) and res.accepted[sc.BLACK] == 0
    tg = targets(name).copy()
    tg[0] = np.nan
    got = solve(m, tg, mode)
    assert got.flags[0] == (align.SINGULAR | align.NO_OVERLAP) and np.array_equal(got.maps[0], sc.start_maps()[0]) and got.accepted[0] == 0
    assert got.mean_first[0] == np.inf and got.mean_best[0] == np.inf and got.count[0] == 0
    assert all(np.array_equal(x[1:], y[1:]) for x, y in zip(got[:9], res[:9]) if x is not None)  # the other slices: untouched by it


def test_refusals_launch_nothing():
    m, img, tg, start, rigid = model("sine5"), vc.images(), targets("sine5"), sc.start_maps(), sc.start_rigid()
    out, rout, rep = np.full((N, 6), -7.0, np.float32), np.full((N, 4), -7.0), np.full((N, 6), -7.0)
    d = m.device_array(img.shape).copy_from(img)
    m.sync()
    profile_on(m)
    try:
        def host(o, **kw):
            a = dict(images=img.ctypes.data, n=N, targets=tg.ctypes.data, th=SHAPE[0], tw=SHAPE[1], maps=start.ctypes.data, rigid=rigid.ctypes.data, out=out.ctypes.data,
                     rep=rep.ctypes.data)
            a.update(kw)
            return m._lib.msiren_align_solve(m._h, a["images"], a["n"], HW, HW, a["targets"], a["th"], a["tw"], C.byref(o) if o is not None else None, a["maps"], a["rigid"],
                                             a["out"], rout.ctypes.data, a["rep"], None)

        def dev(o, **kw):
            a = dict(images=d.ptr, n=N, targets=d.ptr, th=4, tw=4, maps=d.ptr, rigid=d.ptr, out=d.ptr, rout=d.ptr, rep=d.ptr, trace=None)
            a.update(kw)
            return m._lib.msiren_align_solve_dev(m._h, a["images"], a["n"], HW, HW, a["targets"], a["th"], a["tw"], C.byref(o) if o is not None else None, a["maps"], a["rigid"],
                                                 a["out"], a["rout"], a["rep"], a["trace"])

        inf, nan = float("inf"), float("nan")
        bad_opts = [opts(struct_size=64), opts(mode=2), opts(mode=-1), opts(iterations=0), opts(iterations=257), opts(lam_min=0.0), opts(lam_min=1e-2), opts(lam_max=1e-4),
                    opts(lam_max=inf), opts(damping=nan), opts(down=0.0), opts(down=1.5), opts(down=nan), opts(up=0.5), opts(up=inf), opts(up=nan),
                    opts(mode=1, centre_y=nan), opts(mode=1, centre_x=inf)]
        for o in bad_opts:
            assert host(o) == _lib.E_INVALID and _lib.last_error(), (o.mode, o.iterations)
            assert dev(o) == _lib.E_INVALID
        assert host(None) == _lib.E_INVALID and dev(None) == _lib.E_INVALID
        for mode, missing in ((0, "maps"), (1, "rigid")):  # a missing input of the mode, outputs, images, targets
            for key in (missing, "out", "rep", "images", "targets"):
                assert host(opts(mode), **{key: None}) == _lib.E_INVALID and "null" in _lib.last_error(), (mode, key)
                assert dev(opts(mode), **{key: None}) == _lib.E_INVALID, (mode, key)
        for key, off in (("targets", 2), ("maps", 2), ("out", 2), ("rigid", 4), ("rout", 4), ("rep", 4), ("trace", 4)):  # misaligned device pointers
            assert dev(opts(1 if key == "rigid" else 0), **{key: d.ptr + off}) == _lib.E_INVALID and "aligned" in _lib.last_error(), key
        # everything align_check refuses
        for n, th, tw in ((N, 1 << 12, 1 << 12), (1 << 20, 64, 64), (-1, 4, 4)):
            assert host(opts(), n=n, th=th, tw=tw) == _lib.E_INVALID and dev(opts(), n=n, th=th, tw=tw) == _lib.E_INVALID
        # nothing to do
        assert host(opts(), n=0) == 0 and host(opts(), th=0) == 0 and dev(opts(), tw=0) == 0 and dev(opts(), n=0) == 0
        for kw in (dict(iterations=0), dict(damping=0.0), dict(up=0.9)):
            with pytest.raises(ValueError):
                solve(m, tg, 0, **kw)
        with pytest.raises(ValueError):
            m.align_solve(img, tg, start[:, :5])
        with pytest.raises(ValueError):
            m.align_solve_rigid(img, tg, np.zeros(N), np.zeros((N, 2)), (np.nan, 0.0))
        m.sync()
        assert (out == -7.0).all() and (rout == -7.0).all() and (rep == -7.0).all() and np.array_equal(d.numpy(), img) and m.profile_kernels() == []
    finally:
        profile_off(m)
    assert same(solve(m, tg, 0), solved("fp32", "sine5", 0))  # the handle stays usable


@pytest.mark.parametrize("name,act", [("sine5", 0), ("morlet3", 1)])
def test_profile_counts(name, act):
    m, tg = model(name), targets(name)
    trunk = f"siren_trunk_f32_jet_ragged_kernel<256,{act}>"
    per_eval = ("align_bin_kernels", trunk, "align_reduce_kernels")
    profile_on(m)
    try:
        m.align_cost(vc.images(), tg, sc.start_maps())
        m.sync()
        one = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
    finally:
        profile_off(m)
    assert all(one[k] == 1 for k in per_eval) and "align_step_kernel" not in one, one
    profile_on(m)
    try:
        solve(m, tg, align.AFFINE, iterations=5)
        m.sync()
        got = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
    finally:
        profile_off(m)
    assert got["align_step_kernel"] == 5 and all(got[k] == 5 for k in per_eval), got
    prologue = {k: v for k, v in one.items() if k not in per_eval}
    assert {k: v for k, v in got.items() if k not in per_eval + ("align_step_kernel",)} == prologue, (got, one)


def test_a_solve_leaves_align_cost_alone():
    m, tg = model("sine5"), targets("sine5")
    before = m.align_cost(vc.images(), tg, sc.truth(), warped=True, gradient=True)
    solve(m, tg, align.RIGID)
    after = m.align_cost(vc.images(), tg, sc.truth(), warped=True, gradient=True)
    assert np.array_equal(packed(before), packed(after)) and np.array_equal(before.warped, after.warped, equal_nan=True) and np.array_equal(before.wgrad, after.wgrad, equal_nan=True)
