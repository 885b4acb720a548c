"""Target slices aligned to the stack read as a volume on the GPU: model.align_volume_solve / align_volume_solve_rigid,
i.e. msiren_align_volume_solve* -- msiren_align_volume's prologue once, then per evaluation bin -> jet ragged trunk -> reduce ->
align_volume_step_kernel of the mode, on one stream.  Cases: tests/align_volume_cases.py (the targets here are the device's own warped planes at
the truth: zero residual there).

The device loop is pinned bit for bit against the host loop: every traced evaluation has the (cost, count) of model.align_volume_cost at the
traced trial map, and mri_inr_amd.align_volume.lm_step_v produces the next traced trial map from that call's sums.  Convergence is gated by the CPU
variant's distance (tests/test_align_volume_reference.py asserts D_solve <= 1e-6, so the gate is the fp32 resolution of the map entries); the
errors measured on the MI355X are in LAB_NOTES.md section 25.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import align_cases as ac
import align_volume_cases as avc
import volume_cases as vc
from mri_inr_amd import _lib, align, align_volume as av
from test_gpu_align import model, packed as packed2, profile_off, profile_on
from test_gpu_align_volume import packed

pytestmark = pytest.mark.gpu

N, HW, SHAPE, M, IT = avc.N, avc.HW, avc.SOLVE_SHAPE, avc.SOLVE_M, avc.SOLVE_ITERATIONS
ALL = [(prec, name, mode) for prec in ("fp32", "f16x3") for name in avc.MODELS for mode in avc.MODES]


@functools.lru_cache(maxsize=None)
def targets(name, prec="fp32"):
    return model(name, prec).align_volume_cost(vc.images(), np.zeros((M,) + SHAPE, np.float32), avc.truth(), warped=True).warped.copy()


def solve(m, tg, mode, images=None, sub=slice(None), planes=None, start=None, **kw):
    images = vc.images() if images is None else images
    kw.setdefault("iterations", IT)
    if mode == align.RIGID:
        return m.align_volume_solve_rigid(images, tg[sub], (avc.planes() if planes is None else planes)[sub], avc.SPACING, **kw)
    return m.align_volume_solve(images, tg[sub], (avc.start_maps() if start is None else start)[sub], **kw)


@functools.lru_cache(maxsize=None)
def solved(prec, name, mode):
    return solve(model(name, prec), targets(name, prec), mode, trace=True)


def same(a, b):
    """two SolveResultVs, bit for bit (trace aside)"""
    return all(np.array_equal(x, y, equal_nan=True) if x is not None else y is None for x, y in zip(a[:9], b[:9]))


def opts(mode=0, iterations=4, *, struct_size=None, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, spacing=avc.SPACING):
    return _lib.AlignVolumeSolveOpts(C.sizeof(_lib.AlignVolumeSolveOpts) if struct_size is None else struct_size, mode, iterations, 0, damping, down, up, lam_min,
                                     lam_max, spacing)


@pytest.mark.parametrize("prec,name,mode", ALL)
def test_the_device_loop_is_the_host_loop_bit_for_bit(prec, name, mode):
    m, tg, res = model(name, prec), targets(name, prec), solved(prec, name, mode)
    assert res.trace.shape == (IT, M, 11)
    sums = []
    for k in range(IT):  # every evaluation: the bits of align_volume_cost at the traced trial map
        trial = res.trace[k, :, :9].astype(np.float32)
        assert np.array_equal(trial.astype(np.float64), res.trace[k, :, :9], equal_nan=True)
        sums.append(packed(m.align_volume_cost(vc.images(), tg, trial)))
        assert np.array_equal(res.trace[k, :, 9], sums[k][:, 1]) and np.array_equal(res.trace[k, :, 10], sums[k][:, 0]), k
    differs, st = avc.replay(res.trace, lambda k: sums[k], mode, avc.start_maps(), avc.start_rigid(), avc.planes())  # every step: lm_step_v's bits
    assert differs is None, differs
    # hence the outputs are those of solve_on_host_v(model.align_volume_cost)
    rigid = np.array([x["rigid_best"] for x in st]) if mode == align.RIGID else None
    want = av.solve_result_v(np.array([x["best"] for x in st], np.float32), rigid,
                             np.array([[x["accepted"], x["mean_first"], x["mean_best"], x["sums"][0], x["lam"], x["flags"]] for x in st], np.float64), None)
    assert same(res, want), (res[:9], want[:9])
    host, _ = av.solve_on_host_v(lambda maps: packed(m.align_volume_cost(vc.images(), tg, maps)), M, maps=avc.start_maps(), rigid=avc.start_rigid(),
                                 planes=avc.planes(), options=avc.solve_options(mode))
    assert same(res, host)


@pytest.mark.parametrize("mode", avc.MODES)
def test_one_iteration_returns_the_input(mode):
    m, tg = model("sine5"), targets("sine5")
    res = solve(m, tg, mode, iterations=1)
    first = m.align_volume_cost(vc.images(), tg, avc.start_maps())
    assert np.array_equal(res.maps, avc.start_maps()) and not res.accepted.any()
    assert np.array_equal(res.mean_first, first.cost / first.count) and np.array_equal(res.mean_best, res.mean_first) and np.array_equal(res.count, first.count)
    assert np.array_equal(res.damping, np.full(M, 1e-3)) and not res.flags.any()
    if mode == align.RIGID:
        assert np.array_equal(res.rotation, np.tile(np.eye(3), (M, 1, 1))) and not res.shift.any()


@pytest.mark.parametrize("prec,name,mode", ALL)
def test_convergence_on_the_gate_targets(prec, name, mode):
    res, gate = solved(prec, name, mode), avc.device_solve_gate()
    err = avc.solve_errors(res.maps)
    print(f"{prec} {name} mode {mode}: errors {np.array2string(err, precision=2)} gate {gate:.2e}; accepted {res.accepted.tolist()}, lam {res.damping.tolist()}, "
          f"flags {res.flags.tolist()}")
    assert (err[list(avc.GATE_TARGETS[name])] <= gate).all(), (err, gate)
    assert (res.mean_best <= res.mean_first).all() and not res.flags[list(avc.GATE_TARGETS[name])].any()


@pytest.mark.parametrize("mode", avc.MODES)
def test_determinism_and_independence(mode):
    prec, name = "fp32", "morlet3"
    m, tg, res = model(name, prec), targets(name, prec), solved(prec, name, mode)
    again = solve(m, tg, mode, trace=True)
    assert same(again, res) and np.array_equal(again.trace, res.trace)  # two runs
    assert same(solve(m, tg, mode), res)                                # without the trace
    for q in range(M):                                                  # a target alone
        one = solve(m, tg, mode, sub=slice(q, q + 1), trace=True)
        assert all(np.array_equal(x[0], y[q], equal_nan=True) for x, y in zip(one[:9], res[:9]) if x is not None) and np.array_equal(one.trace[:, 0], res.trace[:, q]), q
    # the _dev form against the host form, on one stream and on two alternating, calls back to back without a sync; doubles as pairs of floats
    img, start, rigid, pl = vc.images(), avc.start_maps(), avc.start_rigid(), avc.planes()
    d_i, d_t, d_m = m.device_array(img.shape).copy_from(img), m.device_array(tg.shape).copy_from(tg), m.device_array(start.shape).copy_from(start)
    d_r, d_p = m.device_array((M, 24)).copy_from(rigid.view(np.float32)), m.device_array((M, 24)).copy_from(pl.view(np.float32))
    o = opts(mode, IT)
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array((M, 9)), m.device_array((M, 24)), m.device_array((M, 12)), m.device_array((IT, M, 22)) if k != 1 else None) for k in range(streams + 1)]
            for d_o, d_ro, d_rep, d_tr in outs:
                _lib.check(m._lib.msiren_align_volume_solve_dev(m._h, d_i.ptr, N, HW, HW, d_t.ptr, M, SHAPE[0], SHAPE[1], C.byref(o), d_m.ptr, d_p.ptr, d_r.ptr, d_o.ptr,
                                                                d_ro.ptr, d_rep.ptr, d_tr.ptr if d_tr else None))
            m.sync()
            for d_o, d_ro, d_rep, d_tr in outs:
                got = av.solve_result_v(d_o.numpy(), d_ro.numpy().view(np.float64) if mode == align.RIGID else None, d_rep.numpy().view(np.float64), None)
                assert same(got, res), streams
                assert d_tr is None or np.array_equal(d_tr.numpy().view(np.float64), res.trace), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


@pytest.mark.parametrize("mode", avc.MODES)
def test_invalid_targets_keep_their_inputs(mode):
    """target 0 moved onto a plane between two black slices (H = 0: SINGULAR), target 1 wholly below Z = 0 (no valid pixel: NO_OVERLAP); the others
    are untouched by them"""
    name = "sine5"
    m, res = model(name), solved("fp32", name, mode)
    img = vc.images().copy()
    img[2] = 0.0  # slices 2 and 3 black
    pl = avc.planes().copy()
    pl[0, [6, 9]] = avc.SPACING * 2.5   # o and c of target 0: Z = 2.5
    pl[1, [6, 9]] = avc.SPACING * -5.0  # target 1: Z = -5
    start = av.rigid_maps3(np.eye(3), np.zeros(3), pl, avc.SPACING)
    tg = targets(name)
    ref = solve(m, tg, mode, images=img, trace=True)  # targets 2 and 3 on this stack, in their usual places
    got = solve(m, tg, mode, images=img, planes=pl, start=start)
    assert got.flags[0] == align.SINGULAR and np.array_equal(got.maps[0], start[0]) and got.accepted[0] == 0 and np.isfinite(got.mean_first[0])
    assert got.count[0] == SHAPE[0] * SHAPE[1]
    assert got.flags[1] == (align.SINGULAR | align.NO_OVERLAP) and np.array_equal(got.maps[1], start[1]) and got.accepted[1] == 0
    assert got.mean_first[1] == np.inf and got.mean_best[1] == np.inf and got.count[1] == 0
    if mode == align.RIGID:
        assert np.array_equal(got.rotation[:2], np.tile(np.eye(3), (2, 1, 1))) and not got.shift[:2].any()
    assert all(np.array_equal(x[2:], y[2:]) for x, y in zip(got[:9], ref[:9]) if x is not None)
    assert res.flags[list(avc.GATE_TARGETS[name])].tolist() == [0] * len(avc.GATE_TARGETS[name])


def test_refusals_launch_nothing():
    m, img, tg, start, rigid, pl = model("sine5"), vc.images(), targets("sine5"), avc.start_maps(), avc.start_rigid(), avc.planes()
    out, rout, rep = np.full((M, 9), -7.0, np.float32), np.full((M, 12), -7.0), np.full((M, 6), -7.0)
    d = m.device_array(img.shape).copy_from(img)
    m.sync()
    profile_on(m)
    try:
        def host(o, **kw):
            a = dict(images=img.ctypes.data, n=N, targets=tg.ctypes.data, m=M, th=SHAPE[0], tw=SHAPE[1], maps=start.ctypes.data, planes=pl.ctypes.data,
                     rigid=rigid.ctypes.data, out=out.ctypes.data, rep=rep.ctypes.data)
            a.update(kw)
            return m._lib.msiren_align_volume_solve(m._h, a["images"], a["n"], HW, HW, a["targets"], a["m"], a["th"], a["tw"], C.byref(o) if o is not None else None,
                                                    a["maps"], a["planes"], a["rigid"], a["out"], rout.ctypes.data, a["rep"], None)

        def dev(o, **kw):
            a = dict(images=d.ptr, n=N, targets=d.ptr, m=2, th=4, tw=4, maps=d.ptr, planes=d.ptr, rigid=d.ptr, out=d.ptr, rout=d.ptr, rep=d.ptr, trace=None)
            a.update(kw)
            return m._lib.msiren_align_volume_solve_dev(m._h, a["images"], a["n"], HW, HW, a["targets"], a["m"], a["th"], a["tw"], C.byref(o) if o is not None else None,
                                                        a["maps"], a["planes"], a["rigid"], a["out"], a["rout"], a["rep"], a["trace"])

        inf, nan = float("inf"), float("nan")
        bad_opts = [opts(struct_size=72), opts(mode=2), opts(mode=-1), opts(iterations=0), opts(iterations=257), opts(lam_min=0.0), opts(lam_min=1e-2), opts(lam_max=1e-4),
                    opts(lam_max=inf), opts(damping=nan), opts(down=0.0), opts(down=1.5), opts(down=nan), opts(up=0.5), opts(up=inf), opts(up=nan),
                    opts(mode=1, spacing=0.0), opts(mode=1, spacing=-1.0), opts(mode=1, spacing=inf), opts(mode=1, spacing=nan)]
        for o in bad_opts:
            assert host(o) == _lib.E_INVALID and _lib.last_error(), (o.mode, o.iterations)
            assert dev(o) == _lib.E_INVALID
        assert host(None) == _lib.E_INVALID and dev(None) == _lib.E_INVALID
        for mode, missing in ((0, ("maps",)), (1, ("rigid", "planes"))):  # a missing input of the mode, outputs, images, targets
            for key in missing + ("out", "rep", "images", "targets"):
                assert host(opts(mode), **{key: None}) == _lib.E_INVALID and "null" in _lib.last_error(), (mode, key)
                assert dev(opts(mode), **{key: None}) == _lib.E_INVALID, (mode, key)
        for key, off in (("targets", 2), ("maps", 2), ("out", 2), ("rigid", 4), ("planes", 4), ("rout", 4), ("rep", 4), ("trace", 4)):  # misaligned device pointers
            assert dev(opts(1 if key in ("rigid", "planes") else 0), **{key: d.ptr + off}) == _lib.E_INVALID and "aligned" in _lib.last_error(), key
        # everything msiren_align_volume refuses
        for kw in (dict(th=1 << 12, tw=1 << 12), dict(m=1 << 20, th=64, tw=64), dict(m=-1), dict(n=1), dict(n=1 << 25)):
            assert host(opts(), **kw) == _lib.E_INVALID and dev(opts(), **kw) == _lib.E_INVALID, kw
        # nothing to do
        assert host(opts(), m=0) == 0 and host(opts(), th=0) == 0 and dev(opts(), tw=0) == 0 and dev(opts(), m=0) == 0
        for kw in (dict(iterations=0), dict(damping=0.0), dict(up=0.9)):
            with pytest.raises(ValueError):
                solve(m, tg, 0, **kw)
        with pytest.raises(ValueError):
            m.align_volume_solve(img, tg, start[:, :6])
        with pytest.raises(ValueError):
            m.align_volume_solve_rigid(img, tg, pl, 0.0)
        with pytest.raises(ValueError):
            m.align_volume_solve_rigid(img, tg, pl[:2], avc.SPACING)
        m.sync()
        assert (out == -7.0).all() and (rout == -7.0).all() and (rep == -7.0).all() and np.array_equal(d.numpy(), img) and m.profile_kernels() == []
    finally:
        profile_off(m)
    assert same(solve(m, tg, 0), solved("fp32", "sine5", 0))  # the handle stays usable


@pytest.mark.parametrize("name,act", [("sine5", 0), ("morlet3", 1)])
def test_profile_counts(name, act):
    m, tg = model(name), targets(name)
    trunk = f"siren_trunk_f32_jet_ragged_kernel<256,{act}>"
    per_eval = ("align_volume_bin_kernels", trunk, "align_volume_reduce_kernels")
    profile_on(m)
    try:
        m.align_volume_cost(vc.images(), tg, avc.start_maps())
        m.sync()
        one = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
    finally:
        profile_off(m)
    assert all(one[k] == 1 for k in per_eval) and "align_volume_step_kernel" not in one, one
    for mode in avc.MODES:
        profile_on(m)
        try:
            solve(m, tg, mode, iterations=5)
            m.sync()
            got = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
        finally:
            profile_off(m)
        assert got["align_volume_step_kernel"] == 5 and all(got[k] == 5 for k in per_eval), got
        prologue = {k: v for k, v in one.items() if k not in per_eval}
        assert {k: v for k, v in got.items() if k not in per_eval + ("align_volume_step_kernel",)} == prologue, (got, one)


def test_a_solve_leaves_the_other_calls_alone():
    name, shape = "sine5", (19, 23)
    m, tg, img = model(name), targets(name), vc.images()
    pts = av.map_points3(avc.truth()[2], SHAPE)

    def others():
        two = m.align_cost(img, ac.targets(shape), ac.maps(shape), warped=True, gradient=True)
        three = m.align_volume_cost(img, tg, avc.truth(), warped=True, gradient=True)
        val, grad = m.resample_volume_with_gradient(img, pts)
        s2 = m.align_solve(img, ac.targets(shape), ac.maps(shape), iterations=3)
        return packed2(two), two.warped, two.wgrad, packed(three), three.warped, three.wgrad, val, grad, s2.maps, s2.mean_best

    before = others()
    solve(m, tg, align.RIGID)
    solve(m, tg, align.AFFINE)
    after = others()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, after))
