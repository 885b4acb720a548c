"""Groups of target slices aligned to the stack read as a volume under one shared rigid motion per group, on the GPU:
model.align_volume_solve_group, i.e. msiren_align_volume_solve_group* -- msiren_align_volume_w's prologue once, then per evaluation bin -> jet
ragged trunk -> the 80-sum reduce -> the grouped step stage (decide, project, step, apply), on one stream.  Cases: tests/align_group_cases.py (the
targets here are g_t W + b_t of the device's own warped planes W at the truth, corrupted inside the block the weights mask).

The device loop is pinned bit for bit against the host loop (align_group.solve_on_host_g around model.align_volume_cost_w) in both intensity modes,
trace included; all-singleton groups with the intensity fixed return align_volume_solve_rigid_w's bits.  Convergence is gated by the CPU variant's
distance (tests/test_align_group_reference.py asserts D_solve <= 1e-6, so the gate is the fp32 resolution of the parameters)."""
import ctypes as C
import functools

import numpy as np
import pytest

import align_group_cases as gc
import align_volume_cases as avc
import volume_cases as vc
from mri_inr_amd import _lib, align, align_group as ag, align_volume as av
from test_gpu_align import model, profile_off, profile_on

pytestmark = pytest.mark.gpu

N, HW, SHAPE, M, G, IT = gc.N, gc.HW, gc.SHAPE, gc.M, gc.G, gc.ITERATIONS
ALL = [(prec, name, est) for prec in ("fp32", "f16x3") for name in gc.MODELS for est in gc.MODES]
packed = gc.wc.packed


@functools.lru_cache(maxsize=None)
def targets(name, prec="fp32", corrupted=True):
    warped = model(name, prec).align_volume_cost(vc.images(), np.zeros((M,) + SHAPE, np.float32), gc.truth(), warped=True).warped
    return gc.targets_of(warped, corrupted)


def solve(m, tg, est, rows=slice(None), groups=None, images=None, planes=None, rigid=None, weights="case", intensity="case", **kw):
    """the targets ``rows`` of the case as ``groups`` (None: the case's three)"""
    kw.setdefault("iterations", IT)
    w = gc.weights() if isinstance(weights, str) else weights
    gb = gc.start_intensity(est) if isinstance(intensity, str) else intensity
    pl = (gc.planes() if planes is None else planes)[rows]
    if rigid is not None:
        kw.update(rotation=rigid[:, :9].reshape(-1, 3, 3), shift=rigid[:, 9:])
    return m.align_volume_solve_group(vc.images() if images is None else images, tg[rows], pl, gc.SPACING, gc.GROUP_START if groups is None else groups,
                                      weights=None if w is None else w[rows], intensity=None if gb is None else gb[rows], estimate_intensity=est == av.ESTIMATE, **kw)


@functools.lru_cache(maxsize=None)
def solved(prec, name, est):
    return solve(model(name, prec), targets(name, prec), est, trace=True)


def same(a, b, targets_=slice(None), groups=slice(None), other_targets=slice(None), other_groups=slice(None)):
    """two SolveResultGs, bit for bit (trace aside); with rows: those targets / groups of ``a`` against those of ``b``"""
    return (all(np.array_equal(x[targets_], y[other_targets], equal_nan=True) for x, y in zip(a[:5], b[:5])) and
            all(np.array_equal(x[groups], y[other_groups], equal_nan=True) for x, y in zip(a[5:12], b[5:12])))


def opts(iterations=4, est=1, *, struct_size=None, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, spacing=gc.SPACING):
    return _lib.AlignVolumeSolveGroupOpts(C.sizeof(_lib.AlignVolumeSolveGroupOpts) if struct_size is None else struct_size, iterations, est, 0, damping, down, up, lam_min,
                                          lam_max, spacing)


@pytest.mark.parametrize("prec,name,est", ALL)
def test_the_device_loop_is_the_host_loop_bit_for_bit(prec, name, est):
    m, tg, w, res = model(name, prec), targets(name, prec), gc.weights(), solved(prec, name, est)
    assert res.trace.shape == (IT, G, 15)
    host, _ = ag.solve_on_host_g(lambda maps, gb: packed(m.align_volume_cost_w(vc.images(), tg, maps, weights=w, intensity=gb)), gc.GROUP_START, rigid=gc.start_rigid(),
                                 planes=gc.planes(), intensity=gc.start_intensity(est), options=gc.options(est), trace=True)
    assert same(res, host), (res[:12], host[:12])
    assert np.array_equal(res.trace, host.trace)
    assert (res.accepted >= 3).all() and (res.trace[1:, :, :12] != res.trace[:1, :, :12]).any()
    if est == av.FIXED:
        assert np.array_equal(res.intensity, gc.GB_TRUTH)
    else:
        assert not np.array_equal(res.intensity[:gc.OUTSIDE], np.tile(np.array([1.0, 0.0], np.float32), (gc.OUTSIDE, 1)))


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", list(gc.MODELS))
def test_singleton_groups_with_fixed_intensity_are_align_volume_solve_rigid_w(prec, name):
    m, tg = model(name, prec), targets(name, prec)
    new = solve(m, tg, av.FIXED, groups=np.arange(M + 1), trace=True)
    old = m.align_volume_solve_rigid_w(vc.images(), tg, gc.planes(), gc.SPACING, weights=gc.weights(), intensity=gc.GB_TRUTH, estimate_intensity=False, iterations=IT, trace=True)
    for key in ("maps", "rotation", "shift", "accepted", "mean_first", "mean_best", "count", "wsum", "damping", "flags", "intensity"):
        assert np.array_equal(getattr(new, key), getattr(old, key), equal_nan=True), key
    assert np.array_equal(new.trace[:, :, 12], old.trace[:, :, 11]) and np.array_equal(new.trace[:, :, 13], old.trace[:, :, 12]) and np.array_equal(new.trace[:, :, 14], old.trace[:, :, 13])
    assert old.accepted[:gc.OUTSIDE].sum() >= 2 * gc.OUTSIDE and old.flags[gc.OUTSIDE] == (align.SINGULAR | align.NO_OVERLAP)


def dev_call(model_, d, o, group_start, n_groups, **kw):
    """msiren_align_volume_solve_group_dev on the device buffers ``d`` (a dict), some replaced or left out by ``kw``"""
    a = dict(d)
    a.update(kw)
    gs = None if group_start is None else np.ascontiguousarray(group_start, np.int32)
    p = lambda x: None if x is None else x if isinstance(x, int) else x.ptr  # noqa: E731
    return model_._lib.msiren_align_volume_solve_group_dev(model_._h, p(a["images"]), a.get("n", N), HW, HW, p(a["targets"]), a.get("m", M), a.get("th", SHAPE[0]), a.get("tw", SHAPE[1]),
                                                      C.byref(o) if o is not None else None, None if gs is None else gs.ctypes.data, n_groups, p(a["planes"]), p(a["rigid"]),
                                                      p(a["weights"]), p(a["gb"]), p(a["out"]), p(a["gout"]), p(a["rout"]), p(a["rep"]), p(a["trep"]), p(a["trace"]))


def dev_buffers(m, tg, est, with_optional=True):
    img, rigid, pl, w, gb = vc.images(), gc.start_rigid(), gc.planes(), gc.weights(), gc.start_intensity(est)
    d = dict(images=m.device_array(img.shape).copy_from(img), targets=m.device_array(tg.shape).copy_from(tg), planes=m.device_array((M, 24)).copy_from(pl.view(np.float32)),
             rigid=m.device_array((G, 24)).copy_from(rigid.view(np.float32)), weights=m.device_array(w.shape).copy_from(w),
             gb=None if gb is None else m.device_array(gb.shape).copy_from(gb))
    d.update(outputs(m, with_optional))
    return d


def outputs(m, with_optional=True):
    return dict(out=m.device_array((M, 9)), gout=m.device_array((M, 2)), rep=m.device_array((G, 14)), rout=m.device_array((G, 24)) if with_optional else None,
                trep=m.device_array((M, 6)) if with_optional else None, trace=m.device_array((IT, G, 30)) if with_optional else None)


def dev_result(d):
    f64 = lambda x: x.numpy().view(np.float64)  # noqa: E731
    rout, trep = d["rout"], d["trep"]
    return (d["out"].numpy(), d["gout"].numpy(), f64(d["rep"]), None if rout is None else f64(rout), None if trep is None else f64(trep),
            None if d["trace"] is None else f64(d["trace"]))


@pytest.mark.parametrize("est", gc.MODES)
def test_determinism_and_independence(est):
    prec, name = "fp32", "morlet3"
    m, tg, res = model(name, prec), targets(name, prec), solved(prec, name, est)
    again = solve(m, tg, est, trace=True)
    assert same(again, res) and np.array_equal(again.trace, res.trace)  # two runs
    assert same(solve(m, tg, est), res)                                 # without the trace
    for y in range(G):                                                  # a group alone
        lo, hi = gc.GROUP_START[y], gc.GROUP_START[y + 1]
        one = solve(m, tg, est, rows=slice(lo, hi), groups=[0, hi - lo], trace=True)
        assert same(one, res, other_targets=slice(lo, hi), other_groups=slice(y, y + 1)), y
        assert np.array_equal(one.trace[:, 0], res.trace[:, y]), y
    # inside another batch: the groups in the order 2, 0, 1, and group 0 twice
    order = [4, 5, 0, 1, 2, 3]
    other = solve(m, tg, est, rows=order, groups=[0, 2, 5, 6], trace=True)
    for y, (at, lo, hi) in enumerate([(2, 0, 2), (0, 2, 5), (1, 5, 6)]):
        assert same(other, res, slice(lo, hi), slice(y, y + 1), slice(gc.GROUP_START[at], gc.GROUP_START[at + 1]), slice(at, at + 1)), at
        assert np.array_equal(other.trace[:, y], res.trace[:, at])
    twice = solve(m, tg, est, rows=[0, 1, 2, 0, 1, 2], groups=[3, 3])
    assert same(twice, res, slice(0, 3), slice(0, 1), slice(0, 3), slice(0, 1)) and same(twice, res, slice(3, 6), slice(1, 2), slice(0, 3), slice(0, 1))
    # the _dev form against the host form, on one stream and on two alternating, calls back to back without a sync, with and without the optional outputs
    o = opts(IT, est)
    d = dev_buffers(m, tg, est)
    report = np.stack([res.accepted, res.mean_first, res.mean_best, np.zeros(G), np.zeros(G), res.damping, res.flags], axis=1).astype(np.float64)
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [outputs(m, k != 1) for k in range(streams + 1)]
            for x in outs:
                _lib.check(dev_call(m, d, o, gc.GROUP_START, G, **x))
            m.sync()
            for x in outs:
                out, gout, rep, rout, trep, tr = dev_result(x)
                assert np.array_equal(out, res.maps) and np.array_equal(gout, res.intensity), streams
                assert np.array_equal(rep[:, [0, 1, 2, 5, 6]], report[:, [0, 1, 2, 5, 6]]), streams
                for y in range(G):  # C and W at the best state: the members' counts and weights added in ascending order
                    mem = slice(gc.GROUP_START[y], gc.GROUP_START[y + 1])
                    assert rep[y, 3] == res.count[mem].sum() and rep[y, 4] == ag.group_sum([float(v) for v in res.wsum[mem]]), (streams, y)
                if rout is not None:
                    assert np.array_equal(rout[:, :9].reshape(G, 3, 3), res.rotation) and np.array_equal(rout[:, 9:], res.shift), streams
                    assert np.array_equal(trep, np.stack([res.count.astype(np.float64), res.wsum, res.cost], axis=1)) and np.array_equal(tr, res.trace), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


@pytest.mark.parametrize("est", gc.MODES)
def test_one_iteration_returns_the_input(est):
    m, tg, w = model("sine5"), targets("sine5"), gc.weights()
    gb = np.array([[1.5, -0.25], [0.75, 0.5], [1.0, 0.0], [2.0, 1.0], [0.5, 0.5], [1.25, 0.0]], np.float32)
    rigid = np.concatenate([gc.truth_rotations().reshape(G, 9)[::-1], gc.SHIFTS3], axis=1)
    res = solve(m, tg, est, rigid=rigid, intensity=gb, iterations=1, trace=True)
    start = gc.maps_of(rigid)
    first = m.align_volume_cost_w(vc.images(), tg, start, weights=w, intensity=gb)
    assert np.array_equal(res.maps, start) and np.array_equal(res.intensity, gb) and not res.accepted.any()
    assert np.array_equal(res.rotation.reshape(G, 9), rigid[:, :9]) and np.array_equal(res.shift, rigid[:, 9:])
    assert np.array_equal(res.count, first.count) and np.array_equal(res.wsum, first.wsum) and np.array_equal(res.cost, first.cost)
    E = [ag.group_sum([float(v) for v in first.cost[gc.GROUP_START[y]:gc.GROUP_START[y + 1]]]) for y in range(G)]
    W = [ag.group_sum([float(v) for v in first.wsum[gc.GROUP_START[y]:gc.GROUP_START[y + 1]]]) for y in range(G)]
    assert np.array_equal(res.mean_first, np.array(E) / np.array(W)) and np.array_equal(res.mean_best, res.mean_first)
    assert np.array_equal(res.damping, np.full(G, 1e-3)) and not res.flags.any()
    assert np.array_equal(res.trace[0, :, :12], rigid) and np.array_equal(res.trace[0, :, 12], np.array(E)) and np.array_equal(res.trace[0, :, 14], np.array(W))


@pytest.mark.parametrize("prec,name,est", ALL)
def test_convergence_on_the_gate_groups_and_the_member_outside_is_placed(prec, name, est):
    res, gate, rows = solved(prec, name, est), gc.device_solve_gate(), list(gc.GATE_GROUPS)
    err = gc.errors(res, est)
    q = gc.OUTSIDE
    placed = np.abs(res.maps[q].astype(np.float64) - gc.truth()[q].astype(np.float64)).max()
    print(f"{prec} {name} intensity {est}: errors per group {np.array2string(err, precision=2)} gate {gate:.2e}; the member outside ends {placed:.2e} from its true map; "
          f"accepted {res.accepted.tolist()}, lam {res.damping.tolist()}, flags {res.flags.tolist()}, (g, b) {res.intensity.tolist()}")
    assert (err[rows] <= gate).all(), (err, gate)
    assert (res.mean_best <= res.mean_first).all() and not res.flags.any()
    inside = [t for t in range(M) if t != q]
    assert (res.count[inside] == SHAPE[0] * SHAPE[1] - 24).all() and (res.wsum[inside] < res.count[inside]).all()  # the corrupted block never counts
    # the member that never saw the volume: reported with count 0, placed by the other member of its group
    assert res.count[q] == 0 and res.wsum[q] == 0 and res.cost[q] == 0 and placed <= gate
    assert np.abs(gc.start_maps()[q].astype(np.float64) - gc.truth()[q].astype(np.float64)).max() > 0.1
    assert np.array_equal(res.intensity[q], np.array([1.0, 0.0], np.float32) if est == av.ESTIMATE else gc.GB_TRUTH[q])


@pytest.mark.parametrize("est", gc.MODES)
def test_a_group_wholly_outside_keeps_its_inputs_with_both_flags(est):
    name = "sine5"
    m, tg = model(name), targets(name)
    pl = gc.planes().copy()
    pl[4:6, 6] = [-1.0 * gc.SPACING, -1.5 * gc.SPACING]  # group 2: both planes below the stack
    rigid = gc.start_rigid()
    rigid[2] = np.concatenate([avc.rotation_of(np.deg2rad([0.5, -0.25, 0.75])).ravel(), [0.1, -0.2, 0.3]])
    gb = np.array([[1.5, -0.25], [0.75, 0.5], [1.0, 0.0], [0.9, 0.1], [1.5, -0.25], [0.75, 0.5]], np.float32)
    got = solve(m, tg, est, planes=pl, rigid=rigid, intensity=gb, trace=True)
    ref = solve(m, tg, est, rows=slice(0, 4), groups=[0, 3, 4], rigid=rigid[:2], intensity=gb, trace=True)  # groups 0 and 1 without it
    assert got.flags[2] == (align.SINGULAR | align.NO_OVERLAP) and got.accepted[2] == 0 and got.mean_first[2] == np.inf and got.mean_best[2] == np.inf
    assert np.array_equal(got.rotation[2].ravel(), rigid[2, :9]) and np.array_equal(got.shift[2], rigid[2, 9:]) and np.array_equal(got.intensity[4:], gb[4:])
    assert np.array_equal(got.maps[4:], np.array([av.rigid_map3(rigid[2].tolist(), p.tolist(), gc.SPACING) for p in pl[4:]], np.float32))
    assert not got.count[4:].any() and not got.wsum[4:].any() and np.array_equal(got.trace[:, 2, :12], np.tile(rigid[2], (IT, 1))) and not got.trace[:, 2, 12:].any()
    assert same(got, ref, slice(0, 4), slice(0, 2)) and np.array_equal(got.trace[:, :2], ref.trace)


def test_refusals_launch_nothing():
    m, img, tg, rigid, pl, w = model("sine5"), vc.images(), targets("sine5"), gc.start_rigid(), gc.planes(), gc.weights()
    out, gout, rout, rep = np.full((M, 9), -7.0, np.float32), np.full((M, 2), -7.0, np.float32), np.full((G, 12), -7.0), np.full((G, 7), -7.0)
    trep = np.full((M, 3), -7.0)
    dimg = m.device_array(img.shape).copy_from(img)
    d = dict(images=dimg, targets=dimg, planes=dimg, rigid=dimg, weights=dimg, gb=dimg, out=dimg, gout=dimg, rout=dimg, rep=dimg, trep=dimg, trace=None, m=2, th=4, tw=4)
    m.sync()
    profile_on(m)
    try:
        def host(o, gs=gc.GROUP_START, ng=G, **kw):
            a = dict(images=img.ctypes.data, n=N, targets=tg.ctypes.data, m=M, th=SHAPE[0], tw=SHAPE[1], planes=pl.ctypes.data, rigid=rigid.ctypes.data, weights=w.ctypes.data,
                     gb=None, out=out.ctypes.data, gout=gout.ctypes.data, rep=rep.ctypes.data)
            a.update(kw)
            gs = None if gs is None else np.ascontiguousarray(gs, np.int32)
            return m._lib.msiren_align_volume_solve_group(m._h, a["images"], a["n"], HW, HW, a["targets"], a["m"], a["th"], a["tw"], C.byref(o) if o is not None else None,
                                                          None if gs is None else gs.ctypes.data, ng, a["planes"], a["rigid"], a["weights"], a["gb"], a["out"], a["gout"],
                                                          rout.ctypes.data, a["rep"], trep.ctypes.data, None)

        def dev(o, gs=(0, 1, 2), ng=2, **kw):
            return dev_call(m, d, o, gs, ng, **kw)

        inf, nan = float("inf"), float("nan")
        bad_opts = [opts(struct_size=72), opts(struct_size=0), opts(est=2), opts(est=-1), opts(iterations=0), opts(iterations=257), opts(lam_min=0.0), opts(lam_min=1e-2),
                    opts(lam_max=1e-4), opts(lam_max=inf), opts(damping=nan), opts(down=0.0), opts(down=1.5), opts(down=nan), opts(up=0.5), opts(up=inf), opts(up=nan),
                    opts(spacing=0.0), opts(spacing=-1.0), opts(spacing=inf), opts(spacing=nan)]
        for o in bad_opts:
            assert host(o) == _lib.E_INVALID and _lib.last_error(), (o.iterations, o.intensity_mode)
            assert dev(o) == _lib.E_INVALID
        assert host(opts(est=2)) == _lib.E_INVALID and "intensity_mode" in _lib.last_error()
        assert host(opts(struct_size=72)) == _lib.E_INVALID and "struct_size" in _lib.last_error()
        assert host(None) == _lib.E_INVALID and dev(None) == _lib.E_INVALID
        # the groups: none, a null array, a first offset that is not 0, a last that is not m, offsets not strictly ascending -- the message names the index
        for gs, ng, word in (((0, 3, 4, 6), 0, "n_groups"), ((0, 3, 4, 6), -1, "n_groups"), (None, G, "null"), ((1, 3, 4, 6), G, "group_start[0]"),
                             ((0, 3, 4, 5), G, "group_start[3]"), ((0, 3, 4, 7), G, "group_start[3]"), ((0, 3, 3, 6), G, "group_start[2]"),
                             ((0, 4, 3, 6), G, "group_start[2]"), ((0, 0, 4, 6), G, "group_start[1]"), ((0, 6), 1, None)):
            if word is None:
                continue
            assert host(opts(), gs, ng) == _lib.E_INVALID and word in _lib.last_error(), (gs, ng, _lib.last_error())
        for gs, ng, word in (((0, 1, 2), 0, "n_groups"), (None, 2, "null"), ((1, 1, 2), 2, "group_start[0]"), ((0, 1, 3), 2, "group_start[2]"), ((0, 2, 2), 2, "group_start[2]")):
            assert dev(opts(), gs, ng) == _lib.E_INVALID and word in _lib.last_error(), (gs, ng, _lib.last_error())
        for key in ("rigid", "planes", "out", "gout", "rep", "images", "targets"):  # a missing input or output
            assert host(opts(), **{key: None}) == _lib.E_INVALID and "null" in _lib.last_error(), key
            assert dev(opts(), **{key: None}) == _lib.E_INVALID, key
        for key, off in (("targets", 2), ("out", 2), ("weights", 2), ("gb", 2), ("gout", 2), ("rigid", 4), ("planes", 4), ("rout", 4), ("rep", 4), ("trep", 4),
                         ("trace", 4)):  # misaligned device pointers
            assert dev(opts(), **{key: dimg.ptr + off}) == _lib.E_INVALID and "aligned" in _lib.last_error(), key
        # everything msiren_align_volume_solve_w refuses, the weighted form's own size limit included
        for kw in (dict(th=1 << 12, tw=1 << 12), dict(m=-1), dict(n=1), dict(n=1 << 25)):
            assert host(opts(), **kw) == _lib.E_INVALID and dev(opts(), **kw) == _lib.E_INVALID, kw
        assert host(opts(), (0, 7680), 1, m=7680, th=32, tw=32) == _lib.E_INVALID and "640 bytes per chunk" in _lib.last_error()
        # nothing to do
        assert host(opts(), m=0) == 0 and host(opts(), th=0) == 0 and dev(opts(), tw=0) == 0 and dev(opts(), m=0) == 0
        for kw in (dict(iterations=0), dict(damping=0.0), dict(up=0.9)):
            with pytest.raises(ValueError):
                solve(m, tg, av.ESTIMATE, **kw)
        for groups in ([0, 3, 3, 6], [3, 4], [0, 3, 4, 5]):
            with pytest.raises(ValueError):
                solve(m, tg, av.ESTIMATE, groups=groups)
        with pytest.raises(ValueError):
            m.align_volume_solve_group(img, tg, pl[:2], gc.SPACING, gc.GROUP_START)
        with pytest.raises(ValueError):
            m.align_volume_solve_group(img, tg, pl, gc.SPACING, gc.GROUP_START, weights=w[:2])
        with pytest.raises(ValueError):
            m.align_volume_solve_group(img, tg, pl, 0.0, gc.GROUP_START)
        m.sync()
        assert (out == -7.0).all() and (gout == -7.0).all() and (rout == -7.0).all() and (rep == -7.0).all() and (trep == -7.0).all()
        assert np.array_equal(dimg.numpy(), img) and m.profile_kernels() == []
    finally:
        profile_off(m)
    assert same(solve(m, tg, av.ESTIMATE), solved("fp32", "sine5", av.ESTIMATE))  # the handle stays usable


@pytest.mark.parametrize("name,act", [("sine5", 0), ("morlet3", 1)])
def test_profile_counts(name, act):
    m, tg, w = model(name), targets(name), gc.weights()
    trunk = f"siren_trunk_f32_jet_ragged_kernel<256,{act}>"
    per_eval = ("align_volume_bin_kernels", trunk, "align_volume_reduce_w_kernels")
    profile_on(m)
    try:
        m.align_volume_cost_w(vc.images(), tg, gc.start_maps(), weights=w)
        m.sync()
        one = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
    finally:
        profile_off(m)
    assert all(one[k] == 1 for k in per_eval) and not [k for k in one if "step" in k], one
    for est in gc.MODES:
        profile_on(m)
        try:
            solve(m, tg, est, iterations=5)
            m.sync()
            got = {e["kernel"]: e["launches"] for e in m.profile_kernels()}
        finally:
            profile_off(m)
        assert got["align_group_step_kernels"] == 5 and all(got[k] == 5 for k in per_eval), got
        assert "align_volume_step_w_kernel" not in got and "align_volume_reduce_kernels" not in got, got
        prologue = {k: v for k, v in one.items() if k not in per_eval}
        assert {k: v for k, v in got.items() if k not in per_eval + ("align_group_step_kernels",)} == prologue, (got, one)


def test_a_grouped_solve_leaves_the_other_calls_alone():
    name = "sine5"
    m, tg, img, w = model(name), targets(name), vc.images(), gc.weights()
    pts = av.map_points3(gc.truth()[1], SHAPE)

    def others():
        s = m.align_volume_solve_rigid_w(img, tg, gc.planes(), gc.SPACING, weights=w, iterations=3, trace=True)
        c = m.align_volume_cost_w(img, tg, gc.truth(), weights=w, intensity=gc.GB_TRUTH, warped=True, gradient=True)
        val, grad = m.resample_volume_with_gradient(img, pts)
        return s.maps, s.intensity, s.mean_best, s.trace, s.rotation, s.shift, packed(c), c.warped, c.wgrad, val, grad

    before = others()
    for est in gc.MODES:
        solve(m, tg, est)
    after = others()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, after))
