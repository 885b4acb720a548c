"""The robust scale on the GPU: model.residual_scale, i.e. msiren_residual_scale* -- the kernels of residual_scale.hip.h
(rscale_*), an MSD radix select per segment of targets.  Cases: tests/residual_scale_cases.py.

The device has to equal the normative restatement mri_inr_amd/residual_scale.py: residual_scale_on_host BIT FOR BIT -- scale and stats, -0.0 told from
+0.0 -- on every kind of residual array, lattice, weight mask, quantile, centre, floor and grouping; with more segments than one workgroup has
threads; run to run, on alternating streams, in the host and the _dev form; and chained on the device between msiren_project_volume_dev and
msiren_solve_volume_r_dev it has to reach the hand-tuned reconstruction without the scale ever leaving the device."""
import ctypes as C

import numpy as np
import pytest

import fuse_cases as fc
import project_cases as pc
import residual_scale_cases as cases
import solve_volume_cases as sc
import solve_volume_r_cases as rc
import volume_cases as vc
from mri_inr_amd import _lib
from mri_inr_amd import residual_scale as rs
from test_gpu_align import model, profile_off, profile_on, same

pytestmark = pytest.mark.gpu

bits_equal = cases.bits_equal


def same_result(got, want, stats=True):
    return bits_equal(got.scale, want.scale) and (not stats or bits_equal(got.stats, want.stats))


@pytest.mark.parametrize("shape", cases.LATTICES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", cases.KINDS)
def test_the_device_equals_the_host_rule_bit_for_bit(kind, shape):
    m, e = model(), cases.residuals(kind, shape)
    told = []
    for wname, w in cases.weights_of(shape):
        for s in cases.SETTINGS:
            got = m.residual_scale(e, tune=cases.TUNE, weights=w, stats=True, **s)
            want = rs.residual_scale_on_host(e, tune=cases.TUNE, weights=w, **s)
            assert got.scale.dtype == np.float64 and got.scale.shape == (cases.M,) and got.stats.shape == want.stats.shape
            assert bits_equal(got.stats, want.stats), (wname, s, got.stats, want.stats)
            assert bits_equal(got.scale, want.scale), (wname, s, got.scale, want.scale)
        told.append((wname, want.stats[0].tolist()))
    print(f"{kind} {shape}: {told}")


@pytest.mark.parametrize("shape", cases.LATTICES[:2], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_residual_is_formed_on_the_device_as_the_rule_says(shape):
    m = model()
    T, S, gb = cases.pair(shape)
    w = cases.mask(shape)
    for intensity in (None, gb):
        for s in (dict(centre=False, groups=None), dict(centre=True, groups=(3, 1, 2)), dict(centre=True, groups=(cases.M,), quantile=0.29)):
            got = m.residual_scale(T, S, tune=cases.TUNE, weights=w, intensity=intensity, stats=True, **s)
            assert same_result(got, rs.residual_scale_on_host(T, S, tune=cases.TUNE, weights=w, intensity=intensity, **s)), (intensity is None, s)
            assert got.stats[:, 0].min() > 50
    # without intensity: the same as handing over the residual that msiren_project_volume's rule forms from the two
    e = rs.pixel_residual(T, S, None, None)
    assert same_result(m.residual_scale(T, S, tune=2.0, centre=True, stats=True), m.residual_scale(e, tune=2.0, centre=True, stats=True))


MANY = [("258-singletons", 258, (5, 7), None), ("1030-explicit-singletons", 1030, (2, 3), "singletons"), ("130-groups-over-258", 258, (5, 7), "pairs")]


@pytest.mark.parametrize("name,count,shape,grouping", MANY, ids=[c[0] for c in MANY])
def test_many_segments_equal_the_rule_and_their_chunks(name, count, shape, grouping):
    m, e = model(), cases.many(count, shape, 11)
    # 130 groups over 258 targets: 128 pairs and two singletons at the end
    offsets = None if grouping is None else list(range(count + 1)) if grouping == "singletons" else list(range(0, 257, 2)) + [257, 258]
    kw = dict(tune=cases.TUNE, centre=True, quantile=0.5)
    got = m.residual_scale(e, groups=offsets, stats=True, **kw)
    want = rs.residual_scale_on_host(e, groups=offsets, **kw)
    S = count if offsets is None else len(offsets) - 1
    assert got.stats.shape == (S, 4) and (got.stats[:, 0] > 0).all() and len(np.unique(got.scale)) > S // 2
    assert same_result(got, want)
    seg = list(range(count + 1)) if offsets is None else offsets
    parts = []
    for lo, hi in cases.chunks(S, 64):  # at most 64 segments per call
        a, b = seg[lo], seg[hi]
        sub = None if offsets is None else [x - a for x in seg[lo:hi + 1]]
        parts.append(m.residual_scale(e[a:b], groups=sub, stats=True, **kw))
    assert bits_equal(np.concatenate([p.scale for p in parts]), got.scale) and bits_equal(np.concatenate([p.stats for p in parts]), got.stats)


def opts(centre=1, quantile=0.5, tune=cases.TUNE, floor=0.0):
    return _lib.ScaleOpts(C.sizeof(_lib.ScaleOpts), centre, quantile, tune, floor)


def ptr(a):
    return a.ptr if a is not None else None


def dev_call(m, d_t, d_s, d_w, d_gb, count, shape, o, gs, d_scale, d_stats):
    G = 0 if gs is None else len(gs) - 1
    return m._lib.msiren_residual_scale_dev(m._h, ptr(d_t), ptr(d_s), ptr(d_w), ptr(d_gb), count, shape[0], shape[1], C.byref(o) if o is not None else None,
                                            None if gs is None else gs.ctypes.data, G, ptr(d_scale), ptr(d_stats))


def test_determinism_streams_forms_and_stats():
    m, shape = model(), cases.LATTICES[2]
    T, S, gb = cases.pair(shape)
    w = cases.mask(shape)
    gs = np.array([0, 3, 4, 6], np.int32)
    kw = dict(tune=cases.TUNE, weights=w, intensity=gb, centre=True, groups=gs)
    want = rs.residual_scale_on_host(T, S, **kw)
    for _ in range(2):                                                                                   # run to run
        assert same_result(m.residual_scale(T, S, stats=True, **kw), want)
    r = m.residual_scale(T, S, **kw)                                                                     # without stats
    assert r.stats is None and bits_equal(r.scale, want.scale)
    d_t, d_s, d_w, d_gb = (m.device_array(x.shape).copy_from(x) for x in (T, S, w, gb))
    o = opts()
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array((cases.M, 2)), m.device_array((3, 8)) if i % 2 else None) for i in range(6)]
            for d_scale, d_stats in outs:                                                                # back to back, no sync in between
                offsets = gs.copy()
                _lib.check(dev_call(m, d_t, d_s, d_w, d_gb, cases.M, shape, o, offsets, d_scale, d_stats))
                offsets[:] = -5                                                                          # the caller's array is free as soon as the call returns
            m.sync()
            for d_scale, d_stats in outs:
                assert bits_equal(d_scale.numpy().view(np.float64).reshape(-1), want.scale)
                assert d_stats is None or bits_equal(d_stats.numpy().view(np.float64).reshape(3, 4), want.stats)
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


def test_refusals_launch_nothing_and_name_their_argument():
    m, shape = model(), cases.LATTICES[0]
    T, S, gb = cases.pair(shape)
    th, tw = shape
    profile_on(m)
    try:
        d_t, d_s, d_gb = (m.device_array(x.shape).copy_from(x) for x in (T, S, gb))
        d_scale = m.device_array((cases.M, 2)).copy_from(np.full((cases.M, 2), -7.0, np.float32))
        d_x = m.device_array((8, 4))
        scale = np.full(cases.M, -7.0, np.float64)
        m.sync()

        def refused(word, o=None, mt=cases.M, lattice=(th, tw), t=True, s=True, gb_=False, sc_=True, null_opts=False, gs=None, G=None, dev_only=None):
            o = opts() if o is None else o
            G = (0 if gs is None else len(gs) - 1) if G is None else G
            gsp = None if gs is None else gs.ctypes.data
            if dev_only is None:
                rc_ = m._lib.msiren_residual_scale(m._h, T.ctypes.data if t else None, S.ctypes.data if s else None, None, gb.ctypes.data if gb_ else None, mt, lattice[0],
                                                   lattice[1], None if null_opts else C.byref(o), gsp, G, scale.ctypes.data if sc_ else None, None)
                assert rc_ == _lib.E_INVALID and word in _lib.last_error(), (word, _lib.last_error())
            p = dict(t=d_t.ptr if t else None, s=d_s.ptr if s else None, w=None, gb=d_gb.ptr if gb_ else None, sc=d_scale.ptr if sc_ else None, st=None)
            p.update(dev_only or {})
            rc_ = m._lib.msiren_residual_scale_dev(m._h, p["t"], p["s"], p["w"], p["gb"], mt, lattice[0], lattice[1], None if null_opts else C.byref(o), gsp, G, p["sc"], p["st"])
            assert rc_ == _lib.E_INVALID and word in _lib.last_error(), (word, _lib.last_error())

        for size in (24, 40):
            bad = opts()
            bad.struct_size = size
            refused("struct_size", o=bad)
        refused("opts", null_opts=True)
        for bad in (-1, 2):
            refused("centre", o=opts(centre=bad))
        for bad in (-0.01, 1.01, float("nan")):
            refused("quantile", o=opts(quantile=bad))
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused("tune", o=opts(tune=bad))
        for bad in (-1.0, float("inf"), float("nan")):
            refused("floor", o=opts(floor=bad))
        refused("m_targets", mt=-1)
        refused("th", lattice=(-1, tw))
        refused("tw", lattice=(th, -2))
        refused("m_targets th tw", mt=1 << 10, lattice=(1 << 9, 1 << 9))
        refused("m_targets th tw", mt=1 << 28, lattice=(1, 1))
        refused("targets", t=False)
        refused("scale", sc_=False)
        refused("intensity", s=False, gb_=True)
        refused("n_groups", G=2)
        refused("n_groups", gs=np.array([0, cases.M], np.int32), G=0)
        refused("n_groups", gs=np.array([0, cases.M], np.int32), G=-1)
        refused("group_start[0]", gs=np.array([1, cases.M], np.int32))
        refused("ascending", gs=np.array([0, 3, 3, cases.M], np.int32))
        refused("last offset", gs=np.array([0, 3, cases.M + 1], np.int32))
        for key, name in (("t", "targets"), ("s", "simulated"), ("w", "weights"), ("gb", "intensity")):
            refused(name, s=True, dev_only={key: d_x.ptr + 2})
        for key, name in (("sc", "scale"), ("st", "stats")):
            refused(name, dev_only={key: d_x.ptr + 4})
        for kw in (dict(weights=np.ones((2, th, tw), np.float32)), dict(intensity=gb[:, :1]), dict(groups=[0, 2, 2, cases.M]), dict(groups=[4, 4])):
            with pytest.raises(ValueError):
                m.residual_scale(T, S, tune=1.0, **kw)
        with pytest.raises(ValueError):
            m.residual_scale(T, S[:2], tune=1.0)
        with pytest.raises(ValueError, match="intensity"):
            m.residual_scale(T, tune=1.0, intensity=gb)
        m.sync()
        assert (scale == -7.0).all() and (d_scale.numpy() == -7.0).all() and m.profile_kernels() == []
        # no target, and targets without pixels: accepted, nothing launched, nothing written
        empty = m.residual_scale(np.zeros((0, th, tw), np.float32), tune=1.0, stats=True)
        assert empty.scale.shape == (0,) and empty.stats.shape == (0, 4)
        none = m.residual_scale(np.zeros((3, 0, tw), np.float32), tune=1.0, stats=True)
        assert np.isposinf(none.scale).all() and none.scale.shape == (3,) and not none.stats.any()
        m.sync()
        assert m.profile_kernels() == []
    finally:
        profile_off(m)
    assert same_result(m.residual_scale(T, S, tune=1.0, stats=True), rs.residual_scale_on_host(T, S, tune=1.0))


def test_the_profile_shows_residual_scale_kernels_once_per_call():
    m, shape = model(), cases.LATTICES[1]
    e = cases.residuals("smooth", shape)
    profile_on(m)
    try:
        for calls in (1, 2, 3):
            m.residual_scale(e, tune=1.0, centre=calls == 2, groups=(3, 1, 2) if calls == 3 else None, stats=calls == 1)
            m.sync()
            entries = m.profile_kernels()
            assert [x["kernel"] for x in entries] == ["residual_scale_kernels"] and entries[0]["launches"] == calls and entries[0]["coords"] == calls * e.size, entries
    finally:
        profile_off(m)


def test_a_handle_without_committed_weights_estimates():
    from mri_inr_amd import ModulatedSiren

    m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0, use_bias=True, dropout=0.1, modulate=True,
                       encoder_type="custom", encoder_path=None, outer_patch_size=vc.O, inner_patch_size=vc.I, siren_patch_size=vc.S, device="cuda", activation="sine")
    e = cases.residuals("nonfinite", cases.LATTICES[0])  # (no load_state_dict, no .to(): nothing has committed the fresh model's weights)
    kw = dict(tune=cases.TUNE, centre=True, groups=(3, 1, 2))
    assert same_result(m.residual_scale(e, stats=True, **kw), rs.residual_scale_on_host(e, **kw)) and not m._committed


def test_the_other_geometry_calls_return_the_same_bits_before_and_after_an_estimate():
    m, d = model(), fc.planes()
    grid = sc.GRIDS[1]
    rargs, rkw = rc.all_cases()["planes-grid1-quarter"]
    stack = pc.holes(grid)

    def others():
        p = m.project_volume(stack, d["maps"], pc.SHAPE, pc.SPACING, intensity=d["intensity"], targets=d["targets"], weights=d["weights"], coverage=True, residual=True,
                             stats=True)
        s = m.solve_volume_robust(*rargs, rounds=2, iterations=2, anneal=4.0, lam=0.01, coverage=True, history=True, rweight=True, stats=True, **rkw)
        a = m.align_stack_cost(stack, d["targets"], d["maps"], scale=0.5, weights=d["weights"], intensity=d["intensity"], warped=True, gradient=True, rweight=True)
        return [p.simulated, p.coverage, p.residual, p.stats, p.flags, s.volume, s.coverage, s.history, s.flags, s.stopped_at, s.rweight, s.stats, a.count, a.wsum, a.cost,
                a.grad, a.jtj, a.warped, a.wgrad, a.rweight]

    before = others()
    assert np.isfinite(before[0]).any() and np.isfinite(before[5]).any() and before[12].any()
    e = cases.many(64, (160, 160), 5)                                                                    # (a larger block of the stream's scratch than theirs)
    r = m.residual_scale(e, tune=cases.TUNE, centre=True, groups=[16] * 4, stats=True)
    after = others()
    assert all(same(a, b) for a, b in zip(before, after))
    assert same_result(m.residual_scale(e, tune=cases.TUNE, centre=True, groups=[16] * 4, stats=True), r)


def test_the_scale_never_leaves_the_device_between_projection_and_robust_solve():
    """msiren_project_volume_dev (residual) -> msiren_residual_scale_dev -> msiren_solve_volume_r_dev on the corrupted truth case, per target and pooled:
    the same bits as the three host-form calls, the scale the restatement's, and the reconstruction error a tenth of the quadratic solve's at most"""
    m, c = model(), rc.corrupted()
    tg, maps, grid, sp = c["targets"], c["maps"], fc.TRUTH_GRID, sc.SPACING
    count, (th, tw) = len(tg), tg.shape[1:]
    setting = rc.CORRUPT_SETTING
    clean = m.solve_volume(c["clean"], maps, grid, sp, iterations=15, lam=setting["lam"], thickness=sp).volume
    S = np.isfinite(clean)
    fused = m.fuse_targets(tg, maps, grid, sp, thickness=sp)
    fo = _lib.FuseOpts(C.sizeof(_lib.FuseOpts), 0, sp, sp, 0.0)
    ro = _lib.SolveROpts(C.sizeof(_lib.SolveROpts), setting["iterations"], setting["rounds"], 0, sp, sp, 0.0, setting["lam"], setting["anneal"])
    so = opts(centre=0, quantile=0.5, tune=cases.TUNE)
    d_t, d_m, d_v = (m.device_array(x.shape).copy_from(x) for x in (tg, maps, fused.volume))
    d_sim, d_res, d_scale, d_out = m.device_array(tg.shape), m.device_array(tg.shape), m.device_array((count, 2)), m.device_array(grid)
    for name, groups in (("per target", None), ("pooled", [count])):
        gs = None if groups is None else np.array([0, count], np.int32)
        _lib.check(m._lib.msiren_project_volume_dev(m._h, d_v.ptr, grid[0], grid[1], grid[2], d_m.ptr, None, C.byref(fo), count, th, tw, d_t.ptr, None, d_sim.ptr, None,
                                                    d_res.ptr, None, None))
        _lib.check(dev_call(m, d_res, None, None, None, count, (th, tw), so, gs, d_scale, None))
        _lib.check(m._lib.msiren_solve_volume_r_dev(m._h, d_t.ptr, count, th, tw, d_m.ptr, None, None, d_scale.ptr, C.byref(ro), grid[0], grid[1], grid[2], None, d_out.ptr,
                                                    None, None, None, None, None, None, None))
        m.sync()
        scale, volume = d_scale.numpy().view(np.float64).reshape(-1), d_out.numpy()
        # the same chain through the host forms, and the scale against the restatement on the projection's residual
        p = m.project_volume(fused.volume, maps, (th, tw), sp, thickness=sp, targets=tg, residual=True)
        est = m.residual_scale(p.residual, tune=cases.TUNE, groups=groups)
        host = m.solve_volume_robust(tg, maps, grid, sp, est.scale, thickness=sp, **setting)
        assert bits_equal(scale, est.scale) and bits_equal(scale, rs.residual_scale_on_host(p.residual, tune=cases.TUNE, groups=groups).scale)
        assert bits_equal(scale, m.residual_scale(tg, p.simulated, tune=cases.TUNE, groups=groups).scale)
        assert same(volume, host.volume)
        err = float(np.abs(volume.astype(np.float64) - clean)[S].mean())
        print(f"{name}: scale {scale.min()} .. {scale.max()}, mean |x - x_clean| {err} (quadratic {rc.MEASURED['quadratic_mean']})")
        assert err < 0.1 * rc.MEASURED["quadratic_mean"]
