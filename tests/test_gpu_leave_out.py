"""The leave-one-out prediction on the GPU: model.leave_out_targets, i.e. msiren_leave_out_targets* -- the kernels of
leave_out.hip.h (loo_*) with fuse_setup_kernel and project_stats_kernel.  Cases: tests/leave_out_cases.py.

The device has to equal the normative restatement mri_inr_amd/leave_out.py: leave_out_on_host BIT FOR BIT -- simulated, coverage, residual, stats,
flags, volume and volume_coverage -- on every case, grid, thickness and grouping, the floor's two sides and more than 512 groups included; run to run, on
alternating streams, in the host and the _dev form and for every subset of the optional outputs."""
import ctypes as C
import itertools

import numpy as np
import pytest

import fuse_cases as fc
import leave_out_cases as cases
import project_cases as pc
import solve_volume_cases as sc
from mri_inr_amd import _lib
from mri_inr_amd import leave_out as lo
from test_gpu_align import model, profile_off, profile_on, same

pytestmark = pytest.mark.gpu

bits_equal = cases.bits_equal
EVERYTHING = dict(coverage=True, residual=True, stats=True, volume=True)


@pytest.mark.parametrize("name", list(cases.all_cases()))
def test_the_device_equals_the_host_rule_bit_for_bit(name):
    args, kw = cases.all_cases()[name]
    got, want = model().leave_out_targets(*args, **EVERYTHING, **kw), cases.reference(name)
    for field, g, w in zip(got._fields, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (field, g.shape, g.dtype)
        assert bits_equal(g, w), (field, int((g.view(np.uint8) != w.view(np.uint8)).sum()))
    print(f"{name}: {int(np.isfinite(got.simulated).sum())} of {got.simulated.size} pixels predicted")
    if name in cases.ALL_NAN:
        assert np.isnan(got.simulated).all() and not got.coverage.any()
    elif name != "none" and not name.startswith("planes-grid") and not name.startswith("twin"):
        assert np.isfinite(got.simulated).any()


def test_the_floor_has_two_sides():
    m = model()
    for e in cases.TWIN_PREDICTED + cases.TWIN_FLOORED:
        args, kw = cases.all_cases()[f"twin-{e}"]
        r = m.leave_out_targets(*args, **kw)
        assert bits_equal(r.simulated[3:], args[0][:3]), e                                               # the copies: the originals' bits
        if e in cases.TWIN_PREDICTED:
            assert bits_equal(r.simulated[:3], args[0][3:]), e                                           # the originals: their twins' bits
        else:
            assert np.isnan(r.simulated[:3]).all(), e


def fuse_opts(spacing, thickness, min_coverage):
    return _lib.FuseOpts(C.sizeof(_lib.FuseOpts), 0, spacing, thickness, min_coverage)


def ptr(a):
    return a.ptr if a is not None else None


def dev_call(m, d, count, shape, o, gs, grid, outs):
    """outs: device arrays or None in the order simulated, coverage, residual, stats, flags, volume, volume_coverage"""
    G = 0 if gs is None else len(gs) - 1
    return m._lib.msiren_leave_out_targets_dev(m._h, ptr(d["targets"]), count, shape[0], shape[1], ptr(d["maps"]), ptr(d.get("weights")), ptr(d.get("intensity")),
                                               C.byref(o) if o is not None else None, None if gs is None else gs.ctypes.data, G, grid[0], grid[1], grid[2],
                                               *[ptr(x) for x in outs])


def dev_outputs(m, count, shape, grid, which):
    """device arrays for the outputs named in ``which`` (simulated always), pre-filled with -7"""
    shapes = dict(simulated=(count,) + shape, coverage=(count,) + shape, residual=(count,) + shape, stats=(count, 8), flags=(count, 1), volume=grid, volume_coverage=grid)
    return [m.device_array(shapes[f]).copy_from(np.full(shapes[f], -7.0, np.float32)) if f == "simulated" or f in which else None for f in lo.LeaveOutResult._fields]


def read(outs, count):
    views = dict(stats=lambda a: a.view(np.float64).reshape(count, 4), flags=lambda a: a.view(np.int32).reshape(count))
    return [None if x is None else views.get(f, lambda a: a)(x.numpy()) for f, x in zip(lo.LeaveOutResult._fields, outs)]


def test_determinism_streams_forms_and_every_subset_of_the_outputs():
    m, name = model(), "planes-grid1-full-groups-mc0.25"
    (T, maps, grid, spacing), kw = cases.all_cases()[name]
    want = cases.reference(name)
    count, shape = len(T), T.shape[1:]
    for _ in range(2):                                                                                   # run to run
        assert cases.same_result(m.leave_out_targets(T, maps, grid, spacing, **EVERYTHING, **kw), want)
    optional = ("coverage", "residual", "stats", "volume")
    for k in range(len(optional) + 1):                                                                   # every subset, host form
        for subset in itertools.combinations(optional, k):
            r = m.leave_out_targets(T, maps, grid, spacing, **{f: True for f in subset}, **kw)
            assert cases.same_result(r, want), subset
            given = {f for f in lo.LeaveOutResult._fields if getattr(r, f) is not None}
            assert given == {"simulated", "flags"} | set(subset) | ({"volume_coverage"} if "volume" in subset else set()), subset
    d = {k: m.device_array(x.shape).copy_from(x) for k, x in (("targets", T), ("maps", maps), ("weights", kw["weights"]), ("intensity", kw["intensity"]))}
    o = fuse_opts(spacing, kw["thickness"], kw["min_coverage"])
    gs = np.array([0, 3, 4, 6, 8], np.int32)
    subsets = [(), ("volume_coverage",), ("stats",), ("residual", "flags"), ("coverage", "volume"), lo.LeaveOutResult._fields]
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            runs = [dev_outputs(m, count, shape, grid, which) for which in subsets]
            for outs in runs:                                                                            # back to back, no sync in between
                offsets = gs.copy()
                _lib.check(dev_call(m, d, count, shape, o, offsets, grid, outs))
                offsets[:] = -5                                                                          # the caller's array is free as soon as the call returns
            m.sync()
            for which, outs in zip(subsets, runs):
                assert cases.same_result(read(outs, count), want), (streams, which)
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


def test_no_targets():
    m = model()
    (T, maps, grid, spacing), kw = cases.all_cases()["none"]
    profile_on(m)
    try:
        r = m.leave_out_targets(T, maps, grid, spacing, coverage=True, residual=True, stats=True)
        m.sync()
        assert r.simulated.shape == T.shape and r.stats.shape == (0, 4) and r.volume is None and m.profile_kernels() == []      # nothing to write: nothing launched
        r = m.leave_out_targets(T, maps, grid, spacing, **EVERYTHING)
        m.sync()
        assert np.isnan(r.volume).all() and r.volume.shape == grid and not r.volume_coverage.any()
        assert [(x["kernel"], x["launches"]) for x in m.profile_kernels()] == [("leave_out_kernels", 1)]
    finally:
        profile_off(m)
    assert cases.same_result(r, cases.reference("none"))


def test_refusals_launch_nothing_and_name_their_argument():
    m = model()
    (T, maps, grid, spacing), kw = cases.all_cases()["planes-grid0-full-singletons-mc0.0"]
    count, (th, tw) = len(T), T.shape[1:]
    sim = np.full(T.shape, -7.0, np.float32)
    profile_on(m)
    try:
        d = {k: m.device_array(x.shape).copy_from(x) for k, x in (("targets", T), ("maps", maps))}
        outs = dev_outputs(m, count, (th, tw), grid, lo.LeaveOutResult._fields)
        d_x = m.device_array((8, 4))
        m.sync()

        def refused(word, o=None, mt=count, lattice=(th, tw), g=grid, null=(), null_opts=False, gs=None, G=None, dev_only=None):
            o = fuse_opts(spacing, spacing, 0.0) if o is None else o
            G = (0 if gs is None else len(gs) - 1) if G is None else G
            gsp = None if gs is None else gs.ctypes.data
            op = None if null_opts else C.byref(o)
            if dev_only is None:
                host = dict(targets=T.ctypes.data, maps=maps.ctypes.data, simulated=sim.ctypes.data)
                host.update({k: None for k in null})
                rc_ = m._lib.msiren_leave_out_targets(m._h, host["targets"], mt, lattice[0], lattice[1], host["maps"], None, None, op, gsp, G, g[0], g[1], g[2], host["simulated"],
                                                      None, None, None, None, None, None)
                assert rc_ == _lib.E_INVALID and word in _lib.last_error(), (word, _lib.last_error())
            p = dict(targets=d["targets"].ptr, maps=d["maps"].ptr, weights=None, intensity=None)
            p.update({f: x.ptr for f, x in zip(lo.LeaveOutResult._fields, outs)})
            p.update({k: None for k in null})
            p.update(dev_only or {})
            rc_ = m._lib.msiren_leave_out_targets_dev(m._h, p["targets"], mt, lattice[0], lattice[1], p["maps"], p["weights"], p["intensity"], op, gsp, G, g[0], g[1], g[2],
                                                      *[p[f] for f in lo.LeaveOutResult._fields])
            assert rc_ == _lib.E_INVALID and word in _lib.last_error(), (word, _lib.last_error())

        for size in (24, 40):
            bad = fuse_opts(spacing, spacing, 0.0)
            bad.struct_size = size
            refused("struct_size", o=bad)
        refused("opts", null_opts=True)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused("spacing", o=fuse_opts(bad, 4.0, 0.0))
            refused("thickness", o=fuse_opts(4.0, bad, 0.0))
        for bad in (-0.5, float("nan")):
            refused("min_coverage", o=fuse_opts(4.0, 4.0, bad))
        refused("m_targets", mt=-1)
        refused("th and tw", lattice=(1, tw))
        refused("th and tw", lattice=(th, 1))
        refused("n_slices", g=(0, 4, 4))
        refused("height", g=(4, 0, 4))
        refused("width", g=(4, 4, 0))
        refused("n_slices height width", g=(1 << 10, 1 << 10, 1 << 10))
        refused("m_targets th tw", mt=1 << 10, lattice=(1 << 10, 1 << 10))
        for name in ("targets", "maps", "simulated"):
            refused(name, null=(name,))
        refused("n_groups", G=2)
        refused("n_groups", gs=np.array([0, count], np.int32), G=0)
        refused("n_groups", gs=np.array([0, count], np.int32), G=-1)
        refused("group_start[0]", gs=np.array([1, count], np.int32))
        refused("ascending", gs=np.array([0, 3, 3, count], np.int32))
        refused("last offset", gs=np.array([0, 3, count + 1], np.int32))
        for name in ("targets", "maps", "weights", "intensity", "simulated", "coverage", "residual", "flags", "volume", "volume_coverage"):
            refused(name, dev_only={name: d_x.ptr + 2})
        refused("stats", dev_only={"stats": d_x.ptr + 4})
        for bad in (dict(weights=np.ones((2, th, tw), np.float32)), dict(intensity=np.ones((count, 1), np.float32)), dict(groups=[0, 2, 2, count]), dict(groups=[4, 3])):
            with pytest.raises(ValueError):
                m.leave_out_targets(T, maps, grid, spacing, **bad)
        with pytest.raises(ValueError):
            m.leave_out_targets(T, maps[:3], grid, spacing)
        with pytest.raises(ValueError):
            m.leave_out_targets(T, maps, grid[:2], spacing)
        m.sync()
        assert (sim == -7.0).all() and all((x.numpy() == -7.0).all() for x in outs) and m.profile_kernels() == []
    finally:
        profile_off(m)


def test_the_profile_shows_leave_out_kernels_once_per_call():
    m = model()
    (T, maps, grid, spacing), kw = cases.all_cases()["planes-grid0-full-groups-mc0.0"]
    profile_on(m)
    try:
        for calls in (1, 2, 3):
            m.leave_out_targets(T, maps, grid, spacing, stats=calls == 1, volume=calls == 2, **(kw if calls == 3 else {}))
            m.sync()
            entries = m.profile_kernels()
            assert [x["kernel"] for x in entries] == ["leave_out_kernels"] and entries[0]["launches"] == calls and entries[0]["coords"] == calls * T.size, entries
    finally:
        profile_off(m)


def test_a_handle_without_committed_weights_predicts():
    import volume_cases as vc
    from mri_inr_amd import ModulatedSiren

    m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0, use_bias=True, dropout=0.1, modulate=True,
                       encoder_type="custom", encoder_path=None, outer_patch_size=vc.O, inner_patch_size=vc.I, siren_patch_size=vc.S, device="cuda", activation="sine")
    name = "planes-grid1-quarter-singletons-mc0.25"  # (no load_state_dict, no .to(): nothing has committed the fresh model's weights)
    args, kw = cases.all_cases()[name]
    assert cases.same_result(m.leave_out_targets(*args, **EVERYTHING, **kw), cases.reference(name)) and not m._committed


def test_the_other_geometry_calls_return_the_same_bits_before_and_after_a_call():
    m, d = model(), fc.planes()
    grid = sc.GRIDS[1]
    stack = pc.holes(grid)

    def others():
        f = m.fuse_targets(d["targets"], d["maps"], grid, fc.SPACING, weights=d["weights"], intensity=d["intensity"], coverage=True)
        p = m.project_volume(stack, d["maps"], pc.SHAPE, pc.SPACING, intensity=d["intensity"], targets=d["targets"], weights=d["weights"], coverage=True, residual=True,
                             stats=True)
        s = m.solve_volume(d["targets"], d["maps"], grid, fc.SPACING, iterations=3, lam=0.01, weights=d["weights"], intensity=d["intensity"], coverage=True, history=True)
        return [f.volume, f.coverage, f.flags, p.simulated, p.coverage, p.residual, p.stats, p.flags, s.volume, s.coverage, s.history, s.flags]

    before = others()
    assert np.isfinite(before[0]).any() and np.isfinite(before[3]).any() and np.isfinite(before[8]).any()
    args, kw = cases.all_cases()["truth-full-fours"]                                                     # (a larger block of the stream's scratch than theirs)
    r = m.leave_out_targets(*args, **EVERYTHING, **kw)
    after = others()
    assert all(same(a, b) for a, b in zip(before, after))
    assert cases.same_result(r, cases.reference("truth-full-fours"))
    # the by-product is the fusion's own output
    f = m.fuse_targets(*args, thickness=kw["thickness"], coverage=True)
    assert bits_equal(r.volume, f.volume) and bits_equal(r.volume_coverage, f.coverage)
