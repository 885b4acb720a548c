"""A stack gathered onto the lattices of target slices on the GPU: model.project_volume, i.e. msiren_project_volume* --
fuse_setup_kernel (fuse.hip.h), project_gather_kernel and project_stats_kernel (project.hip.h).  Cases: tests/project_cases.py.

The device has to equal the normative restatements mri_inr_amd/fuse.py: project_on_host and project_stats_on_host BIT FOR BIT -- simulated, coverage,
residual (NaNs in the same places), the four sums per target and flags -- on every case, grid and thickness, with and without intensity, targets and
weights.  The graze cases put the window's edge and the lattice's last row and column on voxels, and one ulp either side; the truth case's targets
overhang the grid on every side: there a box that left out a voxel it must visit, or one that was not clipped, would show as other bits."""
import ctypes as C

import numpy as np
import pytest

import align_group_cases as gc
import fuse_cases as fc
import project_cases as pc
import volume_cases as vc
from mri_inr_amd import _lib, fuse
from test_gpu_align import model, profile_off, profile_on, same

pytestmark = pytest.mark.gpu

CASES = pc.all_cases()


def same_gather(a, b, coverage=True):
    return same(a.simulated, b.simulated) and np.array_equal(a.flags, b.flags) and (not coverage or same(a.coverage, b.coverage))


def host(args, kw, targets=None, weights=None):
    """the host restatement with the residual and the sums"""
    res = fuse.project_on_host(*args, **kw)
    if targets is None:
        return res
    r, st = fuse.project_stats_on_host(targets, res.simulated, weights)
    return res._replace(residual=r, stats=st)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_device_equals_the_host_rule_bit_for_bit(name):
    args, kw = CASES[name]
    got = model().project_volume(*args, coverage=True, **kw)
    want = host(args, kw)
    print(f"{name}: {int(np.isfinite(want.simulated).sum())} of {want.simulated.size} pixels covered, flags {want.flags.tolist()}")
    assert got.simulated.dtype == np.float32 and got.coverage.dtype == np.float32 and got.flags.dtype == np.int32 and got.simulated.shape == want.simulated.shape
    assert got.residual is None and got.stats is None
    if name != "outside":
        assert np.isfinite(want.simulated).sum() > 300
    assert same_gather(got, want)


@pytest.mark.parametrize("weights", [True, False])
@pytest.mark.parametrize("intensity", [True, False])
@pytest.mark.parametrize("thickness", pc.THICKNESSES)
@pytest.mark.parametrize("grid", pc.GRIDS)
def test_the_residual_and_the_sums_equal_the_host_rule_bit_for_bit(grid, thickness, intensity, weights):
    d = fc.planes()
    args, kw = pc.planes(grid, intensity, pc.holes(grid))
    kw = dict(kw, thickness=thickness)
    w = d["weights"] if weights else None
    got = model().project_volume(*args, targets=d["targets"], weights=w, coverage=True, residual=True, stats=True, **kw)
    want = host(args, kw, d["targets"], w)
    assert got.stats.dtype == np.float64 and got.stats.shape == (fc.M, 4) and got.residual.dtype == np.float32
    assert want.stats[1, 0] > 100 and not want.stats[fc.DEGENERATE_AT].any() and np.isnan(want.residual[fc.NAN_PIXEL_AT])
    assert same_gather(got, want) and same(got.residual, want.residual) and np.array_equal(got.stats, want.stats)


def test_identity_returns_the_stacks_bits():
    d = pc.identity()
    res = model().project_volume(d["volume"], d["maps"], pc.SHAPE, pc.SPACING, coverage=True)
    assert same(res.simulated, d["volume"]) and (res.coverage == 1.0).all() and not res.flags.any()


def test_torch_tensors_are_accepted():
    torch = pytest.importorskip("torch")
    d = fc.planes()
    args, kw = pc.planes(pc.GRIDS[0])
    got = model().project_volume(torch.from_numpy(args[0].copy()), torch.from_numpy(args[1].copy()), pc.SHAPE, pc.SPACING, intensity=torch.from_numpy(kw["intensity"].copy()),
                                 targets=torch.from_numpy(d["targets"].copy()), weights=torch.from_numpy(d["weights"].copy()), coverage=True, residual=True, stats=True)
    want = host(args, kw, d["targets"], d["weights"])
    assert same_gather(got, want) and same(got.residual, want.residual) and np.array_equal(got.stats, want.stats)


def opts(thickness=pc.SPACING, min_coverage=0.0, spacing=pc.SPACING):
    return _lib.FuseOpts(C.sizeof(_lib.FuseOpts), 0, spacing, thickness, min_coverage)


def ptr(a):
    return a.ptr if a is not None else None


def dev_call(m, d_v, grid, d_m, d_gb, o, mt, shape, d_t, d_w, d_s, d_c, d_r, d_st, d_f):
    return m._lib.msiren_project_volume_dev(m._h, ptr(d_v), grid[0], grid[1], grid[2], ptr(d_m), ptr(d_gb), C.byref(o) if o is not None else None, mt, shape[0], shape[1],
                                            ptr(d_t), ptr(d_w), ptr(d_s), ptr(d_c), ptr(d_r), ptr(d_st), ptr(d_f))


def test_determinism_streams_forms_and_every_subset_of_optional_outputs():
    m, d, grid = model(), fc.planes(), pc.GRIDS[1]
    args, kw = pc.planes(grid, True, pc.holes(grid))
    vol, maps, gb, tg, w = args[0], args[1], kw["intensity"], d["targets"], d["weights"]
    want = host(args, kw, tg, w)
    full = dict(targets=tg, weights=w, coverage=True, residual=True, stats=True)
    first = m.project_volume(*args, **kw, **full)
    again = m.project_volume(*args, **kw, **full)
    for r in (first, again):                                                                             # run to run
        assert same_gather(r, want) and same(r.residual, want.residual) and np.array_equal(r.stats, want.stats)
    for mask in range(8):                                                                                # every subset of the optional outputs
        cov, res, st = bool(mask & 1), bool(mask & 2), bool(mask & 4)
        r = m.project_volume(*args, **kw, targets=tg, weights=w, coverage=cov, residual=res, stats=st)
        assert same_gather(r, want, coverage=False) and (r.coverage is None) == (not cov) and (r.residual is None) == (not res) and (r.stats is None) == (not st)
        assert (not cov or same(r.coverage, want.coverage)) and (not res or same(r.residual, want.residual)) and (not st or np.array_equal(r.stats, want.stats))
    some = m.project_volume(*args, **kw, min_coverage=1.5, coverage=True)                                # min_coverage only turns values into NaN
    assert same_gather(some, fuse.project_on_host(*args, min_coverage=1.5, **kw)) and 0 < np.isfinite(some.simulated).sum() < np.isfinite(first.simulated).sum()
    # the _dev form against the host form, on one stream and on two alternating, calls back to back without a sync, with and without the optional outputs
    d_v, d_m, d_gb, d_t, d_w = (m.device_array(x.shape).copy_from(x) for x in (vol, maps, gb, tg, w))
    shape = (fc.M,) + pc.SHAPE
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array(shape),) + (tuple(m.device_array(s) for s in (shape, shape, (fc.M, 8), (fc.M,))) if k != 1 else (None,) * 4) for k in range(streams + 2)]
            for d_s, d_c, d_r, d_st, d_f in outs:
                _lib.check(dev_call(m, d_v, grid, d_m, d_gb, opts(), fc.M, pc.SHAPE, d_t, d_w, d_s, d_c, d_r, d_st, d_f))
            m.sync()
            for d_s, d_c, d_r, d_st, d_f in outs:
                assert same(d_s.numpy(), want.simulated)
                if d_c is not None:
                    assert same(d_c.numpy(), want.coverage) and same(d_r.numpy(), want.residual) and np.array_equal(d_st.numpy().view(np.float64), want.stats)
                    assert np.array_equal(d_f.numpy().view(np.int32), want.flags)
            plain = m.device_array(shape)                                                                # without intensity, targets and weights
            _lib.check(dev_call(m, d_v, grid, d_m, None, opts(), fc.M, pc.SHAPE, None, None, plain, None, None, None, None))
            m.sync()
            assert same(plain.numpy(), fuse.project_on_host(vol, maps, pc.SHAPE, pc.SPACING).simulated)
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


def test_no_target_and_a_stack_without_a_finite_voxel():
    m, grid = model(), pc.GRIDS[1]
    res = m.project_volume(pc.stack(grid), np.zeros((0, 9), np.float32), pc.SHAPE, pc.SPACING, coverage=True)
    assert res.simulated.shape == (0,) + pc.SHAPE and res.coverage.shape == (0,) + pc.SHAPE and res.flags.shape == (0,)
    d_v = m.device_array(grid).copy_from(pc.stack(grid))
    assert m._lib.msiren_project_volume_dev(m._h, d_v.ptr, *grid, None, None, None, 0, 0, 0, None, None, None, None, None, None, None) == 0  # opts may be null without a target
    m.sync()
    args, kw = pc.planes(grid, True, np.full(grid, np.nan, np.float32))
    d = fc.planes()
    res = m.project_volume(*args, **kw, targets=d["targets"], coverage=True, residual=True, stats=True)
    assert np.isnan(res.simulated).all() and not res.coverage.any() and np.isnan(res.residual).all() and not res.stats.any()
    assert res.flags.tolist() == [0] * fc.M_PLANES + [fuse.DEGENERATE, fuse.BAD_INTENSITY]


def test_refusals_launch_nothing_and_name_their_argument():
    m, d, grid = model(), fc.planes(), pc.GRIDS[0]
    vol, maps, tg = pc.stack(grid), d["maps"], d["targets"]
    th, tw = pc.SHAPE
    shape = (fc.M, th, tw)
    profile_on(m)
    try:
        d_v, d_m, d_t = m.device_array(grid).copy_from(vol), m.device_array(maps.shape).copy_from(maps), m.device_array(shape).copy_from(tg)
        d_s = m.device_array(shape).copy_from(np.full(shape, -7.0, np.float32))
        d_x = m.device_array((fc.M, 8))
        sim = np.full(shape, -7.0, np.float32)
        extra = np.zeros(shape, np.float64)
        m.sync()

        def refused(word, o=None, mt=fc.M, lattice=(th, tw), g=grid, v=True, mp=True, s=True, null_opts=False, t=False, w=False, r=False, st=False, dev_only=None):
            o = opts() if o is None else o
            if dev_only is None:
                rc = m._lib.msiren_project_volume(m._h, vol.ctypes.data if v else None, g[0], g[1], g[2], maps.ctypes.data if mp else None, None, None if null_opts else C.byref(o), mt,
                                                  lattice[0], lattice[1], tg.ctypes.data if t else None, extra.ctypes.data if w else None, sim.ctypes.data if s else None, None,
                                                  extra.ctypes.data if r else None, extra.ctypes.data if st else None, None)
                assert rc == _lib.E_INVALID and word in _lib.last_error(), (word, _lib.last_error())
            p = dict(v=d_v.ptr if v else None, mp=d_m.ptr if mp else None, gb=None, t=d_t.ptr if t else None, w=d_t.ptr if w else None, s=d_s.ptr if s else None, c=None,
                     r=d_t.ptr if r else None, st=d_x.ptr if st else None, f=None)
            p.update(dev_only or {})
            rc = m._lib.msiren_project_volume_dev(m._h, p["v"], g[0], g[1], g[2], p["mp"], p["gb"], None if null_opts else C.byref(o), mt, lattice[0], lattice[1], p["t"], p["w"],
                                                  p["s"], p["c"], p["r"], p["st"], p["f"])
            assert rc == _lib.E_INVALID and word in _lib.last_error(), (word, _lib.last_error())

        bad_size = opts()
        bad_size.struct_size = 24
        refused("struct_size", o=bad_size)
        for bad in (0.0, -4.0, float("nan"), float("inf")):
            refused("spacing", o=opts(spacing=bad))
            refused("thickness", o=opts(thickness=bad))
        for bad in (-1.0, float("nan")):
            refused("min_coverage", o=opts(min_coverage=bad))
        refused("th", lattice=(1, tw))
        refused("tw", lattice=(th, 1))
        refused("n_slices", g=(0, 40, 40))
        refused("height", g=(4, 0, 40))
        refused("width", g=(4, 40, -1))
        refused("n_slices height width", g=(1 << 10, 1 << 10, 1 << 10))
        refused("m_targets th tw", mt=1 << 12, lattice=(1 << 9, 1 << 9))
        refused("m_targets", mt=-1)
        refused("volume", v=False)
        refused("maps", mp=False)
        refused("simulated", s=False)
        refused("opts", null_opts=True)
        refused("weights", w=True)
        refused("residual", r=True)
        refused("stats", st=True)
        for key, name in (("v", "volume"), ("mp", "maps"), ("gb", "intensity"), ("t", "targets"), ("s", "simulated"), ("c", "coverage"), ("f", "flags")):
            refused(name, dev_only={key: d_v.ptr + 2, "t": d_v.ptr + 2 if key == "t" else d_t.ptr})
        for key, name in (("w", "weights"), ("r", "residual")):
            refused(name, dev_only={key: d_v.ptr + 2, "t": d_t.ptr})
        refused("stats", dev_only={"st": d_x.ptr + 4, "t": d_t.ptr})
        with pytest.raises(ValueError, match="thickness"):
            m.project_volume(vol, maps, pc.SHAPE, pc.SPACING, thickness=0.0)
        for bad_vol, bad_maps, kw in ((vol[0], maps, {}), (vol, maps[:, :5], {}), (vol, maps, dict(intensity=d["intensity"][:, :1])), (vol, maps, dict(targets=tg[:2])),
                                      (vol, maps, dict(weights=d["weights"])), (vol, maps, dict(stats=True)), (vol, maps, dict(targets=tg, weights=d["weights"][:2]))):
            with pytest.raises(ValueError):
                m.project_volume(bad_vol, bad_maps, pc.SHAPE, pc.SPACING, **kw)
        m.sync()
        assert (sim == -7.0).all() and (d_s.numpy() == -7.0).all() and m.profile_kernels() == []
    finally:
        profile_off(m)
    assert same_gather(m.project_volume(vol, maps, pc.SHAPE, pc.SPACING, coverage=True), fuse.project_on_host(vol, maps, pc.SHAPE, pc.SPACING))  # the handle stays usable


def test_the_profile_shows_project_kernels_once_per_call():
    m, d, grid = model(), fc.planes(), pc.GRIDS[0]
    args, kw = pc.planes(grid)
    profile_on(m)
    try:
        for calls in (1, 2, 3):
            m.project_volume(*args, **kw, targets=d["targets"] if calls != 2 else None, stats=calls == 3, residual=calls == 1)
            m.sync()
            entries = m.profile_kernels()
            assert [e["kernel"] for e in entries] == ["project_kernels"] and entries[0]["launches"] == calls and entries[0]["coords"] == calls * fc.M * int(np.prod(pc.SHAPE)), entries
    finally:
        profile_off(m)


def test_a_handle_without_committed_weights_projects():
    from mri_inr_amd import ModulatedSiren

    m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0, use_bias=True, dropout=0.1, modulate=True,
                       encoder_type="custom", encoder_path=None, outer_patch_size=vc.O, inner_patch_size=vc.I, siren_patch_size=vc.S, device="cuda", activation="sine")
    d = pc.identity()  # (no load_state_dict, no .to(): nothing has committed the fresh model's weights)
    res = m.project_volume(d["volume"], d["maps"], pc.SHAPE, pc.SPACING)
    assert same(res.simulated, d["volume"]) and not m._committed


def test_the_other_geometry_calls_return_the_same_bits_before_and_after_a_project_call():
    m, d = model(), fc.planes()
    img = vc.images()
    rng = np.random.default_rng(3)
    maps = gc.truth()[:3]
    tg = rng.random((3,) + fc.SHAPE, dtype=np.float32)
    w = (0.2 + rng.random((3,) + fc.SHAPE, dtype=np.float32)).astype(np.float32)
    grid = pc.GRIDS[1]

    def others():
        r = m.align_volume_cost_w(img, tg, maps, weights=w, intensity=gc.GB_TRUTH[:3], warped=True, gradient=True)
        f = m.fuse_targets(d["targets"], d["maps"], grid, fc.SPACING, weights=d["weights"], intensity=d["intensity"], coverage=True)
        return [r.count, r.wsum, r.cost, r.grad, r.jtj, r.warped, r.wgrad, f.volume, f.coverage, f.flags]

    before = others()
    assert np.isfinite(before[7]).any() and before[0].any()
    args, kw = pc.planes(grid)
    p = m.project_volume(*args, **kw, targets=d["targets"], weights=d["weights"], coverage=True, residual=True, stats=True)
    after = others()
    assert all(same(a, b) for a, b in zip(before, after))
    again = m.project_volume(*args, **kw, targets=d["targets"], weights=d["weights"], coverage=True, residual=True, stats=True)
    assert same_gather(again, p) and same(again.residual, p.residual) and np.array_equal(again.stats, p.stats)


def test_a_fuse_project_round_trip_equals_the_same_chain_on_the_host():
    m, d, grid = model(), fc.planes(), pc.GRIDS[1]
    kw = dict(weights=d["weights"], intensity=d["intensity"])
    fused = m.fuse_targets(d["targets"], d["maps"], grid, fc.SPACING, coverage=True, **kw)
    back = m.project_volume(fused.volume, d["maps"], pc.SHAPE, pc.SPACING, intensity=d["intensity"], targets=d["targets"], weights=d["weights"], coverage=True, residual=True,
                            stats=True)
    h_fused = fuse.fuse_on_host(d["targets"], d["maps"], grid, fc.SPACING, **kw)
    h_back = host((h_fused.volume, d["maps"], pc.SHAPE, pc.SPACING), dict(intensity=d["intensity"]), d["targets"], d["weights"])
    assert same(fused.volume, h_fused.volume) and same_gather(back, h_back) and same(back.residual, h_back.residual) and np.array_equal(back.stats, h_back.stats)
    assert np.isfinite(back.simulated).sum() > 1000 and back.stats[:fc.M_PLANES, 0].min() > 100
