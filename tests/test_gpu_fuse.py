"""Aligned target slices gathered back onto the stack's voxel grid on the GPU: model.fuse_targets, i.e. msiren_fuse_targets* --
fuse_setup_kernel and fuse_gather_kernel (fuse.hip.h).  Cases: tests/fuse_cases.py.

The device has to equal the normative restatement mri_inr_amd/fuse.py: fuse_on_host BIT FOR BIT -- volume, coverage (NaNs in the same places) and
flags -- on every case, grid and thickness, with and without weights and intensity.  The graze cases put the window's edge and the lattice's last row
and column on tile-corner voxels, and one ulp either side: there a tile-level cull that dropped a (tile, target) pair it must visit would show as a
NaN, or as other bits, in that corner row."""
import ctypes as C

import numpy as np
import pytest

import align_group_cases as gc
import fuse_cases as fc
import volume_cases as vc
from mri_inr_amd import _lib, align_volume as av, fuse
from test_gpu_align import model, profile_off, profile_on, same

pytestmark = pytest.mark.gpu


def same_result(a, b, coverage=True):
    return same(a.volume, b.volume) and np.array_equal(a.flags, b.flags) and (not coverage or same(a.coverage, b.coverage))


def optional(d, weights, intensity):
    return dict(weights=d["weights"] if weights else None, intensity=d["intensity"] if intensity else None)


@pytest.mark.parametrize("intensity", [True, False])
@pytest.mark.parametrize("weights", [True, False])
@pytest.mark.parametrize("thickness", fc.THICKNESSES)
@pytest.mark.parametrize("grid", fc.GRIDS)
def test_the_device_equals_the_host_rule_bit_for_bit(grid, thickness, weights, intensity):
    d = fc.planes()
    kw = dict(thickness=thickness, **optional(d, weights, intensity))
    got = model().fuse_targets(d["targets"], d["maps"], grid, fc.SPACING, coverage=True, **kw)
    want = fuse.fuse_on_host(d["targets"], d["maps"], grid, fc.SPACING, **kw)
    print(f"{grid} thickness {thickness} weights {weights} intensity {intensity}: {int(np.isfinite(want.volume).sum())} voxels covered, flags {want.flags.tolist()}")
    assert got.volume.dtype == np.float32 and got.coverage.dtype == np.float32 and got.flags.dtype == np.int32 and got.volume.shape == grid
    assert np.isfinite(want.volume).sum() > 500 and want.flags[fc.DEGENERATE_AT] == fuse.DEGENERATE and bool(want.flags[fc.ZERO_GAIN_AT]) == intensity
    assert same_result(got, want)


@pytest.mark.parametrize("shift", fc.GRAZE_SHIFTS)
@pytest.mark.parametrize("grid", fc.GRIDS)
def test_the_graze_cases_equal_the_host_rule_bit_for_bit(grid, shift):
    d = fc.graze(shift)
    for thickness in fc.GRAZE_THICKNESSES:
        for rows in (slice(None), slice(0, 1), slice(1, 2), slice(2, 3)):  # together, and each target alone: nothing else covers its corner row
            got = model().fuse_targets(d["targets"][rows], d["maps"][rows], grid, fc.SPACING, thickness=thickness, coverage=True)
            want = fuse.fuse_on_host(d["targets"][rows], d["maps"][rows], grid, fc.SPACING, thickness=thickness)
            assert same_result(got, want), (thickness, rows)
    edge = fuse.fuse_on_host(d["targets"][:1], d["maps"][:1], grid, fc.SPACING, thickness=fc.GRAZE_THICKNESSES[2]).coverage[2, 16:32]
    if shift == 0:  # the tile y = 16 .. 31 of slice 2 is reached through its last row alone
        assert not edge[:15].any() and edge[15, :23].all()


def test_identity_returns_the_targets_bits():
    d = fc.identity()
    res = model().fuse_targets(d["targets"], d["maps"], fc.IDENTITY_GRID, fc.SPACING, coverage=True)
    assert same(res.volume, d["targets"]) and (res.coverage == 1.0).all() and not res.flags.any()


def test_torch_tensors_are_accepted():
    torch = pytest.importorskip("torch")
    d = fc.planes()
    got = model().fuse_targets(torch.from_numpy(d["targets"].copy()), torch.from_numpy(d["maps"].copy()), fc.GRIDS[0], fc.SPACING, weights=torch.from_numpy(d["weights"].copy()),
                               intensity=torch.from_numpy(d["intensity"].copy()), coverage=True)
    assert same_result(got, fuse.fuse_on_host(d["targets"], d["maps"], fc.GRIDS[0], fc.SPACING, weights=d["weights"], intensity=d["intensity"]))


def dev_call(m, d_t, mt, th, tw, d_m, d_w, d_gb, o, grid, d_v, d_c, d_f):
    ptr = lambda a: a.ptr if a is not None else None  # noqa: E731
    return m._lib.msiren_fuse_targets_dev(m._h, ptr(d_t), mt, th, tw, ptr(d_m), ptr(d_w), ptr(d_gb), C.byref(o), grid[0], grid[1], grid[2], ptr(d_v), ptr(d_c), ptr(d_f))


def opts(thickness=fc.SPACING, min_coverage=0.0, spacing=fc.SPACING):
    return _lib.FuseOpts(C.sizeof(_lib.FuseOpts), 0, spacing, thickness, min_coverage)


def test_determinism_streams_forms_optional_outputs_and_a_target_that_contributes_nowhere():
    m, d, grid = model(), fc.planes(), fc.GRIDS[1]
    tg, maps, w, gb = d["targets"], d["maps"], d["weights"], d["intensity"]
    th, tw = fc.SHAPE
    want = fuse.fuse_on_host(tg, maps, grid, fc.SPACING, weights=w, intensity=gb)
    first = m.fuse_targets(tg, maps, grid, fc.SPACING, weights=w, intensity=gb, coverage=True)
    again = m.fuse_targets(tg, maps, grid, fc.SPACING, weights=w, intensity=gb, coverage=True)
    assert same_result(first, want) and same_result(again, first)                                        # run to run
    bare = m.fuse_targets(tg, maps, grid, fc.SPACING, weights=w, intensity=gb)                           # without the coverage
    assert bare.coverage is None and same_result(bare, first, coverage=False)
    o = fc.outside_target()                                                                              # a target that contributes nowhere, appended
    more = m.fuse_targets(np.concatenate([tg, o["targets"]]), np.concatenate([maps, o["maps"]]), grid, fc.SPACING, weights=np.concatenate([w, o["weights"]]),
                          intensity=np.concatenate([gb, o["intensity"]]), coverage=True)
    assert same(more.volume, first.volume) and same(more.coverage, first.coverage) and more.flags.tolist() == first.flags.tolist() + [0]
    some = m.fuse_targets(tg, maps, grid, fc.SPACING, weights=w, intensity=gb, min_coverage=0.25, coverage=True)   # min_coverage only turns values into NaN
    assert same_result(some, fuse.fuse_on_host(tg, maps, grid, fc.SPACING, weights=w, intensity=gb, min_coverage=0.25))
    assert 0 < np.isfinite(some.volume).sum() < np.isfinite(first.volume).sum() and same(some.coverage, first.coverage)
    # the _dev form against the host form, on one stream and on two alternating, calls back to back without a sync, with and without the optional outputs
    d_t, d_m, d_w, d_gb = (m.device_array(x.shape).copy_from(x) for x in (tg, maps, w, gb))
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array(grid), m.device_array(grid) if k != 1 else None, m.device_array((fc.M,)) if k != 1 else None) for k in range(streams + 2)]
            for d_v, d_c, d_f in outs:
                _lib.check(dev_call(m, d_t, fc.M, th, tw, d_m, d_w, d_gb, opts(), grid, d_v, d_c, d_f))
            m.sync()
            for d_v, d_c, d_f in outs:
                assert same(d_v.numpy(), first.volume)
                assert d_c is None or same(d_c.numpy(), first.coverage)
                assert d_f is None or np.array_equal(d_f.numpy().view(np.int32), first.flags)
            plain = m.device_array(grid)                                                                 # without weights and intensity
            _lib.check(dev_call(m, d_t, fc.M, th, tw, d_m, None, None, opts(), grid, plain, None, None))
            m.sync()
            assert same(plain.numpy(), fuse.fuse_on_host(tg, maps, grid, fc.SPACING).volume)
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


def test_no_target_gives_nan_and_zero_coverage():
    m, grid = model(), fc.GRIDS[1]
    res = m.fuse_targets(np.zeros((0,) + fc.SHAPE, np.float32), np.zeros((0, 9), np.float32), grid, fc.SPACING, coverage=True)
    assert res.volume.shape == grid and np.isnan(res.volume).all() and res.coverage.shape == grid and not res.coverage.any() and res.flags.shape == (0,)
    want = fuse.fuse_on_host(np.zeros((0,) + fc.SHAPE, np.float32), np.zeros((0, 9), np.float32), grid, fc.SPACING)
    assert same_result(res, want)
    d_v, d_c = m.device_array(grid).copy_from(np.ones(grid, np.float32)), m.device_array(grid).copy_from(np.ones(grid, np.float32))
    assert m._lib.msiren_fuse_targets_dev(m._h, None, 0, 0, 0, None, None, None, None, *grid, d_v.ptr, d_c.ptr, None) == 0  # opts may be null without a target
    m.sync()
    assert np.isnan(d_v.numpy()).all() and not d_c.numpy().any()
    flagged = fc.planes()                                                                               # every target flagged: the same
    res = m.fuse_targets(flagged["targets"][6:], flagged["maps"][6:], grid, fc.SPACING, intensity=flagged["intensity"][6:], coverage=True)
    assert np.isnan(res.volume).all() and not res.coverage.any() and res.flags.tolist() == [fuse.DEGENERATE, fuse.BAD_INTENSITY]


def test_refusals_launch_nothing_and_name_their_argument():
    m, d, grid = model(), fc.planes(), fc.GRIDS[0]
    tg, maps = d["targets"], d["maps"]
    th, tw = fc.SHAPE
    profile_on(m)
    try:
        d_t, d_m = m.device_array(tg.shape).copy_from(tg), m.device_array(maps.shape).copy_from(maps)
        d_v = m.device_array(grid).copy_from(np.full(grid, -7.0, np.float32))
        vol = np.full(grid, -7.0, np.float32)
        m.sync()

        def refused(word, o=None, mt=fc.M, shape=(th, tw), g=grid, t=True, mp=True, v=True, null_opts=False, dev_only=None):
            o = opts() if o is None else o
            if dev_only is None:
                rc = m._lib.msiren_fuse_targets(m._h, tg.ctypes.data if t else None, mt, shape[0], shape[1], maps.ctypes.data if mp else None, None, None,
                                                None if null_opts else C.byref(o), g[0], g[1], g[2], vol.ctypes.data if v else None, None, None)
                assert rc == _lib.E_INVALID and word in _lib.last_error(), (word, _lib.last_error())
            ptrs = dict(t=d_t.ptr if t else None, mp=d_m.ptr if mp else None, w=None, gb=None, v=d_v.ptr if v else None, c=None, f=None)
            ptrs.update(dev_only or {})
            rc = m._lib.msiren_fuse_targets_dev(m._h, ptrs["t"], mt, shape[0], shape[1], ptrs["mp"], ptrs["w"], ptrs["gb"], None if null_opts else C.byref(o), g[0], g[1], g[2],
                                                ptrs["v"], ptrs["c"], ptrs["f"])
            assert rc == _lib.E_INVALID and word in _lib.last_error(), (word, _lib.last_error())

        bad_size = opts()
        bad_size.struct_size = 24
        refused("struct_size", o=bad_size)
        for bad in (0.0, -4.0, float("nan"), float("inf")):
            refused("spacing", o=opts(spacing=bad))
            refused("thickness", o=opts(thickness=bad))
        for bad in (-1.0, float("nan")):
            refused("min_coverage", o=opts(min_coverage=bad))
        refused("th", shape=(1, tw))
        refused("tw", shape=(th, 1))
        refused("n_slices", g=(0, 40, 40))
        refused("height", g=(4, 0, 40))
        refused("width", g=(4, 40, -1))
        refused("n_slices height width", g=(1 << 10, 1 << 10, 1 << 10))
        refused("m_targets th tw", mt=1 << 12, shape=(1 << 9, 1 << 9))
        refused("m_targets", mt=-1)
        refused("targets", t=False)
        refused("maps", mp=False)
        refused("volume", v=False)
        refused("opts", null_opts=True)
        for key, name in (("t", "targets"), ("mp", "maps"), ("w", "weights"), ("gb", "intensity"), ("v", "volume"), ("c", "coverage"), ("f", "flags")):
            refused(name, dev_only={key: d_v.ptr + 2})
        with pytest.raises(ValueError, match="thickness"):
            m.fuse_targets(tg, maps, grid, fc.SPACING, thickness=0.0)
        for bad_tg, bad_maps, kw in ((tg[0], maps, {}), (tg, maps[:, :5], {}), (tg, maps, dict(weights=d["weights"][:2])), (tg, maps, dict(intensity=d["intensity"][:, :1]))):
            with pytest.raises(ValueError):
                m.fuse_targets(bad_tg, bad_maps, grid, fc.SPACING, **kw)
        m.sync()
        assert (vol == -7.0).all() and (d_v.numpy() == -7.0).all() and m.profile_kernels() == []
    finally:
        profile_off(m)
    assert same_result(m.fuse_targets(tg, maps, grid, fc.SPACING, coverage=True), fuse.fuse_on_host(tg, maps, grid, fc.SPACING))  # the handle stays usable


def test_the_profile_shows_fuse_kernels_once_per_call():
    m, d, grid = model(), fc.planes(), fc.GRIDS[0]
    profile_on(m)
    try:
        for calls in (1, 2, 3):
            m.fuse_targets(d["targets"], d["maps"], grid, fc.SPACING, weights=d["weights"], intensity=d["intensity"], coverage=calls == 2)
            m.sync()
            entries = [e for e in m.profile_kernels() if "fuse" in e["kernel"]]
            assert [e["kernel"] for e in entries] == ["fuse_kernels"] and entries[0]["launches"] == calls and entries[0]["coords"] == calls * int(np.prod(grid)), entries
        assert [e["kernel"] for e in m.profile_kernels()] == ["fuse_kernels"]  # no trunk, no prologue: nothing else ran
    finally:
        profile_off(m)


def test_a_handle_without_committed_weights_fuses():
    from mri_inr_amd import ModulatedSiren

    m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0, use_bias=True, dropout=0.1, modulate=True,
                       encoder_type="custom", encoder_path=None, outer_patch_size=vc.O, inner_patch_size=vc.I, siren_patch_size=vc.S, device="cuda", activation="sine")
    d = fc.identity()  # (no load_state_dict, no .to(): nothing has committed the fresh model's weights)
    res = m.fuse_targets(d["targets"], d["maps"], fc.IDENTITY_GRID, fc.SPACING)
    assert same(res.volume, d["targets"]) and not m._committed


def test_the_other_geometry_calls_return_the_same_bits_before_and_after_a_fuse_call():
    m, d = model(), fc.planes()
    img = vc.images()
    rng = np.random.default_rng(3)
    maps = gc.truth()[:3]
    tg = rng.random((3,) + fc.SHAPE, dtype=np.float32)
    w = (0.2 + rng.random((3,) + fc.SHAPE, dtype=np.float32)).astype(np.float32)
    pts = np.concatenate([av.map_points3(mp, (5, 7)) for mp in maps]).astype(np.float32)

    def others():
        r = m.align_volume_cost_w(img, tg, maps, weights=w, intensity=gc.GB_TRUTH[:3], warped=True, gradient=True)
        v, g = m.resample_volume_with_gradient(img, pts)
        return [r.count, r.wsum, r.cost, r.grad, r.jtj, r.warped, r.wgrad, v, g]

    before = others()
    assert np.isfinite(before[7]).any() and before[0].any()
    fused = m.fuse_targets(d["targets"], d["maps"], fc.GRIDS[1], fc.SPACING, weights=d["weights"], intensity=d["intensity"], coverage=True)
    after = others()
    assert all(same(a, b) for a, b in zip(before, after))
    assert same_result(m.fuse_targets(d["targets"], d["maps"], fc.GRIDS[1], fc.SPACING, weights=d["weights"], intensity=d["intensity"], coverage=True), fused)
