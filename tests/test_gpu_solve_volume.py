"""The stack that best explains all aligned targets, solved on the GPU: model.solve_volume, i.e. msiren_solve_volume* --
fuse_setup_kernel and fuse_gather_kernel (fuse.hip.h, untouched) and the kernels of solve_volume.hip.h.  Cases: tests/solve_volume_cases.py.

The device has to equal the normative restatement mri_inr_amd/solve_volume.py: solve_volume_on_host BIT FOR BIT -- volume (NaNs in the same places),
coverage, history (every rho and gamma of every iteration), flags and stopped_at -- on every case, for 0, 1, 2 and 5 iterations and lambda 0 and 0.01.
A changed order in any sum of the forward gather, the transpose, the Laplacian or the inner product shows in the fp64 history long before it would
survive the rounding of the volume to float32."""
import ctypes as C

import numpy as np
import pytest

import align_group_cases as gc
import fuse_cases as fc
import project_cases as pc
import solve_volume_cases as sc
import volume_cases as vc
from mri_inr_amd import _lib, fuse
from mri_inr_amd import solve_volume as sv
from test_gpu_align import model, profile_off, profile_on, same

pytestmark = pytest.mark.gpu

CASES = sc.all_cases()


def same_result(got, want, coverage=True, history=True):
    return (same(got.volume, want.volume) and np.array_equal(got.flags, want.flags) and got.stopped_at == want.stopped_at
            and (not coverage or same(got.coverage, want.coverage)) and (not history or same(got.history, want.history)))


@pytest.mark.parametrize("lam", sc.LAMBDAS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_device_equals_the_host_rule_bit_for_bit(name, lam):
    args, kw = CASES[name]
    m = model()
    for iterations in sc.ITERATIONS:
        got = m.solve_volume(*args, iterations=iterations, lam=lam, coverage=True, history=True, **kw)
        want = sc.expected(name, lam, iterations)
        print(f"{name} lambda {lam} iterations {iterations}: {int(np.isfinite(want.volume).sum())} voxels in the support, stopped_at {want.stopped_at}, "
              f"rho {want.history[:, 0].tolist()}")
        assert got.volume.dtype == np.float32 and got.coverage.dtype == np.float32 and got.history.dtype == np.float64 and got.flags.dtype == np.int32
        assert got.volume.shape == want.volume.shape and got.history.shape == (iterations + 1, 2)
        assert same(got.history, want.history), (iterations, got.history, want.history)
        assert same_result(got, want), iterations
    if name.startswith(("planes", "truth", "tiny", "graze", "holes", "tall")):
        assert want.stopped_at == -1 and np.isfinite(want.volume).sum() > 200 and want.history[-1, 0] < want.history[0, 0]


def test_no_iteration_returns_the_fusions_bits():
    m, d = model(), fc.planes()
    kw = dict(thickness=fc.SPACING / 4, weights=d["weights"], intensity=d["intensity"], min_coverage=0.1)
    got = m.solve_volume(d["targets"], d["maps"], sc.GRIDS[1], sc.SPACING, iterations=0, lam=0.3, coverage=True, history=True, **kw)
    f = m.fuse_targets(d["targets"], d["maps"], sc.GRIDS[1], sc.SPACING, coverage=True, **kw)
    assert same(got.volume, f.volume) and same(got.coverage, f.coverage) and np.array_equal(got.flags, f.flags) and got.stopped_at == -1
    assert np.isfinite(got.volume).sum() > 200 and got.history.shape == (1, 2) and got.history[0, 0] > 0 and np.isnan(got.history[0, 1])


def test_torch_tensors_are_accepted():
    torch = pytest.importorskip("torch")
    d = fc.planes()
    name = "holes-grid1"
    args, kw = CASES[name]
    got = model().solve_volume(torch.from_numpy(args[0].copy()), torch.from_numpy(args[1].copy()), args[2], args[3], iterations=2, lam=0.01, coverage=True, history=True,
                               thickness=kw["thickness"], weights=torch.from_numpy(d["weights"].copy()), intensity=torch.from_numpy(d["intensity"].copy()),
                               start=torch.from_numpy(kw["start"].copy()))
    assert same_result(got, sc.expected(name, 0.01, 2))


def opts(iterations=2, lam=0.01, thickness=sc.SPACING, min_coverage=0.0, spacing=sc.SPACING):
    return _lib.SolveOpts(C.sizeof(_lib.SolveOpts), iterations, spacing, thickness, min_coverage, lam)


def ptr(a):
    return a.ptr if a is not None else None


def dev_call(m, d_t, mt, shape, d_m, d_w, d_gb, o, grid, d_s, d_v, d_c, d_h, d_f, d_st):
    return m._lib.msiren_solve_volume_dev(m._h, ptr(d_t), mt, shape[0], shape[1], ptr(d_m), ptr(d_w), ptr(d_gb), C.byref(o) if o is not None else None, grid[0], grid[1], grid[2],
                                          ptr(d_s), ptr(d_v), ptr(d_c), ptr(d_h), ptr(d_f), ptr(d_st))


def test_determinism_streams_forms_and_every_subset_of_optional_outputs():
    m, d, grid, name, its, lam = model(), fc.planes(), sc.GRIDS[1], "planes-grid1-wgb", 2, 0.01
    args, kw = CASES[name]
    tg, maps, w, gb = d["targets"], d["maps"], d["weights"], d["intensity"]
    want = sc.expected(name, lam, its)
    for _ in range(2):                                                                                   # run to run
        assert same_result(m.solve_volume(*args, iterations=its, lam=lam, coverage=True, history=True, **kw), want)
    for cov in (False, True):                                                                            # the optional outputs of the Python call
        for hist in (False, True):
            r = m.solve_volume(*args, iterations=its, lam=lam, coverage=cov, history=hist, **kw)
            assert same_result(r, want, coverage=cov, history=hist) and (r.coverage is None) == (not cov) and (r.history is None) == (not hist)
    # start NULL against the fusion given as the start: the same support, the same first iterate
    fused = m.fuse_targets(tg, maps, grid, sc.SPACING, thickness=kw["thickness"], weights=w, intensity=gb)
    assert same_result(m.solve_volume(*args, iterations=its, lam=lam, coverage=True, history=True, start=fused.volume, **kw), want)
    # the _dev form against the host form, on one stream and on two alternating, calls back to back without a sync, with every subset of the optional outputs
    d_t, d_m, d_w, d_gb, d_s = (m.device_array(x.shape).copy_from(x) for x in (tg, maps, w, gb, fused.volume))
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = []
            for mask in range(16):
                d_c, d_h = m.device_array(grid) if mask & 1 else None, m.device_array((its + 1, 4)) if mask & 2 else None
                d_f, d_st = m.device_array((fc.M,)) if mask & 4 else None, m.device_array((1,)) if mask & 8 else None
                outs.append((m.device_array(grid), d_c, d_h, d_f, d_st, mask % 3 == 0))
            for d_v, d_c, d_h, d_f, d_st, with_start in outs:
                _lib.check(dev_call(m, d_t, fc.M, sc.SHAPE, d_m, d_w, d_gb, opts(its, lam), grid, d_s if with_start else None, d_v, d_c, d_h, d_f, d_st))
            m.sync()
            for d_v, d_c, d_h, d_f, d_st, with_start in outs:
                assert same(d_v.numpy(), want.volume)
                assert d_c is None or same(d_c.numpy(), want.coverage)
                assert d_h is None or same(d_h.numpy().view(np.float64), want.history)
                assert d_f is None or np.array_equal(d_f.numpy().view(np.int32), want.flags)
                assert d_st is None or d_st.numpy().view(np.int32).tolist() == [want.stopped_at]
            inplace = m.device_array(grid).copy_from(fused.volume)                                       # the start and the volume in one buffer
            _lib.check(dev_call(m, d_t, fc.M, sc.SHAPE, d_m, d_w, d_gb, opts(its, lam), grid, inplace, inplace, None, None, None, None))
            plain = m.device_array(grid)                                                                 # without weights and intensity
            _lib.check(dev_call(m, d_t, fc.M, sc.SHAPE, d_m, None, None, opts(its, lam), grid, None, plain, None, None, None, None))
            m.sync()
            assert same(inplace.numpy(), want.volume) and same(plain.numpy(), sc.expected("planes-grid1-plain", lam, its).volume)
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


def test_a_breakdown_stops_the_solve_and_leaves_the_iterate():
    """identity, lambda 0: the fusion solves the problem exactly, rho is 0 and iteration 0 stops; no target, all flagged, outside: the support is empty"""
    m = model()
    i = fc.identity()
    r = m.solve_volume(i["targets"], i["maps"], fc.IDENTITY_GRID, sc.SPACING, iterations=3, history=True)
    assert r.stopped_at == 0 and same(r.volume, i["targets"]) and (r.history[:, 0] == 0).all() and np.isnan(r.history[:, 1]).all()
    for name in ("none", "flagged", "outside"):
        args, kw = CASES[name]
        r = m.solve_volume(*args, iterations=2, lam=0.01, coverage=True, history=True, **kw)
        assert r.stopped_at == 0 and np.isnan(r.volume).all() and not r.coverage.any() and r.flags.shape == (len(args[0]),), name
        r = m.solve_volume(*args, iterations=0, **kw)
        assert r.stopped_at == -1 and np.isnan(r.volume).all()
    grid = sc.GRIDS[1]
    d_v, d_st = m.device_array(grid), m.device_array((1,))
    assert m._lib.msiren_solve_volume_dev(m._h, None, 0, 0, 0, None, None, None, C.byref(opts(1, 0.0)), *grid, None, d_v.ptr, None, None, None, d_st.ptr) == 0
    m.sync()
    assert np.isnan(d_v.numpy()).all() and d_st.numpy().view(np.int32).tolist() == [0]


def test_refusals_launch_nothing_and_name_their_argument():
    m, d, grid = model(), fc.planes(), sc.GRIDS[0]
    tg, maps = d["targets"], d["maps"]
    th, tw = sc.SHAPE
    shape = (fc.M, th, tw)
    profile_on(m)
    try:
        d_t, d_m = m.device_array(shape).copy_from(tg), m.device_array(maps.shape).copy_from(maps)
        d_v = m.device_array(grid).copy_from(np.full(grid, -7.0, np.float32))
        d_x = m.device_array((8, 4))
        vol = np.full(grid, -7.0, np.float32)
        m.sync()

        def refused(word, o=None, mt=fc.M, lattice=(th, tw), g=grid, t=True, mp=True, v=True, null_opts=False, dev_only=None):
            o = opts() if o is None else o
            if dev_only is None:
                rc = m._lib.msiren_solve_volume(m._h, tg.ctypes.data if t else None, mt, lattice[0], lattice[1], maps.ctypes.data if mp else None, None, None,
                                                None if null_opts else C.byref(o), g[0], g[1], g[2], None, vol.ctypes.data if v else None, None, None, None, None)
                assert rc == _lib.E_INVALID and word in _lib.last_error(), (word, _lib.last_error())
            p = dict(t=d_t.ptr if t else None, mp=d_m.ptr if mp else None, w=None, gb=None, s=None, v=d_v.ptr if v else None, c=None, h=None, f=None, st=None)
            p.update(dev_only or {})
            rc = m._lib.msiren_solve_volume_dev(m._h, p["t"], mt, lattice[0], lattice[1], p["mp"], p["w"], p["gb"], None if null_opts else C.byref(o), g[0], g[1], g[2], p["s"],
                                                p["v"], p["c"], p["h"], p["f"], p["st"])
            assert rc == _lib.E_INVALID and word in _lib.last_error(), (word, _lib.last_error())

        bad_size = opts()
        bad_size.struct_size = 32
        refused("struct_size", o=bad_size)
        refused("opts", null_opts=True)
        for bad in (0.0, -4.0, float("nan"), float("inf")):
            refused("spacing", o=opts(spacing=bad))
            refused("thickness", o=opts(thickness=bad))
        for bad in (-1.0, float("nan")):
            refused("min_coverage", o=opts(min_coverage=bad))
        for bad in (-1, 1025):
            refused("iterations", o=opts(iterations=bad))
        for bad in (-0.5, float("nan"), float("inf")):
            refused("lambda", o=opts(lam=bad))
        refused("th", lattice=(1, tw))
        refused("tw", lattice=(th, 1))
        refused("n_slices", g=(0, 40, 40))
        refused("height", g=(4, 0, 40))
        refused("width", g=(4, 40, -1))
        refused("n_slices height width", g=(1 << 10, 1 << 10, 1 << 10))
        refused("m_targets th tw", mt=1 << 12, lattice=(1 << 9, 1 << 9))
        refused("m_targets", mt=-1)
        refused("targets", t=False)
        refused("maps", mp=False)
        refused("volume", v=False)
        for key, name in (("t", "targets"), ("mp", "maps"), ("w", "weights"), ("gb", "intensity"), ("s", "start"), ("v", "volume"), ("c", "coverage"), ("f", "flags"),
                          ("st", "stopped_at")):
            refused(name, dev_only={key: d_x.ptr + 2})
        refused("history", dev_only={"h": d_x.ptr + 4})
        with pytest.raises(ValueError, match="lambda"):
            m.solve_volume(tg, maps, grid, sc.SPACING, iterations=1, lam=-1.0)
        for kw in (dict(weights=d["weights"][:2]), dict(intensity=d["intensity"][:, :1]), dict(start=np.zeros((4, 40, 41), np.float32))):
            with pytest.raises(ValueError):
                m.solve_volume(tg, maps, grid, sc.SPACING, iterations=1, **kw)
        for bad_t, bad_m, bad_grid in ((tg[0], maps, grid), (tg, maps[:, :5], grid), (tg, maps, grid[:2])):
            with pytest.raises(ValueError):
                m.solve_volume(bad_t, bad_m, bad_grid, sc.SPACING, iterations=1)
        m.sync()
        assert (vol == -7.0).all() and (d_v.numpy() == -7.0).all() and m.profile_kernels() == []
    finally:
        profile_off(m)
    assert same_result(m.solve_volume(*CASES["planes-grid0-plain"][0], iterations=1, coverage=True, history=True, thickness=sc.SPACING), sc.expected("planes-grid0-plain", 0.0, 1))


def test_the_profile_shows_solve_volume_kernels_once_per_call():
    m, grid = model(), sc.GRIDS[0]
    args, kw = CASES["planes-grid0-wgb"]
    profile_on(m)
    try:
        for calls in (1, 2, 3):
            m.solve_volume(*args, iterations=calls - 1, lam=0.01 * (calls - 1), coverage=calls == 2, start=pc.stack(grid) if calls == 3 else None, **kw)
            m.sync()
            entries = m.profile_kernels()
            assert [e["kernel"] for e in entries] == ["solve_volume_kernels"] and entries[0]["launches"] == calls and entries[0]["coords"] == calls * int(np.prod(grid)), entries
    finally:
        profile_off(m)


def test_a_handle_without_committed_weights_solves():
    from mri_inr_amd import ModulatedSiren

    m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0, use_bias=True, dropout=0.1, modulate=True,
                       encoder_type="custom", encoder_path=None, outer_patch_size=vc.O, inner_patch_size=vc.I, siren_patch_size=vc.S, device="cuda", activation="sine")
    args, kw = CASES["tiny"]  # (no load_state_dict, no .to(): nothing has committed the fresh model's weights)
    assert same_result(m.solve_volume(*args, iterations=2, lam=0.01, coverage=True, history=True, **kw), sc.expected("tiny", 0.01, 2)) and not m._committed


def test_the_other_geometry_calls_return_the_same_bits_before_and_after_a_solve():
    m, d = model(), fc.planes()
    img = vc.images()
    rng = np.random.default_rng(3)
    maps = gc.truth()[:3]
    tg = rng.random((3,) + fc.SHAPE, dtype=np.float32)
    w = (0.2 + rng.random((3,) + fc.SHAPE, dtype=np.float32)).astype(np.float32)
    grid = sc.GRIDS[1]

    def others():
        r = m.align_volume_cost_w(img, tg, maps, weights=w, intensity=gc.GB_TRUTH[:3], warped=True, gradient=True)
        f = m.fuse_targets(d["targets"], d["maps"], grid, fc.SPACING, weights=d["weights"], intensity=d["intensity"], coverage=True)
        p = m.project_volume(pc.holes(grid), d["maps"], pc.SHAPE, pc.SPACING, intensity=d["intensity"], targets=d["targets"], weights=d["weights"], coverage=True, residual=True,
                             stats=True)
        return [r.count, r.wsum, r.cost, r.grad, r.jtj, r.warped, r.wgrad, f.volume, f.coverage, f.flags, p.simulated, p.coverage, p.residual, p.stats, p.flags]

    before = others()
    assert np.isfinite(before[7]).any() and before[0].any() and np.isfinite(before[10]).any()
    args, kw = CASES["truth-t4"]                                                                         # (a larger block of the stream's scratch than theirs)
    s = m.solve_volume(*args, iterations=2, lam=0.01, coverage=True, history=True, **kw)
    after = others()
    assert all(same(a, b) for a, b in zip(before, after))
    assert same_result(m.solve_volume(*args, iterations=2, lam=0.01, coverage=True, history=True, **kw), s) and same_result(s, sc.expected("truth-t4", 0.01, 2))


def test_the_device_loop_equals_the_same_chain_of_host_operators():
    """one iteration by hand from the pieces of the restatement, on the device's own fusion: x_1 = x_0 + (rho / gamma) r"""
    m = model()
    args, kw = CASES["truth-t4"]
    got = m.solve_volume(*args, iterations=1, lam=0.01, history=True, **kw)
    fused = m.fuse_targets(*args, **kw)
    S = np.isfinite(fused.volume)
    geo = sv.geometry(args[0], args[1], S, sc.SPACING, thickness=kw["thickness"])
    x = np.where(S, fused.volume.astype(np.float64), 0.0)
    r = sv.transpose_on_host(geo, np.where(geo.active, geo.omega_gg * geo.tau, 0.0)) - sv.apply_on_host(geo, x, 0.01)
    rho = sv.ordered_dot(r, r, S)
    gamma = sv.ordered_dot(r, sv.apply_on_host(geo, r, 0.01), S)
    assert got.history[0].tolist() == [rho, gamma] and same(got.volume, np.where(S, (x + (rho / gamma) * r).astype(np.float32), np.float32(np.nan)))
