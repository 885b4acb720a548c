"""msiren_align_stack_r and msiren_align_stack_solve_group_r on the device against mri_inr_amd/align_stack.py, the host
restatement: warped, wgrad, rweight and all 80 sums bit for bit on every case, scale and lattice of tests/align_stack_cases.py; the solve bit for bit
against the host loop around the device's own cost, report, target report and trace included; determinism; refusals; the profile; a handle without
weights; the neighbours untouched; and one pass of the outer loop reconstruct -> register -> reconstruct against the same chain on the host."""
import ctypes as C
import functools

import numpy as np
import pytest

import align_stack_cases as sc
import fuse_cases as fc
from mri_inr_amd import ModulatedSiren, _lib, align_group as ag, align_robust as ar, align_stack as ast, align_volume as av
from test_gpu_align import profile_off, profile_on, same

pytestmark = pytest.mark.gpu

SUMS = 80
KW = dict(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0, use_bias=True, dropout=0.1, modulate=True, encoder_type="custom",
          encoder_path=None, outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda", activation="sine")


@functools.lru_cache(maxsize=None)
def model():
    """a handle whose weights were never committed: no load_state_dict, no .to()"""
    return ModulatedSiren(**KW)


def f64_dev(m, x):
    x = np.ascontiguousarray(x, np.float64)
    return m.device_array(x.shape + (2,)).copy_from(x.view(np.float32).reshape(x.shape + (2,)))


def f64_of(d):
    a = d.numpy()
    return a.view(np.float64).reshape(a.shape[:-1])


def packed(res):
    iu = np.triu_indices(11)
    return np.concatenate([res.count[:, None].astype(np.float64), res.wsum[:, None], res.cost[:, None], res.grad, res.jtj[:, iu[0], iu[1]]], axis=1)


def same_result(a, b):
    return all(same(x, y) if x is not None and y is not None else x is y for x, y in zip(a, b))


def cost(d, s, **kw):
    return model().align_stack_cost(d["stack"], d["targets"], d["maps"], scale=s, weights=d["weights"], intensity=d["intensity"], **kw)


ALL = dict(warped=True, gradient=True, rweight=True)


# ---- the cost -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", [(n, s) for n in sc.STACKS for s in sc.LATTICES])
def test_every_output_equals_the_restatement_bit_for_bit(name, shape):
    d = sc.data(name, shape)
    for k, s in enumerate(sc.SCALES):
        got = cost(d, s, **ALL)
        want = ast.result_on_host(d["stack"], d["targets"], d["maps"], s, weights=d["weights"], intensity=d["intensity"])
        for f in got._fields:
            assert same(getattr(got, f), getattr(want, f)), (k, f)
        assert got.warped.dtype == np.float32 and got.wgrad.shape == (3, sc.M) + shape and not got.count[list(sc.OUTSIDE)].any()
    plain = model().align_stack_cost(d["stack"], d["targets"], d["maps"])  # scale +inf, no weights, no intensity
    assert same_result(plain, ar.unpack_r(ast.cost_on_host(d["stack"], d["targets"], d["maps"])[0]))


def test_the_same_bits_run_to_run_for_every_subset_of_outputs_alone_or_in_a_batch():
    d = sc.data("holes", (33, 37))
    s = sc.SCALES[1]
    full = cost(d, s, **ALL)
    for bits in range(8):
        kw = dict(warped=bool(bits & 1), gradient=bool(bits & 2), rweight=bool(bits & 4))
        got = cost(d, s, **kw)
        assert np.array_equal(packed(got), packed(full)), bits
        for f, on in (("warped", kw["warped"]), ("wgrad", kw["gradient"]), ("rweight", kw["rweight"])):
            assert same(getattr(got, f), getattr(full, f)) if on else getattr(got, f) is None, (bits, f)
    for q in (0, 4, 5, 10):
        one = model().align_stack_cost(d["stack"], d["targets"][q:q + 1], d["maps"][q:q + 1], scale=s[q:q + 1], weights=d["weights"][q:q + 1],
                                       intensity=d["intensity"][q:q + 1], **ALL)
        assert np.array_equal(packed(one)[0], packed(full)[q]) and same(one.warped[0], full.warped[q]) and same(one.wgrad[:, 0], full.wgrad[:, q]), q


def test_the_dev_form_on_one_and_two_streams_gives_the_host_forms_bits():
    m, shape = model(), (33, 37)
    d = sc.data("smooth", shape)
    s = sc.SCALES[2]
    res = cost(d, s, **ALL)
    th, tw = shape
    dv = {k: m.device_array(d[k].shape).copy_from(d[k]) for k in ("stack", "targets", "maps", "weights", "intensity")}
    d_sc = f64_dev(m, s)
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [(m.device_array((sc.M, 2 * SUMS)),) + tuple(m.device_array(x) if k != 1 else None for x in ((sc.M, th, tw), (3, sc.M, th, tw), (sc.M, th, tw)))
                    for k in range(streams + 2)]
            for d_s, d_wp, d_g, d_rw in outs:  # back to back, no sync in between: the calls alternate over the streams
                _lib.check(m._lib.msiren_align_stack_r_dev(m._h, dv["stack"].ptr, sc.N, sc.H, sc.W, dv["targets"].ptr, sc.M, th, tw, dv["maps"].ptr, dv["weights"].ptr,
                                                           dv["intensity"].ptr, d_sc.ptr, d_s.ptr, d_wp.ptr if d_wp else None, d_g.ptr if d_g else None,
                                                           d_rw.ptr if d_rw else None))
            m.sync()
            for d_s, d_wp, d_g, d_rw in outs:
                assert np.array_equal(d_s.numpy().view(np.float64), packed(res)), streams
                assert d_wp is None or (same(d_wp.numpy(), res.warped) and same(d_g.numpy(), res.wgrad) and same(d_rw.numpy(), res.rweight)), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


def test_targets_that_are_the_warped_planes_cost_exactly_nothing():
    d = sc.data("smooth", (19, 23))
    wp = model().align_stack_cost(d["stack"], d["targets"], d["maps"], warped=True).warped
    tg = np.where(np.isfinite(wp), wp, np.float32(0.5))
    for s in (sc.INF, 0.01):
        res = model().align_stack_cost(d["stack"], tg, d["maps"], scale=s, weights=d["weights"], rweight=True)
        assert (res.cost == 0.0).all() and (res.grad == 0.0).all() and res.count.sum() > 2000
        assert (res.rweight[np.isfinite(res.rweight)] == 1.0).all()


# ---- the solve ----------------------------------------------------------------------------------------------------------------------------------------
def solve(case, est, groups=sc.GROUP_START, rows=slice(None), rigid=None, trace=True):
    w, s = sc.solve_case(case)
    gb = sc.start_intensity(est)
    count = len(w[rows])
    rigid = sc.start_rigid(count if groups is None else len(ag.group_offsets(groups, count)) - 1) if rigid is None else rigid
    return model().align_stack_solve(sc.stack("smooth"), sc.solve_targets()[rows], sc.planes()[rows], sc.SPACING, groups=groups, scale=s[rows],
                                     rotation=rigid[:, :9].reshape(-1, 3, 3), shift=rigid[:, 9:], weights=w[rows], intensity=None if gb is None else gb[rows],
                                     estimate_intensity=est == av.ESTIMATE, iterations=sc.ITERATIONS, trace=trace)


@pytest.mark.parametrize("est", sc.MODES)
@pytest.mark.parametrize("case", ("masked", "robust"))
def test_the_solve_is_the_host_loop_around_the_devices_cost_bit_for_bit(case, est):
    w, s = sc.solve_case(case)
    got = solve(case, est)

    def device_cost(maps, gb, scale):
        return packed(model().align_stack_cost(sc.stack("smooth"), sc.solve_targets(), maps, scale=scale, weights=w, intensity=gb))

    want, _ = ast.solve_on_host_s(None, None, sc.GROUP_START, s, rigid=sc.start_rigid(), planes=sc.planes(), intensity=sc.start_intensity(est), options=sc.options(est),
                                  trace=True, cost_fn=device_cost)
    for f in got._fields:
        assert same(getattr(got, f), getattr(want, f)), f
    assert same_result(got, sc.reference_solve(case, est)[0])  # and the loop on the host restatement: the same bits again
    e = sc.errors(got, est)
    print(case, est, e, "gate", sc.device_solve_gate(case))
    assert (e[list(sc.GATE_GROUPS)] <= sc.device_solve_gate(case)).all()
    assert got.count[sc.SOLVE_OUTSIDE] == 0 and np.abs(got.maps[sc.SOLVE_OUTSIDE].astype(np.float64) - sc.truth()[sc.SOLVE_OUTSIDE]).max() <= sc.device_solve_gate(case)
    assert same_result(solve(case, est), got)  # run to run


def test_no_groups_means_singletons_and_an_all_outside_group_keeps_its_inputs():
    est = av.FIXED
    none = solve("masked", est, groups=None)
    explicit = solve("masked", est, groups=list(range(sc.SOLVE_M + 1)))
    ones = solve("masked", est, groups=[1] * sc.SOLVE_M)
    assert same_result(none, explicit) and same_result(none, ones) and none.rotation.shape == (sc.SOLVE_M, 3, 3) and none.trace.shape == (sc.ITERATIONS, sc.SOLVE_M, 15)
    q = sc.SOLVE_OUTSIDE  # alone, the outside member has nothing to go by: both flags, the inputs kept
    assert none.flags[q] == (av.NO_OVERLAP | av.SINGULAR) and none.count[q] == 0 and none.accepted[q] == 0
    assert np.array_equal(none.rotation[q], np.eye(3)) and not none.shift[q].any() and np.array_equal(none.maps[q], sc.maps_of(sc.start_rigid())[q])
    assert (none.flags[:q] == 0).all()
    alone = solve("masked", est, groups=None, rows=slice(3, 4))  # a target alone or inside a batch
    assert np.array_equal(alone.maps[0], none.maps[3]) and np.array_equal(alone.trace[:, 0], none.trace[:, 3]) and alone.cost[0] == none.cost[3]


def test_the_solves_dev_form_gives_the_host_forms_bits():
    m, est, case = model(), av.ESTIMATE, "robust"
    res = solve(case, est)
    w, s = sc.solve_case(case)
    IT, G, SM = sc.ITERATIONS, sc.G, sc.SOLVE_M
    o = _lib.AlignVolumeSolveGroupOpts(C.sizeof(_lib.AlignVolumeSolveGroupOpts), IT, est, 0, 1e-3, 0.1, 10.0, 1e-9, 1e9, sc.SPACING)
    st, tg = sc.stack("smooth"), sc.solve_targets()
    d = dict(stack=m.device_array(st.shape).copy_from(st), targets=m.device_array(tg.shape).copy_from(tg), planes=f64_dev(m, sc.planes()), rigid=f64_dev(m, sc.start_rigid()),
             weights=m.device_array(w.shape).copy_from(w), scale=f64_dev(m, s))
    gs = np.ascontiguousarray(sc.GROUP_START, np.int32)
    p = lambda x: None if x is None else x.ptr  # noqa: E731
    try:
        for streams in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, streams))
            outs = [dict(out=m.device_array((SM, 9)), gout=m.device_array((SM, 2)), rep=m.device_array((G, 7, 2)), rout=m.device_array((G, 12, 2)) if k != 1 else None,
                         trep=m.device_array((SM, 3, 2)) if k != 1 else None, trace=m.device_array((IT, G, 15, 2)) if k != 1 else None) for k in range(streams + 1)]
            for x in outs:
                _lib.check(m._lib.msiren_align_stack_solve_group_r_dev(m._h, d["stack"].ptr, sc.N, sc.H, sc.W, d["targets"].ptr, SM, sc.SHAPE[0], sc.SHAPE[1], C.byref(o),
                                                                       gs.ctypes.data, G, d["planes"].ptr, d["rigid"].ptr, d["weights"].ptr, None, d["scale"].ptr, x["out"].ptr,
                                                                       x["gout"].ptr, p(x["rout"]), x["rep"].ptr, p(x["trep"]), p(x["trace"])))
            m.sync()
            for x in outs:
                rep = f64_of(x["rep"])
                assert np.array_equal(x["out"].numpy(), res.maps) and np.array_equal(x["gout"].numpy(), res.intensity), streams
                assert np.array_equal(rep[:, 1], res.mean_first) and np.array_equal(rep[:, 2], res.mean_best) and np.array_equal(rep[:, 6], res.flags), streams
                if x["trace"] is not None:
                    assert np.array_equal(f64_of(x["trace"]), res.trace) and np.array_equal(f64_of(x["trep"])[:, 2], res.cost), streams
                    assert np.array_equal(f64_of(x["rout"])[:, 9:], res.shift), streams
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


# ---- refusals, the profile, the handle ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_launches_nothing_and_names_its_argument():
    m, shape = model(), (19, 23)
    d = sc.data("smooth", shape)
    st, tg, mp, w, gb = d["stack"], d["targets"], d["maps"], d["weights"], d["intensity"]
    s = np.full(sc.M, 0.01)
    sums = np.full((sc.M, SUMS), -7.0)
    dbuf = m.device_array(st.shape).copy_from(st)
    m.sync()
    profile_on(m)
    try:
        def host(word, n=sc.N, h=sc.H, wd=sc.W, mm=sc.M, th=shape[0], tw=shape[1], **null):
            a = dict(stack=st.ctypes.data, targets=tg.ctypes.data, maps=mp.ctypes.data, scale=s.ctypes.data, sums=sums.ctypes.data)
            a.update({k: None for k in null})
            rc = m._lib.msiren_align_stack_r(m._h, a["stack"], n, h, wd, a["targets"], mm, th, tw, a["maps"], w.ctypes.data, gb.ctypes.data, a["scale"], a["sums"], None, None, None)
            assert rc == _lib.E_INVALID and word in _lib.last_error(), (word, rc, _lib.last_error())

        def dev(word, n=sc.N, h=sc.H, wd=sc.W, mm=2, th=4, tw=4, **ptr):
            a = dict(stack=dbuf.ptr, targets=dbuf.ptr, maps=dbuf.ptr, weights=None, intensity=None, scale=dbuf.ptr, sums=dbuf.ptr, warped=None, wgrad=None, rweight=None)
            a.update(ptr)
            rc = m._lib.msiren_align_stack_r_dev(m._h, a["stack"], n, h, wd, a["targets"], mm, th, tw, a["maps"], a["weights"], a["intensity"], a["scale"], a["sums"],
                                                 a["warped"], a["wgrad"], a["rweight"])
            assert rc == _lib.E_INVALID and word in _lib.last_error(), (word, rc, _lib.last_error())

        for f in (host, dev):
            f("n =", n=1)
            f("height", h=1)
            f("width", wd=1)
            f("bad arguments", n=-1)
            f("bad arguments", mm=-1)
            f("n height width", n=1 << 10, h=1 << 10, wd=1 << 10)
            f("n height width", n=1 << 25, h=2, wd=2)
            f("m th tw", mm=1 << 12, th=1 << 8, tw=1 << 8)
        for k in ("stack", "targets", "maps", "scale", "sums"):
            host(k, **{k: None})
            dev(k, **{k: None})
        for k, off in (("stack", 2), ("targets", 2), ("maps", 2), ("weights", 2), ("intensity", 2), ("warped", 2), ("wgrad", 2), ("rweight", 2), ("scale", 4), ("sums", 4)):
            dev("aligned", **{k: dbuf.ptr + off})
        with pytest.raises(ValueError, match="stack"):
            m.align_stack_cost(st[0], tg, mp)
        for kw in (dict(weights=w[:2]), dict(intensity=gb[:3]), dict(scale=s[:3])):
            with pytest.raises(ValueError):
                m.align_stack_cost(st, tg, mp, **kw)
        with pytest.raises(ValueError):
            m.align_stack_cost(st, tg, mp[:, :6])
        # nothing to do: no target, or an empty lattice -- whatever the stack is
        assert m._lib.msiren_align_stack_r(m._h, None, 0, 0, 0, None, 0, shape[0], shape[1], None, None, None, None, sums.ctypes.data, None, None, None) == 0
        assert m._lib.msiren_align_stack_r_dev(m._h, dbuf.ptr, 1, 1, 1, dbuf.ptr, 2, 0, 4, dbuf.ptr, None, None, None, dbuf.ptr, None, None, None) == 0

        # the solve
        SM, G = sc.SOLVE_M, sc.G
        stg, pl, rigid, sw = sc.solve_targets(), sc.planes(), sc.start_rigid(), sc.solve_weights(True)
        ssc = np.full(SM, 0.01)
        out, gout, rout, rep = np.full((SM, 9), -7.0, np.float32), np.full((SM, 2), -7.0, np.float32), np.full((G, 12), -7.0), np.full((G, 7), -7.0)
        gs = np.ascontiguousarray(sc.GROUP_START, np.int32)

        def opts(iterations=4, est=1, struct_size=None, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, spacing=sc.SPACING):
            T = _lib.AlignVolumeSolveGroupOpts
            return T(C.sizeof(T) if struct_size is None else struct_size, iterations, est, 0, damping, down, up, lam_min, lam_max, spacing)

        def hsolve(word, o, ng=G, groups=gs, n=sc.N, **null):
            a = dict(stack=st.ctypes.data, targets=stg.ctypes.data, planes=pl.ctypes.data, rigid=rigid.ctypes.data, scale=ssc.ctypes.data, out=out.ctypes.data,
                     gout=gout.ctypes.data, rep=rep.ctypes.data)
            a.update({k: None for k in null})
            for form in ("host", "dev"):
                if form == "dev":  # the same refusals come before any device pointer is looked at
                    a = {k: (dbuf.ptr if v is not None else None) for k, v in a.items()}
                fn = m._lib.msiren_align_stack_solve_group_r if form == "host" else m._lib.msiren_align_stack_solve_group_r_dev
                rc = fn(m._h, a["stack"], n, sc.H, sc.W, a["targets"], SM, sc.SHAPE[0], sc.SHAPE[1], C.byref(o) if o is not None else None, groups.ctypes.data if groups is not None else None,
                        ng, a["planes"], a["rigid"], None if form == "dev" else sw.ctypes.data, None, a["scale"], a["out"], a["gout"], None, a["rep"], None, None)
                assert rc == _lib.E_INVALID and word in _lib.last_error(), (word, form, rc, _lib.last_error())

        inf, nan = float("inf"), float("nan")
        hsolve("options", None)
        hsolve("struct_size", opts(struct_size=72))
        hsolve("intensity_mode", opts(est=2))
        for o in (opts(iterations=0), opts(iterations=257)):
            hsolve("iterations", o)
        for o in (opts(lam_min=0.0), opts(lam_max=inf), opts(damping=nan)):
            hsolve("damping", o)
        hsolve("down", opts(down=0.0))
        hsolve("up", opts(up=0.5))
        for bad in (0.0, nan, inf, -1.0):
            hsolve("spacing", opts(spacing=bad))
        hsolve("n =", opts(), n=1)
        for k, word in (("stack", "stack"), ("targets", "targets"), ("planes", "planes"), ("rigid", "rigid_in"), ("scale", "scale"), ("out", "maps_out"), ("gout", "intensity_out"),
                        ("rep", "report")):
            hsolve(word, opts(), **{k: None})
        hsolve("n_groups", opts(), ng=0)
        hsolve("group_start", opts(), groups=None)
        hsolve("group_start[0]", opts(), groups=np.array([1, 3, 4, 6], np.int32))
        hsolve("group_start[2]", opts(), groups=np.array([0, 3, 3, 6], np.int32))
        hsolve("group_start[3]", opts(), groups=np.array([0, 3, 4, 5], np.int32))
        with pytest.raises(ValueError):
            m.align_stack_solve(st, stg, pl[:3], sc.SPACING)
        with pytest.raises(ValueError):
            m.align_stack_solve(st, stg, pl, sc.SPACING, groups=[2, 2])
        with pytest.raises(ValueError, match="spacing"):
            m.align_stack_solve(st, stg, pl, 0.0)
        m.sync()
        assert m.profile_kernels() == [] and (sums == -7.0).all() and (out == -7.0).all() and (rep == -7.0).all() and same(dbuf.numpy(), st)
    finally:
        profile_off(m)
    assert same_result(cost(d, sc.SCALES[0], **ALL), ast.result_on_host(st, tg, mp, sc.SCALES[0], weights=w, intensity=gb))  # the handle stays usable


def test_the_profile_shows_one_reduce_entry_per_evaluation_and_nothing_of_the_trunk():
    m, d = model(), sc.data("smooth", (33, 37))
    profile_on(m)
    try:
        for calls in (1, 2, 3):
            cost(d, sc.SCALES[0], warped=calls == 2)
            m.sync()
            entries = m.profile_kernels()
            assert [e["kernel"] for e in entries] == ["align_stack_reduce_kernels"], entries
            assert entries[0]["launches"] == calls and entries[0]["coords"] == calls * sc.M * 33 * 37, entries
        solve("masked", av.ESTIMATE, trace=False)
        m.sync()
        entries = {e["kernel"]: e for e in m.profile_kernels()}
        assert sorted(entries) == ["align_group_step_kernels", "align_stack_reduce_kernels"], entries
        assert entries["align_stack_reduce_kernels"]["launches"] == 3 + sc.ITERATIONS and entries["align_group_step_kernels"]["launches"] == sc.ITERATIONS
    finally:
        profile_off(m)


def test_a_handle_that_never_had_weights_committed_runs_both_calls():
    m = ModulatedSiren(**KW)  # a fresh model of its own: nothing before these calls can have committed anything
    d = sc.data("ramp", (19, 23))
    res = m.align_stack_cost(d["stack"], d["targets"], d["maps"], gradient=True)
    assert same_result(res, ast.result_on_host(d["stack"], d["targets"], d["maps"])._replace(warped=None, rweight=None)) and not m._committed
    ins = np.isfinite(res.wgrad[0])
    assert (res.wgrad[0][ins] == sc.RAMP[1]).all() and (res.wgrad[1][ins] == sc.RAMP[2]).all() and (res.wgrad[2][ins] == sc.RAMP[3]).all()  # exact on the ramp
    w, s = sc.solve_case("masked")
    got = m.align_stack_solve(sc.stack("smooth"), sc.solve_targets(), sc.planes(), sc.SPACING, groups=sc.SIZES, weights=w, iterations=sc.ITERATIONS, trace=True)
    assert same_result(got, sc.reference_solve("masked", av.ESTIMATE)[0]) and not m._committed
    rc = m._lib.msiren_align_volume_r(m._h, None, 2, 40, 40, None, 1, 4, 4, None, None, None, None, None, None, None, None)
    assert rc == _lib.E_STATE and "not committed" in _lib.last_error()  # the calls that evaluate the model still ask for its weights on this handle


# ---- the neighbours, and the loop the call closes --------------------------------------------------------------------------------------------------------
def test_the_neighbours_return_the_same_bits_before_and_after_a_call():
    import align_group_cases as gc
    import align_robust_cases as rc
    import volume_cases as vc
    from test_gpu_align import model as trained

    m = trained("sine5")
    d = rc.data("sine5", (19, 23))
    f = fc.planes()

    def neighbours():
        a = m.align_volume_cost_r(vc.images(), d["targets"], d["maps"], d["scale"], weights=d["weights"], intensity=d["intensity"], warped=True, gradient=True, rweight=True)
        b = m.align_volume_solve_group_robust(vc.images(), d["targets"][:gc.M], gc.planes(), gc.SPACING, gc.GROUP_START, 0.01, weights=rc.weights(), iterations=3, trace=True)
        c = m.solve_volume_robust(f["targets"], f["maps"], fc.GRIDS[0], fc.SPACING, 0.05, rounds=2, iterations=2, weights=f["weights"], intensity=f["intensity"], rweight=True,
                                  stats=True, history=True, coverage=True)
        e = m.fuse_targets(f["targets"], f["maps"], fc.GRIDS[0], fc.SPACING, weights=f["weights"], intensity=f["intensity"], coverage=True)
        return a, b, c, e

    before = neighbours()
    s = sc.data("holes", (33, 37))
    mine = m.align_stack_cost(s["stack"], s["targets"], s["maps"], scale=sc.SCALES[0], weights=s["weights"], intensity=s["intensity"], **ALL)  # on the trained handle too
    w, sv = sc.solve_case("robust")
    m.align_stack_solve(sc.stack("smooth"), sc.solve_targets(), sc.planes(), sc.SPACING, groups=sc.GROUP_START, scale=sv, weights=w, iterations=4)
    after = neighbours()
    for x, y in zip(before, after):
        for fx, fy in zip(x, y):
            assert (fx is None and fy is None) or same(fx, fy)
    assert same_result(mine, cost(s, sc.SCALES[0], **ALL))  # and the trained handle gives the bare handle's bits


def test_one_pass_of_the_outer_loop_equals_the_chain_on_the_host():
    m, c = model(), sc.outer_case()
    kw = dict(rounds=sc.OUTER_ROUNDS, iterations=sc.OUTER_CG)
    h1, h2, h3 = sc.outer_on_host()
    first = m.solve_volume_robust(c["targets"], c["start"], c["grid"], c["spacing"], sc.OUTER_SCALE, **kw)
    assert same(first.volume, h1.volume) and np.array_equal(first.flags, h1.flags)
    reg = m.align_stack_solve(first.volume, c["targets"], c["planes"], c["spacing"], scale=sc.OUTER_SCALE, shift=c["shift"], estimate_intensity=False,
                              iterations=sc.OUTER_ITERATIONS, trace=True)
    assert same_result(reg, h2)
    second = m.solve_volume_robust(c["targets"], reg.maps, c["grid"], c["spacing"], sc.OUTER_SCALE, **kw)
    assert same(second.volume, h3.volume) and np.array_equal(second.stopped_at, h3.stopped_at)
    start, after = sc.outer_error(c["start"]), sc.outer_error(reg.maps)
    print("map error", start, "->", after)
    assert after < start
