"""Every registration and reconstruction family past 256 units on the GPU (cases: tests/many_units_cases.py): the second and later workgroups of the
one-thread-per-unit kernels (the solve init and step kernels of csrc/align*.hip.h, the five grouped kernels of csrc/align_group.hip.h,
fuse_setup_kernel), the second and third launch of align_group_upload_kernel, the search over more than a thousand group offsets, groups whose members
lie in two workgroups, the second lap of the column loops of project_stats_kernel and irls_stats_kernel, and the record loop of fuse_visit_targets over
260 targets.

The oracle is the promise every one of these kernels makes: a unit's result depends on that unit alone.  So one long call has to return, bit for bit,
the concatenation of calls over consecutive chunks of at most 64 units -- one workgroup, one upload launch, the regime the other GPU tests pin against the
host restatements -- and sampled units are compared with the host loops and restatements directly.  No tolerance anywhere: np.array_equal, with NaNs in
the same places where NaN is an output."""
import ctypes as C
import functools

import numpy as np
import pytest

import align_group_cases as gc
import align_solve_cases as s2
import align_stack_cases as sc
import align_w_cases as w2
import many_units_cases as mu
import volume_cases as vc
from mri_inr_amd import _lib, align, align_group as ag, align_robust as ar, align_stack as ast, align_volume as av, fuse, solve_volume as sv, solve_volume_robust as svr
from test_gpu_align import model as trained, packed as packed29, same
from test_gpu_align_stack import f64_dev, f64_of, model as bare
from test_gpu_align_volume import packed as packed56
from test_gpu_solve_volume_robust import dev_call as solve_r_dev, doubles, opts as solve_r_opts

pytestmark = pytest.mark.gpu

packed47, packed80 = w2.packed, gc.wc.packed
NAME = "morlet3"
UNITS = 258            # the per-target and per-slice solves: two workgroups, the second with two units
TRUNK_ITERATIONS = 4
CHUNK = 64
EST = (av.FIXED, av.ESTIMATE)


def joined(parts):
    """the results of calls over consecutive chunks of units as one result: every field along the units, the trace along its second axis"""
    T = type(parts[0])
    return T(*[None if parts[0][k] is None else np.concatenate([p[k] for p in parts], axis=1 if f == "trace" else 0) for k, f in enumerate(T._fields)])


def differing(a, b):
    """the fields in which two results differ (bit for bit, NaNs in the same places)"""
    return [f for f, x, y in zip(type(a)._fields, a, b) if not ((x is None and y is None) or (x is not None and y is not None and same(x, y)))]


def rows_of(res, units, groups=None):
    """a result cut down to the units (and, for a grouped one, the groups) given as slices"""
    T = type(res)
    per_group = ("rotation", "shift", "accepted", "mean_first", "mean_best", "damping", "flags") if T is ag.SolveResultG else ()
    out = []
    for f, x in zip(T._fields, res):
        s = groups if f in per_group or (f == "trace" and groups is not None) else units
        out.append(None if x is None else x[:, s] if f == "trace" else x[s])
    return T(*out)


def intensity_of(c, est, rows=slice(None)):
    return None if est == av.ESTIMATE else c["intensity"][rows]


def pairwise_different(states):
    return len(np.unique(np.asarray(states).reshape(len(states), -1), axis=0)) == len(states)


# ---- the grouped solve on the voxel stack: 1030 groups, 2054 targets -----------------------------------------------------------------------------------------
def stack_solve(c, est, lo=0, hi=None, iterations=sc.ITERATIONS):
    """align_stack_solve on the groups lo .. hi - 1 of the case as a call of their own"""
    r = mu.group_rows(c, lo, len(c["base"]) if hi is None else hi)
    rows, rigid = r["targets"], c["rigid"][r["groups"]]
    return bare().align_stack_solve(c["stack"], c["targets"][rows], c["planes"][rows], mu.SPACING, groups=r["group_start"], scale=c["scales"][rows],
                                    rotation=rigid[:, :9].reshape(-1, 3, 3), shift=rigid[:, 9:], weights=c["weights_unmasked"][rows], intensity=intensity_of(c, est, rows),
                                    estimate_intensity=est == av.ESTIMATE, iterations=iterations, trace=True)


@functools.lru_cache(maxsize=None)
def stack_solved(est):
    return stack_solve(mu.grouped(mu.G_STACK), est)


@pytest.mark.parametrize("est", EST)
def test_the_long_grouped_stack_solve_is_its_chunks_and_the_host_loop(est):
    c = mu.grouped(mu.G_STACK)
    G, m = mu.G_STACK, len(c["planes"])
    got = stack_solved(est)
    assert got.trace.shape == (sc.ITERATIONS, G, 15) and got.maps.shape == (m, 9) and got.rotation.shape == (G, 3, 3)
    want = joined([stack_solve(c, est, lo, hi) for lo, hi in mu.chunks(G, CHUNK)])
    assert differing(got, want) == []
    for y in mu.sampled_groups(c):      # one group per upload launch and the one across target 256: the normative loop on the host restatement
        r = mu.group_rows(c, y, y + 1)
        rows = r["targets"]
        host, _ = ast.solve_on_host_s(c["stack"], c["targets"][rows], r["group_start"], c["scales"][rows], rigid=c["rigid"][r["groups"]], planes=c["planes"][rows],
                                      weights=c["weights_unmasked"][rows], intensity=intensity_of(c, est, rows), options=sc.options(est), trace=True)
        assert differing(rows_of(got, rows, r["groups"]), host) == [], y
        assert mu.errors(c, got.maps[rows], got.intensity[rows], rows, est) <= sc.device_solve_gate("robust"), y
    assert (got.accepted >= 1).all() and not got.flags.any()
    states = np.concatenate([got.rotation.reshape(G, 9), got.shift], axis=1)
    for b in range(3):                  # no instance returns another instance's state
        ys = np.nonzero(c["base"] == b)[0]
        assert pairwise_different(states[ys]) and pairwise_different(got.maps[c["group_start"][ys]]), b


def test_three_hundred_singleton_groups_are_their_chunks():
    c, est, U = mu.grouped(mu.G_STACK), av.FIXED, 300
    rigid = c["rigid"][c["group_of"][:U]]

    def run(lo, hi):
        return bare().align_stack_solve(c["stack"], c["targets"][lo:hi], c["planes"][lo:hi], mu.SPACING, groups=None, scale=c["scales"][lo:hi],
                                        rotation=rigid[lo:hi, :9].reshape(-1, 3, 3), shift=rigid[lo:hi, 9:], weights=c["weights_unmasked"][lo:hi], intensity=c["intensity"][lo:hi],
                                        estimate_intensity=False, iterations=sc.ITERATIONS, trace=True)

    got = run(0, U)
    assert got.trace.shape == (sc.ITERATIONS, U, 15) and got.rotation.shape == (U, 3, 3)
    assert differing(got, joined([run(lo, hi) for lo, hi in mu.chunks(U, CHUNK)])) == []
    outside = c["member"][:U] == sc.SOLVE_OUTSIDE          # alone, the member outside keeps its inputs with both flags
    assert outside[256:].any() and (got.flags[outside] == (av.NO_OVERLAP | av.SINGULAR)).all() and not got.count[outside].any() and not got.flags[~outside].any()
    assert np.array_equal(got.shift[outside], rigid[outside, 9:]) and (got.accepted[~outside] >= 1).all()
    states = np.concatenate([got.rotation.reshape(U, 9), got.shift], axis=1)
    for q in range(sc.SOLVE_M):
        if q != sc.SOLVE_OUTSIDE:
            assert pairwise_different(states[c["member"][:U] == q]), q


@pytest.mark.parametrize("est", EST)
def test_one_group_of_260_is_the_host_loop_around_the_devices_cost(est):
    c, its = mu.one_big_group(), 3
    got = stack_solve(c, est, iterations=its)

    def device_cost(maps, gb, scale):
        r = bare().align_stack_cost(c["stack"], c["targets"], maps, scale=scale, weights=c["weights_unmasked"], intensity=gb)
        return packed80(r)

    want, _ = ast.solve_on_host_s(None, None, c["group_start"], c["scales"], rigid=c["rigid"], planes=c["planes"], intensity=intensity_of(c, est), options=sc.options(est, its),
                                  trace=True, cost_fn=device_cost)
    assert differing(got, want) == []
    assert got.trace.shape == (its, 1, 15) and got.accepted[0] >= 1 and got.flags[0] == 0 and (got.count[256:] > 300).all()
    assert (got.trace[1:, 0, :12] != got.trace[0, 0, :12]).any() and pairwise_different(got.maps)


def test_the_dev_form_of_the_long_grouped_stack_solve_on_two_streams():
    m, est = bare(), av.ESTIMATE
    c, res = mu.grouped(mu.G_STACK), stack_solved(est)
    IT, G, SM = sc.ITERATIONS, mu.G_STACK, len(c["planes"])
    o = _lib.AlignVolumeSolveGroupOpts(C.sizeof(_lib.AlignVolumeSolveGroupOpts), IT, est, 0, 1e-3, 0.1, 10.0, 1e-9, 1e9, mu.SPACING)
    st, tg, w = c["stack"], c["targets"], c["weights_unmasked"]
    d = dict(stack=m.device_array(st.shape).copy_from(st), targets=m.device_array(tg.shape).copy_from(tg), planes=f64_dev(m, c["planes"]), rigid=f64_dev(m, c["rigid"]),
             weights=m.device_array(w.shape).copy_from(w), scale=f64_dev(m, c["scales"]))
    gs = np.ascontiguousarray(c["group_start"], np.int32)
    try:
        _lib.check(m._lib.msiren_set_streams(m._h, 2))
        outs = [dict(out=m.device_array((SM, 9)), gout=m.device_array((SM, 2)), rep=m.device_array((G, 7, 2)), rout=m.device_array((G, 12, 2)), trep=m.device_array((SM, 3, 2)),
                     trace=m.device_array((IT, G, 15, 2))) for _ in range(3)]
        for x in outs:  # back to back, no sync in between: the calls alternate over the streams
            _lib.check(m._lib.msiren_align_stack_solve_group_r_dev(m._h, d["stack"].ptr, sc.N, sc.H, sc.W, d["targets"].ptr, SM, mu.SHAPE[0], mu.SHAPE[1], C.byref(o), gs.ctypes.data,
                                                                   G, d["planes"].ptr, d["rigid"].ptr, d["weights"].ptr, None, d["scale"].ptr, x["out"].ptr, x["gout"].ptr,
                                                                   x["rout"].ptr, x["rep"].ptr, x["trep"].ptr, x["trace"].ptr))
        gs[:] = -1      # the offsets travelled in the launches' arguments: the caller's array is free again
        m.sync()
        for x in outs:
            rep, rout, trep = f64_of(x["rep"]), f64_of(x["rout"]), f64_of(x["trep"])
            assert np.array_equal(x["out"].numpy(), res.maps) and np.array_equal(x["gout"].numpy(), res.intensity)
            assert np.array_equal(rep[:, 0], res.accepted) and same(rep[:, 1], res.mean_first) and same(rep[:, 2], res.mean_best)
            assert np.array_equal(rep[:, 5], res.damping) and np.array_equal(rep[:, 6], res.flags)
            assert np.array_equal(rout[:, :9].reshape(G, 3, 3), res.rotation) and np.array_equal(rout[:, 9:], res.shift)
            assert np.array_equal(trep[:, 0], res.count) and np.array_equal(trep[:, 1], res.wsum) and np.array_equal(trep[:, 2], res.cost)
            assert same(f64_of(x["trace"]), res.trace)
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


# ---- the grouped solves on the stack the network reconstructs: 129 groups, 264 targets -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trunk_case(prec="fp32"):
    c = mu.grouped(mu.G_TRUNK, family="trunk")
    warped = trained(NAME, prec).align_volume_cost(vc.images(), np.zeros((len(c["planes"]),) + mu.SHAPE, np.float32), c["truth_maps"], warped=True).warped
    return mu.with_warped(c, warped)


def trunk_solve(m, c, est, robust, lo=0, hi=None):
    r = mu.group_rows(c, lo, len(c["base"]) if hi is None else hi)
    rows, rigid = r["targets"], c["rigid"][r["groups"]]
    kw = dict(rotation=rigid[:, :9].reshape(-1, 3, 3), shift=rigid[:, 9:], weights=c["weights_unmasked" if robust else "weights"][rows], intensity=intensity_of(c, est, rows),
              estimate_intensity=est == av.ESTIMATE, iterations=TRUNK_ITERATIONS, trace=True)
    if robust:
        return m.align_volume_solve_group_robust(vc.images(), c["targets"][rows], c["planes"][rows], mu.SPACING, r["group_start"], c["scales"][rows], **kw)
    return m.align_volume_solve_group(vc.images(), c["targets"][rows], c["planes"][rows], mu.SPACING, r["group_start"], **kw)


@pytest.mark.parametrize("est", EST)
@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_the_long_grouped_volume_solve_is_its_chunks_and_the_host_loop(prec, robust, est):
    m, c = trained(NAME, prec), trunk_case(prec)
    G = mu.G_TRUNK
    got = trunk_solve(m, c, est, robust)
    assert got.trace.shape == (TRUNK_ITERATIONS, G, 15) and len(got.maps) == len(c["planes"]) >= UNITS
    assert differing(got, joined([trunk_solve(m, c, est, robust, lo, hi) for lo, hi in mu.chunks(G, CHUNK)])) == []
    o = gc.options(est, iterations=TRUNK_ITERATIONS)
    for y in (c["straddling"], G - 1):  # the group across target 256 and the last one: the host loop around the device's cost on those rows alone
        r = mu.group_rows(c, y, y + 1)
        rows = r["targets"]
        tg, w = c["targets"][rows], c["weights_unmasked" if robust else "weights"][rows]
        kw = dict(rigid=c["rigid"][r["groups"]], planes=c["planes"][rows], intensity=intensity_of(c, est, rows), options=o, trace=True)
        if robust:
            host, _ = ar.solve_on_host_r(lambda maps, gb, s: packed80(m.align_volume_cost_r(vc.images(), tg, maps, s, weights=w, intensity=gb)), r["group_start"], c["scales"][rows], **kw)
        else:
            host, _ = ag.solve_on_host_g(lambda maps, gb: packed80(m.align_volume_cost_w(vc.images(), tg, maps, weights=w, intensity=gb)), r["group_start"], **kw)
        assert differing(rows_of(got, rows, r["groups"]), host) == [], y
    assert (got.accepted >= 1).any() and (got.trace[1:, :, :12] != got.trace[:1, :, :12]).any()
    states = np.concatenate([got.rotation.reshape(G, 9), got.shift], axis=1)
    for b in range(3):
        assert pairwise_different(states[c["base"] == b]), b


# ---- the per-target solves against the volume: 258 targets ----------------------------------------------------------------------------------------------------
def volume_units():
    """the first 258 targets of the trunk problem, every one starting from its group's start state on its own plane"""
    c = trunk_case()
    rigid = c["rigid"][c["group_of"][:UNITS]]
    start = np.array([av.rigid_map3([float(x) for x in rigid[q]], [float(x) for x in c["planes"][q]], mu.SPACING) for q in range(UNITS)], np.float32)
    return c, rigid, start


VOLUME_SOLVES = [("plain", align.AFFINE, None), ("plain", align.RIGID, None)] + [("w", mode, est) for mode in (align.AFFINE, align.RIGID) for est in EST]


@pytest.mark.parametrize("kind,mode,est", VOLUME_SOLVES)
def test_the_per_target_volume_solves_are_their_chunks_and_the_host_loop(kind, mode, est):
    m = trained(NAME)
    c, rigid, start = volume_units()
    tg, pl, w = c["targets"][:UNITS], c["planes"][:UNITS], c["weights"][:UNITS]
    gb = None if est != av.FIXED else c["intensity"][:UNITS]
    it = dict(iterations=TRUNK_ITERATIONS, trace=True)

    def run(s):
        geo = dict(rotation=rigid[s, :9].reshape(-1, 3, 3), shift=rigid[s, 9:])
        wkw = dict(weights=w[s], intensity=None if gb is None else gb[s], estimate_intensity=est == av.ESTIMATE)
        if kind == "plain":
            return m.align_volume_solve_rigid(vc.images(), tg[s], pl[s], mu.SPACING, **geo, **it) if mode == align.RIGID else m.align_volume_solve(vc.images(), tg[s], start[s], **it)
        if mode == align.RIGID:
            return m.align_volume_solve_rigid_w(vc.images(), tg[s], pl[s], mu.SPACING, **geo, **wkw, **it)
        return m.align_volume_solve_w(vc.images(), tg[s], start[s], **wkw, **it)

    got = run(slice(0, UNITS))
    assert got.trace.shape[:2] == (TRUNK_ITERATIONS, UNITS) and len(got.maps) == UNITS
    assert differing(got, joined([run(slice(lo, hi)) for lo, hi in mu.chunks(UNITS, CHUNK)])) == []
    u = slice(UNITS - 1, UNITS)             # the last unit of the second workgroup: the family's host loop around the device's cost on that target alone
    if kind == "plain":
        host, _ = av.solve_on_host_v(lambda maps: packed56(m.align_volume_cost(vc.images(), tg[u], maps)), 1, maps=start[u], rigid=rigid[u], planes=pl[u],
                                     options=av.SolveOptionsV(mode=mode, iterations=TRUNK_ITERATIONS, spacing=mu.SPACING), trace=True)
    else:
        host, _ = av.solve_on_host_vw(lambda maps, g: packed80(m.align_volume_cost_w(vc.images(), tg[u], maps, weights=w[u], intensity=g)), 1, maps=start[u], rigid=rigid[u],
                                      planes=pl[u], intensity=None if gb is None else gb[u],
                                      options=av.SolveOptionsVW(mode=mode, iterations=TRUNK_ITERATIONS, spacing=mu.SPACING, intensity_mode=est), trace=True)
    assert differing(rows_of(got, u), host) == []
    assert (got.accepted >= 1).any() and pairwise_different(got.maps[c["member"][:UNITS] != gc.OUTSIDE])


# ---- the per-slice solves: 258 slices ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def slices():
    """258 slices, tests/volume_cases.py's four images tiled, every copy dimmed by a factor of its own (1 down to 0.904: but for the black image no two slices hold
    the same pixels, so slice 256 is not slice 0 again); slice s is aligned to its image's plane at tests/align_solve_cases.py's truth for image s % 4, with its own
    seeded gain and bias, and starts from its own map: the case's start moved by up to 0.05 pixel"""
    rng = np.random.default_rng([mu.SEED, 5])
    base = np.arange(UNITS) % vc.N
    images = np.ascontiguousarray(vc.images()[base] * (1.0 - 0.0015 * (np.arange(UNITS) // vc.N)).astype(np.float32)[:, None, None])
    truth = s2.truth()[base]
    shift = np.asarray(s2.START_SHIFT) + rng.uniform(-mu.START_SHIFT, mu.START_SHIFT, (UNITS, 2))
    gb = (w2.GB_TRUTH[base].astype(np.float64) + rng.uniform(-1.0, 1.0, (UNITS, 2)) * np.array([0.1, 0.05])).astype(np.float32)
    warped = trained(NAME).align_cost(images, np.zeros((UNITS,) + s2.SHAPE, np.float32), truth, warped=True).warped
    plain = np.asarray(warped, np.float32)
    t = gb[:, 0].astype(np.float64)[:, None, None] * warped.astype(np.float64) + gb[:, 1].astype(np.float64)[:, None, None]
    t[(slice(None),) + w2.BLOCK] += w2.CORRUPTION
    weights = w2.solve_weights()[base]
    return dict(images=images, base=base, shift=shift, start=align.rigid_maps(np.zeros(UNITS), shift, s2.CENTRE), rigid=np.concatenate([np.tile([1.0, 0.0], (UNITS, 1)), shift], axis=1),
                intensity=gb, targets=plain, targets_w=t.astype(np.float32), weights=weights)


SLICE_SOLVES = [("plain", align.AFFINE, None), ("plain", align.RIGID, None)] + [("w", mode, est) for mode in (align.AFFINE, align.RIGID) for est in (align.FIXED, align.ESTIMATE)]


@pytest.mark.parametrize("kind,mode,est", SLICE_SOLVES)
def test_the_per_slice_solves_are_their_chunks_and_the_host_loop(kind, mode, est):
    m, d = trained(NAME), slices()
    img, tg, w = d["images"], d["targets" if kind == "plain" else "targets_w"], d["weights"]
    gb = None if est != align.FIXED else d["intensity"]
    it = dict(iterations=TRUNK_ITERATIONS, trace=True)

    def run(s):
        wkw = dict(weights=w[s], intensity=None if gb is None else gb[s], estimate_intensity=est == align.ESTIMATE)
        if kind == "plain":
            return m.align_solve_rigid(img[s], tg[s], np.zeros(UNITS)[s], d["shift"][s], s2.CENTRE, **it) if mode == align.RIGID else m.align_solve(img[s], tg[s], d["start"][s], **it)
        if mode == align.RIGID:
            return m.align_solve_rigid_w(img[s], tg[s], np.zeros(UNITS)[s], d["shift"][s], s2.CENTRE, **wkw, **it)
        return m.align_solve_w(img[s], tg[s], d["start"][s], **wkw, **it)

    got = run(slice(0, UNITS))
    assert got.trace.shape[:2] == (TRUNK_ITERATIONS, UNITS) and len(got.maps) == UNITS
    assert differing(got, joined([run(slice(lo, hi)) for lo, hi in mu.chunks(UNITS, CHUNK)])) == []
    u = slice(UNITS - 1, UNITS)             # slice 257 (image 1): the family's host loop around the device's cost on that slice alone
    if kind == "plain":
        host, _ = align.solve_on_host(lambda maps: packed29(m.align_cost(img[u], tg[u], maps)), 1, maps=d["start"][u], rigid=d["rigid"][u],
                                      options=align.SolveOptions(mode=mode, iterations=TRUNK_ITERATIONS, centre=s2.CENTRE), trace=True)
    else:
        host, _ = align.solve_on_host_w(lambda maps, g: packed47(m.align_cost_w(img[u], tg[u], maps, weights=w[u], intensity=g)), 1, maps=d["start"][u], rigid=d["rigid"][u],
                                        intensity=None if gb is None else gb[u],
                                        options=align.SolveOptionsW(mode=mode, iterations=TRUNK_ITERATIONS, centre=s2.CENTRE, intensity_mode=est), trace=True)
    assert differing(rows_of(got, u), host) == []
    seen = d["base"] != s2.BLACK            # (the black image's slices keep their inputs)
    assert (got.accepted[seen] >= 1).any() and pairwise_different(got.maps[seen])


# ---- the cost calls behind those solves, at the same counts -----------------------------------------------------------------------------------------------------
def cost_is_its_chunks(call, pack, count):
    """``call(slice)`` -> a result with warped and wgrad: the long call's sums and planes are those of its chunks"""
    got = call(slice(0, count))
    parts = [call(slice(lo, hi)) for lo, hi in mu.chunks(count, CHUNK)]
    assert np.array_equal(pack(got), np.concatenate([pack(p) for p in parts])) and len(pack(got)) == count
    assert same(got.warped, np.concatenate([p.warped for p in parts])) and same(got.wgrad, np.concatenate([p.wgrad for p in parts], axis=1))
    if getattr(got, "rweight", None) is not None:
        assert same(got.rweight, np.concatenate([p.rweight for p in parts]))
    assert (got.count[256:] > 0).any() and np.isfinite(got.warped[256:]).any()
    return got


def test_the_slice_costs_are_their_chunks():
    m, d = trained(NAME), slices()
    out = dict(warped=True, gradient=True)
    cost_is_its_chunks(lambda s: m.align_cost(d["images"][s], d["targets"][s], d["start"][s], **out), packed29, UNITS)
    cost_is_its_chunks(lambda s: m.align_cost_w(d["images"][s], d["targets_w"][s], d["start"][s], weights=d["weights"][s], intensity=d["intensity"][s], **out), packed47, UNITS)


def test_the_volume_costs_are_their_chunks():
    m, c = trained(NAME), trunk_case()
    count = len(c["planes"])
    tg, mp, out = c["targets"], c["truth_maps"], dict(warped=True, gradient=True)
    cost_is_its_chunks(lambda s: m.align_volume_cost(vc.images(), tg[s], mp[s], **out), packed56, count)
    cost_is_its_chunks(lambda s: m.align_volume_cost_w(vc.images(), tg[s], mp[s], weights=c["weights"][s], intensity=c["intensity"][s], **out), packed80, count)
    cost_is_its_chunks(lambda s: m.align_volume_cost_r(vc.images(), tg[s], mp[s], c["scales"][s], weights=c["weights_unmasked"][s], intensity=c["intensity"][s], rweight=True, **out),
                       packed80, count)


def test_the_stack_cost_is_its_chunks_and_the_restatement():
    c = mu.grouped(mu.G_STACK)
    count = len(c["planes"])
    start = np.array([av.rigid_map3([float(x) for x in c["rigid"][y]], [float(x) for x in p], mu.SPACING) for p, y in zip(c["planes"], c["group_of"])], np.float32)
    kw = dict(warped=True, gradient=True, rweight=True)
    got = cost_is_its_chunks(lambda s: bare().align_stack_cost(c["stack"], c["targets"][s], start[s], scale=c["scales"][s], weights=c["weights_unmasked"][s],
                                                               intensity=c["intensity"][s], **kw), packed80, count)
    rows = slice(250, 262)   # across the first workgroup's end: the host restatement
    want = ast.result_on_host(c["stack"], c["targets"][rows], start[rows], c["scales"][rows], weights=c["weights_unmasked"][rows], intensity=c["intensity"][rows])
    assert np.array_equal(packed80(got)[rows], packed80(want)) and same(got.warped[rows], want.warped) and same(got.rweight[rows], want.rweight)


# ---- fuse, project and the volume solves: 260 targets; 300 columns ----------------------------------------------------------------------------------------------
def recon_kw(d):
    return dict(weights=d["weights"], intensity=d["intensity"])


def test_fuse_targets_over_260_targets_equals_the_restatement():
    d = mu.many_targets()
    got = bare().fuse_targets(d["targets"], d["maps"], d["grid"], d["spacing"], coverage=True, **recon_kw(d))
    want = fuse.fuse_on_host(d["targets"], d["maps"], d["grid"], d["spacing"], **recon_kw(d))
    assert same(got.volume, want.volume) and same(got.coverage, want.coverage) and np.array_equal(got.flags, want.flags)
    assert got.flags[256:].tolist() == [0, 0, fuse.DEGENERATE, fuse.BAD_INTENSITY] and np.isfinite(got.volume[:, :, 9:]).sum() >= 20   # the voxels only targets 256, 257 reach


@pytest.mark.parametrize("case", ["many", "wide"])
def test_project_volume_past_256_targets_and_past_256_columns_equals_the_restatement(case):
    d = mu.many_targets() if case == "many" else mu.wide_target()
    shape = d["targets"].shape[1:]
    volume = fuse.fuse_on_host(d["targets"], d["maps"], d["grid"], d["spacing"], **recon_kw(d)).volume
    got = bare().project_volume(volume, d["maps"], shape, d["spacing"], intensity=d["intensity"], targets=d["targets"], weights=d["weights"], coverage=True, residual=True, stats=True)
    want = fuse.project_on_host(volume, d["maps"], shape, d["spacing"], intensity=d["intensity"])
    residual, stats = fuse.project_stats_on_host(d["targets"], want.simulated, d["weights"])
    assert same(got.simulated, want.simulated) and same(got.coverage, want.coverage) and np.array_equal(got.flags, want.flags)
    assert same(got.residual, residual) and np.array_equal(got.stats, stats), (got.stats, stats)
    assert (stats[:256 if case == "many" else 2, 0] > 10).all() and np.isfinite(residual[-4 if case == "many" else 0:, :, -44:]).any()


def test_solve_volume_over_260_targets_equals_the_restatement():
    d = mu.many_targets()
    got = bare().solve_volume(d["targets"], d["maps"], d["grid"], d["spacing"], iterations=2, lam=0.01, coverage=True, history=True, **recon_kw(d))
    want = sv.solve_volume_on_host(d["targets"], d["maps"], d["grid"], d["spacing"], iterations=2, lam=0.01, **recon_kw(d))
    assert same(got.volume, want.volume) and same(got.coverage, want.coverage) and same(got.history, want.history), (got.history, want.history)
    assert np.array_equal(got.flags, want.flags) and got.stopped_at == want.stopped_at == -1 and np.isfinite(got.volume[:, :, 9:]).sum() >= 20


@pytest.mark.parametrize("case", ["many", "wide"])
def test_solve_volume_robust_past_256_targets_and_past_256_columns_equals_the_restatement(case):
    m, d = bare(), mu.many_targets() if case == "many" else mu.wide_target()
    run = dict(rounds=2, iterations=2, lam=0.01)
    its = []
    want = svr.solve_volume_robust_on_host(d["targets"], d["maps"], d["grid"], d["spacing"], d["scales"], iterates=its, **run, **recon_kw(d))
    _, residual, _ = svr.final_pass_on_host(its[0], its[-1], d["targets"], d["weights"], d["scales"])
    got = m.solve_volume_robust(d["targets"], d["maps"], d["grid"], d["spacing"], d["scales"], coverage=True, history=True, rweight=True, stats=True, **run, **recon_kw(d))
    assert np.array_equal(got.stats, want.stats), (got.stats, want.stats)
    assert same(got.volume, want.volume) and same(got.coverage, want.coverage) and same(got.history, want.history) and same(got.rweight, want.rweight)
    assert np.array_equal(got.flags, want.flags) and np.array_equal(got.stopped_at, want.stopped_at) and (want.stopped_at == -1).all()
    # the residual leaves the call in its _dev form only
    count, shape, grid = len(d["targets"]), d["targets"].shape[1:], d["grid"]
    d_t, d_m, d_w, d_gb = (m.device_array(x.shape).copy_from(x) for x in (d["targets"], d["maps"], d["weights"], d["intensity"]))
    d_v, d_rw, d_res, d_ss = m.device_array(grid), m.device_array(d["targets"].shape), m.device_array(d["targets"].shape), m.device_array((count, 8))
    d_sc = doubles(m, d["scales"])
    _lib.check(solve_r_dev(m, d_t, count, shape, d_m, d_w, d_gb, d_sc, solve_r_opts(2, 2, 0.01, 1.0, thickness=d["spacing"], spacing=d["spacing"]), grid, None, d_v,
                           d_rw=d_rw, d_res=d_res, d_ss=d_ss))
    m.sync()
    assert same(d_v.numpy(), want.volume) and same(d_rw.numpy(), want.rweight) and same(d_res.numpy(), residual) and np.array_equal(d_ss.numpy().view(np.float64), want.stats)
    assert (want.rweight[np.isfinite(want.rweight)] < 0.5).any() and np.isfinite(residual[-4 if case == "many" else 0:, :, -44 if case == "wide" else 0:]).any()
    assert (want.stats[:256 if case == "many" else 2, 0] > 10).all()
