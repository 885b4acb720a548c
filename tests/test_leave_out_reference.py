"""mri_inr_amd/leave_out.py: leave_out_on_host, the normative restatement of msiren_leave_out_targets, on the CPU.

It is measured against what it replaces -- per group one fuse_on_host of the targets outside the group and one project_on_host of the group's own
(leave_out_chain_on_host) -- never against the device: the finite masks are identical on planes, truth and many, where the floor excludes no pair, and
the values agree within a bound the test derives per pixel from the rule's own terms:

    |g| 2^-24 max |U|                                   the chain rounds its intermediate stack to float32, the rule keeps U in fp64
    |g| m 2^-52 max (sum |k sn| + |U| den_v) / denL     the rule subtracts the group's terms from sums of m rounded additions; the chain adds the others
    2^-23 max(|simulated|)                              the two output roundings

the maxima over the voxels that reach the pixel.  Then the twin identities bit for bit, the targets that must not matter, the by-products, and seeded
mutants of every piece of the rule, each rejected by one of these checks."""
import functools

import numpy as np
import pytest

import fuse_cases as fc
import leave_out_cases as cases
from mri_inr_amd import fuse
from mri_inr_amd import leave_out as lo

bits_equal = cases.bits_equal
CHAINED = [n for n in cases.all_cases() if n.startswith(("planes", "truth", "many"))]


def quick_chain(targets, maps, shape, spacing, *, groups=None, thickness=None, weights=None, intensity=None, min_coverage=0.0, only=None):
    """leave_out_chain_on_host's bits at a fraction of its cost, for the case with 600 groups: every target's terms are formed once, as dense (n H W) arrays
    with +0.0 where the target does not contribute, and the fusion without a group is the running sum of the targets in front of it carried on through the
    targets behind it -- the additions of fuse_on_host on the rest, in its order (adding +0.0 changes no bit of a sum that started at +0.0).
    ``only``: these groups alone.  test_the_quick_chain_is_the_chain holds it against the plain chain"""
    tg, mp = np.ascontiguousarray(targets, dtype=np.float32), np.ascontiguousarray(maps, dtype=np.float32).reshape(-1, 9)
    m, th, tw = tg.shape
    grid = tuple(int(s) for s in shape)
    wt = np.ones(tg.shape, np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    r = fuse.target_records(mp, intensity, np.float64(spacing), spacing if thickness is None else thickness)
    dn, dd = np.zeros((m,) + grid), np.zeros((m,) + grid)
    sim, cov = np.full(tg.shape, np.nan, np.float32), np.zeros(tg.shape, np.float32)
    with np.errstate(all="ignore"):
        for q in range(m):
            taps = None if r.flags[q] else fuse.voxel_taps(r, q, np.ones(grid, bool), grid, (th, tw), np.float64(spacing))
            if taps is not None:
                dn[q][taps[0]], dd[q][taps[0]] = lo.own_terms(r, q, tg[q].ravel(), wt[q].ravel(), taps)
        offsets = lo.segments(groups, m)
        num, den, at = np.zeros(grid), np.zeros(grid), 0
        for y, (lo_, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
            while at < lo_:
                num, den, at = num + dn[at], den + dd[at], at + 1
            if only is not None and y not in only:
                continue
            n2, d2 = num, den
            for q in range(hi, m):
                n2, d2 = n2 + dn[q], d2 + dd[q]
            volume = np.where(d2 > np.float64(min_coverage), (n2 / d2).astype(np.float32), np.float32(np.nan)).astype(np.float32)
            p = fuse.project_on_host(volume, mp[lo_:hi], (th, tw), spacing, thickness=thickness, intensity=None if intensity is None else np.asarray(intensity)[lo_:hi],
                                     min_coverage=min_coverage)
            sim[lo_:hi], cov[lo_:hi] = p.simulated, p.coverage
    return sim, cov


@functools.lru_cache(maxsize=None)
def chain(name):
    args, kw = cases.all_cases()[name]
    return (quick_chain if name.startswith("many") else lo.leave_out_chain_on_host)(*args, **kw)


@pytest.mark.parametrize("name", ["planes-grid1-full-groups-mc0.25", "planes-grid0-quarter-singletons-mc0.0", "truth-full-fours", "truth-quarter-singletons"])
def test_the_quick_chain_is_the_chain(name):
    args, kw = cases.all_cases()[name]
    assert all(bits_equal(a, b) for a, b in zip(quick_chain(*args, **kw), chain(name)))


def test_the_quick_chain_is_the_chain_on_sampled_groups_of_many():
    for name, only in (("many-singletons", (0, 1, 299, 511, 512, 599)), ("many-threes", (0, 100, 199))):
        (T, maps, grid, spacing), kw = cases.all_cases()[name]
        sim, cov = chain(name)
        offsets = lo.segments(kw["groups"], len(T))
        for y in only:
            rest = np.ones(len(T), bool)
            rest[offsets[y]:offsets[y + 1]] = False
            stack = fuse.fuse_on_host(T[rest], maps[rest], grid, spacing)
            p = fuse.project_on_host(stack.volume, maps[~rest], T.shape[1:], spacing)
            assert bits_equal(sim[~rest], p.simulated) and bits_equal(cov[~rest], p.coverage), (name, y)


def against_chain(name, **pieces):
    """-> (pixels whose finiteness differs, pixels beyond the bound, the largest difference, pairs the floor excluded, pixels compared)"""
    args, kw = cases.all_cases()[name]
    sim, cov = chain(name)
    trace = {}
    r = lo.leave_out_on_host(*args, trace=trace, **kw, **pieces) if pieces else None
    if r is None:
        r = cases.reference(name)
        lo.leave_out_sums_on_host(*args, trace=trace, **kw)
    m, th, tw = r.simulated.shape
    g = np.abs(np.ones(m) if kw.get("intensity") is None else np.asarray(kw["intensity"], np.float64)[:, 0]).reshape(m, 1, 1)
    mine, theirs = r.simulated.astype(np.float64), sim.astype(np.float64)
    both = np.isfinite(mine) & np.isfinite(theirs)
    with np.errstate(all="ignore"):
        bound = g * 2.0 ** -24 * trace["umax"].reshape(m, th, tw) + g * m * 2.0 ** -52 * trace["cancel"].reshape(m, th, tw) + 2.0 ** -23 * np.maximum(np.abs(mine), np.abs(theirs))
        diff = np.abs(mine - theirs)
    return int((np.isfinite(mine) != np.isfinite(theirs)).sum()), int((diff > bound)[both].sum()), float(diff[both].max()) if both.any() else 0.0, trace["floored"], int(both.sum())


@pytest.mark.parametrize("name", CHAINED)
def test_the_rule_agrees_with_one_fusion_and_one_projection_per_group(name):
    masks, beyond, worst, floored, compared = against_chain(name)
    print(f"{name}: {compared} pixels compared, largest difference {worst}, floor excluded {floored} pairs")
    assert masks == 0 and floored == 0                                                                   # conditions on the cases
    assert beyond == 0
    if "quarter-groups" not in name:
        assert compared > 500


def test_coverage_is_the_chains_where_the_same_voxels_take_part():
    for name in ("planes-grid1-full-groups-mc0.25", "truth-quarter-fours"):
        assert bits_equal(cases.reference(name).coverage, chain(name)[1])


@pytest.mark.parametrize("name", cases.ALL_NAN)
def test_targets_that_do_not_overlap_predict_nothing(name):
    r = cases.reference(name)
    assert np.isnan(r.simulated).all() and not r.coverage.any() and np.isnan(r.residual).all() and not r.stats.any()


@pytest.mark.parametrize("e", cases.TWIN_PREDICTED + cases.TWIN_FLOORED)
def test_the_twin_identities_hold_bit_for_bit(e):
    T = cases.twin(e)["targets"]
    r = cases.reference(f"twin-{e}")
    assert bits_equal(r.simulated[3:], T[:3])                                                            # the copies are predicted with the originals' bits
    if e in cases.TWIN_PREDICTED:
        assert bits_equal(r.simulated[:3], T[3:])                                                        # and the originals with their twins'
        assert bits_equal(r.coverage, np.ones(T.shape, np.float32))
    else:
        assert np.isnan(r.simulated[:3]).all() and not r.coverage[:3].any()                              # denL = 2^-e is not above 2^-20 den_v


def test_flagged_zero_weight_and_outside_targets_change_no_bit_of_the_others():
    d, o = fc.planes(), fc.outside_target()
    grid, kw = fc.GRIDS[1], dict(thickness=fc.SPACING, min_coverage=0.25)
    keep = slice(0, fc.M_PLANES)
    base = lo.leave_out_on_host(d["targets"][keep], d["maps"][keep], grid, fc.SPACING, weights=d["weights"][keep], intensity=d["intensity"][keep], **kw)
    T = np.concatenate([d["targets"], o["targets"], d["targets"][:1]])                                   # + the flagged two, the outside one, a copy of target 0 ...
    maps = np.concatenate([d["maps"], o["maps"], d["maps"][:1]])
    w = np.concatenate([d["weights"], o["weights"], np.zeros_like(d["weights"][:1])])                    # ... whose weights are all zero
    gb = np.concatenate([d["intensity"], o["intensity"], d["intensity"][:1]])
    more = lo.leave_out_on_host(T, maps, grid, fc.SPACING, weights=w, intensity=gb, **kw)
    assert np.isfinite(base.simulated).sum() > 2000
    for a, b in zip(base[:4], more[:4]):
        assert bits_equal(a, b[keep])
    assert bits_equal(base.volume, more.volume) and bits_equal(base.volume_coverage, more.volume_coverage)
    assert np.isnan(more.simulated[fc.M_PLANES:fc.M + 1]).all() and np.isfinite(more.simulated[-1]).any()  # the zero-weight copy is still predicted


def test_singletons_given_as_groups_equal_no_groups():
    for name in ("planes-grid1-full-singletons-mc0.25", "truth-quarter-singletons"):
        args, kw = cases.all_cases()[name]
        m = len(args[0])
        for groups in (list(range(m + 1)), [1] * m):
            assert cases.same_result(lo.leave_out_on_host(*args, **dict(kw, groups=groups)), cases.reference(name))
    k = cases.all_cases()["many-singletons"]
    assert cases.same_result(lo.leave_out_on_host(*k[0]), cases.reference("many-singletons"))


@pytest.mark.parametrize("name", ["planes-grid0-full-groups-mc0.25", "planes-grid1-quarter-singletons-mc0.0", "truth-full-fours", "twin-30", "pooled", "none"])
def test_the_by_products_are_the_fusion_and_the_projections_statistics(name):
    args, kw = cases.all_cases()[name]
    r = cases.reference(name)
    f = fuse.fuse_on_host(*args, **{k: v for k, v in kw.items() if k != "groups"})
    assert bits_equal(r.volume, f.volume) and bits_equal(r.volume_coverage, f.coverage) and bits_equal(r.flags, f.flags)
    res, stats = fuse.project_stats_on_host(args[0], r.simulated, kw.get("weights"))
    assert bits_equal(r.residual, res) and bits_equal(r.stats, stats)


def test_the_left_out_residual_reports_what_the_self_residual_hides():
    """the numbers of DESIGN.md section 5.24: truth thinned to every 4th target, + 0.5 on a 20 x 20 block of one of them"""
    t = fc.truth_case()
    T, maps = t["targets"][::4].copy(), t["maps"][::4]
    T[2, 10:30, 10:30] += np.float32(0.5)
    block = np.zeros(T.shape, bool)
    block[2, 10:30, 10:30] = True
    told = {}
    for thickness in (fc.SPACING, fc.SPACING / 2):
        f = fuse.fuse_on_host(T, maps, fc.TRUTH_GRID, fc.SPACING, thickness=thickness)
        p = fuse.project_on_host(f.volume, maps, T.shape[1:], fc.SPACING, thickness=thickness)
        own = np.abs(fuse.residual_on_host(T, p.simulated))
        left = np.abs(lo.leave_out_on_host(T, maps, fc.TRUTH_GRID, fc.SPACING, thickness=thickness).residual)
        ok = np.isfinite(own) & np.isfinite(left)
        told[thickness] = [float(x[ok & s].mean()) for x in (own, left) for s in (block, ~block)]
        print(f"thickness {thickness}: self {told[thickness][:2]}, left out {told[thickness][2:]} (mean |r| in the block, elsewhere)")
    wide, narrow = told[fc.SPACING], told[fc.SPACING / 2]
    assert wide[0] < wide[2] and narrow[0] < narrow[2]                                                   # the self-residual hides part of the error the left-out one shows
    assert narrow[1] < wide[1] and narrow[3] > 0.9 * wide[3]                                             # and only the self-residual rewards a narrower window


# ---- seeded mutants: each piece of the rule replaced by a wrong one, each rejected by a check above ---------------------------------------------------
def sums_of(name, **pieces):
    args, kw = cases.all_cases()[name]
    return lo.leave_out_sums_on_host(*args, **kw, **pieces)[:2]


def test_mutant_own_terms_not_subtracted():
    masks, beyond, worst, _, _ = against_chain("truth-full-singletons", sums=lambda num, den, terms, members: (num, den))
    assert beyond > 1000 and worst > 1e-3


def test_mutant_only_the_target_itself_subtracted_in_a_group():
    name = "truth-full-fours"
    masks, beyond, worst, _, _ = against_chain(name, members=lambda lo_, hi, q: (q,))
    assert beyond > 1000 and worst > 1e-3
    assert against_chain(name, members=lambda lo_, hi, q: tuple(range(lo_, hi)))[:2] == (0, 0)            # (the hook itself is sound)


def test_mutant_the_floor_removed():
    args, kw = cases.all_cases()["twin-30"]
    r = lo.leave_out_on_host(*args, takes=lambda denL, den, mc: denL > np.float64(mc), **kw)
    assert np.isfinite(r.simulated[:3]).all()                                                            # the rule says NaN: test_the_twin_identities rejects it
    assert not bits_equal(r.simulated[:3], args[0][3:])                                                  # and what it predicts there is rounding noise, not the twin


def test_mutant_min_coverage_tested_on_the_whole_coverage():
    takes = lambda denL, den, mc: (den > np.float64(mc)) & (denL > den * np.float64(lo.LEAVE_OUT_FLOOR))  # noqa: E731
    masks, beyond, *_ = against_chain("planes-grid0-quarter-singletons-mc0.25", takes=takes)
    assert masks > 50


def test_mutant_the_left_out_value_rounded_to_float32():
    name = "truth-full-singletons"
    N, D = sums_of(name)
    Nm, Dm = sums_of(name, value=lambda numL, denL: (numL / denL).astype(np.float32).astype(np.float64))
    assert bits_equal(D, Dm) and not bits_equal(N, Nm) and (N != Nm).sum() > 0.9 * (D > 0).sum()          # seen in the fp64 sums ...
    assert against_chain(name, value=lambda numL, denL: (numL / denL).astype(np.float32).astype(np.float64))[:2] == (0, 0)  # ... which is why the chain cannot tell


def test_mutant_tap_major_order():
    name = "truth-full-singletons"
    N, D = sums_of(name)
    Nm, Dm = sums_of(name, scatter=lambda acc, pixel, terms: np.add.at(acc, pixel.T.ravel(), terms.T.ravel()))
    assert (not bits_equal(N, Nm) or not bits_equal(D, Dm)) and np.allclose(N, Nm, rtol=1e-12, atol=0) and np.allclose(D, Dm, rtol=1e-12, atol=0)
