"""The cases of msiren_leave_out_targets shared by tests/test_leave_out_reference.py (CPU) and tests/test_gpu_leave_out.py, on top
of tests/fuse_cases.py.  Not a test module; no GPU and no model needed: pure numpy, small enough that every GPU test takes seconds.

    planes      fuse_cases.planes() (m = 8 with the degenerate map, the gain 0, a NaN weight and a NaN pixel; lattice 19 x 23: ragged pixel tiles) on both
                grids -- (5, 37, 45) has ragged voxel tiles and a slice no target reaches -- at both thicknesses, as singletons and in the groups
                (3, 1, 2, 2), with min_coverage 0 and 0.25
    truth       fuse_cases.truth_case() (24 targets of 44 x 46) at both thicknesses, as singletons and in groups of 4
    graze       fuse_cases.graze: nine cases; identity: their targets do not overlap, so every prediction is NaN with coverage 0
    twin        identity's three targets and behind them copies with + 0.25 added, the copies weighted 2^-e.  Every voxel has exactly two contributors,
                weights 1 and 2^-e, so leaving out the original leaves denL = 2^-e of den_v = 1 + 2^-e: for e <= 19 that is above the floor 2^-20 den_v and
                the original is predicted with its copy's bits; for e >= 20 it is not and the original is NaN everywhere.  The copies are always
                predicted, with the originals' bits
    outside     fuse_cases.outside_target() alone;  none: m = 0;  flagged: only the two flagged targets of planes;  pooled: planes as one group (all NaN:
                the group's own sums are the voxels' sums bit for bit)
    many        600 targets of 5 x 6 into (3, 12, 12) with 600 explicit groups: 601 offsets (two upload launches) and units past 256; and in groups of 3

``reference(name)`` computes leave_out_on_host once per case and shares it."""
import functools

import numpy as np

import fuse_cases as fc
from mri_inr_amd import leave_out as lo

PLANES_GROUPS = (3, 1, 2, 2)
MIN_COVERAGES = (0.0, 0.25)
TWIN_PREDICTED, TWIN_FLOORED = (10, 19), (20, 21, 30)
MANY_M, MANY_SHAPE, MANY_GRID = 600, (5, 6), (3, 12, 12)


def bits_equal(a, b):
    """the same shape, dtype and bit patterns (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_result(got, want):
    """every field of ``got`` that is not None has the bits of ``want``'s"""
    return all(g is None or bits_equal(g, w) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def twin(e):
    d = fc.identity()
    targets = np.concatenate([d["targets"], d["targets"] + np.float32(0.25)])
    weights = np.ones(targets.shape, np.float32)
    weights[3:] = np.float32(2.0 ** -e)
    return dict(targets=targets, maps=np.concatenate([d["maps"], d["maps"]]), weights=weights)


@functools.lru_cache(maxsize=None)
def many():
    rng = np.random.default_rng(23)
    maps = np.zeros((MANY_M, 9), np.float32)
    for q in range(MANY_M):
        ang, s = rng.uniform(-0.2, 0.2), rng.uniform(1.4, 1.9)
        c, sn = s * np.cos(ang), s * np.sin(ang)
        maps[q] = (rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(-0.2, 2.2), c, -sn, rng.uniform(0.0, 3.5), sn, c, rng.uniform(0.0, 2.5))
    targets = fc.targets_of(maps, MANY_SHAPE) + (0.05 * rng.standard_normal((MANY_M,) + MANY_SHAPE)).astype(np.float32)
    return dict(targets=targets, maps=maps)


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> ((targets, maps, grid, spacing), keywords of leave_out_on_host / model.leave_out_targets)"""
    out = {}
    d = fc.planes()
    for g, grid in enumerate(fc.GRIDS):
        for tname, thickness in zip(("full", "quarter"), fc.THICKNESSES):
            for gname, groups in (("singletons", None), ("groups", PLANES_GROUPS)):
                for mc in MIN_COVERAGES:
                    out[f"planes-grid{g}-{tname}-{gname}-mc{mc}"] = ((d["targets"], d["maps"], grid, fc.SPACING), dict(groups=groups, thickness=thickness,
                                                                     weights=d["weights"], intensity=d["intensity"], min_coverage=mc))
    t = fc.truth_case()
    for tname, thickness in zip(("full", "quarter"), fc.THICKNESSES):
        for gname, groups in (("singletons", None), ("fours", (4,) * 6)):
            out[f"truth-{tname}-{gname}"] = ((t["targets"], t["maps"], fc.TRUTH_GRID, fc.SPACING), dict(groups=groups, thickness=thickness))
    for shift in fc.GRAZE_SHIFTS:
        for thickness in fc.GRAZE_THICKNESSES:
            g = fc.graze(shift)
            out[f"graze{shift:+d}-{thickness!r}"] = ((g["targets"], g["maps"], fc.GRIDS[0], fc.SPACING), dict(thickness=thickness))
    i = fc.identity()
    out["identity"] = ((i["targets"], i["maps"], fc.IDENTITY_GRID, fc.SPACING), {})
    for e in TWIN_PREDICTED + TWIN_FLOORED:
        w = twin(e)
        out[f"twin-{e}"] = ((w["targets"], w["maps"], fc.IDENTITY_GRID, fc.SPACING), dict(weights=w["weights"]))
    o = fc.outside_target()
    out["outside"] = ((o["targets"], o["maps"], fc.GRIDS[0], fc.SPACING), dict(weights=o["weights"], intensity=o["intensity"]))
    out["none"] = ((np.zeros((0,) + fc.SHAPE, np.float32), np.zeros((0, 9), np.float32), fc.GRIDS[1], fc.SPACING), {})
    f = slice(fc.DEGENERATE_AT, fc.M)
    out["flagged"] = ((d["targets"][f], d["maps"][f], fc.GRIDS[0], fc.SPACING), dict(weights=d["weights"][f], intensity=d["intensity"][f]))
    out["pooled"] = ((d["targets"], d["maps"], fc.GRIDS[0], fc.SPACING), dict(groups=(fc.M,), weights=d["weights"], intensity=d["intensity"]))
    k = many()
    out["many-singletons"] = ((k["targets"], k["maps"], MANY_GRID, fc.SPACING), dict(groups=tuple(range(MANY_M + 1))))
    out["many-threes"] = ((k["targets"], k["maps"], MANY_GRID, fc.SPACING), dict(groups=(3,) * (MANY_M // 3)))
    return out


ALL_NAN = tuple(n for n in all_cases() if n.startswith("graze") or n in ("identity", "outside", "flagged", "pooled"))


@functools.lru_cache(maxsize=None)
def reference(name):
    """leave_out_on_host of the case, computed once and shared (its arrays are read-only)"""
    args, kw = all_cases()[name]
    r = lo.leave_out_on_host(*args, **kw)
    for x in r:
        x.setflags(write=False)
    return r
