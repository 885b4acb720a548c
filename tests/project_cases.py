"""The cases of msiren_project_volume shared by tests/test_project_reference.py (CPU) and tests/test_gpu_project.py.  Not a
test module; no GPU and no model needed: pure numpy on top of tests/fuse_cases.py, small enough that every GPU test takes seconds.

    planes      fuse_cases.planes()'s eight maps (six planes, the DEGENERATE map, the target whose gain is 0) on the lattice 19 x 23, projecting the
                analytic volume sampled on either grid.  At thickness spacing / 4 the window is one pixel wide and the planes 0, 2 and 3 pass between
                the slices wherever they cross the grid: they are covered nowhere (checked below) -- the whole-target NaN path.  For the residual
                and the sums: planes()'s targets and weights with their zero block, the NaN weight and the NaN pixel
    graze       fuse_cases.graze(shift) x GRAZE_THICKNESSES: the window's edge and the last row and column sit on voxels, one ulp either side
    identity    a random stack (3, 19, 23) under unit maps on integer Z: the projection returns its bits with coverage 1
    truth       fuse_cases.truth_case(): 24 targets of 44 x 46 overhang the (4, 40, 40) grid on every side, so the box is clipped on every face
    holes       the planes case on a stack with a NaN slab and single NaN voxels: a NaN voxel only thins the coverage
    outside     fuse_cases.outside_target(): covered nowhere
ONE_STEP: the mean error against the analytic volume over the covered voxels after one back-projection step V + fuse(T - project(V)) on the truth case
at thickness = spacing, measured from the host restatements (before the step: fuse_cases.TRUTH_ERRORS[SPACING])."""
import functools

import numpy as np

import fuse_cases as fc

SPACING, SHAPE, GRIDS, THICKNESSES = fc.SPACING, fc.SHAPE, fc.GRIDS, fc.THICKNESSES
UNCOVERED_AT_QUARTER = (0, 2, 3)      # planes covered nowhere at thickness spacing / 4 (besides the flagged ones and plane 5, below the stack)
TRUTH_COVERED_PIXELS = 0.838          # the share of the truth case's target pixels that are covered at thickness = spacing, measured
ONE_STEP = 0.02777                    # mean |V1 - V| over the covered voxels, measured (0.0767 before the step)


@functools.lru_cache(maxsize=None)
def stack(grid):
    """the analytic volume on the voxels of ``grid``, float32"""
    z, y, x = np.mgrid[0:grid[0], 0:grid[1], 0:grid[2]].astype(np.float64)
    v = fc.volume_at(z, y, x).astype(np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def holes(grid):
    """the stack with a NaN slab, single NaN voxels and an infinity"""
    v = stack(grid).copy()
    v[1, 10:20, 5:30] = np.nan
    v[0, 3, 7] = v[2, 17, 17] = v[2, 30, 2] = np.nan
    v[1, 25, 33] = np.inf
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def identity():
    rng = np.random.default_rng(12)
    v = rng.standard_normal(fc.IDENTITY_GRID).astype(np.float32)
    v.setflags(write=False)
    return dict(volume=v, maps=fc.identity()["maps"])


def planes(grid, intensity=True, volume=None):
    """-> (args, kwargs) of project_on_host / model.project_volume without the thickness"""
    d = fc.planes()
    return (stack(grid) if volume is None else volume, d["maps"], SHAPE, SPACING), dict(intensity=d["intensity"] if intensity else None)


def truth():
    t = fc.truth_case()
    return (stack(fc.TRUTH_GRID), t["maps"], fc.TRUTH_SHAPE, SPACING), {}


def all_cases():
    """name -> (args, kwargs with the thickness): every case of the bit-for-bit comparison"""
    out = {}
    for g, grid in enumerate(GRIDS):
        for thickness in THICKNESSES:
            for gb in (True, False):
                args, kw = planes(grid, gb)
                out[f"planes-grid{g}-t{thickness:g}-{'gb' if gb else 'plain'}"] = (args, dict(kw, thickness=thickness))
        args, kw = planes(grid, True, holes(grid))
        out[f"holes-grid{g}"] = (args, dict(kw, thickness=SPACING))
    for shift in fc.GRAZE_SHIFTS:
        for t, thickness in enumerate(fc.GRAZE_THICKNESSES):
            out[f"graze{shift:+d}-t{t}"] = ((stack(GRIDS[0]), fc.graze(shift)["maps"], SHAPE, SPACING), dict(thickness=thickness))
    d = identity()
    out["identity"] = ((d["volume"], d["maps"], SHAPE, SPACING), dict(thickness=SPACING))
    for thickness in THICKNESSES:
        args, kw = truth()
        out[f"truth-t{thickness:g}"] = (args, dict(kw, thickness=thickness))
    o = fc.outside_target()
    out["outside"] = ((stack(GRIDS[1]), o["maps"], SHAPE, SPACING), dict(intensity=o["intensity"], thickness=SPACING))
    return out
