"""The cases of msiren_fuse_targets shared by tests/test_fuse_reference.py (CPU) and tests/test_gpu_fuse.py.  Not a test
module; no GPU and no model needed: pure numpy, small enough that every GPU test takes seconds.

    planes      tests/align_group_cases.py's six planes (tilted; the last one wholly below the stack in section 5.15's sense, 0.76 pixels under slice 0)
                at their truth maps, target lattice 19 x 23, spacing 4; behind them a DEGENERATE map (b = 2 a) and a target whose gain is 0: m = 8.
                Targets g_t V + b_t of the analytic volume V below, section 5.14's smooth weights with their zero block, one NaN weight and one NaN
                target pixel
    graze       three targets whose window edge (cp cp = dt) and last row / column (i = th - 1, j = tw - 1) fall ON tile-corner voxels, and one float32
                ulp either side of them; thickness 4 and the two doubles next to it move dt by ulps of a double: the test of the tile-level cull
    identity    flat targets on integer Z with unit in-plane maps: the fusion returns their bits
    truth       24 targets of 44 x 46 at Z = -0.3 + 0.15 q, tilts within +-0.02 slice per pixel, in-plane rotation within +-0.1 rad, fused into
                (4, 40, 40): how close the fused stack is to V, measured from fuse_on_host and recorded in TRUTH_ERRORS
Output grids (4, 40, 40) and (5, 37, 45): the second has ragged 16 x 16 tiles on both axes and a slice (Z = 4) that no target reaches: its
voxels are NaN with coverage 0."""
import functools

import numpy as np

import align_group_cases as gc

SPACING = 4.0
SHAPE = (19, 23)
GRIDS = ((4, 40, 40), (5, 37, 45))
THICKNESSES = (SPACING, SPACING / 4)
M_PLANES = 6
M = 8                   # the six planes, the degenerate map, the target with gain 0
DEGENERATE_AT, ZERO_GAIN_AT = 6, 7
NAN_WEIGHT_AT, NAN_PIXEL_AT = (1, 4, 7), (2, 9, 11)


def volume_at(Z, Y, X):
    """the analytic volume: Z in slices, (Y, X) in pixels"""
    return 1.5 + np.sin(0.9 * Z + 0.3) * np.cos(0.11 * Y) + 0.5 * np.sin(0.13 * X + 0.05 * Y)


def points_of(maps, shape):
    """maps (m, 9) -> Z, Y, X (m, th, tw) float64 of the target pixels (section 5.13's convention)"""
    mp = np.asarray(maps, np.float64).reshape(-1, 9)[:, :, None, None]
    i, j = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    return tuple(mp[:, 3 * r] * i + mp[:, 3 * r + 1] * j + mp[:, 3 * r + 2] for r in range(3))


def targets_of(maps, shape, intensity=None):
    """float32 targets g V + b of the analytic volume on the planes of ``maps``"""
    v = volume_at(*points_of(maps, shape))
    if intensity is not None:
        gb = np.asarray(intensity, np.float64)
        v = gb[:, 0, None, None] * v + gb[:, 1, None, None]
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def planes():
    """-> dict(targets (8, 19, 23), maps (8, 9), weights, intensity (8, 2)): the main case"""
    maps = np.zeros((M, 9), np.float32)
    maps[:M_PLANES] = gc.truth()
    a = maps[0, 0::3].copy()
    maps[DEGENERATE_AT, 0::3], maps[DEGENERATE_AT, 1::3], maps[DEGENERATE_AT, 2::3] = a, 2 * a, maps[0, 2::3]   # b = 2 a
    maps[ZERO_GAIN_AT] = maps[3]
    gb = np.concatenate([gc.GB_TRUTH, np.array([[1.1, 0.05], [0.0, 0.3]], np.float32)])
    ok = np.isfinite(maps).all(axis=1)
    assert ok.all()
    targets = targets_of(maps, SHAPE, np.where(gb[:, :1] == 0, np.float32(1), gb))
    w = np.concatenate([gc.weights(), gc.weights()[:2]])
    w[NAN_WEIGHT_AT] = np.nan
    targets[NAN_PIXEL_AT] = np.nan
    for x in (targets, maps, w, gb):
        x.setflags(write=False)
    return dict(targets=targets, maps=maps, weights=w, intensity=gb)


def _ulps32(x, s):
    """the float32 x moved by s float32 ulps"""
    x = np.float32(x)
    for _ in range(abs(s)):
        x = np.nextafter(x, np.float32(np.inf if s > 0 else -np.inf))
    return x


GRAZE_SHIFTS = (-1, 0, 1)
GRAZE_THICKNESSES = (float(np.nextafter(4.0, 0.0)), 4.0, float(np.nextafter(4.0, 8.0)))


@functools.lru_cache(maxsize=None)
def graze(shift):
    """-> dict(targets (3, 19, 23), maps (3, 9)), spacing 4, to be fused with GRAZE_THICKNESSES.  All numbers are small dyadic rationals, so cp, i and
    j are exact at the voxels that matter.
        0   a = (3/4, 1, 0), b = (0, 0, 1): det = 25/16, c = (1, -3/4, 0), dt = 25 at thickness 4.  cp = 4 z + 8.25 - 0.75 (y - 16) is 5 (k = 0, the
            window's edge) at z = 2, y = 31: the last row of the tiles y = 16 .. 31, whose other rows have cp > 5 -- the tile contributes through that
            corner row alone, or not at all.  `shift` moves ty by float32 ulps, the thicknesses dt by ulps of a double
        1   a = (0, 1, 0), b = (0, 0, 1), t = (2, -2, -6): on slice 2, i = y + 2 is th - 1 = 18 at y = 16 and j = x + 6 is tw - 1 = 22 at x = 16, the FIRST
            row and column of their tiles: the tiles y >= 16 (x >= 16) contribute through that corner row (column) alone.  `shift` moves ty and tx
        2   the same on slice 1 with i = 0 at y = 15 and j = 0 at x = 31: the last row / column of their tiles"""
    maps = np.zeros((3, 9), np.float32)
    maps[0] = (3.0 / 16, 0, -2.0625, 1, 0, _ulps32(16, shift), 0, 1, 0)
    maps[1] = (0, 0, 2, 1, 0, _ulps32(-2, shift), 0, 1, _ulps32(-6, shift))
    maps[2] = (0, 0, 1, 1, 0, _ulps32(15, shift), 0, 1, _ulps32(31, shift))
    targets = targets_of(maps, SHAPE) + np.float32(1.0)
    targets.setflags(write=False), maps.setflags(write=False)
    return dict(targets=targets, maps=maps)


IDENTITY_GRID = (3, 19, 23)


@functools.lru_cache(maxsize=None)
def identity():
    """three flat targets on Z = 0, 1, 2 covering the grid exactly: unit in-plane maps, thickness = spacing"""
    rng = np.random.default_rng(11)
    targets = rng.standard_normal((3,) + SHAPE).astype(np.float32)
    maps = np.array([[0, 0, z, 1, 0, 0, 0, 1, 0] for z in range(3)], np.float32)
    return dict(targets=targets, maps=maps)


def outside_target():
    """a target five slices below the stack: it contributes nowhere"""
    maps = np.array([[0.01, 0, -5, 1, 0, 3, 0, 1, 2]], np.float32)
    return dict(targets=targets_of(maps, SHAPE), maps=maps, weights=np.ones((1,) + SHAPE, np.float32), intensity=np.array([[2.0, 0.5]], np.float32))


# ---- closeness to the truth ---------------------------------------------------------------------------------------------------------------------------
TRUTH_M, TRUTH_SHAPE, TRUTH_GRID = 24, (44, 46), (4, 40, 40)
TRUTH_COVERED = 0.99  # a condition on the case, not a measurement: at least this share of the voxels is covered
# measured from fuse_on_host on this case: thickness -> (share covered, max |fused - V|, mean |fused - V|) over the covered voxels
TRUTH_ERRORS = {SPACING: (1.0, 0.2813322628885373, 0.07665992225660602), SPACING / 4: (0.99296875, 0.22147512411277082, 0.024412606193894286)}


@functools.lru_cache(maxsize=None)
def truth_case():
    rng = np.random.default_rng(5)
    maps = np.zeros((TRUTH_M, 9), np.float32)
    ci, cj = 0.5 * (TRUTH_SHAPE[0] - 1), 0.5 * (TRUTH_SHAPE[1] - 1)
    for q in range(TRUTH_M):
        ang, z0, z1 = rng.uniform(-0.1, 0.1), rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)
        c, s = np.cos(ang), np.sin(ang)
        tz = (-0.3 + 0.15 * q) - z0 * ci - z1 * cj    # Z at the target's centre
        ty, tx = 19.5 - (c * ci - s * cj), 19.5 - (s * ci + c * cj)
        maps[q] = (z0, z1, tz, c, -s, ty, s, c, tx)
    targets = targets_of(maps, TRUTH_SHAPE)
    z, y, x = np.mgrid[0:TRUTH_GRID[0], 0:TRUTH_GRID[1], 0:TRUTH_GRID[2]].astype(np.float64)
    return dict(targets=targets, maps=maps, volume=volume_at(z, y, x))
