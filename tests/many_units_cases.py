"""Long problems for the registration and reconstruction families: more than 256 units (targets, groups, columns), where the one-thread-per-unit kernels
run their second workgroup, align_group_upload_kernel its second and third launch, the column loops of project_stats_kernel and irls_stats_kernel their
second lap, and a group's members lie in two workgroups.  Shared by tests/test_many_units_reference.py (CPU) and tests/test_gpu_many_units.py.  Not a
test module; pure numpy on top of tests/align_stack_cases.py, tests/align_group_cases.py and tests/fuse_cases.py, no GPU and no model needed.

    grouped(n_groups, seed, family)   a long grouped problem whose instances are the base case's three groups (sizes 3, 1, 2) in a seeded, non-periodic
                                      order, every instance with its own planes (the base planes moved in plane by up to 0.4 pixel), weights (the bump's
                                      centre moved), truth intensity, start state (the identity and an in-plane shift of at most 0.05 pixel) and targets.
                                      ``family`` "stack": tests/align_stack_cases.py's solve on the voxel stack, the targets included; "trunk":
                                      tests/align_group_cases.py's on the stack the network reconstructs -- its targets are g W + b of the warped planes W
                                      at ``truth_maps``, which only a model gives: ``with_warped`` completes the case
    one_big_group()                   260 targets on the stack case's group 0 planes, z spread over its range, as ONE group
    many_targets()                    260 targets of 6 x 7 over a (3, 12, 14) grid for fuse / project / solve_volume(_robust)
    wide_target()                     two targets of 3 x 300 over a (2, 5, 310) grid

The order of the sizes is drawn once for ORDER groups and nudged so that one 3-member group holds targets 255, 256 and 257; a problem of n groups is its
first n, so G_TRUNK (the shortest with m >= 258 and G >= 129 that ends behind that group) and G_STACK (1030 groups: 1031 offsets, three upload launches
of 512, the last one partial) share their first groups."""
import functools

import numpy as np

import align_group_cases as gc
import align_stack_cases as sc
import align_volume_w_cases as wc
import fuse_cases as fc
from mri_inr_amd import align_stack as ast, align_volume as av

SEED = 3
ORDER = 2048                 # groups drawn; every problem is a prefix
STRADDLE_AT = 255            # the first target of the 3-member group that holds 255, 256 and 257
WORKGROUP, UPLOAD = 256, 512  # units per workgroup of the per-unit kernels; group offsets per launch of align_group_upload_kernel
G_STACK = 1030
G_TRUNK = 129
SIZES = np.array(sc.SIZES)
SHAPE, SPACING = sc.SHAPE, sc.SPACING
assert gc.SIZES == sc.SIZES and gc.SHAPE == sc.SHAPE and gc.SPACING == sc.SPACING and wc.BLOCK == sc.BLOCK
PLANE_MOVE, START_SHIFT, WEIGHT_MOVE = 0.4, 0.05, 1.5


@functools.lru_cache(maxsize=None)
def order(seed=SEED):
    """-> (base (ORDER,) the base group of every instance, the index of the group that holds targets 255 .. 257)"""
    base = np.random.default_rng([seed, 0]).integers(0, 3, ORDER)
    start = np.concatenate([[0], np.cumsum(SIZES[base])])
    y = int(np.searchsorted(start, STRADDLE_AT, side="right")) - 1   # the group that holds target 255
    d = STRADDLE_AT - int(start[y])
    if d:                                                            # make it end in front of 255: a group of d = 1 or 2 targets
        base[y] = {1: 1, 2: 2}[d]
        y += 1
    base[y] = 0                                                      # and the next one is the 3-member group
    return base, y


def shortest_trunk(seed=SEED):
    """the smallest number of groups with m >= 258, G >= 129 and the straddling group complete"""
    return max(order(seed)[1] + 1, 129)


def _weights(rows, move, masked):
    th, tw = SHAPE
    i, j = np.mgrid[0:th, 0:tw]
    w = np.stack([0.2 + 0.8 * np.exp(-(((i - 0.5 * th - a) / (0.6 * th)) ** 2 + ((j - 0.5 * tw - q - b) / (0.6 * tw)) ** 2)) for q, (a, b) in zip(rows, move)]).astype(np.float32)
    if masked:
        w[(slice(None),) + sc.BLOCK] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def grouped(n_groups, seed=SEED, family="stack"):
    """-> dict: base (G,), group_start (G + 1,) int32, group_of (m,), member (m,) the base case's row of every target, planes (m, 12), rigid (G, 12) the
    start states, truth_rigid (G, 12), truth_maps (m, 9) float32, intensity (m, 2) float32 the truth (g, b), weights (m, th, tw) float32 (the block
    masked), weights_unmasked, scales (m,), targets (m, th, tw) float32 (stack family; None for the trunk family until ``with_warped``), straddling: the
    group that holds targets 255 .. 257"""
    case = sc if family == "stack" else gc
    base, straddling = order(seed)
    base = base[:n_groups].copy()
    G = len(base)
    rng = np.random.default_rng([seed, 1])
    move = rng.uniform(-PLANE_MOVE, PLANE_MOVE, (ORDER, 2))[:G]
    shift = rng.uniform(-START_SHIFT, START_SHIFT, (ORDER, 2))[:G]
    wmove = rng.uniform(-WEIGHT_MOVE, WEIGHT_MOVE, (ORDER, 2))[:G]
    dgb = rng.uniform(-1.0, 1.0, (ORDER, 3, 2))[:G] * np.array([0.1, 0.05])
    group_start = np.concatenate([[0], np.cumsum(SIZES[base])]).astype(np.int32)
    group_of = np.repeat(np.arange(G), SIZES[base])
    member = np.concatenate([np.arange(case.GROUP_START[b], case.GROUP_START[b + 1]) for b in base])
    within = np.arange(len(member)) - group_start[group_of]
    planes = case.planes()[member].copy()
    planes[:, 7:9] += move[group_of]      # the origin and the centre, in plane: the whole instance moves
    planes[:, 10:12] += move[group_of]
    rigid = case.start_rigid(G)
    rigid[:, 10:12] = shift
    truth_rigid = case.truth_rigid()[base]
    truth_maps = np.array([av.rigid_map3([float(x) for x in truth_rigid[y]], [float(x) for x in p], SPACING) for p, y in zip(planes, group_of)], np.float32)
    intensity = (case.GB_TRUTH[member].astype(np.float64) + dgb[group_of, within]).astype(np.float32)
    out = dict(family=family, base=base, group_start=group_start, group_of=group_of, member=member, planes=planes, rigid=rigid, truth_rigid=truth_rigid, truth_maps=truth_maps,
               intensity=intensity, weights=_weights(member, wmove[group_of], True), weights_unmasked=_weights(member, wmove[group_of], False),
               scales=np.full(len(member), sc.SOLVE_SCALE, np.float64), straddling=straddling if straddling < G else None, targets=None)
    if family == "stack":
        out["stack"] = sc.stack("smooth")
        warped = np.stack([ast.read_stack(out["stack"], av.map_points3(mp, SHAPE))[0].reshape(SHAPE) for mp in truth_maps])
        out = with_warped(out, warped)
    return out


def with_warped(case, warped):
    """the case with its targets: g W + b of the planes W (m, th, tw) at ``truth_maps``, rounded to float32, the block corrupted by + 5 (an uncovered
    pixel stays NaN: masked)"""
    gb = case["intensity"].astype(np.float64)
    t = gb[:, 0, None, None] * np.asarray(warped, np.float64).reshape((-1,) + SHAPE) + gb[:, 1, None, None]
    t[(slice(None),) + sc.BLOCK] += sc.CORRUPTION
    return dict(case, targets=t.astype(np.float32))


def group_rows(case, lo, hi):
    """the groups lo .. hi - 1 of a grouped case as a problem of their own -> dict(targets=slice, groups=slice, group_start (hi - lo + 1,))"""
    gs = case["group_start"]
    return dict(targets=slice(int(gs[lo]), int(gs[hi])), groups=slice(lo, hi), group_start=(gs[lo:hi + 1] - gs[lo]).astype(np.int32))


def chunks(count, size=64):
    """consecutive (lo, hi) of at most ``size`` units that cover ``count``"""
    return [(lo, min(lo + size, count)) for lo in range(0, count, size)]


def sampled_groups(case):
    """the first group, the one that holds targets 255 .. 257, the first with index >= 512, the last"""
    return (0, case["straddling"], UPLOAD, len(case["base"]) - 1)


def errors(case, maps, intensity, rows, est):
    """the largest |parameter - truth| over the targets ``rows`` (a slice): the nine map entries of every member and, where it is estimated, (g, b) of
    every member that sees the stack (``maps``, ``intensity``: those of the rows)"""
    family = sc if case["family"] == "stack" else gc
    e = np.abs(np.asarray(maps, np.float64) - case["truth_maps"][rows].astype(np.float64)).max(axis=1)
    if est == av.ESTIMATE:
        gbe = np.abs(np.asarray(intensity, np.float64) - case["intensity"][rows].astype(np.float64)).max(axis=1)
        outside = family.SOLVE_OUTSIDE if case["family"] == "stack" else family.OUTSIDE
        e = np.maximum(e, np.where(case["member"][rows] == outside, 0.0, gbe))
    return float(e.max())


# ---- one group of 260 ---------------------------------------------------------------------------------------------------------------------------------
BIG = 260


@functools.lru_cache(maxsize=None)
def one_big_group():
    """260 targets on the planes of the stack case's group 0 (its centre, its truth), z spread evenly over 0.4 .. 1.6 slices, as one group: its members span
    two workgroups of the per-target kernels while one thread decides and steps.  -> the keys of ``grouped``"""
    rng = np.random.default_rng([SEED, 2])
    z = np.linspace(sc._Z[0], sc._Z[2], BIG)
    planes = np.tile(sc.planes()[0], (BIG, 1))
    planes[:, 6] = SPACING * z
    truth_rigid = sc.truth_rigid()[:1]
    truth_maps = np.array([av.rigid_map3([float(x) for x in truth_rigid[0]], [float(x) for x in p], SPACING) for p in planes], np.float32)
    intensity = (np.array([1.0, 0.0]) + rng.uniform(-1.0, 1.0, (BIG, 2)) * np.array([0.25, 0.1])).astype(np.float32)
    member = np.arange(BIG) % 3
    out = dict(family="stack", base=np.zeros(1, np.int64), group_start=np.array([0, BIG], np.int32), group_of=np.zeros(BIG, np.int64), member=member, planes=planes,
               rigid=sc.start_rigid(1), truth_rigid=truth_rigid, truth_maps=truth_maps, intensity=intensity, weights=_weights(member, rng.uniform(-1.5, 1.5, (BIG, 2)), True),
               weights_unmasked=_weights(member, rng.uniform(-1.5, 1.5, (BIG, 2)), False), scales=np.full(BIG, sc.SOLVE_SCALE, np.float64), straddling=0, targets=None,
               stack=sc.stack("smooth"))
    warped = np.stack([ast.read_stack(out["stack"], av.map_points3(mp, SHAPE))[0].reshape(SHAPE) for mp in truth_maps])
    return with_warped(out, warped)


# ---- fuse / project / solve_volume(_robust) -----------------------------------------------------------------------------------------------------------------
MANY, MANY_SHAPE, MANY_GRID = 260, (6, 7), (3, 12, 14)
MANY_DEGENERATE_AT, MANY_ZERO_GAIN_AT = 258, 259
MANY_LATE = (256, 257)       # the two ordinary targets past the first workgroup: they alone reach the voxels with x >= 9
MANY_SCALE = 0.05


@functools.lru_cache(maxsize=None)
def many_targets():
    """-> dict(targets (260, 6, 7), maps (260, 9), weights, intensity (260, 2), scales (260,), grid, spacing).  Targets 0 .. 255 lie over x <= 8.5 of the
    grid, 256 and 257 over 6.6 <= x <= 12.6: the voxels with x >= 9 have no other source.  258 is a degenerate map (b = 2 a), 259 has gain 0."""
    rng = np.random.default_rng([SEED, 3])
    th, tw = MANY_SHAPE
    maps = np.zeros((MANY, 9), np.float32)
    for q in range(MANY):
        ang, z0, z1 = rng.uniform(-0.1, 0.1), rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03)
        c, s = np.cos(ang), np.sin(ang)
        late = q in MANY_LATE
        ty, tx = (5.3, 6.6) if late else (rng.uniform(0.5, 5.5), rng.uniform(0.6, 2.0))
        maps[q] = (z0, z1, rng.uniform(-0.1, 2.1), c, -s, ty, s, c, tx) if not late else (z0, z1, 0.4 + 1.1 * (q - 256), 1.0, 0.0, ty, 0.0, 1.0, tx)
    a = maps[0, 0::3].copy()
    maps[MANY_DEGENERATE_AT, 0::3], maps[MANY_DEGENERATE_AT, 1::3] = a, 2 * a
    gb = (np.array([1.0, 0.0]) + rng.uniform(-1.0, 1.0, (MANY, 2)) * np.array([0.2, 0.1])).astype(np.float32)
    gb[MANY_ZERO_GAIN_AT] = (0.0, 0.3)
    targets = fc.targets_of(maps, MANY_SHAPE, np.where(gb[:, :1] == 0, np.float32(1), gb))
    targets = (targets + rng.normal(0.0, 0.02, targets.shape)).astype(np.float32)
    hit = rng.random(targets.shape) < 0.03
    targets[hit] += np.float32(2.0)          # outliers for the robust rounds
    w = rng.uniform(0.2, 1.0, targets.shape).astype(np.float32)
    w[rng.random(w.shape) < 0.05] = 0.0
    w[257, 2, 3], targets[256, 4, 1] = np.nan, np.nan
    scales = np.full(MANY, MANY_SCALE, np.float64)
    scales[5::17] = np.inf
    for x in (targets, maps, w, gb, scales):
        x.setflags(write=False)
    return dict(targets=targets, maps=maps, weights=w, intensity=gb, scales=scales, grid=MANY_GRID, spacing=fc.SPACING)


WIDE_SHAPE, WIDE_GRID = (3, 300), (2, 5, 310)
WIDE_NAN_PIXEL = (1, 1, 283)


@functools.lru_cache(maxsize=None)
def wide_target():
    """two targets of 3 x 300 -- 256 + 44 columns -- flat at Z = 0.3 and 0.8 over a (2, 5, 310) grid; seeded weights everywhere, zeros and one NaN pixel
    among the columns >= 256 -> the keys of ``many_targets``"""
    rng = np.random.default_rng([SEED, 4])
    maps = np.array([[0.0, 0.0, 0.3, 1.0, 0.0, 0.7, 0.0, 1.0, 3.2], [0.001, 0.0002, 0.8, 0.98, 0.0, 1.1, 0.0, 1.01, 2.4]], np.float32)
    gb = np.array([[1.1, 0.05], [0.9, -0.1]], np.float32)
    targets = (fc.targets_of(maps, WIDE_SHAPE, gb) + rng.normal(0.0, 0.02, (2,) + WIDE_SHAPE)).astype(np.float32)
    targets[:, :, 260::7] += np.float32(1.5)
    w = rng.uniform(0.2, 1.0, targets.shape).astype(np.float32)
    w[:, :, 270:275] = 0.0
    targets[WIDE_NAN_PIXEL] = np.nan
    for x in (targets, maps, w, gb):
        x.setflags(write=False)
    return dict(targets=targets, maps=maps, weights=w, intensity=gb, scales=np.array([MANY_SCALE, 0.2]), grid=WIDE_GRID, spacing=fc.SPACING)
