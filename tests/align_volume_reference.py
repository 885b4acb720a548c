"""Reference for target slices scored against a stack read as a volume (msiren_align_volume*): numpy, fp64, on top of
tests/volume_reference.volume.  Not a test module: tests/test_align_volume_reference.py checks it on the CPU, tests/test_gpu_align_volume.py
gates the kernels against it.

    map (z0, z1, tz, y0, y1, ty, x0, x1, tx), lattice (th, tw):  pixel (i, j) is read at
        Z = ((z0 i) + (z1 j)) + tz      Y = ((y0 i) + (y1 j)) + ty      X = ((x0 i) + (x1 j)) + tx      in fp32, one rounding per operation
    R, gZ, gY, gX: volume_reference.volume of the stack at (Z, Y, X);  valid iff target, R, gZ, gY, gX are all finite
    r = R - T,  J = (gZ i, gZ j, gZ, gY i, gY j, gY, gX i, gX j, gX);  count = sum 1, cost = sum r r, dcost[a] = sum (2 r) J[a],
    jtj[a, b] = sum J[a] J[b];  sums = [count, cost, dcost[0..8], jtj upper triangle row-major]   (56)
``sums_of_planes`` also returns the sum of the magnitudes of every sum's terms: what errors are measured against.

``seed`` plants one error of the kinds an implementation can make (SEEDS: in the sums; VOLUME_SEEDS: in how the pair of slices is read);
tests/test_align_volume_reference.py asserts that the gate of tests/align_volume_cases.py rejects every one of them.
"""
import numpy as np

import volume_reference as vr

SUMS = 56
CHUNK = 1024
PACK = [(a, b) for a in range(9) for b in range(a, 9)]  # the upper triangle, row-major
SEEDS = ("zy_swapped", "factor2_dropped", "packing_transposed", "invalid_z_counted", "chunk_dropped")
VOLUME_SEEDS = ("gz_of_blend", "second_slice_ignored")


def points(map_row, shape):
    """(th tw, 3) float32: the rule above, operation by operation in float32"""
    a = [np.float32(x) for x in np.asarray(map_row, dtype=np.float32)]
    th, tw = shape
    i = np.repeat(np.arange(th), tw).astype(np.float32)
    j = np.tile(np.arange(tw), th).astype(np.float32)
    rows = []
    for r in range(3):
        p0, p1 = a[3 * r] * i, a[3 * r + 1] * j
        rows.append((p0 + p1) + a[3 * r + 2])
    assert all(x.dtype == np.float32 for x in rows)
    return np.stack(rows, axis=1)


def sums_of_planes(R, gZ, gY, gX, target, shape, seed=None, valid_z=None):
    """planes and target (th tw) or (th, tw) -> (sums (56), magnitudes (56)) in fp64 from whatever precision the planes have.  ``valid_z`` (th tw)
    bool: which pixels have a valid Z (the seed "invalid_z_counted" counts the others)."""
    th, tw = shape
    R, gZ, gY, gX, T = (np.asarray(x).reshape(th * tw).astype(np.float64) for x in (R, gZ, gY, gX, target))
    i = np.repeat(np.arange(th), tw).astype(np.float64)
    j = np.tile(np.arange(tw), th).astype(np.float64)
    ok = np.isfinite(T) & np.isfinite(R) & np.isfinite(gZ) & np.isfinite(gY) & np.isfinite(gX)
    if seed == "chunk_dropped":  # the last chunk of 1024 pixels never added
        ok = ok & (np.arange(th * tw) < (th * tw - 1) // CHUNK * CHUNK)
    if seed == "zy_swapped":
        gZ, gY = gY, gZ
    extra = 0.0
    if seed == "invalid_z_counted":
        extra = float((np.isfinite(T) & ~np.asarray(valid_z).reshape(th * tw)).sum())
    R, gZ, gY, gX, T, i, j = (x[ok] for x in (R, gZ, gY, gX, T, i, j))
    r = R - T
    J = [gZ * i, gZ * j, gZ, gY * i, gY * j, gY, gX * i, gX * j, gX]
    two = 1.0 if seed == "factor2_dropped" else 2.0
    pack = sorted(PACK, key=lambda ab: (ab[1], ab[0])) if seed == "packing_transposed" else PACK
    terms = [np.ones_like(r), r * r] + [(two * r) * J[a] for a in range(9)] + [J[a] * J[b] for a, b in pack]
    sums = np.array([t.sum() for t in terms], np.float64)
    mags = np.array([np.abs(t).sum() for t in terms], np.float64)
    sums[0] += extra
    mags[0] += extra
    return sums, mags


def seeded_volume(slice_fn, pts, n, dtype, seed):
    """volume_reference.volume with one error in how the pair is read: "gz_of_blend" takes grad[0] as the blended value's difference to the first
    slice, value - R0 = f (R1 - R0), instead of R1 - R0; "second_slice_ignored" reads the first slice of the pair alone (value and in-plane
    gradient as if f' were 0)"""
    z0, f = vr.pairs(pts, n)

    value, grad = vr.volume(slice_fn, pts, n, dtype)
    at_first = np.asarray(pts, np.float32).copy()
    at_first[:, 0] = np.where(z0 >= 0, z0, np.nan).astype(np.float32)  # f' = 0 there: the value and in-plane planes are the first slice's
    v0, g0 = vr.volume(slice_fn, at_first, n, dtype)
    grad = grad.copy()
    if seed == "gz_of_blend":
        grad[0] = value - v0
    elif seed == "second_slice_ignored":
        value, grad[1], grad[2] = v0, g0[1], g0[2]
    else:
        raise ValueError(seed)
    return value, grad


def align_volume(slice_fn, n, maps, targets, seed=None, dtype=np.float64):
    """``slice_fn(s, yx)`` -> (value (k), grad (2, k)) of slice s of n at the points yx (k, 2), as resample_reference.resample returns them
    -> (sums (m, 56), magnitudes (m, 56), planes (4, m, th, tw) = R, gZ, gY, gX)"""
    targets = np.asarray(targets, dtype=np.float32)
    m, th, tw = targets.shape
    sums, mags, planes = np.zeros((m, SUMS)), np.zeros((m, SUMS)), None
    for q in range(m):
        pts = points(maps[q], (th, tw))
        val, grad = seeded_volume(slice_fn, pts, n, dtype, seed) if seed in VOLUME_SEEDS else vr.volume(slice_fn, pts, n, dtype)
        if planes is None:
            planes = np.zeros((4, m, th, tw), val.dtype)
        planes[0, q] = val.reshape(th, tw)
        planes[1:, q] = grad.reshape(3, th, tw)
        sums[q], mags[q] = sums_of_planes(val, grad[0], grad[1], grad[2], targets[q], (th, tw), seed if seed in SEEDS else None, vr.pairs(pts, n)[0] >= 0)
    return sums, mags, planes


def align_volume_of_stack(sd, mods, black, maps, targets, nV, nH, S, I, *, num_layers, activation="sine", dtype=np.float64, perturbed=False, seed=None,
                          cache=None):
    """mods[s] (L, nV nH, H), black[s]: what resample_reference.resample takes for slice s; dtype / perturbed are passed through to it
    (fp32 + perturbed is the variant that sizes the gate; its sums are fp64 from the fp32 planes, as the kernels' are).  ``cache``: a dict that
    keeps every slice's planes by (slice, points), so that a seeded run after the plain one evaluates no network again."""
    import resample_reference as rr

    def slice_fn(s, yx):
        key = (s, np.ascontiguousarray(yx).tobytes())
        if cache is None or key not in cache:
            out = rr.resample(sd, mods[s], black[s], yx, nV, nH, S, I, num_layers=num_layers, activation=activation, dtype=dtype, perturbed=perturbed)
            if cache is None:
                return out
            cache[key] = out
        return cache[key]

    return align_volume(slice_fn, len(mods), maps, targets, seed, dtype)
