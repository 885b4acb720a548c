"""Reference for slices scored under affine maps against targets (msiren_align_slices*): numpy, fp64, on top of
tests/resample_reference.resample one slice at a time.  Not a test module: tests/test_align_reference.py checks it on the CPU,
tests/test_gpu_align.py gates the kernels against it.

    map (a00, a01, t0, a10, a11, t1), lattice (th, tw):  pixel (i, j) is read at
        Y = ((a00 i) + (a01 j)) + t0      X = ((a10 i) + (a11 j)) + t1      in fp32, one rounding per operation
    R, gY, gX: resample_reference of the slice at (Y, X);  valid iff target, R, gY, gX are all finite
    r = R - T,  J = (gY i, gY j, gY, gX i, gX j, gX);  count = sum 1, cost = sum r r, dcost[a] = sum (2 r) J[a], jtj[a, b] = sum J[a] J[b]
    sums = [count, cost, dcost[0..5], jtj upper triangle row-major]   (29)
``sums_of_planes`` also returns the sum of the magnitudes of every sum's terms: what errors are measured against.

``seed`` plants one error of the kinds an implementation of the sums can make (SEEDS); tests/test_align_reference.py asserts that the gate of
tests/align_cases.py rejects every one of them.
"""
import numpy as np

import resample_reference as rr

SUMS = 29
CHUNK = 1024
PACK = [(a, b) for a in range(6) for b in range(a, 6)]  # the upper triangle, row-major
SEEDS = ("ij_swapped", "g_swapped", "factor2_dropped", "packing_transposed", "invalid_counted", "chunk_dropped")


def points(map_row, shape):
    """(th tw, 2) float32: the rule above, operation by operation in float32"""
    a = [np.float32(x) for x in np.asarray(map_row, dtype=np.float32)]
    th, tw = shape
    i = np.repeat(np.arange(th), tw).astype(np.float32)
    j = np.tile(np.arange(tw), th).astype(np.float32)
    y0, y1, x0, x1 = a[0] * i, a[1] * j, a[3] * i, a[4] * j
    Y, X = (y0 + y1) + a[2], (x0 + x1) + a[5]
    assert Y.dtype == np.float32 and X.dtype == np.float32
    return np.stack([Y, X], axis=1)


def sums_of_planes(R, gY, gX, target, shape, seed=None):
    """planes and target (th tw) or (th, tw) -> (sums (29), magnitudes (29)) in fp64 from whatever precision the planes have"""
    th, tw = shape
    R, gY, gX, T = (np.asarray(x).reshape(th * tw).astype(np.float64) for x in (R, gY, gX, target))
    i = np.repeat(np.arange(th), tw).astype(np.float64)
    j = np.tile(np.arange(tw), th).astype(np.float64)
    ok = np.isfinite(T) & np.isfinite(R) & np.isfinite(gY) & np.isfinite(gX)
    if seed == "chunk_dropped":  # the last chunk of 1024 pixels never added
        ok = ok & (np.arange(th * tw) < (th * tw - 1) // CHUNK * CHUNK)
    if seed == "ij_swapped":
        i, j = j, i
    if seed == "g_swapped":
        gY, gX = gX, gY
    R, gY, gX, T, i, j = (x[ok] for x in (R, gY, gX, T, i, j))
    r = R - T
    J = [gY * i, gY * j, gY, gX * i, gX * j, gX]
    two = 1.0 if seed == "factor2_dropped" else 2.0
    pack = sorted(PACK, key=lambda ab: (ab[1], ab[0])) if seed == "packing_transposed" else PACK
    terms = [np.ones_like(r), r * r] + [(two * r) * J[a] for a in range(6)] + [J[a] * J[b] for a, b in pack]
    sums = np.array([t.sum() for t in terms], np.float64)
    mags = np.array([np.abs(t).sum() for t in terms], np.float64)
    if seed == "invalid_counted":
        sums[0] = mags[0] = float(th * tw)
    return sums, mags


def align(slice_fn, maps, targets, seed=None):
    """``slice_fn(s, yx)`` -> (value (m), grad (2, m)) of slice s at the points yx (m, 2), as resample_reference.resample returns them
    -> (sums (n, 29), magnitudes (n, 29), planes (3, n, th, tw))"""
    targets = np.asarray(targets, dtype=np.float32)
    n, th, tw = targets.shape
    sums, mags, planes = np.zeros((n, SUMS)), np.zeros((n, SUMS)), None
    for s in range(n):
        val, grad = slice_fn(s, points(maps[s], (th, tw)))
        if planes is None:
            planes = np.zeros((3, n, th, tw), val.dtype)
        planes[0, s], planes[1, s], planes[2, s] = val.reshape(th, tw), grad[0].reshape(th, tw), grad[1].reshape(th, tw)
        sums[s], mags[s] = sums_of_planes(val, grad[0], grad[1], targets[s], (th, tw), seed)
    return sums, mags, planes


def align_of_stack(sd, mods, black, maps, targets, nV, nH, S, I, *, num_layers, activation="sine", dtype=np.float64, perturbed=False):
    """mods[s] (L, nV nH, H), black[s]: what resample_reference.resample takes for slice s; dtype / perturbed are passed through to it
    (fp32 + perturbed is the variant that sizes the gate; its sums are fp64 from the fp32 planes, as the kernels' are)"""
    def slice_fn(s, yx):
        return rr.resample(sd, mods[s], black[s], yx, nV, nH, S, I, num_layers=num_layers, activation=activation, dtype=dtype, perturbed=perturbed)

    return align(slice_fn, maps, targets)
