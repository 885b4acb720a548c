"""Reference for weighted, gain/bias-compensated slice alignment (msiren_align_slices_w*): numpy, fp64, on top of
tests/resample_reference.resample one slice at a time, as tests/align_reference.py is for section 5.10.  Not a test module:
tests/test_align_w_reference.py checks it on the CPU, tests/test_gpu_align_w.py gates the kernels against it.

    R, gY, gX: resample_reference of the slice at align_reference.points(map);  weight w, intensity (g, b)
    valid iff target, R, gY, gX are all finite and w is finite and > 0
    m = g R + b,  r = m - T,  J = (g gY i, g gY j, g gY, g gX i, g gX j, g gX, R, 1),  wr = w r
    count = sum 1, wsum = sum w, cost = sum wr r, dcost[a] = sum (2 wr) J[a], jtj[a, b] = sum (w J[a]) J[b]
    sums = [count, wsum, cost, dcost[0..7], jtj upper triangle row-major]   (47)
``sums_of_planes`` also returns the sum of the magnitudes of every sum's terms: what errors are measured against.

``seed`` plants one error of the kinds an implementation of the weighted sums can make (SEEDS); tests/test_align_w_reference.py asserts that
the gate of tests/align_w_cases.py rejects every one of them.
"""
import numpy as np

import align_reference as ar

SUMS = 47
PACK = [(a, b) for a in range(8) for b in range(a, 8)]  # the upper triangle, row-major
SHARED = [0, 2] + list(range(3, 9)) + [11 + q for q, (a, b) in enumerate(PACK) if b < 6]  # section 5.10's 29 entries inside the 47, in its order
SEEDS = ("w_applied_twice", "w_missing_from_jtj", "g_missing_from_J", "J6_is_gR", "b_dropped", "nonpositive_weight_counted", "packing_transposed",
         "wsum_is_count")


def sums_of_planes(R, gY, gX, target, weight, gb, shape, seed=None):
    """planes, target and weight (th tw) or (th, tw), gb = (g, b) -> (sums (47), magnitudes (47)) in fp64 from whatever precision they have"""
    th, tw = shape
    R, gY, gX, T, w = (np.asarray(x).reshape(th * tw).astype(np.float64) for x in (R, gY, gX, target, weight))
    g, b = float(gb[0]), float(gb[1])
    i = np.repeat(np.arange(th), tw).astype(np.float64)
    j = np.tile(np.arange(tw), th).astype(np.float64)
    ok = np.isfinite(T) & np.isfinite(R) & np.isfinite(gY) & np.isfinite(gX)
    with np.errstate(invalid="ignore"):
        ok = ok & np.isfinite(w) & ((w >= 0) if seed == "nonpositive_weight_counted" else (w > 0))
    R, gY, gX, T, w, i, j = (x[ok] for x in (R, gY, gX, T, w, i, j))
    r = (g * R + (0.0 if seed == "b_dropped" else b)) - T
    gj = 1.0 if seed == "g_missing_from_J" else g
    gy, gx = gj * gY, gj * gX
    J = [gy * i, gy * j, gy, gx * i, gx * j, gx, (g * R if seed == "J6_is_gR" else R), np.ones_like(R)]
    wr = w * r
    if seed == "w_applied_twice":
        wr = w * wr
    wj = np.ones_like(w) if seed == "w_missing_from_jtj" else w
    pack = sorted(PACK, key=lambda ab: (ab[1], ab[0])) if seed == "packing_transposed" else PACK
    terms = [np.ones_like(r), (np.ones_like(w) if seed == "wsum_is_count" else w), wr * r] + [(2.0 * wr) * J[a] for a in range(8)] + [(wj * J[a]) * J[c] for a, c in pack]
    sums = np.array([t.sum() for t in terms], np.float64)
    mags = np.array([np.abs(t).sum() for t in terms], np.float64)
    return sums, mags


def align(planes, targets, weights, intensity, seed=None):
    """planes (3, n, th, tw) as align_reference.align returns them -> (sums (n, 47), magnitudes (n, 47))"""
    targets = np.asarray(targets, dtype=np.float32)
    n, th, tw = targets.shape
    weights = np.ones((n, th, tw), np.float32) if weights is None else np.asarray(weights, np.float32)
    intensity = np.tile(np.array([1.0, 0.0], np.float32), (n, 1)) if intensity is None else np.asarray(intensity, np.float32)
    sums, mags = np.zeros((n, SUMS)), np.zeros((n, SUMS))
    for s in range(n):
        sums[s], mags[s] = sums_of_planes(planes[0, s], planes[1, s], planes[2, s], targets[s], weights[s], intensity[s], (th, tw), seed)
    return sums, mags


def align_of_stack(sd, mods, black, maps, targets, weights, intensity, nV, nH, S, I, **kw):
    """align_reference.align_of_stack's arguments with weights (n, th, tw) and intensity (n, 2) (either may be None)
    -> (sums (n, 47), magnitudes (n, 47), planes (3, n, th, tw))"""
    planes = ar.align_of_stack(sd, mods, black, maps, targets, nV, nH, S, I, **kw)[2]
    return align(planes, targets, weights, intensity) + (planes,)
