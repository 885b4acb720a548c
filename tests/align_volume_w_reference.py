"""Reference for weighted, gain/bias-compensated alignment of target slices to a stack read as a volume (DESIGN.md section 5.14,
msiren_align_volume_w*): numpy, fp64, on the planes of tests/align_volume_reference.py (volume_reference.volume at the map's points), as
tests/align_w_reference.py is for section 5.12.  Not a test module: tests/test_align_volume_w_reference.py checks it on the CPU,
tests/test_gpu_align_volume_w.py gates the kernels against it.

    R, gZ, gY, gX: align_volume_reference's planes of the target under its map;  weight w per pixel, intensity (g, b) per target
    valid iff target, R, gZ, gY, gX are all finite and w is finite and > 0
    mm = g R + b,  r = mm - T,  gz = g gZ, gy = g gY, gx = g gX,  J = (gz i, gz j, gz, gy i, gy j, gy, gx i, gx j, gx, R, 1),  wr = w r
    count = sum 1, wsum = sum w, cost = sum wr r, dcost[a] = sum (2 wr) J[a], jtj[a, b] = sum (w J[a]) J[b]
    sums = [count, wsum, cost, dcost[0..10], jtj upper triangle row-major]   (80)
``sums_of_planes`` also returns the sum of the magnitudes of every sum's terms: what errors are measured against.

``seed`` plants one error of the kinds an implementation of the weighted sums can make (SEEDS); tests/test_align_volume_w_reference.py asserts
that the gate of tests/align_volume_w_cases.py rejects every one of them.
"""
import numpy as np

import align_volume_reference as avr

SUMS = 80
CHUNK = avr.CHUNK
PACK = [(a, b) for a in range(11) for b in range(a, 11)]  # the upper triangle, row-major
SHARED = [0, 2] + list(range(3, 12)) + [14 + q for q, (a, b) in enumerate(PACK) if b < 9]  # section 5.13's 56 entries inside the 80, in its order
SEEDS = ("gain_dropped_from_gz", "w_applied_twice", "wsum_counts_masked", "packing_transposed", "chunk_dropped", "b_added_before_gain", "w_missing_from_jtj",
         "J9_is_gR", "nonpositive_weight_counted")


def sums_of_planes(R, gZ, gY, gX, target, weight, gb, shape, seed=None):
    """planes, target and weight (th tw) or (th, tw), gb = (g, b) -> (sums (80), magnitudes (80)) in fp64 from whatever precision they have"""
    th, tw = shape
    R, gZ, gY, gX, T, w = (np.asarray(x).reshape(th * tw).astype(np.float64) for x in (R, gZ, gY, gX, target, weight))
    g, b = float(gb[0]), float(gb[1])
    i = np.repeat(np.arange(th), tw).astype(np.float64)
    j = np.tile(np.arange(tw), th).astype(np.float64)
    finite = np.isfinite(T) & np.isfinite(R) & np.isfinite(gZ) & np.isfinite(gY) & np.isfinite(gX)
    with np.errstate(invalid="ignore"):
        ok = finite & np.isfinite(w) & ((w >= 0) if seed == "nonpositive_weight_counted" else (w > 0))
    if seed == "chunk_dropped":  # the last chunk of 1024 pixels never added
        ok = ok & (np.arange(th * tw) < (th * tw - 1) // CHUNK * CHUNK)
    with np.errstate(invalid="ignore"):  # "wsum_counts_masked": wsum also takes the weight of a pixel that the planes or the target mask
        masked_w = float(w[~finite & np.isfinite(w) & (w > 0)].sum()) if seed == "wsum_counts_masked" else 0.0
    R, gZ, gY, gX, T, w, i, j = (x[ok] for x in (R, gZ, gY, gX, T, w, i, j))
    r = (g * (R + b) if seed == "b_added_before_gain" else g * R + b) - T
    gz = (1.0 if seed == "gain_dropped_from_gz" else g) * gZ
    gy, gx = g * gY, g * gX
    J = [gz * i, gz * j, gz, gy * i, gy * j, gy, gx * i, gx * j, gx, (g * R if seed == "J9_is_gR" else R), np.ones_like(R)]
    wr = w * r
    if seed == "w_applied_twice":
        wr = w * wr
    wj = np.ones_like(w) if seed == "w_missing_from_jtj" else w
    pack = sorted(PACK, key=lambda ab: (ab[1], ab[0])) if seed == "packing_transposed" else PACK
    terms = [np.ones_like(r), w, wr * r] + [(2.0 * wr) * J[a] for a in range(11)] + [(wj * J[a]) * J[c] for a, c in pack]
    sums = np.array([t.sum() for t in terms], np.float64)
    mags = np.array([np.abs(t).sum() for t in terms], np.float64)
    sums[1] += masked_w
    mags[1] += masked_w
    return sums, mags


def align(planes, targets, weights, intensity, seed=None):
    """planes (4, m, th, tw) = R, gZ, gY, gX as align_volume_reference.align_volume returns them -> (sums (m, 80), magnitudes (m, 80))"""
    targets = np.asarray(targets, dtype=np.float32)
    m, th, tw = targets.shape
    weights = np.ones((m, th, tw), np.float32) if weights is None else np.asarray(weights, np.float32)
    intensity = np.tile(np.array([1.0, 0.0], np.float32), (m, 1)) if intensity is None else np.asarray(intensity, np.float32)
    sums, mags = np.zeros((m, SUMS)), np.zeros((m, SUMS))
    for q in range(m):
        sums[q], mags[q] = sums_of_planes(planes[0, q], planes[1, q], planes[2, q], planes[3, q], targets[q], weights[q], intensity[q], (th, tw), seed)
    return sums, mags
