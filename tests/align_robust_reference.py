"""Reference for robust alignment of target slices to a stack read as a volume (msiren_align_volume_r*): numpy, fp64, on the
planes of tests/align_volume_w_reference.py, with a Geman-McClure loss of one scale s per target in place of the square.  Not a test module:
tests/test_align_robust_reference.py checks it on the CPU, tests/test_gpu_align_robust.py gates the kernel against it.

    R, gZ, gY, gX, w, (g, b), r and J[11]: align_volume_w_reference's;  s = scale of the target, in squared intensity units
    valid iff align_volume_w_reference's condition holds and s > 0 (a NaN, zero or negative s: count 0; s = +inf is allowed)
    u = r r / s,  v = 1 + u,  om = 1 / v,  wl = w om,  wq = wl om
    count = sum 1, wsum = sum w, cost = sum (wl r) r, dcost[a] = sum (2 (wq r)) J[a], jtj[a, b] = sum (wq J[a]) J[b]
    sums = [count, wsum, cost, dcost[0..10], jtj upper triangle row-major]   (80)
cost is sum w rho(r) with rho(r) = r^2 / (1 + r^2 / s), dcost its exact gradient (rho' = 2 r / (1 + r^2 / s)^2), jtj the Gauss-Newton matrix of the
quadratic majoriser, wsum the plain sum of the weights.  With s = +inf the terms, and numpy's sums of them, are align_volume_w_reference's.
``sums_of_planes`` also returns the sum of the magnitudes of every sum's terms and the per-pixel factor om^2 (NaN at an invalid pixel).

``seed`` plants one error of the kinds an implementation of the robust terms can make (SEEDS); tests/test_align_robust_reference.py asserts that
the gate of tests/align_robust_cases.py rejects every one of them.
"""
import numpy as np

import align_volume_w_reference as avwr

SUMS, PACK = avwr.SUMS, avwr.PACK
SEEDS = ("om_once_in_jtj", "om_twice_in_cost", "wsum_takes_wq", "u_is_r_over_s", "nonpositive_scale_counted", "dcost_with_wl")


def sums_of_planes(R, gZ, gY, gX, target, weight, gb, s, shape, seed=None):
    """planes, target and weight (th tw) or (th, tw), gb = (g, b), s the scale -> (sums (80), magnitudes (80), om^2 (th tw), NaN where invalid)"""
    th, tw = shape
    R, gZ, gY, gX, T, w = (np.asarray(x).reshape(th * tw).astype(np.float64) for x in (R, gZ, gY, gX, target, weight))
    g, b, s = float(gb[0]), float(gb[1]), float(s)
    i = np.repeat(np.arange(th), tw).astype(np.float64)
    j = np.tile(np.arange(tw), th).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(T) & np.isfinite(R) & np.isfinite(gZ) & np.isfinite(gY) & np.isfinite(gX) & np.isfinite(w) & (w > 0)
    if not (s > 0) and seed != "nonpositive_scale_counted":
        ok = np.zeros_like(ok)
    rw = np.full(th * tw, np.nan)
    R, gZ, gY, gX, T, w, i, j = (x[ok] for x in (R, gZ, gY, gX, T, w, i, j))
    r = (g * R + b) - T
    gz, gy, gx = g * gZ, g * gY, g * gX
    J = [gz * i, gz * j, gz, gy * i, gy * j, gy, gx * i, gx * j, gx, R, np.ones_like(R)]
    with np.errstate(invalid="ignore", divide="ignore"):  # (only the mutant that counts a scale that is not > 0 divides by it)
        u = (r / s) if seed == "u_is_r_over_s" else (r * r) / s
        om = 1.0 / (1.0 + u)
    wl = w * om
    wq = wl * om
    rw[ok] = om * om
    wc_ = wq if seed == "om_twice_in_cost" else wl
    wd_ = wl if seed == "dcost_with_wl" else wq
    wj = wl if seed == "om_once_in_jtj" else wq
    ws = wq if seed == "wsum_takes_wq" else w
    with np.errstate(invalid="ignore"):
        terms = [np.ones_like(r), ws, (wc_ * r) * r] + [(2.0 * (wd_ * r)) * J[a] for a in range(11)] + [(wj * J[a]) * J[c] for a, c in PACK]
        sums = np.array([t.sum() for t in terms], np.float64)
        mags = np.array([np.abs(t).sum() for t in terms], np.float64)
    return sums, mags, rw


def align(planes, targets, weights, intensity, scale, seed=None, rweight=False):
    """planes (4, m, th, tw) = R, gZ, gY, gX as align_volume_reference.align_volume returns them, scale (m,) or a scalar ->
    (sums (m, 80), magnitudes (m, 80)), and om^2 (m, th, tw) behind them with ``rweight``"""
    targets = np.asarray(targets, dtype=np.float32)
    m, th, tw = targets.shape
    weights = np.ones((m, th, tw), np.float32) if weights is None else np.asarray(weights, np.float32)
    intensity = np.tile(np.array([1.0, 0.0], np.float32), (m, 1)) if intensity is None else np.asarray(intensity, np.float32)
    scale = np.broadcast_to(np.asarray(scale, np.float64), (m,))
    sums, mags, rw = np.zeros((m, SUMS)), np.zeros((m, SUMS)), np.zeros((m, th, tw))
    for q in range(m):
        sums[q], mags[q], x = sums_of_planes(planes[0, q], planes[1, q], planes[2, q], planes[3, q], targets[q], weights[q], intensity[q], scale[q], (th, tw), seed)
        rw[q] = x.reshape(th, tw)
    return (sums, mags, rw) if rweight else (sums, mags)
