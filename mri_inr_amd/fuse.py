"""Helpers for ``ModulatedSiren.fuse_targets`` (msiren_fuse_targets): the aligned targets of the volume alignment calls put
back onto the stack's voxel grid, and the rule's normative restatement ``fuse_on_host``.

Everything here is numpy fp64, ELEMENTWISE, in the associations of include/msiren.h -- no ``@``, ``dot``, ``cross`` or ``sum``, whose order of
operations is numpy's business -- so the device equals ``fuse_on_host`` bit for bit.  The rule is cut into the small functions below (the window,
the in-plane coordinates, the base index, a tap's validity, weight and value) so that a test can replace one of them by a wrong one and see its
checks fail; ``voxel_taps`` is the one statement of which voxels reach which taps of a target, for the fusion, the projection and the solve.  Below them the way back, ``ModulatedSiren.project_volume`` (section 5.18; msiren_project_volume): ``project_on_host`` and
``project_stats_on_host``, cut up in the same way."""
import collections

import numpy as np

DEGENERATE, BAD_INTENSITY = 1, 2

FuseResult = collections.namedtuple("FuseResult", "volume coverage flags")
FuseResult.__doc__ = """volume (n, H, W) float32, NaN where the coverage is not above ``min_coverage``; coverage (n, H, W) float32, the sum of window x
bilinear weight x pixel weight over the taps that reached the voxel, or None; flags (m,) int32 per target: DEGENERATE (1) a map entry not finite or the
plane's Gram determinant not > 0 or not finite, BAD_INTENSITY (2) g or b not finite or g == 0 -- a flagged target contributes nothing."""

TargetRecords = collections.namedtuple("TargetRecords", "a b t G11 G12 G22 det dt c g bias flags")
TargetRecords.__doc__ = """What fuse_setup_kernel leaves per target: a, b, t, c as tuples of three (m,) float64 arrays, the rest (m,) float64, flags (m,) int32"""


def z_row(x, spacing):
    """a Z entry of a map, in slice units -> pixels"""
    return x * spacing


def target_records(maps, intensity, spacing, thickness):
    """maps (m, 9) float32, intensity (m, 2) float32 or None -> TargetRecords: the per-target part of the rule"""
    mp = np.ascontiguousarray(maps, dtype=np.float32).reshape(-1, 9)
    m = len(mp)
    gb = np.tile(np.array([1.0, 0.0], np.float32), (m, 1)) if intensity is None else np.ascontiguousarray(intensity, dtype=np.float32).reshape(m, 2)
    d = mp.astype(np.float64)
    spacing, thickness = np.float64(spacing), np.float64(thickness)
    with np.errstate(all="ignore"):
        a = (z_row(d[:, 0], spacing), d[:, 3], d[:, 6])
        b = (z_row(d[:, 1], spacing), d[:, 4], d[:, 7])
        t = (z_row(d[:, 2], spacing), d[:, 5], d[:, 8])
        G11 = ((a[0] * a[0]) + (a[1] * a[1])) + (a[2] * a[2])
        G12 = ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])
        G22 = ((b[0] * b[0]) + (b[1] * b[1])) + (b[2] * b[2])
        det = (G11 * G22) - (G12 * G12)
        tt = thickness * thickness
        dt = det * tt
        c = ((a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0]))
        degenerate = ~np.isfinite(mp).all(axis=1) | ~(det > 0) | ~np.isfinite(det)
        bad = ~np.isfinite(gb[:, 0]) | ~np.isfinite(gb[:, 1]) | (gb[:, 0] == 0)
    flags = (np.where(degenerate, DEGENERATE, 0) | np.where(bad, BAD_INTENSITY, 0)).astype(np.int32)
    return TargetRecords(a, b, t, G11, G12, G22, det, dt, c, gb[:, 0].astype(np.float64), gb[:, 1].astype(np.float64), flags)


def window(cp, dt):
    """k: the quadratic (Welch) window in the distance to the plane, cp = c . p, dt = det thickness^2"""
    return 1.0 - ((cp * cp) / dt)


def in_plane(pa, pb, G11, G12, G22, det):
    """(i, j): the target's row and column of the voxel's foot point"""
    return ((G22 * pa) - (G12 * pb)) / det, ((G11 * pb) - (G12 * pa)) / det


def base_index(i, size):
    """the first of the two taps along an axis of ``size`` pixels: floor, clamped so that i = size - 1 reads the last pair"""
    return np.minimum(np.floor(i), np.float64(size - 2))


def tap_valid(T, w):
    """float32 pixel and weight -> the tap counts"""
    return np.isfinite(T) & np.isfinite(w) & (w > 0)


def tap_weight(beta, w):
    return beta * w


def tap_value(T, bias, g):
    """the pixel back in the stack's intensity: T ~ g R + b"""
    return (T - bias) / g


def fuse_on_host(targets, maps, shape, spacing, *, thickness=None, weights=None, intensity=None, min_coverage=0.0):
    """The normative restatement of msiren_fuse_targets -> FuseResult (coverage always).  targets (m, th, tw), maps (m, 9), shape = (n, H, W);
    ``thickness`` None: ``spacing``; weights (m, th, tw) or None (all 1); intensity (m, 2) or None ((1, 0))."""
    tg = np.ascontiguousarray(targets, dtype=np.float32)
    m, th, tw = tg.shape
    n, H, W = (int(s) for s in shape)
    wt = np.ones(tg.shape, np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    spacing = np.float64(spacing)
    r = target_records(maps, intensity, spacing, spacing if thickness is None else thickness)
    num, den = np.zeros((n, H, W), np.float64), np.zeros((n, H, W), np.float64)
    everywhere = np.ones((n, H, W), bool)
    with np.errstate(all="ignore"):
        for q in range(m):
            taps = None if r.flags[q] else voxel_taps(r, q, everywhere, (n, H, W), (th, tw), spacing)
            if taps is None:
                continue
            at, k, pixel, beta = taps
            Tq, wq = tg[q].ravel(), wt[q].ravel()
            sn, sd = np.zeros(len(k), np.float64), np.zeros(len(k), np.float64)
            for tap in range(4):
                T, w = Tq[pixel[:, tap]], wq[pixel[:, tap]]
                ok = tap_valid(T, w)
                bw = tap_weight(beta[:, tap], w.astype(np.float64))
                sn = sn + np.where(ok, bw * tap_value(T.astype(np.float64), r.bias[q], r.g[q]), 0.0)
                sd = sd + np.where(ok, bw, 0.0)
            num[at] = num[at] + (k * sn)
            den[at] = den[at] + (k * sd)
        volume = np.where(den > np.float64(min_coverage), (num / den).astype(np.float32), np.float32(np.nan)).astype(np.float32)
    return FuseResult(volume, den.astype(np.float32), r.flags)


# ---- the way back: msiren_project_volume --------------------------------------------------------------------------------------
ProjectResult = collections.namedtuple("ProjectResult", "simulated coverage residual stats flags")
ProjectResult.__doc__ = """simulated (m, th, tw) float32: what each target should look like given the stack, NaN where the coverage is not above
``min_coverage`` and everywhere on a flagged target; coverage (m, th, tw) float32, the sum of window x bilinear weight over the valid voxels that have
the pixel among their taps, or None; residual (m, th, tw) float32 = targets - simulated, NaN where either is not finite, or None; stats (m, 4) float64 =
(count, sum w, sum w r, sum (w r) r) over the pixels whose residual is finite and whose weight is finite and > 0, or None; flags (m,) int32 as in
FuseResult."""


def voxel_valid(V):
    """float32 voxel -> it takes part"""
    return np.isfinite(V)


def tap_terms(k, beta, V):
    """one (voxel, tap) pair -> what it adds to (num, den) of the tap's pixel"""
    kb = k * beta
    return kb * V, kb


def scatter(acc, pixel, terms):
    """acc (th tw,) += terms at the flat pixel indices; both (voxels, 4), the voxels in ascending flat index.  Raveled voxel-major, ``np.add.at`` adds
    one term after the other in that order: per pixel the rule's order (the four taps of a voxel are distinct pixels)"""
    np.add.at(acc, pixel.ravel(), terms.ravel())


def apply_intensity(ratio, g, bias):
    """the stack's intensity as the target sees it: T ~ g R + b"""
    return (g * ratio) + bias


def voxel_taps(r, q, valid, grid, shape, spacing):
    """The (voxel, tap) pairs of target q of the records ``r`` -> (at, k, pixel, beta) or None: ``at`` the index arrays of the valid voxels (``valid``
    (n, H, W) bool) that contribute, in ascending flat index; k (voxels,); pixel (voxels, 4) the flat index i th-major of the four taps in the order
    (0,0), (0,1), (1,0), (1,1); beta (voxels, 4) their bilinear weights -- msiren_fuse_targets' expressions"""
    n, H, W = grid
    th, tw = shape
    v0 = (np.arange(n, dtype=np.float64) * spacing).reshape(n, 1, 1)
    vy = np.arange(H, dtype=np.float64).reshape(1, H, 1)
    vx = np.arange(W, dtype=np.float64).reshape(1, 1, W)
    th1, tw1 = np.float64(th - 1), np.float64(tw - 1)
    with np.errstate(all="ignore"):
        a, b, c = [x[q] for x in r.a], [x[q] for x in r.b], [x[q] for x in r.c]
        p0, p1, p2 = v0 - r.t[0][q], vy - r.t[1][q], vx - r.t[2][q]
        pa = ((a[0] * p0) + (a[1] * p1)) + (a[2] * p2)
        pb = ((b[0] * p0) + (b[1] * p1)) + (b[2] * p2)
        cp = ((c[0] * p0) + (c[1] * p1)) + (c[2] * p2)
        i, j = in_plane(pa, pb, r.G11[q], r.G12[q], r.G22[q], r.det[q])
        k = window(cp, r.dt[q])
        at = np.nonzero(valid & (k > 0) & (i >= 0) & (i <= th1) & (j >= 0) & (j <= tw1))  # C order: ascending flat voxel index; a NaN fails every comparison
        if not len(at[0]):
            return None
        i, j, k = i[at], j[at], k[at]
        fi0, fj0 = base_index(i, th), base_index(j, tw)
        fi, fj = i - fi0, j - fj0
        gi, gj = 1.0 - fi, 1.0 - fj
        i0, j0 = fi0.astype(np.int64), fj0.astype(np.int64)
        pixel = np.stack([(i0 + di) * tw + (j0 + dj) for di, dj in ((0, 0), (0, 1), (1, 0), (1, 1))], axis=1)
        beta = np.stack([gi * gj, gi * fj, fi * gj, fi * fj], axis=1)
    return at, k, pixel, beta


def project_sums_on_host(volume, maps, shape, spacing, *, thickness=None, intensity=None):
    """-> (num, den (m, th tw) float64, TargetRecords): the two sums of the rule per target pixel, in the rule's order (a flagged target: zeros)"""
    vol = np.ascontiguousarray(volume, dtype=np.float32)
    th, tw = (int(s) for s in shape)
    spacing = np.float64(spacing)
    r = target_records(maps, intensity, spacing, spacing if thickness is None else thickness)
    m = len(r.flags)
    valid = voxel_valid(vol)
    vd = vol.astype(np.float64)
    num, den = np.zeros((m, th * tw), np.float64), np.zeros((m, th * tw), np.float64)
    with np.errstate(all="ignore"):
        for q in range(m):
            taps = None if r.flags[q] else voxel_taps(r, q, valid, vol.shape, (th, tw), spacing)
            if taps is not None:
                at, k, pixel, beta = taps
                tn, td = tap_terms(k[:, None], beta, vd[at][:, None])
                scatter(num[q], pixel, tn)
                scatter(den[q], pixel, td)
    return num, den, r


def project_on_host(volume, maps, shape, spacing, *, thickness=None, intensity=None, min_coverage=0.0):
    """The normative restatement of msiren_project_volume's gather -> ProjectResult (coverage always; residual and stats None: project_stats_on_host).
    volume (n, H, W), maps (m, 9), shape = (th, tw) the targets' lattice; ``thickness`` None: ``spacing``; intensity (m, 2) or None ((1, 0))."""
    th, tw = (int(s) for s in shape)
    num, den, r = project_sums_on_host(volume, maps, shape, spacing, thickness=thickness, intensity=intensity)
    m = len(r.flags)
    simulated = np.full((m, th, tw), np.nan, np.float32)
    with np.errstate(all="ignore"):
        for q in range(m):
            if not r.flags[q]:
                value = apply_intensity(num[q] / den[q], r.g[q], r.bias[q]).astype(np.float32)
                simulated[q] = np.where(den[q] > np.float64(min_coverage), value, np.float32(np.nan)).reshape(th, tw)
    return ProjectResult(simulated, den.astype(np.float32).reshape(m, th, tw), None, None, r.flags)


def residual_on_host(targets, simulated):
    """float32 (m, th, tw) x 2 -> residual float32: (float)((double)T - (double)simulated), NaN where either is not finite"""
    T, S = np.ascontiguousarray(targets, dtype=np.float32), np.ascontiguousarray(simulated, dtype=np.float32)
    with np.errstate(all="ignore"):
        r = (T.astype(np.float64) - S.astype(np.float64)).astype(np.float32)
    return np.where(np.isfinite(T) & np.isfinite(S), r, np.float32(np.nan)).astype(np.float32)


def ordered_sum(terms):
    """terms (th, tw) float64 -> their sum in the rule's order: per column down the rows from 0.0, then the column sums for j ascending from 0.0"""
    col = np.zeros(terms.shape[1], np.float64)
    for row in terms:
        col = col + row
    s = np.float64(0.0)
    for x in col:
        s = s + x
    return s


def project_stats_on_host(targets, simulated, weights=None):
    """The normative restatement of msiren_project_volume's residual and sums -> (residual (m, th, tw) float32, stats (m, 4) float64)"""
    res = residual_on_host(targets, simulated)
    w = np.ones(res.shape, np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    counts = np.isfinite(res) & np.isfinite(w) & (w > 0)
    stats = np.zeros((len(res), 4), np.float64)
    with np.errstate(all="ignore"):
        rd, wd = res.astype(np.float64), w.astype(np.float64)
        wr = wd * rd
        for q in range(len(res)):
            for e, terms in enumerate((np.ones(rd[q].shape), wd[q], wr[q], wr[q] * rd[q])):
                stats[q, e] = ordered_sum(np.where(counts[q], terms, 0.0))
    return res, stats
