"""Helpers for ``ModulatedSiren.fuse_targets`` (msiren_fuse_targets): the aligned targets of the volume alignment calls put
back onto the stack's voxel grid, and the rule's normative restatement ``fuse_on_host``.

Everything here is numpy fp64, ELEMENTWISE, in the associations of include/msiren.h -- no ``@``, ``dot``, ``cross`` or ``sum``, whose order of
operations is numpy's business -- so the device equals ``fuse_on_host`` bit for bit.  The rule is cut into the small functions below (the window,
the in-plane coordinates, the base index, a tap's validity, weight and value) so that a test can replace one of them by a wrong one and see its
checks fail."""
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
    v0 = (np.arange(n, dtype=np.float64) * spacing).reshape(n, 1, 1)
    vy = np.arange(H, dtype=np.float64).reshape(1, H, 1)
    vx = np.arange(W, dtype=np.float64).reshape(1, 1, W)
    num, den = np.zeros((n, H, W), np.float64), np.zeros((n, H, W), np.float64)
    th1, tw1 = np.float64(th - 1), np.float64(tw - 1)
    with np.errstate(all="ignore"):
        for q in range(m):
            if r.flags[q]:
                continue
            a, b, c = [x[q] for x in r.a], [x[q] for x in r.b], [x[q] for x in r.c]
            p0, p1, p2 = v0 - r.t[0][q], vy - r.t[1][q], vx - r.t[2][q]
            pa = ((a[0] * p0) + (a[1] * p1)) + (a[2] * p2)
            pb = ((b[0] * p0) + (b[1] * p1)) + (b[2] * p2)
            cp = ((c[0] * p0) + (c[1] * p1)) + (c[2] * p2)
            i, j = in_plane(pa, pb, r.G11[q], r.G12[q], r.G22[q], r.det[q])
            k = window(cp, r.dt[q])
            at = np.nonzero((k > 0) & (i >= 0) & (i <= th1) & (j >= 0) & (j <= tw1))  # a NaN fails every comparison
            if not len(at[0]):
                continue
            i, j, k = i[at], j[at], k[at]
            fi0, fj0 = base_index(i, th), base_index(j, tw)
            fi, fj = i - fi0, j - fj0
            gi, gj = 1.0 - fi, 1.0 - fj
            i0, j0 = fi0.astype(np.int64), fj0.astype(np.int64)
            sn, sd = np.zeros(len(k), np.float64), np.zeros(len(k), np.float64)
            for di, dj, beta in ((0, 0, gi * gj), (0, 1, gi * fj), (1, 0, fi * gj), (1, 1, fi * fj)):
                T, w = tg[q][i0 + di, j0 + dj], wt[q][i0 + di, j0 + dj]
                ok = tap_valid(T, w)
                bw = tap_weight(beta, w.astype(np.float64))
                sn = sn + np.where(ok, bw * tap_value(T.astype(np.float64), r.bias[q], r.g[q]), 0.0)
                sd = sd + np.where(ok, bw, 0.0)
            num[at] = num[at] + (k * sn)
            den[at] = den[at] + (k * sd)
        volume = np.where(den > np.float64(min_coverage), (num / den).astype(np.float32), np.float32(np.nan)).astype(np.float32)
    return FuseResult(volume, den.astype(np.float32), r.flags)
