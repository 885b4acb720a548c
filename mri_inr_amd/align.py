"""Helpers for ``ModulatedSiren.align_cost``: the affine maps slices are read under, the call's packed sums, and a
Gauss-Newton step on them.  Pure numpy.

A map is six float32 numbers (a00, a01, t0, a10, a11, t1): pixel (i, j) of the target lattice is read at
    Y = ((a00 i) + (a01 j)) + t0        X = ((a10 i) + (a11 j)) + t1
in reconstruction pixel coordinates, in fp32 with every operation rounded on its own -- what the kernels compute, bit for bit."""
import collections

import numpy as np

SUMS = 29  # count, cost, dcost[6], jtj packed upper triangle row-major [21]
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
_IU = np.triu_indices(6)

AlignResult = collections.namedtuple("AlignResult", "count cost grad jtj warped wgrad")
AlignResult.__doc__ = """count (n,) int64 valid pixels, cost (n,) the sum of squared differences over them, grad (n, 6) its gradient over
(a00, a01, t0, a10, a11, t1), jtj (n, 6, 6) the Gauss-Newton matrix (symmetric); warped (n, th, tw) / wgrad (2, n, th, tw) or None."""


def map_points(maps_row, shape):
    """One map (6,) on the lattice ``shape = (th, tw)`` -> (th * tw, 2) float32 points (Y, X), row i * tw + j: the fp32 rule above."""
    a = np.asarray(maps_row, dtype=np.float32)
    if a.shape != (6,):
        raise ValueError(f"expected one map of 6 numbers, got {a.shape}")
    th, tw = (int(x) for x in shape)
    if th < 0 or tw < 0:
        raise ValueError(f"shape must be non-negative, got {shape}")
    i = np.arange(th, dtype=np.float32)[:, None]
    j = np.arange(tw, dtype=np.float32)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        Y = ((a[0] * i) + (a[1] * j)) + a[2]
        X = ((a[3] * i) + (a[4] * j)) + a[5]
    assert Y.dtype == np.float32 and X.dtype == np.float32
    return np.stack([Y, X], axis=-1).reshape(th * tw, 2)


def rigid_maps(angle, shift, centre):
    """Rotations by ``angle`` (n,) radians about ``centre`` (2,) = (Y, X) followed by ``shift`` (n, 2) -> maps (n, 6) float32:
    p' = R (p - centre) + centre + shift, R = [[cos, -sin], [sin, cos]] on (row, column).  Formed in fp64 and rounded once."""
    angle = np.atleast_1d(np.asarray(angle, dtype=np.float64))
    shift = np.broadcast_to(np.asarray(shift, dtype=np.float64), (len(angle), 2))
    cy, cx = np.asarray(centre, dtype=np.float64)
    c, s = np.cos(angle), np.sin(angle)
    maps = np.empty((len(angle), 6), np.float64)
    maps[:, 0], maps[:, 1], maps[:, 2] = c, -s, cy - (c * cy - s * cx) + shift[:, 0]
    maps[:, 3], maps[:, 4], maps[:, 5] = s, c, cx - (s * cy + c * cx) + shift[:, 1]
    return maps.astype(np.float32)


def unpack(sums, warped=None, wgrad=None):
    """sums (n, 29) float64 as msiren_align_slices writes them -> AlignResult (jtj unpacked to symmetric (n, 6, 6))"""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] != SUMS:
        raise ValueError(f"expected sums of shape (n, {SUMS}), got {sums.shape}")
    n = len(sums)
    jtj = np.zeros((n, 6, 6), np.float64)
    jtj[:, _IU[0], _IU[1]] = sums[:, 8:]
    jtj[:, _IU[1], _IU[0]] = sums[:, 8:]
    return AlignResult(sums[:, 0].astype(np.int64), sums[:, 1].copy(), sums[:, 2:8].copy(), jtj, warped, wgrad)


def gauss_newton_step(result, damping=0.0):
    """(n, 6) float64: per slice the solution of (JtJ + damping diag(JtJ)) delta = -grad / 2 (grad = 2 J^T r).  A slice with fewer than six
    valid pixels, or a singular system, gives a zero step."""
    n = len(result.count)
    step = np.zeros((n, 6), np.float64)
    for s in range(n):
        if result.count[s] < 6:
            continue
        A = result.jtj[s] + float(damping) * np.diag(np.diag(result.jtj[s]))
        try:
            step[s] = np.linalg.solve(A, -0.5 * result.grad[s])
        except np.linalg.LinAlgError:
            pass
    return step
