"""Reference for a stack of slices read as a volume (msiren_resample_volume*): numpy, fp64, on top of
tests/resample_reference.resample one slice at a time.  Not a test module: tests/test_volume_reference.py checks it on the CPU,
tests/test_gpu_volume.py gates the kernels against it.

    points (M, 3) = (Z, Y, X);  valid iff 0 <= Z <= n - 1 (the fp32 Z against the integers)
    z0 = min(floor(Z), n - 2),  f = Z - z0 in [0, 1]  (exact in fp32);   R0, R1, G0, G1: resample_reference of slices z0, z0 + 1 at (Y, X)
    value = R0 if f == 0, R1 if f == 1, else (1 - f) R0 + f R1          grad[0] = R1 - R0        grad[1:] = the same selection over G0, G1
An invalid Z gives NaN in every plane; a point without a covering tile is NaN through R0 and R1.  n = 1: the value alone (grad None).
"""
import numpy as np

import resample_reference as rr


def pairs(points, n):
    """per point: first slice of its pair (-1: invalid Z) and the second slice's weight f, as the gradient forms define them (n >= 2);
    n = 1: the slice itself, f = 0"""
    Z = np.asarray(points, dtype=np.float32)[:, 0]
    with np.errstate(invalid="ignore"):
        valid = (np.float32(0) <= Z) & (Z <= np.float32(n - 1))
    z0 = np.full(len(Z), -1, np.int64)
    z0[valid] = np.minimum(np.floor(Z[valid]).astype(np.int64), max(n - 2, 0))
    f = np.zeros(len(Z), np.float64)
    f[valid] = Z[valid].astype(np.float64) - z0[valid]
    assert np.all(f.astype(np.float32) == f) and np.all((0 <= f) & (f <= 1))  # the fp32 subtraction is exact
    return z0, f


def slices_read(points, n, value_form=False):
    """per point the slices it evaluates: both of the pair, or (value_form) only those of non-zero weight"""
    z0, f = pairs(points, n)
    out = []
    for z, w in zip(z0, f):
        if z < 0:
            out.append([])
        elif n == 1:
            out.append([0])
        elif value_form:
            out.append([z] if w == 0 else [z + 1] if w == 1 else [z, z + 1])
        else:
            out.append([z, z + 1])
    return out


def select(f, a0, a1, dtype):
    """a0 where f == 0, a1 where f == 1, the linear blend between"""
    f = f.astype(dtype)
    with np.errstate(invalid="ignore"):
        mix = (1 - f) * a0 + f * a1
    return np.where(f == 0, a0, np.where(f == 1, a1, mix))


def volume(slice_fn, points, n, dtype=np.float64):
    """``slice_fn(s, yx)`` -> (value (m), grad (2, m)) of slice s at the points yx (m, 2), as resample_reference.resample returns them
    -> (value (M), grad (3, M)) of ``dtype``; grad is None for n = 1."""
    points = np.asarray(points, dtype=np.float32)
    M = len(points)
    z0, f = pairs(points, n)
    R = np.full((2, 3, M), np.nan, dtype)  # [slice of the pair][value, d/d row, d/d column]
    for s in range(n):
        for j in range(2 if n > 1 else 1):
            idx = np.flatnonzero(z0 + j == s) if n > 1 else np.flatnonzero(z0 == 0)
            if len(idx):
                val, grad = slice_fn(s, points[idx, 1:])
                R[j, 0, idx], R[j, 1, idx], R[j, 2, idx] = val, grad[0], grad[1]
    if n == 1:
        return R[0, 0], None
    value = select(f, R[0, 0], R[1, 0], dtype)
    grad = np.stack([R[1, 0] - R[0, 0], select(f, R[0, 1], R[1, 1], dtype), select(f, R[0, 2], R[1, 2], dtype)])
    return value, grad


def volume_of_stack(sd, mods, black, points, nV, nH, S, I, *, num_layers, activation="sine", dtype=np.float64, perturbed=False):
    """mods[s] (L, nV nH, H), black[s]: what resample_reference.resample takes for slice s; dtype / perturbed are passed through to it
    (fp32 + perturbed is the variant that sizes the gradient gate)"""
    def slice_fn(s, yx):
        return rr.resample(sd, mods[s], black[s], yx, nV, nH, S, I, num_layers=num_layers, activation=activation, dtype=dtype, perturbed=perturbed)

    return volume(slice_fn, points, len(mods), dtype)
