"""Geometry helpers for ``ModulatedSiren.resample_volume``: point sets in the stack's (Z, Y, X) coordinates --
Z in slice units, (Y, X) in reconstruction pixels.  Pure numpy."""
import numpy as np


def plane_points(origin, u, v, shape):
    """The lattice ``origin + i u + j v`` (i < shape[0], j < shape[1]; origin, u, v in (Z, Y, X)) -> (shape[0] * shape[1], 3) float32, row
    i * shape[1] + j: an oblique or through-plane cut for multi-planar reformatting.  Formed in fp64 and rounded once."""
    origin, u, v = (np.asarray(a, dtype=np.float64) for a in (origin, u, v))
    if origin.shape != (3,) or u.shape != (3,) or v.shape != (3,):
        raise ValueError(f"origin, u and v must be (Z, Y, X) triples, got {origin.shape}, {u.shape}, {v.shape}")
    rows, cols = (int(x) for x in shape)
    if rows < 0 or cols < 0:
        raise ValueError(f"shape must be non-negative, got {shape}")
    i = np.arange(rows, dtype=np.float64)[:, None, None]
    j = np.arange(cols, dtype=np.float64)[None, :, None]
    return (origin + i * u + j * v).reshape(rows * cols, 3).astype(np.float32)
