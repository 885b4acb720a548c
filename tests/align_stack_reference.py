"""Reference for the trilinear read of msiren_align_stack_r, independent of mri_inr_amd/align_stack.py: a dense trilinear
matrix -- every value and every derivative as a sum of the eight corner weights times the corners, in another association (weights first) -- with the
sum of the magnitudes of the terms, against which errors are measured.  Not a test module.

``mutant_read`` is align_stack.read_stack's rule with one error planted, of the kinds an implementation can make (SEEDS);
tests/test_align_stack_reference.py asserts that each is rejected.
"""
import numpy as np

SEEDS = ("gz_from_blend", "fz_without_clamp", "xy_passes_swapped", "upper_face_refused", "nan_corner_skipped", "yx_extents_swapped")


def dense(stack, points):
    """stack (n, H, W), points (M, 3) -> (values (4, M) = R, gZ, gY, gX in fp64, magnitudes (4, M) = sum |weight corner|); NaN outside.  The cell is
    the one that holds the point, the last cell at an upper face."""
    v = np.asarray(stack, np.float64)
    n, H, W = v.shape
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    out, mag = np.full((4, len(p)), np.nan), np.full((4, len(p)), np.nan)
    for k, (Z, Y, X) in enumerate(p):
        if not (0 <= Z <= n - 1 and 0 <= Y <= H - 1 and 0 <= X <= W - 1):
            continue
        c = [min(int(np.floor(a)), L - 2) for a, L in ((Z, n), (Y, H), (X, W))]
        f = [a - b for a, b in zip((Z, Y, X), c)]
        wt = [np.array([1.0 - t, t]) for t in f]
        dw = np.array([-1.0, 1.0])
        cell = v[c[0]:c[0] + 2, c[1]:c[1] + 2, c[2]:c[2] + 2]
        for r, (a, b, d) in enumerate(((wt[0], wt[1], wt[2]), (dw, wt[1], wt[2]), (wt[0], dw, wt[2]), (wt[0], wt[1], dw))):
            w3 = a[:, None, None] * b[None, :, None] * d[None, None, :]
            with np.errstate(invalid="ignore", over="ignore"):
                out[r, k], mag[r, k] = (w3 * cell).sum(), np.abs(w3 * cell).sum()
    return out, mag


def mutant_read(stack, points, seed, rounded=True):
    """align_stack.read_stack with the error ``seed`` -> (R, gZ, gY, gX) float32 (``rounded`` False: the fp64 values in front of the last rounding)"""
    assert seed in SEEDS
    v = np.ascontiguousarray(stack, np.float32)
    n, H, W = v.shape
    p = np.asarray(points, np.float32).reshape(-1, 3)
    Z, Y, X = p[:, 0], p[:, 1], p[:, 2]
    eh, ew = (W, H) if seed == "yx_extents_swapped" else (H, W)
    with np.errstate(invalid="ignore"):
        if seed == "upper_face_refused":
            inside = (Z >= 0) & (Z < np.float32(n - 1)) & (Y >= 0) & (Y < np.float32(eh - 1)) & (X >= 0) & (X < np.float32(ew - 1))
        else:
            inside = (Z >= 0) & (Z <= np.float32(n - 1)) & (Y >= 0) & (Y <= np.float32(eh - 1)) & (X >= 0) & (X <= np.float32(ew - 1))
    out = [np.full(len(p), np.nan, np.float32 if rounded else np.float64) for _ in range(4)]

    def cell(a, length, clamp=True):
        c = np.floor(a).astype(np.int64)
        f = a.astype(np.float64) - (c if not clamp else np.minimum(c, length - 2)).astype(np.float64)
        return np.minimum(c, length - 2), f, 1.0 - f

    z0, fz, az = cell(Z[inside], n, seed != "fz_without_clamp")
    y0, fy, ay = cell(Y[inside], eh)
    x0, fx, ax = cell(X[inside], ew)
    y0, x0 = np.minimum(y0, H - 2), np.minimum(x0, W - 2)  # (the swapped extents: stay inside the array)
    with np.errstate(invalid="ignore", over="ignore"):
        V = [[[v[z0 + a, y0 + b, x0 + c].astype(np.float64) for c in range(2)] for b in range(2)] for a in range(2)]
        if seed == "nan_corner_skipped":  # a corner that is not finite counts as 0
            V = [[[np.where(np.isfinite(V[a][b][c]), V[a][b][c], 0.0) for c in range(2)] for b in range(2)] for a in range(2)]
        e, ex, ey = [], [], []
        for dz in range(2):
            if seed == "xy_passes_swapped":  # y first, then x: the same polynomial in another association
                cy = [(ay * V[dz][0][c]) + (fy * V[dz][1][c]) for c in range(2)]
                dy = [V[dz][1][c] - V[dz][0][c] for c in range(2)]
                e.append((ax * cy[0]) + (fx * cy[1]))
                ey.append((ax * dy[0]) + (fx * dy[1]))
                ex.append(cy[1] - cy[0])
            else:
                c = [(ax * V[dz][b][0]) + (fx * V[dz][b][1]) for b in range(2)]
                d = [V[dz][b][1] - V[dz][b][0] for b in range(2)]
                e.append((ay * c[0]) + (fy * c[1]))
                ex.append((ay * d[0]) + (fy * d[1]))
                ey.append(c[1] - c[0])
        R = (az * e[0]) + (fz * e[1])
        gz = (R - e[0]) if seed == "gz_from_blend" else e[1] - e[0]
        vals = (R, gz, (az * ey[0]) + (fz * ey[1]), (az * ex[0]) + (fz * ex[1]))
        for o, x in zip(out, vals):
            o[inside] = x.astype(o.dtype)
    return tuple(out)
