"""An independent reference for msiren_solve_volume on a case small enough for a dense matrix, for
tests/test_solve_volume_reference.py.  Not a test module.

P is built row by row in tests/project_reference.py's per-pixel formulation: per target every voxel is placed at (i, j, d) on the target by solving
[a b n] (i, j, d) = v - t with the unit normal n, and the weight of voxel v in pixel (pi, pj) is k tent(i - pi) tent(j - pj), tent(u) = max(0, 1 - |u|),
k = 1 - (d / thickness)^2 -- no floor, no base index, no tap -- over the voxels of the support, divided by the row's sum.  The Laplacian comes from a list
of edges.  The normal equations (Pt Omega P + lambda L) x = Pt Omega tau are then solved by ``np.linalg.solve``.  Nothing is shared with
mri_inr_amd/solve_volume.py but the support (an input) and the definition of the result."""
import collections

import numpy as np

Dense = collections.namedtuple("Dense", "x A rhs P active cond lam_min")


def projection_matrix(support, maps, shape, spacing, thickness, min_coverage=0.0):
    """-> (P (m th tw, voxels) with rows of sum 1 on the covered pixels and 0 elsewhere, covered (m th tw,) bool)"""
    n, H, W = support.shape
    th, tw = shape
    mp = np.asarray(maps, np.float32).astype(np.float64).reshape(-1, 3, 3)
    z, y, x = np.mgrid[0:n, 0:H, 0:W].astype(np.float64)
    v = np.stack([z.ravel() * spacing, y.ravel(), x.ravel()])
    S = support.ravel()
    rows, covered = [], []
    for q in range(len(mp)):
        A = mp[q].copy()
        A[0] *= spacing
        a, b = A[:, 0], A[:, 1]
        nrm = np.cross(a, b)
        M = np.stack([a, b, nrm / np.linalg.norm(nrm)], axis=1)
        i, j, d = np.linalg.solve(M, v - A[:, 2:3])
        k = 1.0 - (d / thickness) ** 2
        inside = S & (k > 0) & (i >= 0) & (i <= th - 1) & (j >= 0) & (j <= tw - 1)
        for pi in range(th):
            ti = np.maximum(0.0, 1.0 - np.abs(i - pi))
            for pj in range(tw):
                kw = np.where(inside, k * ti * np.maximum(0.0, 1.0 - np.abs(j - pj)), 0.0)
                den = kw.sum()
                ok = den > min_coverage
                rows.append(kw / den if ok else np.zeros_like(kw))
                covered.append(bool(ok))
    return np.array(rows), np.array(covered)


def laplacian_matrix(support, spacing):
    n, H, W = support.shape
    idx = np.arange(support.size).reshape(support.shape)
    L = np.zeros((support.size, support.size))
    for axis, c in ((0, 1.0 / (spacing * spacing)), (1, 1.0), (2, 1.0)):
        a, b = [slice(None)] * 3, [slice(None)] * 3
        a[axis], b[axis] = slice(None, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        both = support[a] & support[b]
        for u, w in zip(idx[a][both], idx[b][both]):
            L[u, u] += c
            L[w, w] += c
            L[u, w] -= c
            L[w, u] -= c
    return L


def solve(targets, maps, support, spacing, *, lam, thickness, weights=None, intensity=None, min_coverage=0.0):
    """-> Dense: x (n, H, W) float64 on the support (0 elsewhere), the matrix, its condition number and smallest eigenvalue on the support"""
    T = np.asarray(targets, np.float32)
    m, th, tw = T.shape
    w = np.ones(T.shape, np.float32) if weights is None else np.asarray(weights, np.float32)
    gb = np.tile([1.0, 0.0], (m, 1)) if intensity is None else np.asarray(intensity, np.float32).astype(np.float64)
    P, covered = projection_matrix(support, maps, (th, tw), spacing, thickness, min_coverage)
    valid = (np.isfinite(T) & np.isfinite(w) & (w > 0)).ravel()
    active = covered & valid
    g, b = np.repeat(gb[:, 0], th * tw), np.repeat(gb[:, 1], th * tw)
    omega = np.where(active, w.astype(np.float64).ravel() * g * g, 0.0)
    tau = np.where(active, (T.astype(np.float64).ravel() - b) / g, 0.0)
    P = np.where(active[:, None], P, 0.0)
    A = P.T @ (omega[:, None] * P) + lam * laplacian_matrix(support, spacing)
    rhs = P.T @ (omega * tau)
    S = support.ravel()
    As = A[np.ix_(S, S)]
    eig = np.linalg.eigvalsh(As)
    x = np.zeros(support.size)
    x[S] = np.linalg.solve(As, rhs[S])
    return Dense(x.reshape(support.shape), A, rhs, P, active, float(eig[-1] / eig[0]), float(eig[0]))
