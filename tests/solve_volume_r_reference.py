"""An independent reference for one round of msiren_solve_volume_r on a case small enough for a dense matrix, for
tests/test_solve_volume_robust_reference.py.  Not a test module.

Given the iterate x that enters a round and the round's scales, the weights are formed from the dense tent-function P of tests/solve_volume_reference.py
(no floor, no base index, no tap): u = P x, e = T - (g u + b), omega = 1 / (1 + e^2 / s)^2 in one expression, zero where s is not > 0.  The round's normal
equations (Pt (w g^2 omega) P + lambda L) x = Pt (w g^2 omega) tau are then solved by ``np.linalg.solve``.  Nothing is shared with
mri_inr_amd/solve_volume_robust.py but the support and the entering iterate (inputs) and the definition of the result."""
import collections

import numpy as np

import solve_volume_reference as ref

DenseRound = collections.namedtuple("DenseRound", "x omega active cond lam_min")


def solve_round(targets, maps, support, spacing, x_in, scale, *, lam, thickness, weights=None, intensity=None, min_coverage=0.0):
    """-> DenseRound: x (n, H, W) float64 on the support (0 elsewhere), the weights omega (m th tw,), the condition number and the smallest eigenvalue of
    the round's matrix on the support"""
    T = np.asarray(targets, np.float32)
    m, th, tw = T.shape
    w = np.ones(T.shape, np.float32) if weights is None else np.asarray(weights, np.float32)
    gb = np.tile([1.0, 0.0], (m, 1)) if intensity is None else np.asarray(intensity, np.float32).astype(np.float64)
    P, covered = ref.projection_matrix(support, maps, (th, tw), spacing, thickness, min_coverage)
    valid = (np.isfinite(T) & np.isfinite(w) & (w > 0)).ravel()
    active = covered & valid
    g, b = np.repeat(gb[:, 0], th * tw), np.repeat(gb[:, 1], th * tw)
    s = np.repeat(np.broadcast_to(np.asarray(scale, np.float64), (m,)), th * tw)
    P = np.where(active[:, None], P, 0.0)
    Td = T.astype(np.float64).ravel()
    with np.errstate(all="ignore"):
        e = np.where(active, Td - (g * (P @ np.asarray(x_in, np.float64).ravel()) + b), 0.0)
        omega = np.where(active & (s > 0), 1.0 / (1.0 + e ** 2 / s) ** 2, 0.0)
    W = np.where(active, w.astype(np.float64).ravel() * g * g * omega, 0.0)
    tau = np.where(active, (Td - b) / g, 0.0)
    A = P.T @ (W[:, None] * P) + lam * ref.laplacian_matrix(support, spacing)
    rhs = P.T @ (W * tau)
    S = support.ravel()
    As = A[np.ix_(S, S)]
    eig = np.linalg.eigvalsh(As)
    x = np.zeros(support.size)
    x[S] = np.linalg.solve(As, rhs[S])
    return DenseRound(x.reshape(support.shape), omega, active, float(eig[-1] / eig[0]), float(eig[0]))
