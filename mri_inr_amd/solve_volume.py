"""Helpers for ``ModulatedSiren.solve_volume`` (msiren_solve_volume): the stack that best explains all aligned targets at
once -- a fixed number of conjugate-gradient iterations on the weighted, regularised normal equations (Pt Omega P + lambda L) x = Pt Omega tau, with P
the row-normalised projection of ``fuse.project_on_host`` -- and the rule's normative restatement ``solve_volume_on_host``.

Like ``fuse.py``, on whose functions it builds: numpy fp64, ELEMENTWISE, in the associations of include/msiren.h, so the device equals
``solve_volume_on_host`` bit for bit.  The rule is cut into small functions (the forward operator, its transpose, the Laplacian, the ordered inner
product, the pixel weight, the step's two quotients) so that a test can replace one of them by a wrong one and see its checks fail."""
import collections

import numpy as np

from . import fuse

SolveVolumeResult = collections.namedtuple("SolveVolumeResult", "volume coverage history flags stopped_at")
SolveVolumeResult.__doc__ = """volume (n, H, W) float32: the iterate after ``iterations`` steps on the support (the finite voxels of the start), NaN
elsewhere; coverage (n, H, W) float32, msiren_fuse_targets' coverage, or None; history (iterations + 1, 2) float64 = (rho_k, gamma_k) with rho = <r, r>
and gamma = <p, A p>, gamma NaN in the last row and from a stop on, or None; flags (m,) int32 as in ``fuse.FuseResult``; stopped_at: the iteration at
which the solve stopped (rho == 0, or gamma not finite or not > 0), -1 if it never did."""

Geometry = collections.namedtuple("Geometry", "records support taps D active omega_gg tau grid shape cz")
Geometry.__doc__ = """What stays fixed over the iterations: records (fuse.TargetRecords); support (n, H, W) bool; taps: per target None or fuse.voxel_taps'
(at, k, pixel, beta) over the support; D (m, th tw) float64, section 5.18's den over the support; active (m, th tw) bool; omega_gg (m, th tw) = (w g) g;
tau (m, th tw) = ((double)T - b) / g; grid = (n, H, W); shape = (th, tw); cz = 1 / (spacing spacing), the through-plane edge weight"""


def pixel_weight(w, g):
    """Omega: the weight of a pixel's squared residual in the stack's intensity, (w g) g"""
    return (w * g) * g


def geometry(targets, maps, support, spacing, *, thickness=None, weights=None, intensity=None, min_coverage=0.0):
    """targets (m, th, tw) float32, support (n, H, W) bool -> Geometry"""
    tg = np.ascontiguousarray(targets, dtype=np.float32)
    m, th, tw = tg.shape
    sup = np.ascontiguousarray(support, dtype=bool)
    wt = np.ones(tg.shape, np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    spacing = np.float64(spacing)
    r = fuse.target_records(maps, intensity, spacing, spacing if thickness is None else thickness)
    taps = [None if r.flags[q] else fuse.voxel_taps(r, q, sup, sup.shape, (th, tw), spacing) for q in range(m)]
    D = np.zeros((m, th * tw), np.float64)
    with np.errstate(all="ignore"):
        for q in range(m):
            if taps[q] is not None:
                at, k, pixel, beta = taps[q]
                fuse.scatter(D[q], pixel, fuse.tap_terms(k[:, None], beta, np.float64(1.0))[1])
        active = (r.flags == 0)[:, None] & fuse.tap_valid(tg, wt).reshape(m, th * tw) & (D > np.float64(min_coverage))
        g, bias = r.g[:, None], r.bias[:, None]
        omega_gg = pixel_weight(wt.astype(np.float64).reshape(m, th * tw), g)
        tau = fuse.tap_value(tg.astype(np.float64).reshape(m, th * tw), bias, g)
        cz = np.float64(1.0) / (spacing * spacing)
    return Geometry(r, sup, taps, D, active, omega_gg, tau, sup.shape, (th, tw), cz)


def forward_sums_on_host(geo, v):
    """v (n, H, W) float64 -> num (m, th tw): section 5.18's sum with the fp64 entry of v in place of (double)V, over the support, in its order"""
    num = np.zeros(geo.D.shape, np.float64)
    with np.errstate(all="ignore"):
        for q, taps in enumerate(geo.taps):
            if taps is not None:
                at, k, pixel, beta = taps
                fuse.scatter(num[q], pixel, fuse.tap_terms(k[:, None], beta, v[at][:, None])[0])
    return num


def forward_on_host(geo, v):
    """u = P v (m, th tw): num / D on the active pixels, 0.0 elsewhere"""
    num = forward_sums_on_host(geo, v)
    with np.errstate(all="ignore"):
        return np.where(geo.active, num / geo.D, 0.0)


def tap_share(beta, y, D):
    """what one active tap of a voxel adds to sn: the pixel's value over its row sum, times the bilinear weight"""
    return beta * (y / D)


def transpose_on_host(geo, y):
    """Pt y (n, H, W): per voxel of the support, for q ascending, acc += k sn with sn the sum over the four taps in tap order of beta (y_p / D_p) over
    the active taps; 0.0 outside the support"""
    acc = np.zeros(geo.grid, np.float64)
    with np.errstate(all="ignore"):
        for q, taps in enumerate(geo.taps):
            if taps is None:
                continue
            at, k, pixel, beta = taps
            sn = np.zeros(len(k), np.float64)
            for tap in range(4):
                p = pixel[:, tap]
                sn = sn + np.where(geo.active[q][p], tap_share(beta[:, tap], y[q][p], geo.D[q][p]), 0.0)
            acc[at] = acc[at] + (k * sn)
    return acc


def edge_term(c, vu, vn):
    """one neighbour's term of the Laplacian"""
    return c * (vu - vn)


def laplacian_on_host(geo, v):
    """(L v)_u = the sum from 0.0 of c (v_u - v_u') over the neighbours z-, z+, y-, y+, x-, x+ that are in the grid and in the support, c = 1 in plane
    and 1 / (spacing spacing) through plane; 0.0 outside the support"""
    out = np.zeros(geo.grid, np.float64)
    S = geo.support
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        for axis, c in ((0, geo.cz), (1, one), (2, one)):
            for step in (-1, 1):
                lo, hi = [slice(None)] * 3, [slice(None)] * 3                    # u runs over `here`, its neighbour over `there`
                lo[axis], hi[axis] = (slice(1, None), slice(None, -1)) if step < 0 else (slice(None, -1), slice(1, None))
                here, there = tuple(lo), tuple(hi)
                both = S[here] & S[there]
                out[here] = out[here] + np.where(both, edge_term(c, v[here], v[there]), 0.0)
    return np.where(S, out, 0.0)


def ordered_dot(a, b, support):
    """<a, b> in the rule's order: per slice fuse.ordered_sum (per column down the rows from 0.0, then the columns ascending from 0.0), then the slices
    ascending from 0.0; terms outside the support are 0.0"""
    with np.errstate(all="ignore"):
        terms = np.where(support, a * b, 0.0)
        s = np.float64(0.0)
        for z in range(terms.shape[0]):
            s = s + fuse.ordered_sum(terms[z])
    return s


def apply_on_host(geo, v, lam, *, forward=None, transpose=None, laplacian=None):
    """A v = Pt (Omega (P v)) + (lambda (L v))"""
    forward, transpose, laplacian = forward or forward_on_host, transpose or transpose_on_host, laplacian or laplacian_on_host
    with np.errstate(all="ignore"):
        y = geo.omega_gg * forward(geo, v)
        return transpose(geo, y) + (np.float64(lam) * laplacian(geo, v))


def step_length(rho, gamma):
    """alpha"""
    return rho / gamma


def direction_weight(rho_new, rho):
    """beta of the new search direction"""
    return rho_new / rho


def objective_on_host(geo, x, lam):
    """F(x) = 1/2 sum over the active pixels of Omega (tau - P x)^2 + 1/2 lambda sum over the edges of c (x_u - x_v)^2 (plain numpy sums: a figure,
    not part of the rule)"""
    with np.errstate(all="ignore"):
        res = np.where(geo.active, geo.tau - forward_on_host(geo, x), 0.0)
        data = 0.5 * float(np.sum(np.where(geo.active, geo.omega_gg, 0.0) * res * res))
        reg = 0.0
        S = geo.support
        for axis, c in ((0, float(geo.cz)), (1, 1.0), (2, 1.0)):
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[axis], b[axis] = slice(None, -1), slice(1, None)
            a, b = tuple(a), tuple(b)
            d = np.where(S[a] & S[b], x[a] - x[b], 0.0)
            reg += c * float(np.sum(d * d))
    return data + 0.5 * float(lam) * reg


def solve_volume_on_host(targets, maps, shape, spacing, *, iterations, lam=0.0, thickness=None, weights=None, intensity=None, min_coverage=0.0, start=None,
                         iterates=None, forward=None, transpose=None, laplacian=None, dot=None, weight=None, beta=None):
    """The normative restatement of msiren_solve_volume -> SolveVolumeResult (coverage and history always).  targets (m, th, tw), maps (m, 9), shape =
    (n, H, W); ``start`` (n, H, W) float32 or None: ``fuse.fuse_on_host``'s volume.  ``iterates``: a list that receives (geometry, x_0, .., x_iterations)
    in fp64.  The remaining keywords replace one piece of the rule (tests)."""
    dot, beta = dot or ordered_dot, beta or direction_weight
    fused = fuse.fuse_on_host(targets, maps, shape, spacing, thickness=thickness, weights=weights, intensity=intensity, min_coverage=min_coverage)
    first = fused.volume if start is None else np.ascontiguousarray(start, dtype=np.float32)
    if first.shape != tuple(int(s) for s in shape):
        raise ValueError(f"expected start of shape {tuple(shape)}, got {first.shape}")
    S = np.isfinite(first)
    geo = geometry(targets, maps, S, spacing, thickness=thickness, weights=weights, intensity=intensity, min_coverage=min_coverage)
    if weight is not None:
        geo = geo._replace(omega_gg=weight(geo))
    ops = dict(forward=forward, transpose=transpose, laplacian=laplacian)
    history = np.full((iterations + 1, 2), np.nan, np.float64)
    stopped_at = -1
    with np.errstate(all="ignore"):
        x = np.where(S, first.astype(np.float64), 0.0)
        rhs = (transpose or transpose_on_host)(geo, np.where(geo.active, geo.omega_gg * geo.tau, 0.0))
        r = rhs - apply_on_host(geo, x, lam, **ops)
        p = r.copy()
        rho = dot(r, r, S)
        if iterates is not None:
            iterates += [geo, x.copy()]
        for it in range(iterations):
            history[it, 0] = rho
            if stopped_at < 0:
                q = apply_on_host(geo, p, lam, **ops)
                gamma = dot(p, q, S)
                if rho == 0 or not np.isfinite(gamma) or not gamma > 0:
                    stopped_at = it
                else:
                    history[it, 1] = gamma
                    alpha = step_length(rho, gamma)
                    x = np.where(S, x + (alpha * p), 0.0)
                    r = np.where(S, r - (alpha * q), 0.0)
                    rho_new = dot(r, r, S)
                    p = np.where(S, r + (beta(rho_new, rho) * p), 0.0)
                    rho = rho_new
            if iterates is not None:
                iterates.append(x.copy())
        history[iterations, 0] = rho
        volume = np.where(S, x.astype(np.float32), np.float32(np.nan)).astype(np.float32)
    return SolveVolumeResult(volume, fused.coverage, history, fused.flags, stopped_at)
