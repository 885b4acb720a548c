"""Helpers for ``ModulatedSiren.solve_volume_robust`` (msiren_solve_volume_r): ``solve_volume``'s conjugate gradients in rounds,
each on the normal equations reweighted by the Geman-McClure weight of every pixel's residual against the current iterate, under a scale that is
annealed down to the caller's -- and the rule's normative restatement ``solve_volume_robust_on_host``.

Like ``solve_volume.py`` and ``fuse.py``, on whose functions it builds and which it leaves as they are: numpy fp64, ELEMENTWISE, in the associations of
include/msiren.h, so the device equals ``solve_volume_robust_on_host`` bit for bit.  The rule is cut into small functions (the schedule, the weight,
the residual, the reweighting pass, what enters a round, the right-hand side's weights, the stop state, the sums' order) so that a test can replace one
of them by a wrong one and see its checks fail."""
import collections

import numpy as np

from . import align_robust, fuse
from . import solve_volume as sv

SolveVolumeRobustResult = collections.namedtuple("SolveVolumeRobustResult", "volume coverage history flags stopped_at rweight stats")
SolveVolumeRobustResult.__doc__ = """volume, coverage, flags as in ``solve_volume.SolveVolumeResult``; history (rounds, iterations + 1, 2) float64 or None,
per round the block of ``SolveVolumeResult.history``; stopped_at (rounds,) int32, per round the iteration at which it stopped, else -1; rweight
(m, th, tw) float32 or None: omega of the final iterate under the caller's scale, NaN where the pixel is not active or its target's scale is not > 0;
stats (m, 4) float64 or None = (count, sum w, sum w omega, sum ((w om) e) e) over those pixels."""

Reweighted = collections.namedtuple("Reweighted", "u e om omega counts Wt")
Reweighted.__doc__ = """One reweighting pass, all (m, th tw): u = P x on the active pixels (0.0 elsewhere); e the residual in the target's intensity; om =
1 / (1 + e e / s) and omega = om om (+0.0 where s is not > 0); counts bool: active and s > 0; Wt = Wt0 omega, the round's pixel weight"""


def schedule(rounds, anneal):
    """c (rounds,) float64: the factor of every target's scale per round; c[rounds - 1] = 1.0, c[t] = c[t + 1] anneal"""
    c = np.ones(max(int(rounds), 0), np.float64)
    with np.errstate(all="ignore"):
        for t in range(len(c) - 2, -1, -1):
            c[t] = c[t + 1] * np.float64(anneal)
    return c


def robust_weight(e, s):
    """the residual e and the scale s -> (om, omega): a = (e e) / s, v = 1.0 + a, om = 1.0 / v, omega = om om (``align_robust.robust_terms``' om, squared)"""
    a = (e * e) / s
    v = 1.0 + a
    om = 1.0 / v
    return om, om * om


def pixel_residual(T, u, g, bias):
    """e = (double)T - ((g u) + b): the target's pixel against the stack's intensity as the target sees it"""
    return T - fuse.apply_intensity(u, g, bias)


def reweight_on_host(geo, x, targets, s, *, weight=None, residual=None, forward=None):
    """The reweighting pass -> Reweighted.  geo: ``solve_volume.geometry`` (omega_gg = Wt0); x (n, H, W) float64; targets (m, th, tw) float32; s (m,)
    float64, this round's scales"""
    weight, residual, forward = weight or robust_weight, residual or pixel_residual, forward or sv.forward_on_host
    m = len(geo.D)
    T = np.ascontiguousarray(targets, dtype=np.float32).astype(np.float64).reshape(geo.D.shape)
    s = np.asarray(s, np.float64).reshape(m, 1)
    with np.errstate(all="ignore"):
        u = forward(geo, x)
        e = residual(T, u, geo.records.g[:, None], geo.records.bias[:, None])
        om, omega = weight(e, s)
        positive = np.broadcast_to(s > 0, u.shape)  # (a NaN fails)
        omega = np.where(positive, omega, 0.0)
        Wt = np.where(geo.active, geo.omega_gg * omega, 0.0)
    return Reweighted(u, e, om, omega, geo.active & positive, Wt)


def robust_stats_on_host(weights, rew, shape, *, stats_sum=None):
    """-> stats (m, 4) float64 = (count, sum w, sum w omega, sum ((w om) e) e) over ``rew.counts``, each in ``fuse.ordered_sum``'s order"""
    stats_sum = stats_sum or fuse.ordered_sum
    m = len(rew.e)
    th, tw = shape
    w = np.ones((m, th * tw), np.float64) if weights is None else np.ascontiguousarray(weights, dtype=np.float32).astype(np.float64).reshape(m, th * tw)
    stats = np.zeros((m, 4), np.float64)
    with np.errstate(all="ignore"):
        terms = (np.ones_like(w), w, w * (rew.om * rew.om), ((w * rew.om) * rew.e) * rew.e)
        for q in range(m):
            for k, term in enumerate(terms):
                stats[q, k] = stats_sum(np.where(rew.counts[q], term[q], 0.0).reshape(th, tw))
    return stats


def final_pass_on_host(geo, x, targets, weights, scale, *, weight=None, residual=None, forward=None, stats_sum=None):
    """What the call reports of the final iterate, under the caller's scale (factor 1.0) -> (rweight (m, th, tw) float32, residual (m, th, tw) float32,
    stats (m, 4) float64)"""
    m = len(geo.D)
    th, tw = geo.shape
    rew = reweight_on_host(geo, x, targets, scale, weight=weight, residual=residual, forward=forward)
    with np.errstate(all="ignore"):
        rw = np.where(rew.counts, rew.omega.astype(np.float32), np.float32(np.nan)).astype(np.float32).reshape(m, th, tw)
        res = np.where(geo.active, rew.e.astype(np.float32), np.float32(np.nan)).astype(np.float32).reshape(m, th, tw)
    return rw, res, robust_stats_on_host(weights, rew, (th, tw), stats_sum=stats_sum)


def robust_objective_on_host(geo, x, targets, weights, s, lam):
    """1/2 sum over the active pixels of w rho_s(e) + 1/2 lambda reg, rho_s(e) = e e / (1 + e e / s) (e e where s = +inf; 0 where s is not > 0), reg
    ``solve_volume.objective_on_host``'s sum over the edges (plain numpy sums: a figure, not part of the rule)"""
    m = len(geo.D)
    w = np.ones(geo.D.shape) if weights is None else np.asarray(weights, np.float64).reshape(geo.D.shape)
    s = np.asarray(s, np.float64).reshape(m, 1)
    with np.errstate(all="ignore"):
        rew = reweight_on_host(geo, x, targets, s)
        ee = rew.e * rew.e
        rho = np.where(rew.counts, ee / (1.0 + ee / s), 0.0)
        data = 0.5 * float(np.sum(np.where(rew.counts, w, 0.0) * rho))
    return data + sv.objective_on_host(geo._replace(active=np.zeros_like(geo.active)), x, lam)


def same_iterate(x, x0, t):
    """what enters round t: the iterate the round before left (x0: the start)"""
    return x


def current_weights(now, before):
    """the pixel weights of the round's right-hand side: this round's (``before``: the round before's, None in round 0)"""
    return now.Wt


def fresh_stop_state(stopped):
    """the stop state at the start of a round: not stopped, whatever the round before left"""
    return -1


def solve_volume_robust_on_host(targets, maps, shape, spacing, scale, *, rounds, iterations, anneal=1.0, lam=0.0, thickness=None, weights=None, intensity=None,
                                min_coverage=0.0, start=None, iterates=None, schedule_of=None, weight=None, residual=None, reweight=None, entering=None, rhs_weights=None,
                                stop_state=None, stats_sum=None, forward=None, transpose=None, laplacian=None, dot=None, beta=None):
    """The normative restatement of msiren_solve_volume_r -> SolveVolumeRobustResult (coverage, history, rweight and stats always).  targets (m, th, tw),
    maps (m, 9), shape = (n, H, W), ``scale`` a scalar or (m,); ``start`` (n, H, W) float32 or None: ``fuse.fuse_on_host``'s volume.  ``iterates``: a
    list that receives (geometry, x_0, then x after every step of every round) in fp64: round t is entered with iterates[1 + t iterations].  The
    remaining keywords replace one piece of the rule (tests): ``schedule_of`` (rounds, anneal) -> c; ``weight``, ``residual``: ``robust_weight``,
    ``pixel_residual``; ``reweight`` (geo, x, s, t, before) -> Reweighted; ``entering`` (x, x0, t) -> x; ``rhs_weights`` (now, before) -> Wt of the
    right-hand side; ``stop_state`` (stopped) -> the stop state a round starts with; ``stats_sum``: ``fuse.ordered_sum``; the others are
    ``solve_volume_on_host``'s."""
    dot, beta = dot or sv.ordered_dot, beta or sv.direction_weight
    entering, rhs_weights, stop_state = entering or same_iterate, rhs_weights or current_weights, stop_state or fresh_stop_state
    tg = np.ascontiguousarray(targets, dtype=np.float32)
    m = len(tg)
    rounds, iterations = int(rounds), int(iterations)
    scale = align_robust.scales(scale, m)
    fused = fuse.fuse_on_host(targets, maps, shape, spacing, thickness=thickness, weights=weights, intensity=intensity, min_coverage=min_coverage)
    first = fused.volume if start is None else np.ascontiguousarray(start, dtype=np.float32)
    if first.shape != tuple(int(s) for s in shape):
        raise ValueError(f"expected start of shape {tuple(shape)}, got {first.shape}")
    S = np.isfinite(first)
    geo = sv.geometry(targets, maps, S, spacing, thickness=thickness, weights=weights, intensity=intensity, min_coverage=min_coverage)
    ops = dict(forward=forward, transpose=transpose, laplacian=laplacian)
    pieces = dict(weight=weight, residual=residual, forward=forward)
    if reweight is None:
        def reweight(geo, x, s, t, before):
            return reweight_on_host(geo, x, tg, s, **pieces)
    c = (schedule_of or schedule)(rounds, anneal)
    history = np.full((rounds, iterations + 1, 2), np.nan, np.float64)
    stopped_at = np.full(rounds, -1, np.int32)
    with np.errstate(all="ignore"):
        x0 = np.where(S, first.astype(np.float64), 0.0)
        x = x0
        if iterates is not None:
            iterates += [geo, x.copy()]
        before, stopped = None, -1
        for t in range(rounds):
            x = entering(x, x0, t)
            now = reweight(geo, x, scale * c[t], t, before)
            geo_t = geo._replace(omega_gg=now.Wt)
            rhs = (transpose or sv.transpose_on_host)(geo, np.where(geo.active, rhs_weights(now, before) * geo.tau, 0.0))
            r = rhs - sv.apply_on_host(geo_t, x, lam, **ops)
            p = r.copy()
            rho = dot(r, r, S)
            stopped = stop_state(stopped)
            for it in range(iterations):
                history[t, it, 0] = rho
                if stopped < 0:
                    q = sv.apply_on_host(geo_t, p, lam, **ops)
                    gamma = dot(p, q, S)
                    if rho == 0 or not np.isfinite(gamma) or not gamma > 0:
                        stopped = it
                    else:
                        history[t, it, 1] = gamma
                        alpha = sv.step_length(rho, gamma)
                        x = np.where(S, x + (alpha * p), 0.0)
                        r = np.where(S, r - (alpha * q), 0.0)
                        rho_new = dot(r, r, S)
                        p = np.where(S, r + (beta(rho_new, rho) * p), 0.0)
                        rho = rho_new
                if iterates is not None:
                    iterates.append(x.copy())
            history[t, iterations, 0] = rho
            stopped_at[t] = stopped
            before = now
        volume = np.where(S, x.astype(np.float32), np.float32(np.nan)).astype(np.float32)
        rw, _, stats = final_pass_on_host(geo, x, tg, weights, scale, stats_sum=stats_sum, **pieces)
    return SolveVolumeRobustResult(volume, fused.coverage, history, fused.flags, stopped_at, rw, stats)
