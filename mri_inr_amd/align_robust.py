"""Helpers for ``ModulatedSiren.align_volume_cost_r`` and ``align_volume_solve_group_robust``: section 5.14's 80 sums with
a Geman-McClure loss rho(r) = r^2 / (1 + r^2 / s) in place of the square, one scale s = (c sigma)^2 > 0 per target in squared intensity units.
Only how a pixel's terms are formed is new (``robust_terms``: what align_volume_partial_r_kernel computes, in Python floats, bit for bit); the record,
its packing and the whole step stage of section 5.15 (``align_group.lm_step_g``) are unchanged, so the solve is ``align_group.solve_on_host_g``
around a robust ``cost_fn``.  All groups of one target make it the robust rigid solve per target.

The scale is FIXED for a solve: every evaluation of one call scores the same objective, and mean = cost / wsum with the plain sum of the weights
cannot be lowered by rejecting pixels.  ``scale_from`` gives a first scale from a quadratic pass; s = +inf is the quadratic loss itself."""
import collections

import numpy as np

from . import align_group as ag
from .align import INF
from .align_volume import SUMS_VW, unpack_vw

AlignResultR = collections.namedtuple("AlignResultR", "count wsum cost grad jtj warped wgrad rweight")
AlignResultR.__doc__ = """align_volume.AlignResultVW's fields under the robust loss: count (m,) int64 valid pixels (a target whose scale is not > 0 has
none), wsum (m,) the plain sum of their weights, cost (m,) sum w rho(r), grad (m, 11) its exact gradient, jtj (m, 11, 11) the majoriser's
Gauss-Newton matrix; warped / wgrad as there; rweight (m, th, tw) float32 = 1 / (1 + r^2 / s)^2 at a valid pixel, NaN elsewhere, or None."""

RobustTerms = collections.namedtuple("RobustTerms", "om wl wq cost dfac")
RobustTerms.__doc__ = """One valid pixel's factors: om = 1 / (1 + r^2 / s), wl = w om, wq = wl om, cost = (wl r) r what the pixel adds to the cost, dfac =
2 (wq r) what multiplies J[a] in dcost; jtj takes (wq J[a]) J[b]."""


def robust_terms(r, w, s):
    """The residual r, the weight w and the scale s > 0 of one valid pixel, as Python floats -> RobustTerms.  fp64 + - * / one at a time, in the
    kernel's association.  s = +inf: om = 1, wl = wq = w -- section 5.14's terms."""
    r, w, s = float(r), float(w), float(s)
    u = (r * r) / s
    v = 1.0 + u
    om = 1.0 / v
    wl = w * om
    wq = wl * om
    return RobustTerms(om, wl, wq, (wl * r) * r, 2.0 * (wq * r))


def scales(scale, m):
    """``scale``, a scalar or (m,), as (m,) contiguous float64"""
    s = np.asarray(scale, dtype=np.float64)
    if s.ndim == 0:
        s = np.full(m, float(s), np.float64)
    if s.shape != (m,):
        raise ValueError(f"expected a scalar scale or one of shape ({m},), got {s.shape}")
    return np.ascontiguousarray(s)


def scale_from(result, tune):
    """A first scale per target from any weighted result (fields ``cost`` and ``wsum``: an AlignResultVW, an AlignResultR, a SolveResultG):
    tune^2 cost / wsum, the mean weighted squared residual times tune^2; +inf (the quadratic loss) where wsum is 0"""
    cost, wsum = np.asarray(result.cost, np.float64).reshape(-1), np.asarray(result.wsum, np.float64).reshape(-1)
    out = np.full(cost.shape, INF, np.float64)
    ok = wsum != 0
    out[ok] = (float(tune) * float(tune)) * cost[ok] / wsum[ok]
    return out


def unpack_r(sums, warped=None, wgrad=None, rweight=None):
    """sums (m, 80) as msiren_align_volume_r writes them -> AlignResultR"""
    return AlignResultR(*unpack_vw(sums, warped, wgrad), rweight)


def solve_on_host_r(cost_fn, group_start, scale, *, rigid, planes, intensity=None, options=ag.SolveOptionsG(), trace=False, step=None):
    """msiren_align_volume_solve_group_r's loop around any robust ``cost_fn(maps (m, 9) float32, intensity (m, 2) float32, scale (m,) float64) ->
    sums (m, 80)``: ``align_group.solve_on_host_g`` with the scale held fixed.  -> (SolveResultG, the final states (groups, targets))"""
    s = scales(scale, len(np.asarray(planes).reshape(-1, 12)))
    return ag.solve_on_host_g(lambda maps, gb: np.asarray(cost_fn(maps, gb, s), np.float64).reshape(-1, SUMS_VW), group_start, rigid=rigid, planes=planes,
                              intensity=intensity, options=options, trace=trace, step=step)
