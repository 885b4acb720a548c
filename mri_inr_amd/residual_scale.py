"""Helpers for ``ModulatedSiren.residual_scale`` (msiren_residual_scale): the ``scale`` of the robust calls from an exact order
statistic of the residuals -- per target, or pooled over groups of consecutive targets -- and the rule's normative restatement
``residual_scale_on_host``.

numpy, ELEMENTWISE, in the associations of include/msiren.h, so the device equals ``residual_scale_on_host`` bit for bit.  The rule is cut into small
functions (the residual, which pixels count, the key of the order, the rank, the deviation, the scale) so that a test can replace one of them by a wrong
one and see its checks fail.  ``tune = 6 MAD_TO_SIGMA`` with the defaults (the median, not centred) gives the scale that reaches the hand-tuned result
of DESIGN.md section 5.20 without hand tuning."""
import collections

import numpy as np

from . import align_group as ag

MAD_TO_SIGMA = 1.482602218505602  # 1 / Phi^-1(3 / 4): the median absolute deviation of a normal sample, times this, estimates its sigma

ResidualScaleResult = collections.namedtuple("ResidualScaleResult", "scale stats")
ResidualScaleResult.__doc__ = """scale (m,) float64: per target (tune d)^2 of its segment, at least ``floor``; +inf for a segment without a pixel that
counts.  stats (S, 4) float64 or None = (count, k, c, d) per segment: the pixels that count, the rank taken, the centre and the deviation of that rank."""


def pixel_residual(T, S, g, bias):
    """float32 T, S and float64 g, b (None: no intensity) -> e float32: (float)((double)T - ((g (double)S) + b)); without intensity (float)((double)T -
    (double)S), ``fuse.residual_on_host``'s bits wherever that one is finite; S None: T itself"""
    if S is None:
        return T
    Td, Sd = T.astype(np.float64), S.astype(np.float64)
    if g is None:
        return (Td - Sd).astype(np.float32)
    return (Td - ((g * Sd) + bias)).astype(np.float32)


def pixel_counts(e, w):
    """which pixels count: e finite, w finite and > 0"""
    return np.isfinite(e) & np.isfinite(w) & (w > 0)


def sort_key(x):
    """float32 -> uint32, ascending in the rule's total order of the bit patterns: -0 before +0, every pattern a place of its own"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)


def magnitude_key(d):
    """float32, not negative -> uint32: such values order as their bits"""
    return np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)


def rank(quantile, count):
    """k = (int64)floor(quantile (double)(count - 1)): one fp64 multiply"""
    return int(np.floor(np.float64(quantile) * np.float64(count - 1)))


def element_of_rank(x, k, key):
    """the element of rank k (0-based, ascending by ``key``) of the float32 values x"""
    return x[np.argsort(key(x), kind="stable")[k]]


def deviation(e, c):
    """d = fabsf(e - c): one fp32 subtraction"""
    return np.abs(e - np.float32(c))


def scale_of(d, tune, floor):
    """t = tune (double)d, s = t t; s if s > floor, else floor"""
    t = np.float64(tune) * np.float64(d)
    s = t * t
    return s if s > floor else np.float64(floor)


def segments(groups, m):
    """``groups`` as ``align_group.group_offsets`` takes them, None: one segment per target -> the (S + 1) offsets"""
    return np.arange(m + 1, dtype=np.int64) if groups is None else np.asarray(ag.group_offsets(groups, m), np.int64)


def residual_scale_on_host(targets, simulated=None, *, tune, weights=None, intensity=None, groups=None, quantile=0.5, centre=False, floor=0.0, residual=None,
                           counts=None, key=None, rank_of=None, deviation_of=None, scale_from_d=None):
    """The normative restatement of msiren_residual_scale -> ResidualScaleResult (stats always).  targets (m, th, tw); simulated (m, th, tw) or None (the
    targets are residuals already); weights (m, th, tw) or None; intensity (m, 2) or None, only with simulated; ``groups``: the (G + 1) offsets or the G
    sizes of groups of consecutive targets, None: every target on its own.  The remaining keywords replace one piece of the rule (tests): ``residual``:
    ``pixel_residual``; ``counts``: ``pixel_counts``; ``key``: ``sort_key`` (the order of the e themselves); ``rank_of``: ``rank``; ``deviation_of``:
    ``deviation``; ``scale_from_d``: ``scale_of``."""
    residual, counts, key, rank_of = residual or pixel_residual, counts or pixel_counts, key or sort_key, rank_of or rank
    deviation_of, scale_from_d = deviation_of or deviation, scale_from_d or scale_of
    T = np.ascontiguousarray(targets, dtype=np.float32)
    if T.ndim != 3:
        raise ValueError(f"expected targets of shape (m, th, tw), got {T.shape}")
    m = len(T)
    S = None if simulated is None else np.ascontiguousarray(simulated, dtype=np.float32)
    if intensity is not None and S is None:
        raise ValueError("intensity given without simulated")
    w = np.ones(T.shape, np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    gb = None if intensity is None else np.ascontiguousarray(intensity, dtype=np.float32).astype(np.float64).reshape(m, 2)
    offsets = segments(groups, m)
    scale = np.full(m, np.inf, np.float64)
    stats = np.zeros((len(offsets) - 1, 4), np.float64)
    with np.errstate(all="ignore"):
        e = residual(T, S, None if gb is None else gb[:, 0].reshape(m, 1, 1), None if gb is None else gb[:, 1].reshape(m, 1, 1))
        take = counts(e, w)
        for s, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
            es = e[lo:hi][take[lo:hi]]
            count = len(es)
            if count == 0:
                continue
            k = rank_of(quantile, count)
            c = element_of_rank(es, k, key) if centre else np.float32(0.0)
            d = element_of_rank(deviation_of(es, c), k, magnitude_key)
            scale[lo:hi] = scale_from_d(d, tune, floor)
            stats[s] = (count, k, np.float64(c), np.float64(d))
    return ResidualScaleResult(scale, stats)
