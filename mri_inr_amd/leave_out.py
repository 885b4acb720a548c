"""Helpers for ``ModulatedSiren.leave_out_targets`` (msiren_leave_out_targets): every target predicted from the stack that all
the OTHER targets build -- its own group of consecutive targets left out -- and the rule's normative restatement ``leave_out_on_host``.

Everything here is numpy fp64, ELEMENTWISE, in the associations of include/msiren.h, on top of ``fuse.py`` (imported, not changed): the records, the
contribution test, the taps and their weights are ``fuse.voxel_taps``', the per-target terms ``fuse_on_host``'s, the scatter ``fuse.scatter`` in
voxel-major order -- so the device equals ``leave_out_on_host`` bit for bit.  The rule is cut into small functions (a target's terms, which members are
subtracted, the left-out sums, which voxels take part, the left-out value) so that a test can replace one of them by a wrong one and see its checks
fail."""
import collections

import numpy as np

from . import align_group as ag
from . import fuse

LEAVE_OUT_FLOOR = 2.0 ** -20  # MSIREN_LEAVE_OUT_FLOOR: a power of two, so den_v times it is exact

LeaveOutResult = collections.namedtuple("LeaveOutResult", "simulated coverage residual stats flags volume volume_coverage")
LeaveOutResult.__doc__ = """simulated (m, th, tw) float32: every target as the stack of all targets outside its group predicts it, NaN where the
coverage is not above ``min_coverage`` and everywhere on a flagged target; coverage (m, th, tw) float32, the sum of window x bilinear weight over the
voxels that take part, or None; residual (m, th, tw) float32 = targets - simulated and stats (m, 4) float64 as in ``fuse.ProjectResult``, or None;
flags (m,) int32 as in ``fuse.FuseResult``; volume, volume_coverage (n, H, W) float32: the plain fusion of ALL targets, ``fuse_on_host``'s bits, or
None."""


def own_terms(r, q, Tq, wq, taps):
    """target q's terms (k sn, k sd) at the voxels ``taps`` = ``fuse.voxel_taps`` lists: ``fuse_on_host``'s expressions.  Tq, wq: the target's pixels
    and weights, flat float32"""
    _, k, pixel, beta = taps
    sn, sd = np.zeros(len(k), np.float64), np.zeros(len(k), np.float64)
    for tap in range(4):
        T, w = Tq[pixel[:, tap]], wq[pixel[:, tap]]
        ok = fuse.tap_valid(T, w)
        bw = fuse.tap_weight(beta[:, tap], w.astype(np.float64))
        sn = sn + np.where(ok, bw * fuse.tap_value(T.astype(np.float64), r.bias[q], r.g[q]), 0.0)
        sd = sd + np.where(ok, bw, 0.0)
    return k * sn, k * sd


def members_left_out(lo, hi, q):
    """the targets whose terms are subtracted for target q of the group [lo, hi): the whole group, ascending"""
    return tuple(range(lo, hi))


def left_out_sums(num, den, terms, members):
    """(num_v, den_v) of all targets and ``terms`` = {q': (at, k sn, k sd)} -> (numL, denL): the members' terms added from 0.0 in ascending q', then
    subtracted"""
    own_n, own_d = np.zeros(num.shape, np.float64), np.zeros(den.shape, np.float64)
    for q in members:
        if q in terms:  # (unflagged and contributing somewhere)
            at, kn, kd = terms[q]
            own_n[at] = own_n[at] + kn
            own_d[at] = own_d[at] + kd
    return num - own_n, den - own_d


def voxel_takes(denL, den, min_coverage):
    """the voxel takes part in the prediction: enough left-out coverage, and more of it than the rounding noise of den_v"""
    return (denL > np.float64(min_coverage)) & (denL > den * np.float64(LEAVE_OUT_FLOOR))


def left_out_value(numL, denL):
    """U: the left-out stack's voxel, kept in fp64"""
    return numL / denL


def segments(groups, m):
    """``groups`` as ``align_group.group_offsets`` takes them, None: every target its own group -> the (G + 1) offsets"""
    return np.arange(m + 1, dtype=np.int64) if groups is None else np.asarray(ag.group_offsets(groups, m), np.int64)


def leave_out_sums_on_host(targets, maps, shape, spacing, *, groups=None, thickness=None, weights=None, intensity=None, min_coverage=0.0, own=None, members=None,
                           sums=None, takes=None, value=None, scatter=None, trace=None):
    """-> (N, D (m, th tw) float64, num, den (n, H, W) float64, TargetRecords): the two sums of the rule per target pixel and per voxel.  The keywords
    ``own`` .. ``scatter`` replace one piece of the rule (tests).  ``trace``: a dict that receives what a test needs to bound the distance to the chain of
    fusions and projections -- ``floored``: the (voxel, target) pairs that the floor alone excludes; ``umax``, ``cancel`` (m, th tw): per pixel the largest
    |U| and the largest (sum |k sn| + |U| den_v) / denL over its voxels"""
    own, members, sums, takes = own or own_terms, members or members_left_out, sums or left_out_sums, takes or voxel_takes
    value, scatter = value or left_out_value, scatter or fuse.scatter
    tg = np.ascontiguousarray(targets, dtype=np.float32)
    m, th, tw = tg.shape
    n, H, W = (int(s) for s in shape)
    wt = np.ones(tg.shape, np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    spacing = np.float64(spacing)
    r = fuse.target_records(maps, intensity, spacing, spacing if thickness is None else thickness)
    offsets = segments(groups, m)
    everywhere = np.ones((n, H, W), bool)

    def taps_of(q):
        return None if r.flags[q] else fuse.voxel_taps(r, q, everywhere, (n, H, W), (th, tw), spacing)

    num, den = np.zeros((n, H, W), np.float64), np.zeros((n, H, W), np.float64)
    absn = np.zeros((n, H, W), np.float64)
    N, D = np.zeros((m, th * tw), np.float64), np.zeros((m, th * tw), np.float64)
    if trace is not None:
        trace.update(floored=0, umax=np.zeros((m, th * tw)), cancel=np.zeros((m, th * tw)))
    with np.errstate(all="ignore"):
        for q in range(m):  # pass 1: msiren_fuse_targets' sums
            taps = taps_of(q)
            if taps is not None:
                kn, kd = own(r, q, tg[q].ravel(), wt[q].ravel(), taps)
                num[taps[0]] = num[taps[0]] + kn
                den[taps[0]] = den[taps[0]] + kd
                if trace is not None:
                    absn[taps[0]] = absn[taps[0]] + np.abs(kn)
        for lo, hi in zip(offsets[:-1], offsets[1:]):  # pass 2
            lo, hi = int(lo), int(hi)
            taps, terms, left = {}, {}, {}
            for q in range(lo, hi):
                taps[q] = taps_of(q)
                if taps[q] is not None:
                    terms[q] = (taps[q][0],) + tuple(own(r, q, tg[q].ravel(), wt[q].ravel(), taps[q]))
            for q in range(lo, hi):
                if taps[q] is None:
                    continue
                who = tuple(members(lo, hi, q))
                if who not in left:
                    numL, denL = sums(num, den, terms, who)
                    left[who] = (takes(denL, den, min_coverage), value(numL, denL), denL)
                take, U, denL = left[who]
                at, k, pixel, beta = taps[q]
                keep = take[at]
                at = tuple(x[keep] for x in at)
                tn, td = fuse.tap_terms(k[keep][:, None], beta[keep], U[at][:, None])
                scatter(N[q], pixel[keep], tn)
                scatter(D[q], pixel[keep], td)
                if trace is not None:
                    trace["floored"] += int((~keep & (denL[taps[q][0]] > np.float64(min_coverage))).sum())
                    touched = beta[keep] > 0
                    for name, per_voxel in (("umax", np.abs(U[at])), ("cancel", (absn[at] + np.abs(U[at]) * den[at]) / denL[at])):
                        np.maximum.at(trace[name][q], pixel[keep][touched], np.broadcast_to(per_voxel[:, None], touched.shape)[touched])
    return N, D, num, den, r


def leave_out_on_host(targets, maps, shape, spacing, *, groups=None, thickness=None, weights=None, intensity=None, min_coverage=0.0, **pieces):
    """The normative restatement of msiren_leave_out_targets -> LeaveOutResult (every optional output given).  targets (m, th, tw), maps (m, 9), shape =
    (n, H, W); ``groups``: the (G + 1) offsets or the G sizes of groups of consecutive targets, None: every target on its own; ``thickness`` None:
    ``spacing``; weights (m, th, tw) or None (all 1); intensity (m, 2) or None ((1, 0)).  ``pieces``: ``leave_out_sums_on_host``'s replaceable parts."""
    tg = np.ascontiguousarray(targets, dtype=np.float32)
    m, th, tw = tg.shape
    N, D, num, den, r = leave_out_sums_on_host(tg, maps, shape, spacing, groups=groups, thickness=thickness, weights=weights, intensity=intensity,
                                               min_coverage=min_coverage, **pieces)
    simulated = np.full((m, th, tw), np.nan, np.float32)
    with np.errstate(all="ignore"):
        for q in range(m):
            if not r.flags[q]:
                v = fuse.apply_intensity(N[q] / D[q], r.g[q], r.bias[q]).astype(np.float32)
                simulated[q] = np.where(D[q] > np.float64(min_coverage), v, np.float32(np.nan)).reshape(th, tw)
        volume = np.where(den > np.float64(min_coverage), (num / den).astype(np.float32), np.float32(np.nan)).astype(np.float32)
    residual, stats = fuse.project_stats_on_host(tg, simulated, weights)
    return LeaveOutResult(simulated, D.astype(np.float32).reshape(m, th, tw), residual, stats, r.flags, volume, den.astype(np.float32))


def leave_out_chain_on_host(targets, maps, shape, spacing, *, groups=None, thickness=None, weights=None, intensity=None, min_coverage=0.0):
    """What the call replaces, for tests and tools: per group one ``fuse_on_host`` of the targets outside it and one ``project_on_host`` of its own ->
    (simulated, coverage) (m, th, tw) float32.  It differs from the rule by the float32 rounding of the intermediate stack."""
    tg = np.ascontiguousarray(targets, dtype=np.float32)
    mp = np.ascontiguousarray(maps, dtype=np.float32).reshape(-1, 9)
    m, th, tw = tg.shape
    sim, cov = np.full(tg.shape, np.nan, np.float32), np.zeros(tg.shape, np.float32)
    part = lambda x, keep: None if x is None else np.asarray(x)[keep]  # noqa: E731
    offsets = segments(groups, m)
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        rest = np.ones(m, bool)
        rest[lo:hi] = False
        stack = fuse.fuse_on_host(tg[rest], mp[rest], shape, spacing, thickness=thickness, weights=part(weights, rest), intensity=part(intensity, rest),
                                  min_coverage=min_coverage)
        p = fuse.project_on_host(stack.volume, mp[lo:hi], (th, tw), spacing, thickness=thickness, intensity=part(intensity, slice(lo, hi)), min_coverage=min_coverage)
        sim[lo:hi], cov[lo:hi] = p.simulated, p.coverage
    return sim, cov
