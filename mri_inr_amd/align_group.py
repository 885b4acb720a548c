"""Helpers for ``ModulatedSiren.align_volume_solve_group``: groups of consecutive targets under one shared rigid motion per
group, every target with its own plane, weights and intensity (g, b).  The step rule of msiren_align_volume_solve_group restated operation by
operation (``lm_init_g``, ``lm_step_g``, ``solve_on_host_g``) on section 5.14's 80 sums: plain Python floats, fp64 + - * / one at a time, no fused
operation, every sum in the order written -- what the kernels of csrc/align_group.hip.h compute, bit for bit.  No numpy arithmetic in the rule.

Every sum over the members of a group starts with the first member's term (not with 0.0) and adds the others in ascending index, so a group of one
target with the intensity fixed reproduces ``align_volume.lm_step_vw``'s arithmetic.

One PHYSICAL motion per group needs the same centre c in every member's plane (e_i, e_j, o, c): the state (Rot, u) moves a point p of member q to
Rot (p - c_q) + c_q + u.  The rule does not check it."""
import collections

import numpy as np

from .align import INF, NO_OVERLAP, RIGID, SINGULAR, _f32, ldl_solve, lm_decide  # noqa: F401
from .align_volume import (ESTIMATE, FIXED, SUMS_VW, cayley3, cayley_update, intensity_update_vw, project_rigid, rigid_jacobian3,  # noqa: F401
                           rigid_jacobian3_w, rigid_map3)

SolveOptionsG = collections.namedtuple("SolveOptionsG", "iterations damping down up lam_min lam_max spacing intensity_mode",
                                       defaults=(12, 1e-3, 0.1, 10.0, 1e-9, 1e9, 1.0, ESTIMATE))
SolveResultG = collections.namedtuple("SolveResultG", "maps intensity count wsum cost rotation shift accepted mean_first mean_best damping flags trace")
SolveResultG.__doc__ = """Per target: maps (m, 9) float32 the best map, intensity (m, 2) float32 the best (g, b), count (m,) int64 / wsum (m,) / cost
(m,) of the target at the best state.  Per group: rotation (G, 3, 3) and shift (G, 3) of the best rigid state; accepted (G,) int64 steps accepted
after the first evaluation; mean_first / mean_best (G,) = sum cost / sum wsum over the members at the input and at the best state (+inf: fewer valid
pixels in the group than solved parameters); damping (G,) the final lambda; flags (G,) int64 (SINGULAR: the last 6 x 6 solve failed, the proposed
motion was zero; NO_OVERLAP: mean_first is +inf); trace (iterations, G, 15) or None: per evaluation the trial state (Rot 9, u 3), then E, C, W."""


def group_offsets(groups, m):
    """``groups``: the (G + 1) offsets (first 0, last m, strictly ascending) or a list of G positive sizes that add up to m -> the offsets as a list
    of ints.  A list that reads as valid offsets is taken as offsets."""
    g = [int(x) for x in np.asarray(groups).reshape(-1)]
    if len(g) >= 2 and g[0] == 0 and g[-1] == m and all(b > a for a, b in zip(g, g[1:])):
        return g
    if g and all(x > 0 for x in g) and sum(g) == m:
        out = [0]
        for x in g:
            out.append(out[-1] + x)
        return out
    raise ValueError(f"groups must be offsets from 0 to {m}, strictly ascending, or positive sizes that add up to {m}; got {g}")


def solved_parameters_g(o, size):
    """P of a group: the six of the motion, and two per member where the intensity is estimated"""
    return 6 + (2 * size if o.intensity_mode == ESTIMATE else 0)


def group_sum(terms):
    """the first term, then the others added in ascending index"""
    t = terms[0]
    for x in terms[1:]:
        t = t + x
    return t


def lm_init_g(o, group_start, rigid_in, planes, intensity_in=None):
    """The state before the first evaluation -> (groups, targets): per group a dict (lo, hi, rigid_trial, rigid_best, mean_best, mean_first, lam,
    accepted, flags), per target a dict (plane, trial, best, gb_trial, gb_best, sums).  rigid_in (G, 12) = (Rot, u), planes (m, 12)."""
    sp = float(o.spacing)
    gs, ts = [], []
    for y in range(len(group_start) - 1):
        r = [float(x) for x in rigid_in[y]]
        gs.append(dict(lo=int(group_start[y]), hi=int(group_start[y + 1]), rigid_trial=r, rigid_best=list(r), mean_best=INF, mean_first=INF, lam=float(o.damping),
                       accepted=0, flags=0))
        for q in range(gs[-1]["lo"], gs[-1]["hi"]):
            pl = [float(x) for x in planes[q]]
            trial = rigid_map3(r, pl, sp)
            gb = [1.0, 0.0] if intensity_in is None else [_f32(x) for x in intensity_in[q]]
            ts.append(dict(plane=pl, trial=trial, best=list(trial), gb_trial=gb, gb_best=list(gb), sums=[0.0] * SUMS_VW))
    return gs, ts


def project_member(bs, B, est):
    """One member's sums at the best state (80) and its B (11 x 8 estimated, 9 x 6 fixed) -> (t (Q), HQ (Q x Q, the lower triangle k >= r filled)):
    t[k] = sum_a B[a][k] g[a], HQ = B^T (H B), align_volume_step_w_kernel's expressions, undamped"""
    N, Q = (11, 8) if est else (9, 6)
    H = [[0.0] * 11 for _ in range(11)]
    s = 14
    for a in range(11):
        for b in range(a, 11):
            H[a][b] = H[b][a] = bs[s]
            s += 1
    return project_rigid(H, bs[3:14], B, N, Q)


def eliminate_member(t, HQ, count, lam):
    """One member's 2 x 2 intensity block, damped by lam, eliminated exactly -> (X (2 x 6) = D^-1 C, y (2) = D^-1 c, eliminates): D = HQ[6:8, 6:8],
    C = HQ[6:8, 0:6], c = -0.5 t[6:8].  A member with fewer than two valid pixels, or whose D does not factorise, does not eliminate: zeros."""
    D = [[HQ[6][6] + lam * HQ[6][6], 0.0], [HQ[7][6], HQ[7][7] + lam * HQ[7][7]]]
    X = [[0.0] * 6 for _ in range(2)]
    ok = True
    for k in range(6):
        x, ok = ldl_solve(D, [HQ[6][k], HQ[7][k]], 2)
        X[0][k], X[1][k] = x[0], x[1]
    y, ok = ldl_solve(D, [-0.5 * t[6], -0.5 * t[7]], 2)
    if not (count >= 2.0 and ok):
        return [[0.0] * 6 for _ in range(2)], [0.0, 0.0], False
    return X, y, True


def group_mean(sums, o):
    """the members' sums at one state (size x 80) -> (mean, E, C, W): mean = E / W where the group has at least P valid pixels, +inf otherwise"""
    C = group_sum([s[0] for s in sums])
    W = group_sum([s[1] for s in sums])
    E = group_sum([s[2] for s in sums])
    return (E / W if C >= float(solved_parameters_g(o, len(sums))) else INF), E, C, W


def member_jacobian(rb, planes, i, spacing, est):
    """B of member i of a group whose members lie on ``planes``, at the group's best state rb: 11 x 8 where the intensity is estimated, 9 x 6 fixed"""
    return rigid_jacobian3_w(rb, planes[i], spacing) if est else rigid_jacobian3(rb, planes[i], spacing)


def schur_apply(A, rhs, HQ, X, y):
    """A -= C^T X (its lower triangle), rhs -= C^T y for one eliminating member, C = HQ[6:8, 0:6]; in place"""
    for a in range(6):
        for b in range(a + 1):
            A[a][b] = A[a][b] - ((HQ[6][a] * X[0][b]) + (HQ[7][a] * X[1][b]))
        rhs[a] = rhs[a] - ((HQ[6][a] * y[0]) + (HQ[7][a] * y[1]))


def back_substitute(X, y, d):
    """(dg, db) = y - X d of one eliminating member"""
    out = []
    for i in range(2):
        x = 0.0
        for a in range(6):
            x = x + X[i][a] * d[a]
        out.append(y[i] - x)
    return out


def project_group(bests, planes, rb, lam, o):
    """step 2 for the members of one group: ``bests`` their sums at the best state -> the records [(t, HQ, X, y, eliminates)]"""
    est = o.intensity_mode == ESTIMATE
    rec = []
    for i, bs in enumerate(bests):
        tq, HQ = project_member(bs, member_jacobian(rb, planes, i, float(o.spacing), est), est)
        X, y, elim = eliminate_member(tq, HQ, bs[0], lam) if est else (None, None, False)
        rec.append((tq, HQ, X, y, elim))
    return rec


def solve_group(rec, lam):
    """step 3 on the records of one group -> (d (6), ok, [(dg, db) or None per member])"""
    A = [[0.0] * 6 for _ in range(6)]
    for a in range(6):
        for b in range(a + 1):
            A[a][b] = group_sum([r[1][a][b] for r in rec])
    tm = [group_sum([r[0][a] for r in rec]) for a in range(6)]
    for a in range(6):
        A[a][a] = A[a][a] + lam * A[a][a]
    rhs = [-0.5 * tm[a] for a in range(6)]
    for tq, HQ, X, y, elim in rec:  # the Schur complement of every eliminating member, in ascending order, behind the damping
        if elim:
            schur_apply(A, rhs, HQ, X, y)
    d, ok = ldl_solve(A, rhs, 6)
    return d, ok, [back_substitute(X, y, d) if elim else None for tq, HQ, X, y, elim in rec]


def lm_step_group(g, ts, sums, k, o):
    """One group after evaluation k: ``ts`` its members' states, ``sums`` (size, 80) msiren_align_volume_w's at their trials.  Decide on the group's
    mean, then propose the next trial from the best state.  Updated in place."""
    sums = [[float(x) for x in row] for row in sums]
    sp = float(o.spacing)
    # 1. decide
    mean = group_mean(sums, o)[0]
    accept, counted, g["lam"] = lm_decide(k, mean, g["mean_best"], g["lam"], o)
    if accept:
        for t, s in zip(ts, sums):
            t["best"], t["gb_best"], t["sums"] = list(t["trial"]), list(t["gb_trial"]), s
        g["rigid_best"], g["mean_best"] = list(g["rigid_trial"]), mean
        if k == 0:
            g["mean_first"] = mean
        if counted:
            g["accepted"] += 1
    lam, rb = g["lam"], g["rigid_best"]
    # 2. project, per member;  3. reduce and solve, per group
    d, ok, dgb = solve_group(project_group([t["sums"] for t in ts], [t["plane"] for t in ts], rb, lam, o), lam)
    # 4. propose
    rt = cayley_update(rb, d)
    g["rigid_trial"] = rt
    for t, x in zip(ts, dgb):
        t["trial"] = rigid_map3(rt, t["plane"], sp)
        t["gb_trial"] = list(t["gb_best"]) if x is None else intensity_update_vw(t["gb_best"], x[0], x[1])
    g["flags"] = (0 if ok else SINGULAR) | (NO_OVERLAP if g["mean_first"] == INF else 0)
    return g


def lm_step_g(gs, ts, sums, k, o):
    """Every group after evaluation k: ``sums`` (m, 80) at the targets' trials.  (gs, ts) are updated in place and returned."""
    for g in gs:
        lm_step_group(g, ts[g["lo"]:g["hi"]], sums[g["lo"]:g["hi"]], k, o)
    return gs, ts


def report_g(gs, ts):
    """-> (report (G, 7), target_report (m, 3)) of msiren_align_volume_solve_group from the states: accepted, mean_first, mean_best, C, W, lam, flags
    per group at the best state; count, wsum, cost per target"""
    rep = []
    for g in gs:
        mem = ts[g["lo"]:g["hi"]]
        rep.append([g["accepted"], g["mean_first"], g["mean_best"], group_sum([t["sums"][0] for t in mem]), group_sum([t["sums"][1] for t in mem]), g["lam"], g["flags"]])
    return np.array(rep, np.float64).reshape(len(gs), 7), np.array([t["sums"][:3] for t in ts], np.float64).reshape(len(ts), 3)


def solve_result_g(maps, intensity, rigid, report, target_report, trace):
    """what msiren_align_volume_solve_group writes -> SolveResultG"""
    return SolveResultG(maps, intensity, target_report[:, 0].astype(np.int64), target_report[:, 1].copy(), target_report[:, 2].copy(),
                        rigid[:, :9].reshape(-1, 3, 3).copy(), rigid[:, 9:12].copy(), report[:, 0].astype(np.int64), report[:, 1].copy(), report[:, 2].copy(),
                        report[:, 5].copy(), report[:, 6].astype(np.int64), trace)


def solve_on_host_g(cost_fn, group_start, *, rigid, planes, intensity=None, options=SolveOptionsG(), trace=False, step=None):
    """msiren_align_volume_solve_group's loop around any ``cost_fn(maps (m, 9) float32, intensity (m, 2) float32) -> sums (m, 80)``:
    ``options.iterations`` evaluations, ``lm_step_g`` after each (``step``: another rule with its signature).  rigid (G, 12), planes (m, 12).
    -> (SolveResultG, the final states (groups, targets))"""
    o, step = options, lm_step_g if step is None else step
    gs, ts = lm_init_g(o, group_start, rigid, planes, intensity)
    G, m = len(gs), len(ts)
    tr = np.zeros((o.iterations, G, 15), np.float64) if trace else None
    for k in range(o.iterations):
        trial = np.array([t["trial"] for t in ts], np.float32).reshape(m, 9)
        gb = np.array([t["gb_trial"] for t in ts], np.float32).reshape(m, 2)
        sums = np.asarray(cost_fn(trial, gb), np.float64).reshape(m, SUMS_VW)
        if trace:
            for y, g in enumerate(gs):
                tr[k, y, :12] = g["rigid_trial"]
                tr[k, y, 12:] = group_mean([[float(x) for x in row] for row in sums[g["lo"]:g["hi"]]], o)[1:]
        step(gs, ts, sums, k, o)
    rep, trep = report_g(gs, ts)
    res = solve_result_g(np.array([t["best"] for t in ts], np.float32).reshape(m, 9), np.array([t["gb_best"] for t in ts], np.float32).reshape(m, 2),
                         np.array([g["rigid_best"] for g in gs], np.float64).reshape(G, 12), rep, trep, tr)
    return res, (gs, ts)
