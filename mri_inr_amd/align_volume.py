"""Helpers for ``ModulatedSiren.align_volume_cost`` and ``align_volume_solve`` / ``align_volume_solve_rigid``: the 3 x 3
maps target slices are read under in a stack taken as a volume, the call's packed sums, a Gauss-Newton step on them, and the step rule of
msiren_align_volume_solve restated operation by operation (``lm_step_v``, ``solve_on_host_v``); below them the same for the weighted,
gain/bias-compensated forms ``align_volume_cost_w`` / ``align_volume_solve_w`` / ``align_volume_solve_rigid_w`` (section 5.14: ``lm_step_vw``,
``solve_on_host_vw``).  Pure numpy; the step rules in plain Python floats.

A map is nine float32 numbers (z0, z1, tz, y0, y1, ty, x0, x1, tx): pixel (i, j) of the target lattice is read at
    Z = ((z0 i) + (z1 j)) + tz      Y = ((y0 i) + (y1 j)) + ty      X = ((x0 i) + (x1 j)) + tx
Z in slice units, (Y, X) in reconstruction pixel coordinates, in fp32 with every operation rounded on its own -- what the kernels compute, bit
for bit."""
import collections

import numpy as np

from .align import AFFINE, INF, NO_OVERLAP, RIGID, SINGULAR, _f32, ldl_solve, lm_decide  # noqa: F401  (the modes and flags are section 5.11's)

SUMS_V = 56  # count, cost, dcost[9], jtj packed upper triangle row-major [45]
IDENTITY_V = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0)  # the lattice on slice 0
_IU9 = np.triu_indices(9)

AlignResultV = collections.namedtuple("AlignResultV", "count cost grad jtj warped wgrad")
AlignResultV.__doc__ = """count (m,) int64 valid pixels, cost (m,) the sum of squared differences over them, grad (m, 9) its gradient over
(z0, z1, tz, y0, y1, ty, x0, x1, tx), jtj (m, 9, 9) the Gauss-Newton matrix (symmetric); warped (m, th, tw) / wgrad (3, m, th, tw) or None."""


def map_points3(map_row, shape):
    """One map (9,) on the lattice ``shape = (th, tw)`` -> (th * tw, 3) float32 points (Z, Y, X), row i * tw + j: the fp32 rule above."""
    a = np.asarray(map_row, dtype=np.float32)
    if a.shape != (9,):
        raise ValueError(f"expected one map of 9 numbers, got {a.shape}")
    th, tw = (int(x) for x in shape)
    if th < 0 or tw < 0:
        raise ValueError(f"shape must be non-negative, got {shape}")
    i = np.arange(th, dtype=np.float32)[:, None]
    j = np.arange(tw, dtype=np.float32)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        rows = [((a[3 * r] * i) + (a[3 * r + 1] * j)) + a[3 * r + 2] for r in range(3)]
    assert all(x.dtype == np.float32 for x in rows)
    return np.stack(rows, axis=-1).reshape(th * tw, 3)


def unpack_v(sums, warped=None, wgrad=None):
    """sums (m, 56) float64 as msiren_align_volume writes them -> AlignResultV (jtj unpacked to symmetric (m, 9, 9))"""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] != SUMS_V:
        raise ValueError(f"expected sums of shape (m, {SUMS_V}), got {sums.shape}")
    m = len(sums)
    jtj = np.zeros((m, 9, 9), np.float64)
    jtj[:, _IU9[0], _IU9[1]] = sums[:, 11:]
    jtj[:, _IU9[1], _IU9[0]] = sums[:, 11:]
    return AlignResultV(sums[:, 0].astype(np.int64), sums[:, 1].copy(), sums[:, 2:11].copy(), jtj, warped, wgrad)


def gauss_newton_step_v(result, damping=0.0):
    """(m, 9) float64: per target the solution of (JtJ + damping diag(JtJ)) delta = -grad / 2.  A target with fewer than nine valid pixels, or
    a singular system, gives a zero step."""
    m = len(result.count)
    step = np.zeros((m, 9), np.float64)
    for q in range(m):
        if result.count[q] < 9:
            continue
        A = result.jtj[q] + float(damping) * np.diag(np.diag(result.jtj[q]))
        try:
            step[q] = np.linalg.solve(A, -0.5 * result.grad[q])
        except np.linalg.LinAlgError:
            pass
    return step


# ---- msiren_align_volume_solve's step rule, one target, in Python floats: fp64 + - * / one at a time, no fused operation,
# every sum in the order written -- what align_volume_step_kernel computes, bit for bit.  No numpy arithmetic below.
SolveOptionsV = collections.namedtuple("SolveOptionsV", "mode iterations damping down up lam_min lam_max spacing", defaults=(AFFINE, 12, 1e-3, 0.1, 10.0, 1e-9, 1e9, 1.0))
SolveResultV = collections.namedtuple("SolveResultV", "maps rotation shift accepted mean_first mean_best count damping flags trace")
SolveResultV.__doc__ = """maps (m, 9) float32 the best map of every target; rotation (m, 3, 3) and shift (m, 3) of the best rigid state (None in
affine mode); accepted (m,) int64 steps accepted after the first evaluation; mean_first / mean_best (m,) cost / count at the input and at the best
map (+inf: fewer valid pixels than solved parameters); count (m,) int64 valid pixels at the best map; damping (m,) the final lambda; flags (m,)
int64 (SINGULAR: the last proposal was zero, NO_OVERLAP: mean_first is +inf); trace (iterations, m, 11) or None: per evaluation the trial map,
cost, count."""


def solved_parameters_v(o):
    """P: affine 9, rigid 6"""
    return 6 if o.mode == RIGID else 9


def _rot_apply(R, x):
    """Rot (9, row-major) x (3): each row ((r0 x0) + (r1 x1)) + r2 x2"""
    return [((R[3 * r] * x[0]) + (R[3 * r + 1] * x[1])) + (R[3 * r + 2] * x[2]) for r in range(3)]


def rigid_vectors3(state, plane):
    """-> (v_i, v_j, v_o) = (Rot e_i, Rot e_j, Rot (o - c)) of the state (Rot 9, u 3) on the plane (e_i, e_j, o, c)"""
    R = state[:9]
    oc = [plane[6 + a] - plane[9 + a] for a in range(3)]
    return _rot_apply(R, plane[0:3]), _rot_apply(R, plane[3:6]), _rot_apply(R, oc)


def rigid_map3(state, plane, spacing):
    """One state on one plane, in Python floats -> the nine float32 entries (as floats): row r = (v_i[r], v_j[r], (v_o[r] + c[r]) + u[r]), the Z row
    (r = 0) divided by ``spacing`` before rounding"""
    vi, vj, vo = rigid_vectors3(state, plane)
    out = []
    for r in range(3):
        t = (vo[r] + plane[9 + r]) + state[9 + r]
        row = [vi[r], vj[r], t]
        out += [_f32(x / spacing) for x in row] if r == 0 else [_f32(x) for x in row]
    return out


def rigid_maps3(rotation, shift, planes, spacing, dtype=np.float32):
    """rotation (m, 3, 3), shift (m, 3), planes (m, 12) = (e_i, e_j, o, c) -> maps (m, 9): a point p of the nominal plane moves to
    Rot (p - c) + c + shift in physical pixels, slices ``spacing`` pixels apart.  fp64, rounded once (``dtype=np.float64``: not rounded, the
    expressions evaluated without the final rounding)."""
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, 12)
    m = len(planes)
    rot = np.broadcast_to(np.asarray(rotation, dtype=np.float64), (m, 3, 3)).reshape(m, 9)
    sh = np.broadcast_to(np.asarray(shift, dtype=np.float64), (m, 3))
    out = np.empty((m, 9), np.float64)
    sp = float(spacing)
    for q in range(m):
        st, pl = [float(x) for x in rot[q]] + [float(x) for x in sh[q]], [float(x) for x in planes[q]]
        if dtype == np.float64:
            vi, vj, vo = rigid_vectors3(st, pl)
            for r in range(3):
                row = [vi[r], vj[r], (vo[r] + pl[9 + r]) + st[9 + r]]
                out[q, 3 * r:3 * r + 3] = [x / sp for x in row] if r == 0 else row
        else:
            out[q] = rigid_map3(st, pl, sp)
    return out.astype(dtype)


def rigid_jacobian3(state, plane, spacing):
    """B (9 x 6): d map / d (w0, w1, w2, u0, u1, u2) at the state, for Rot' = exp([w]x) Rot: B[3 r + col][k] = (e_k x v_col)[r] with v_col = v_i,
    v_j, v_o; B[3 r + 2][3 + k] = [r == k]; the rows of Z (r = 0) divided by spacing.  With e_k a unit vector the cross product is
    e_0 x v = (0, -v2, v1), e_1 x v = (v2, 0, -v0), e_2 x v = (-v1, v0, 0): those entries, the others 0.0."""
    B = [[0.0] * 6 for _ in range(9)]
    for col, v in enumerate(rigid_vectors3(state, plane)):
        B[col][1], B[col][2] = v[2] / spacing, (-v[1]) / spacing
        B[3 + col][0], B[3 + col][2] = -v[2], v[0]
        B[6 + col][0], B[6 + col][1] = v[1], -v[0]
    B[2][3], B[5][4], B[8][5] = 1.0 / spacing, 1.0, 1.0
    return B


def cayley3(a):
    """Cay (3 x 3, rows) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a): the rotation by 2 atan|a| about a, exact up to rounding, no trigonometry"""
    a0, a1, a2 = a
    aa = ((a0 * a0) + (a1 * a1)) + (a2 * a2)
    den, sc = 1.0 + aa, 1.0 - aa
    t0, t1, t2 = 2.0 * a0, 2.0 * a1, 2.0 * a2
    return [[(sc + (t0 * a0)) / den, ((t0 * a1) - t2) / den, ((t0 * a2) + t1) / den],
            [((t1 * a0) + t2) / den, (sc + (t1 * a1)) / den, ((t1 * a2) - t0) / den],
            [((t2 * a0) - t1) / den, ((t2 * a1) + t0) / den, (sc + (t2 * a2)) / den]]


def project_rigid(H, g, B, N, Q):
    """The system over the rigid parameters from the one over the map's: H (at least N x N, symmetric), g (at least N), B (N x Q) ->
    (t (Q), HQ (Q x Q, the lower triangle k >= r filled, which ldl_solve reads)): t[k] = sum_a B[a][k] g[a], HQ = B^T (H B) column by column,
    T[., r] = H B[., r], then HQ[k][r] = sum_a B[a][k] T[a][r] -- the expressions of align_volume_step_kernel, align_volume_step_w_kernel (rigid
    mode) and align_group_project_kernel, undamped"""
    t = [0.0] * Q
    for k in range(Q):
        x = 0.0
        for a in range(N):
            x = x + B[a][k] * g[a]
        t[k] = x
    HQ = [[0.0] * Q for _ in range(Q)]
    for r in range(Q):
        Tc = [0.0] * N
        for a in range(N):
            x = 0.0
            for b in range(N):
                x = x + H[a][b] * B[b][r]
            Tc[a] = x
        for k in range(r, Q):
            x = 0.0
            for a in range(N):
                x = x + B[a][k] * Tc[a]
            HQ[k][r] = x
    return t, HQ


def cayley_update(rb, d):
    """the rigid state (Rot 9, u 3) behind the step d (w 3, u 3, ...): Rot' = Cay(w / 2) Rot, u' = u + d[3:6] -- align_cayley_update's expressions"""
    Cay = cayley3([d[0] / 2.0, d[1] / 2.0, d[2] / 2.0])
    rt = [0.0] * 12
    for r in range(3):
        for c in range(3):
            rt[3 * r + c] = ((Cay[r][0] * rb[c]) + (Cay[r][1] * rb[3 + c])) + (Cay[r][2] * rb[6 + c])
    for a in range(3):
        rt[9 + a] = rb[9 + a] + d[3 + a]
    return rt


def lm_init_v(o, map_in=None, rigid_in=None, plane=None):
    """the state of one target before its first evaluation: a dict (trial, best, rigid_trial, rigid_best, plane, sums, mean_best, mean_first, lam,
    accepted, flags).  Affine: map_in (9); rigid: rigid_in (Rot 9, u 3) on plane (12), the trial map formed from it."""
    st = dict(sums=[0.0] * SUMS_V, mean_best=INF, mean_first=INF, lam=float(o.damping), accepted=0, flags=0, plane=None)
    if o.mode == RIGID:
        r = [float(x) for x in rigid_in]
        st["plane"] = [float(x) for x in plane]
        st["rigid_trial"], st["rigid_best"] = r, list(r)
        st["trial"] = rigid_map3(r, st["plane"], float(o.spacing))
    else:
        st["rigid_trial"] = st["rigid_best"] = [0.0] * 12
        st["trial"] = [_f32(x) for x in map_in]
    st["best"] = list(st["trial"])
    return st


def lm_step_v(st, sums, k, o):
    """One target after evaluation k: ``sums`` (56) are msiren_align_volume's at st["trial"].  Accept or reject, then propose the next trial from
    the best map.  ``st`` is updated in place and returned."""
    sums = [float(x) for x in sums]
    P = solved_parameters_v(o)
    mean = sums[1] / sums[0] if sums[0] >= float(P) else INF
    accept, counted, st["lam"] = lm_decide(k, mean, st["mean_best"], st["lam"], o)
    if accept:
        st["best"], st["rigid_best"], st["sums"], st["mean_best"] = list(st["trial"]), list(st["rigid_trial"]), sums, mean
        if k == 0:
            st["mean_first"] = mean
        if counted:
            st["accepted"] += 1
    lam, bs = st["lam"], st["sums"]
    g = bs[2:11]
    H = [[0.0] * 9 for _ in range(9)]
    s = 11
    for a in range(9):
        for b in range(a, 9):
            H[a][b] = H[b][a] = bs[s]
            s += 1
    if o.mode == AFFINE:
        A = [row[:] for row in H]
        for a in range(9):
            A[a][a] = H[a][a] + lam * H[a][a]
        d, ok = ldl_solve(A, [-0.5 * g[a] for a in range(9)], 9)
        st["trial"] = [_f32(st["best"][a] + d[a]) for a in range(9)]
    else:
        rb, pl, sp = st["rigid_best"], st["plane"], float(o.spacing)
        B = rigid_jacobian3(rb, pl, sp)
        g6, A = project_rigid(H, g, B, 9, 6)
        for p in range(6):
            A[p][p] = A[p][p] + lam * A[p][p]
        d, ok = ldl_solve(A, [-0.5 * g6[p] for p in range(6)], 6)
        rt = cayley_update(rb, d)
        st["rigid_trial"] = rt
        st["trial"] = rigid_map3(rt, pl, sp)
    st["flags"] = (0 if ok else SINGULAR) | (NO_OVERLAP if st["mean_first"] == INF else 0)
    return st


def solve_on_host_v(cost_fn, m, *, maps=None, rigid=None, planes=None, options=SolveOptionsV(), trace=False):
    """msiren_align_volume_solve's loop around any ``cost_fn(maps (m, 9) float32) -> sums (m, 56)``: ``options.iterations`` evaluations,
    ``lm_step_v`` per target after each.  Affine: ``maps`` (m, 9); rigid: ``rigid`` (m, 12) = (Rot, u) on ``planes`` (m, 12).
    -> (SolveResultV, rigid (m, 12) float64 best states)"""
    o = options
    st = [lm_init_v(o, None if maps is None else maps[q], None if rigid is None else rigid[q], None if planes is None else planes[q]) for q in range(m)]
    tr = np.zeros((o.iterations, m, 11), np.float64) if trace else None
    for k in range(o.iterations):
        trial = np.array([x["trial"] for x in st], np.float32).reshape(m, 9)
        sums = np.asarray(cost_fn(trial), np.float64).reshape(m, SUMS_V)
        if trace:
            tr[k, :, :9], tr[k, :, 9], tr[k, :, 10] = trial, sums[:, 1], sums[:, 0]
        for q in range(m):
            lm_step_v(st[q], sums[q], k, o)
    rb = np.array([x["rigid_best"] for x in st], np.float64).reshape(m, 12)
    return solve_result_v(np.array([x["best"] for x in st], np.float32).reshape(m, 9), rb if o.mode == RIGID else None,
                          np.array([[x["accepted"], x["mean_first"], x["mean_best"], x["sums"][0], x["lam"], x["flags"]] for x in st], np.float64).reshape(m, 6), tr), rb


def solve_result_v(maps, rigid, report, trace):
    """what msiren_align_volume_solve writes -> SolveResultV"""
    rotation = shift = None
    if rigid is not None:
        rotation, shift = rigid[:, :9].reshape(-1, 3, 3).copy(), rigid[:, 9:12].copy()
    return SolveResultV(maps, rotation, shift, report[:, 0].astype(np.int64), report[:, 1].copy(), report[:, 2].copy(), report[:, 3].astype(np.int64),
                        report[:, 4].copy(), report[:, 5].astype(np.int64), trace)


# ---- weighted, gain/bias-compensated alignment to the volume (msiren_align_volume_w, msiren_align_volume_solve_w) ------------
# Parameter order: the map's nine (z0, z1, tz, y0, y1, ty, x0, x1, tx), then g, b: the model of a target pixel is g R + b, every pixel carries a
# weight w, every TARGET its own (g, b).
SUMS_VW = 80  # count, wsum, cost, dcost[11], jtj packed upper triangle row-major [66]
FIXED, ESTIMATE = 0, 1
_IU11 = np.triu_indices(11)

AlignResultVW = collections.namedtuple("AlignResultVW", "count wsum cost grad jtj warped wgrad")
AlignResultVW.__doc__ = """count (m,) int64 valid pixels (finite, weight > 0), wsum (m,) the sum of their weights, cost (m,) sum w (g R + b - T)^2, grad
(m, 11) its gradient over (z0, z1, tz, y0, y1, ty, x0, x1, tx, g, b), jtj (m, 11, 11) the weighted Gauss-Newton matrix (symmetric); warped
(m, th, tw) / wgrad (3, m, th, tw) (R, gZ, gY, gX before gain and bias) or None."""

SolveOptionsVW = collections.namedtuple("SolveOptionsVW", "mode iterations damping down up lam_min lam_max spacing intensity_mode",
                                        defaults=(AFFINE, 12, 1e-3, 0.1, 10.0, 1e-9, 1e9, 1.0, ESTIMATE))
SolveResultVW = collections.namedtuple("SolveResultVW", "maps rotation shift accepted mean_first mean_best count damping flags trace intensity wsum")
SolveResultVW.__doc__ = """SolveResultV's fields (mean_* = cost / wsum; +inf: fewer valid pixels than solved parameters; trace (iterations, m, 14) or None:
per evaluation the trial map, the trial g, b, cost, count, wsum), then intensity (m, 2) float32 the best (g, b) and wsum (m,) at the best map."""


def unpack_vw(sums, warped=None, wgrad=None):
    """sums (m, 80) float64 as msiren_align_volume_w writes them -> AlignResultVW (jtj unpacked to symmetric (m, 11, 11))"""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] != SUMS_VW:
        raise ValueError(f"expected sums of shape (m, {SUMS_VW}), got {sums.shape}")
    m = len(sums)
    jtj = np.zeros((m, 11, 11), np.float64)
    jtj[:, _IU11[0], _IU11[1]] = sums[:, 14:]
    jtj[:, _IU11[1], _IU11[0]] = sums[:, 14:]
    return AlignResultVW(sums[:, 0].astype(np.int64), sums[:, 1].copy(), sums[:, 2].copy(), sums[:, 3:14].copy(), jtj, warped, wgrad)


def gauss_newton_step_vw(result, damping=0.0, estimate_intensity=True):
    """(m, 11) float64: per target the solution of (JtJ + damping diag(JtJ)) delta = -grad / 2 over all 11 parameters, or over the nine of the map
    (the last two entries zero).  A target with fewer valid pixels than parameters, or a singular system, gives a zero step."""
    m, P = len(result.count), 11 if estimate_intensity else 9
    step = np.zeros((m, 11), np.float64)
    for q in range(m):
        if result.count[q] < P:
            continue
        H = result.jtj[q][:P, :P]
        try:
            step[q, :P] = np.linalg.solve(H + float(damping) * np.diag(np.diag(H)), -0.5 * result.grad[q][:P])
        except np.linalg.LinAlgError:
            pass
    return step


# msiren_align_volume_solve_w's step rule, one target, in Python floats as lm_step_v above -- what align_volume_step_w_kernel computes, bit for bit.
def solved_parameters_vw(o):
    """P: affine 9 / rigid 6, and the two of the intensity where they are estimated"""
    return (6 if o.mode == RIGID else 9) + (2 if o.intensity_mode == ESTIMATE else 0)


def lm_mean_vw(sums, P):
    """cost / wsum where at least P pixels are valid, +inf otherwise"""
    return sums[2] / sums[1] if sums[0] >= float(P) else INF


def intensity_update_vw(gb, dg, db):
    """(g', b') as float32 from the best (g, b) and the step's last two entries"""
    return [_f32(gb[0] + dg), _f32(gb[1] + db)]


def rigid_jacobian3_w(state, plane, spacing):
    """B (11 x 8): rigid_jacobian3's 9 x 6 block, then d (g, b) / d (g, b) = 1, every other entry 0.0"""
    B9 = rigid_jacobian3(state, plane, spacing)
    B = [[0.0] * 8 for _ in range(11)]
    for a in range(9):
        for k in range(6):
            B[a][k] = B9[a][k]
    B[9][6] = 1.0
    B[10][7] = 1.0
    return B


def lm_init_vw(o, map_in=None, rigid_in=None, plane=None, intensity_in=None):
    """lm_init_v's state with gb_trial, gb_best (float32 as floats; None: (1, 0)) and sums of 80"""
    st = lm_init_v(o, map_in, rigid_in, plane)
    st["sums"] = [0.0] * SUMS_VW
    st["gb_trial"] = [1.0, 0.0] if intensity_in is None else [_f32(x) for x in intensity_in]
    st["gb_best"] = list(st["gb_trial"])
    return st


def lm_step_vw(st, sums, k, o):
    """One target after evaluation k: ``sums`` (80) are msiren_align_volume_w's at (st["trial"], st["gb_trial"]).  Accept or reject, then propose
    the next trial from the best state.  ``st`` is updated in place and returned."""
    sums = [float(x) for x in sums]
    est = o.intensity_mode == ESTIMATE
    mean = lm_mean_vw(sums, solved_parameters_vw(o))
    accept, counted, st["lam"] = lm_decide(k, mean, st["mean_best"], st["lam"], o)
    if accept:
        st["best"], st["rigid_best"], st["gb_best"], st["sums"], st["mean_best"] = list(st["trial"]), list(st["rigid_trial"]), list(st["gb_trial"]), sums, mean
        if k == 0:
            st["mean_first"] = mean
        if counted:
            st["accepted"] += 1
    lam, bs = st["lam"], st["sums"]
    N = 11 if est else 9  # the leading block of the 11 parameters the proposal reads
    g = bs[3:14]
    H = [[0.0] * 11 for _ in range(11)]
    s = 14
    for a in range(11):
        for b in range(a, 11):
            H[a][b] = H[b][a] = bs[s]
            s += 1
    if o.mode == AFFINE:
        A = [row[:N] for row in H[:N]]
        for a in range(N):
            A[a][a] = H[a][a] + lam * H[a][a]
        d, ok = ldl_solve(A, [-0.5 * g[a] for a in range(N)], N)
        st["trial"] = [_f32(st["best"][a] + d[a]) for a in range(9)]
        dg, db = (d[9], d[10]) if est else (0.0, 0.0)
    else:
        rb, pl, sp = st["rigid_best"], st["plane"], float(o.spacing)
        Q = 8 if est else 6
        B = rigid_jacobian3_w(rb, pl, sp) if est else rigid_jacobian3(rb, pl, sp)
        gq, A = project_rigid(H, g, B, N, Q)
        for p in range(Q):
            A[p][p] = A[p][p] + lam * A[p][p]
        d, ok = ldl_solve(A, [-0.5 * gq[p] for p in range(Q)], Q)
        rt = cayley_update(rb, d)
        st["rigid_trial"] = rt
        st["trial"] = rigid_map3(rt, pl, sp)
        dg, db = (d[6], d[7]) if est else (0.0, 0.0)
    st["gb_trial"] = intensity_update_vw(st["gb_best"], dg, db) if est else list(st["gb_best"])
    st["flags"] = (0 if ok else SINGULAR) | (NO_OVERLAP if st["mean_first"] == INF else 0)
    return st


def solve_on_host_vw(cost_fn, m, *, maps=None, rigid=None, planes=None, intensity=None, options=SolveOptionsVW(), trace=False):
    """msiren_align_volume_solve_w's loop around any ``cost_fn(maps (m, 9) float32, intensity (m, 2) float32) -> sums (m, 80)``:
    ``options.iterations`` evaluations, ``lm_step_vw`` per target after each.  -> (SolveResultVW, rigid (m, 12) float64 best states)"""
    o = options
    st = [lm_init_vw(o, None if maps is None else maps[q], None if rigid is None else rigid[q], None if planes is None else planes[q],
                     None if intensity is None else intensity[q]) for q in range(m)]
    tr = np.zeros((o.iterations, m, 14), np.float64) if trace else None
    for k in range(o.iterations):
        trial = np.array([x["trial"] for x in st], np.float32).reshape(m, 9)
        gb = np.array([x["gb_trial"] for x in st], np.float32).reshape(m, 2)
        sums = np.asarray(cost_fn(trial, gb), np.float64).reshape(m, SUMS_VW)
        if trace:
            tr[k, :, :9], tr[k, :, 9:11], tr[k, :, 11], tr[k, :, 12], tr[k, :, 13] = trial, gb, sums[:, 2], sums[:, 0], sums[:, 1]
        for q in range(m):
            lm_step_vw(st[q], sums[q], k, o)
    rb = np.array([x["rigid_best"] for x in st], np.float64).reshape(m, 12)
    return solve_result_vw(np.array([x["best"] for x in st], np.float32).reshape(m, 9), np.array([x["gb_best"] for x in st], np.float32).reshape(m, 2),
                           rb if o.mode == RIGID else None, report_vw(st), tr), rb


def report_vw(states):
    """the (m, 7) report of msiren_align_volume_solve_w from the states of lm_step_vw"""
    return np.array([[x["accepted"], x["mean_first"], x["mean_best"], x["sums"][0], x["sums"][1], x["lam"], x["flags"]] for x in states], np.float64).reshape(len(states), 7)


def solve_result_vw(maps, intensity, rigid, report, trace):
    """what msiren_align_volume_solve_w writes -> SolveResultVW"""
    rotation = shift = None
    if rigid is not None:
        rotation, shift = rigid[:, :9].reshape(-1, 3, 3).copy(), rigid[:, 9:12].copy()
    return SolveResultVW(maps, rotation, shift, report[:, 0].astype(np.int64), report[:, 1].copy(), report[:, 2].copy(), report[:, 3].astype(np.int64),
                         report[:, 5].copy(), report[:, 6].astype(np.int64), trace, intensity, report[:, 4].copy())
