"""Helpers for ``ModulatedSiren.align_cost`` and ``align_solve`` (section 5.11): the affine maps slices are read
under, the call's packed sums, a Gauss-Newton step on them, and the Levenberg-Marquardt rule of msiren_align_solve restated operation by
operation (``lm_step``, ``solve_on_host``); at the end their weighted, gain/bias-compensated forms (section 5.12: ``unpack_w``, ``lm_step_w``,
``solve_on_host_w``).  Pure numpy; the step rules in plain Python floats.

A map is six float32 numbers (a00, a01, t0, a10, a11, t1): pixel (i, j) of the target lattice is read at
    Y = ((a00 i) + (a01 j)) + t0        X = ((a10 i) + (a11 j)) + t1
in reconstruction pixel coordinates, in fp32 with every operation rounded on its own -- what the kernels compute, bit for bit."""
import collections

import numpy as np

SUMS = 29  # count, cost, dcost[6], jtj packed upper triangle row-major [21]
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
_IU = np.triu_indices(6)

AlignResult = collections.namedtuple("AlignResult", "count cost grad jtj warped wgrad")
AlignResult.__doc__ = """count (n,) int64 valid pixels, cost (n,) the sum of squared differences over them, grad (n, 6) its gradient over
(a00, a01, t0, a10, a11, t1), jtj (n, 6, 6) the Gauss-Newton matrix (symmetric); warped (n, th, tw) / wgrad (2, n, th, tw) or None."""


def map_points(maps_row, shape):
    """One map (6,) on the lattice ``shape = (th, tw)`` -> (th * tw, 2) float32 points (Y, X), row i * tw + j: the fp32 rule above."""
    a = np.asarray(maps_row, dtype=np.float32)
    if a.shape != (6,):
        raise ValueError(f"expected one map of 6 numbers, got {a.shape}")
    th, tw = (int(x) for x in shape)
    if th < 0 or tw < 0:
        raise ValueError(f"shape must be non-negative, got {shape}")
    i = np.arange(th, dtype=np.float32)[:, None]
    j = np.arange(tw, dtype=np.float32)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        Y = ((a[0] * i) + (a[1] * j)) + a[2]
        X = ((a[3] * i) + (a[4] * j)) + a[5]
    assert Y.dtype == np.float32 and X.dtype == np.float32
    return np.stack([Y, X], axis=-1).reshape(th * tw, 2)


def rigid_maps(angle, shift, centre, dtype=np.float32):
    """Rotations by ``angle`` (n,) radians about ``centre`` (2,) = (Y, X) followed by ``shift`` (n, 2) -> maps (n, 6) float32:
    p' = R (p - centre) + centre + shift, R = [[cos, -sin], [sin, cos]] on (row, column).  Formed in fp64 and rounded once
    (``dtype=np.float64``: not rounded)."""
    angle = np.atleast_1d(np.asarray(angle, dtype=np.float64))
    shift = np.broadcast_to(np.asarray(shift, dtype=np.float64), (len(angle), 2))
    cy, cx = np.asarray(centre, dtype=np.float64)
    c, s = np.cos(angle), np.sin(angle)
    maps = np.empty((len(angle), 6), np.float64)
    maps[:, 0], maps[:, 1], maps[:, 2] = c, -s, cy - (c * cy - s * cx) + shift[:, 0]
    maps[:, 3], maps[:, 4], maps[:, 5] = s, c, cx - (s * cy + c * cx) + shift[:, 1]
    return maps.astype(dtype)


def unpack(sums, warped=None, wgrad=None):
    """sums (n, 29) float64 as msiren_align_slices writes them -> AlignResult (jtj unpacked to symmetric (n, 6, 6))"""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] != SUMS:
        raise ValueError(f"expected sums of shape (n, {SUMS}), got {sums.shape}")
    n = len(sums)
    jtj = np.zeros((n, 6, 6), np.float64)
    jtj[:, _IU[0], _IU[1]] = sums[:, 8:]
    jtj[:, _IU[1], _IU[0]] = sums[:, 8:]
    return AlignResult(sums[:, 0].astype(np.int64), sums[:, 1].copy(), sums[:, 2:8].copy(), jtj, warped, wgrad)


def gauss_newton_step(result, damping=0.0):
    """(n, 6) float64: per slice the solution of (JtJ + damping diag(JtJ)) delta = -grad / 2 (grad = 2 J^T r).  A slice with fewer than six
    valid pixels, or a singular system, gives a zero step."""
    n = len(result.count)
    step = np.zeros((n, 6), np.float64)
    for s in range(n):
        if result.count[s] < 6:
            continue
        A = result.jtj[s] + float(damping) * np.diag(np.diag(result.jtj[s]))
        try:
            step[s] = np.linalg.solve(A, -0.5 * result.grad[s])
        except np.linalg.LinAlgError:
            pass
    return step


# ---- msiren_align_solve's step rule, one slice, in Python floats: fp64 + - * / one at a time, no fused operation, every
# sum in the order written -- what align_step_kernel computes, bit for bit.  No numpy arithmetic below: its summation order is not defined.
AFFINE, RIGID = 0, 1
SINGULAR, NO_OVERLAP = 1, 2
INF = float("inf")

SolveOptions = collections.namedtuple("SolveOptions", "mode iterations damping down up lam_min lam_max centre", defaults=(AFFINE, 12, 1e-3, 0.1, 10.0, 1e-9, 1e9, (0.0, 0.0)))
SolveResult = collections.namedtuple("SolveResult", "maps angle shift accepted mean_first mean_best count damping flags trace")
SolveResult.__doc__ = """maps (n, 6) float32 the best map of every slice; angle (n,) = atan2(s, c) and shift (n, 2) of the best rigid state (None in
affine mode); accepted (n,) int64 steps accepted after the first evaluation; mean_first / mean_best (n,) cost / count at the input and at the best
map (+inf: fewer than six valid pixels); count (n,) int64 valid pixels at the best map; damping (n,) the final lambda; flags (n,) int64
(SINGULAR: the last proposal was zero, NO_OVERLAP: mean_first is +inf); trace (iterations, n, 8) or None: per evaluation the trial map, cost, count."""


def _f32(x):
    """a Python float rounded to float32 (nearest even; beyond the range: inf), back as a Python float"""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(x))


def _finite(x):
    return x - x == 0.0  # (false for inf and NaN)


def ldl_solve(A, b, m):
    """A (m x m, its lower triangle and diagonal are read), b (m) -> (x, ok): A = L D L^T without pivoting, then the three substitutions.  A pivot
    that is not positive and finite: (zeros, False)."""
    L = [[0.0] * m for _ in range(m)]
    D = [0.0] * m
    for j in range(m):
        dj = A[j][j]
        for k in range(j):
            dj = dj - (L[j][k] * L[j][k]) * D[k]
        if not (dj > 0.0) or not _finite(dj):
            return [0.0] * m, False
        D[j] = dj
        for i in range(j + 1, m):
            v = A[i][j]
            for k in range(j):
                v = v - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = v / dj
    y = [float(x) for x in b]
    for i in range(m):
        for k in range(i):
            y[i] = y[i] - L[i][k] * y[k]
    for i in range(m):
        y[i] = y[i] / D[i]
    for i in range(m - 1, -1, -1):
        for k in range(i + 1, m):
            y[i] = y[i] - L[k][i] * y[k]
    return y, True


def rigid_jacobian(c, s, cy, cx):
    """B (6 x 3): d map / d (angle, uY, uX) at the rigid state (c, s, ., .) about (cy, cx)"""
    B = [[0.0] * 3 for _ in range(6)]
    B[0][0], B[1][0], B[2][0] = -s, -c, s * cy + c * cx
    B[3][0], B[4][0], B[5][0] = c, -s, -(c * cy - s * cx)
    B[2][1] = 1.0
    B[5][2] = 1.0
    return B


def cayley(u):
    """(cos, sin) of the rotation by 2 atan(u): an exact rotation up to rounding, no trigonometry"""
    uu = u * u
    return (1.0 - uu) / (1.0 + uu), (2.0 * u) / (1.0 + uu)


def rigid_map(c, s, uY, uX, cy, cx):
    """rigid_maps' formula for one state, in Python floats -> the six float32 entries (as floats)"""
    return [_f32(c), _f32(-s), _f32(cy - (c * cy - s * cx) + uY), _f32(s), _f32(c), _f32(cx - (s * cy + c * cx) + uX)]


def lm_decide(k, mean, mean_best, lam, o):
    """-> (accept, counted, lam): the first evaluation is accepted and changes nothing else; a lower mean is accepted and lowers lam; everything
    else (a NaN included) is rejected and raises it"""
    if k == 0:
        return True, False, lam
    if mean < mean_best:
        x = lam * o.down
        return True, True, (x if x > o.lam_min else o.lam_min)
    x = lam * o.up
    return False, False, (x if x < o.lam_max else o.lam_max)


def lm_init(o, map_in=None, rigid_in=None):
    """the state of one slice before its first evaluation: a dict (trial, best, rigid_trial, rigid_best, sums, mean_best, mean_first, lam,
    accepted, flags).  Affine: map_in (6); rigid: rigid_in (c, s, uY, uX), the trial map formed from it."""
    st = dict(sums=[0.0] * SUMS, mean_best=INF, mean_first=INF, lam=float(o.damping), accepted=0, flags=0)
    if o.mode == RIGID:
        r = [float(x) for x in rigid_in]
        st["rigid_trial"], st["rigid_best"] = r, list(r)
        st["trial"] = rigid_map(r[0], r[1], r[2], r[3], float(o.centre[0]), float(o.centre[1]))
    else:
        st["rigid_trial"] = st["rigid_best"] = [0.0] * 4
        st["trial"] = [_f32(x) for x in map_in]
    st["best"] = list(st["trial"])
    return st


def lm_step(st, sums, k, o):
    """One slice after evaluation k: ``sums`` (29) are msiren_align_slices' at st["trial"].  Accept or reject, then propose the next trial from
    the best map.  ``st`` is updated in place and returned."""
    sums = [float(x) for x in sums]
    mean = sums[1] / sums[0] if sums[0] >= 6.0 else INF
    accept, counted, st["lam"] = lm_decide(k, mean, st["mean_best"], st["lam"], o)
    if accept:
        st["best"], st["rigid_best"], st["sums"], st["mean_best"] = list(st["trial"]), list(st["rigid_trial"]), sums, mean
        if k == 0:
            st["mean_first"] = mean
        if counted:
            st["accepted"] += 1
    lam, bs = st["lam"], st["sums"]
    g = bs[2:8]
    H = [[0.0] * 6 for _ in range(6)]
    q = 8
    for a in range(6):
        for b in range(a, 6):
            H[a][b] = H[b][a] = bs[q]
            q += 1
    if o.mode == AFFINE:
        A = [row[:] for row in H]
        for a in range(6):
            A[a][a] = H[a][a] + lam * H[a][a]
        d, ok = ldl_solve(A, [-0.5 * g[a] for a in range(6)], 6)
        st["trial"] = [_f32(st["best"][a] + d[a]) for a in range(6)]
    else:
        c, s, uY, uX = st["rigid_best"]
        cy, cx = float(o.centre[0]), float(o.centre[1])
        B = rigid_jacobian(c, s, cy, cx)
        g3 = [0.0] * 3
        for p in range(3):
            t = 0.0
            for a in range(6):
                t = t + B[a][p] * g[a]
            g3[p] = t
        T = [[0.0] * 3 for _ in range(6)]
        for a in range(6):
            for p in range(3):
                t = 0.0
                for b in range(6):
                    t = t + H[a][b] * B[b][p]
                T[a][p] = t
        A = [[0.0] * 3 for _ in range(3)]
        for p in range(3):
            for r in range(3):
                t = 0.0
                for a in range(6):
                    t = t + B[a][p] * T[a][r]
                A[p][r] = t
        for p in range(3):
            A[p][p] = A[p][p] + lam * A[p][p]
        d, ok = ldl_solve(A, [-0.5 * g3[p] for p in range(3)], 3)
        cd, sd = cayley(d[0] / 2.0)
        c2, s2 = c * cd - s * sd, s * cd + c * sd
        st["rigid_trial"] = [c2, s2, uY + d[1], uX + d[2]]
        st["trial"] = rigid_map(c2, s2, uY + d[1], uX + d[2], cy, cx)
    st["flags"] = (0 if ok else SINGULAR) | (NO_OVERLAP if st["mean_first"] == INF else 0)
    return st


def solve_on_host(cost_fn, n, *, maps=None, rigid=None, options=SolveOptions(), trace=False):
    """msiren_align_solve's loop around any ``cost_fn(maps (n, 6) float32) -> sums (n, 29)``: ``options.iterations`` evaluations, ``lm_step``
    per slice after each.  Affine: ``maps`` (n, 6); rigid: ``rigid`` (n, 4) = (c, s, uY, uX).  -> (SolveResult, rigid (n, 4) float64 best states)"""
    o = options
    st = [lm_init(o, None if maps is None else maps[s], None if rigid is None else rigid[s]) for s in range(n)]
    tr = np.zeros((o.iterations, n, 8), np.float64) if trace else None
    for k in range(o.iterations):
        trial = np.array([x["trial"] for x in st], np.float32).reshape(n, 6)
        sums = np.asarray(cost_fn(trial), np.float64).reshape(n, SUMS)
        if trace:
            tr[k, :, :6], tr[k, :, 6], tr[k, :, 7] = trial, sums[:, 1], sums[:, 0]
        for s in range(n):
            lm_step(st[s], sums[s], k, o)
    rb = np.array([x["rigid_best"] for x in st], np.float64).reshape(n, 4)
    return solve_result(np.array([x["best"] for x in st], np.float32).reshape(n, 6), rb if o.mode == RIGID else None,
                        np.array([[x["accepted"], x["mean_first"], x["mean_best"], x["sums"][0], x["lam"], x["flags"]] for x in st], np.float64).reshape(n, 6), tr), rb


def solve_result(maps, rigid, report, trace):
    """what msiren_align_solve writes -> SolveResult"""
    angle = shift = None
    if rigid is not None:
        angle, shift = np.arctan2(rigid[:, 1], rigid[:, 0]), rigid[:, 2:4].copy()
    return SolveResult(maps, angle, shift, report[:, 0].astype(np.int64), report[:, 1].copy(), report[:, 2].copy(), report[:, 3].astype(np.int64),
                       report[:, 4].copy(), report[:, 5].astype(np.int64), trace)


# ---- weighted, gain/bias-compensated alignment (msiren_align_slices_w, msiren_align_solve_w) ----------------------------
# Parameter order a00, a01, t0, a10, a11, t1, g, b: the model of a target pixel is g R + b, every pixel carries a weight w.
SUMS_W = 47  # count, wsum, cost, dcost[8], jtj packed upper triangle row-major [36]
FIXED, ESTIMATE = 0, 1
_IU8 = np.triu_indices(8)

AlignResultW = collections.namedtuple("AlignResultW", "count wsum cost grad jtj warped wgrad")
AlignResultW.__doc__ = """count (n,) int64 valid pixels (finite, weight > 0), wsum (n,) the sum of their weights, cost (n,) sum w (g R + b - T)^2, grad
(n, 8) its gradient over (a00, a01, t0, a10, a11, t1, g, b), jtj (n, 8, 8) the weighted Gauss-Newton matrix (symmetric); warped (n, th, tw) /
wgrad (2, n, th, tw) (R, gY, gX before gain and bias) or None."""

SolveOptionsW = collections.namedtuple("SolveOptionsW", "mode iterations damping down up lam_min lam_max centre intensity_mode",
                                       defaults=(AFFINE, 12, 1e-3, 0.1, 10.0, 1e-9, 1e9, (0.0, 0.0), ESTIMATE))
SolveResultW = collections.namedtuple("SolveResultW", "maps angle shift accepted mean_first mean_best count damping flags trace intensity wsum")
SolveResultW.__doc__ = """SolveResult's fields (mean_* = cost / wsum; +inf: fewer valid pixels than solved parameters; trace (iterations, n, 11) or None: per
evaluation the trial map, the trial g, b, cost, count, wsum), then intensity (n, 2) float32 the best (g, b) and wsum (n,) at the best map."""


def unpack_w(sums, warped=None, wgrad=None):
    """sums (n, 47) float64 as msiren_align_slices_w writes them -> AlignResultW (jtj unpacked to symmetric (n, 8, 8))"""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] != SUMS_W:
        raise ValueError(f"expected sums of shape (n, {SUMS_W}), got {sums.shape}")
    n = len(sums)
    jtj = np.zeros((n, 8, 8), np.float64)
    jtj[:, _IU8[0], _IU8[1]] = sums[:, 11:]
    jtj[:, _IU8[1], _IU8[0]] = sums[:, 11:]
    return AlignResultW(sums[:, 0].astype(np.int64), sums[:, 1].copy(), sums[:, 2].copy(), sums[:, 3:11].copy(), jtj, warped, wgrad)


def gauss_newton_step_w(result, damping=0.0, estimate_intensity=True):
    """(n, 8) float64: per slice the solution of (JtJ + damping diag(JtJ)) delta = -grad / 2 over all 8 parameters, or over the six of the map
    (the last two entries zero).  A slice with fewer valid pixels than parameters, or a singular system, gives a zero step."""
    n, P = len(result.count), 8 if estimate_intensity else 6
    step = np.zeros((n, 8), np.float64)
    for s in range(n):
        if result.count[s] < P:
            continue
        H = result.jtj[s][:P, :P]
        try:
            step[s, :P] = np.linalg.solve(H + float(damping) * np.diag(np.diag(H)), -0.5 * result.grad[s][:P])
        except np.linalg.LinAlgError:
            pass
    return step


# msiren_align_solve_w's step rule, one slice, in Python floats as lm_step above -- what align_step_w_kernel computes, bit for bit.
def solved_parameters(o):
    """P: affine 6 / rigid 3, and the two of the intensity where they are estimated"""
    return (3 if o.mode == RIGID else 6) + (2 if o.intensity_mode == ESTIMATE else 0)


def lm_mean_w(sums, P):
    """cost / wsum where at least P pixels are valid, +inf otherwise"""
    return sums[2] / sums[1] if sums[0] >= float(P) else INF


def rigid_jacobian_w(c, s, cy, cx):
    """B (8 x 5): rigid_jacobian's 6 x 3 block, then d (g, b) / d (g, b) = 1"""
    B6 = rigid_jacobian(c, s, cy, cx)
    B = [[0.0] * 5 for _ in range(8)]
    for a in range(6):
        for q in range(3):
            B[a][q] = B6[a][q]
    B[6][3] = 1.0
    B[7][4] = 1.0
    return B


def intensity_update(gb, dg, db):
    """(g', b') as float32 from the best (g, b) and the step's last two entries"""
    return [_f32(gb[0] + dg), _f32(gb[1] + db)]


def lm_init_w(o, map_in=None, rigid_in=None, intensity_in=None):
    """lm_init's state with gb_trial, gb_best (float32 as floats; None: (1, 0)) and sums of 47"""
    st = lm_init(o, map_in, rigid_in)
    st["sums"] = [0.0] * SUMS_W
    st["gb_trial"] = [1.0, 0.0] if intensity_in is None else [_f32(x) for x in intensity_in]
    st["gb_best"] = list(st["gb_trial"])
    return st


def lm_step_w(st, sums, k, o):
    """One slice after evaluation k: ``sums`` (47) are msiren_align_slices_w's at (st["trial"], st["gb_trial"]).  Accept or reject, then propose the
    next trial from the best state.  ``st`` is updated in place and returned."""
    sums = [float(x) for x in sums]
    est = o.intensity_mode == ESTIMATE
    mean = lm_mean_w(sums, solved_parameters(o))
    accept, counted, st["lam"] = lm_decide(k, mean, st["mean_best"], st["lam"], o)
    if accept:
        st["best"], st["rigid_best"], st["gb_best"], st["sums"], st["mean_best"] = list(st["trial"]), list(st["rigid_trial"]), list(st["gb_trial"]), sums, mean
        if k == 0:
            st["mean_first"] = mean
        if counted:
            st["accepted"] += 1
    lam, bs = st["lam"], st["sums"]
    g = bs[3:11]
    H = [[0.0] * 8 for _ in range(8)]
    q = 11
    for a in range(8):
        for b in range(a, 8):
            H[a][b] = H[b][a] = bs[q]
            q += 1
    if o.mode == AFFINE:
        P = 8 if est else 6
        A = [row[:P] for row in H[:P]]
        for a in range(P):
            A[a][a] = H[a][a] + lam * H[a][a]
        d, ok = ldl_solve(A, [-0.5 * g[a] for a in range(P)], P)
        st["trial"] = [_f32(st["best"][a] + d[a]) for a in range(6)]
        dg, db = (d[6], d[7]) if est else (0.0, 0.0)
    else:
        c, s, uY, uX = st["rigid_best"]
        cy, cx = float(o.centre[0]), float(o.centre[1])
        P, Q = (8, 5) if est else (6, 3)
        B = rigid_jacobian_w(c, s, cy, cx) if est else rigid_jacobian(c, s, cy, cx)
        gq = [0.0] * Q
        for p in range(Q):
            t = 0.0
            for a in range(P):
                t = t + B[a][p] * g[a]
            gq[p] = t
        T = [[0.0] * Q for _ in range(P)]
        for a in range(P):
            for p in range(Q):
                t = 0.0
                for b in range(P):
                    t = t + H[a][b] * B[b][p]
                T[a][p] = t
        A = [[0.0] * Q for _ in range(Q)]
        for p in range(Q):
            for r in range(Q):
                t = 0.0
                for a in range(P):
                    t = t + B[a][p] * T[a][r]
                A[p][r] = t
        for p in range(Q):
            A[p][p] = A[p][p] + lam * A[p][p]
        d, ok = ldl_solve(A, [-0.5 * gq[p] for p in range(Q)], Q)
        cd, sd = cayley(d[0] / 2.0)
        c2, s2 = c * cd - s * sd, s * cd + c * sd
        st["rigid_trial"] = [c2, s2, uY + d[1], uX + d[2]]
        st["trial"] = rigid_map(c2, s2, uY + d[1], uX + d[2], cy, cx)
        dg, db = (d[3], d[4]) if est else (0.0, 0.0)
    st["gb_trial"] = intensity_update(st["gb_best"], dg, db) if est else list(st["gb_best"])
    st["flags"] = (0 if ok else SINGULAR) | (NO_OVERLAP if st["mean_first"] == INF else 0)
    return st


def solve_on_host_w(cost_fn, n, *, maps=None, rigid=None, intensity=None, options=SolveOptionsW(), trace=False):
    """msiren_align_solve_w's loop around any ``cost_fn(maps (n, 6) float32, intensity (n, 2) float32) -> sums (n, 47)``: ``options.iterations``
    evaluations, ``lm_step_w`` per slice after each.  -> (SolveResultW, rigid (n, 4) float64 best states)"""
    o = options
    st = [lm_init_w(o, None if maps is None else maps[s], None if rigid is None else rigid[s], None if intensity is None else intensity[s]) for s in range(n)]
    tr = np.zeros((o.iterations, n, 11), np.float64) if trace else None
    for k in range(o.iterations):
        trial = np.array([x["trial"] for x in st], np.float32).reshape(n, 6)
        gb = np.array([x["gb_trial"] for x in st], np.float32).reshape(n, 2)
        sums = np.asarray(cost_fn(trial, gb), np.float64).reshape(n, SUMS_W)
        if trace:
            tr[k, :, :6], tr[k, :, 6:8], tr[k, :, 8], tr[k, :, 9], tr[k, :, 10] = trial, gb, sums[:, 2], sums[:, 0], sums[:, 1]
        for s in range(n):
            lm_step_w(st[s], sums[s], k, o)
    rb = np.array([x["rigid_best"] for x in st], np.float64).reshape(n, 4)
    return solve_result_w(np.array([x["best"] for x in st], np.float32).reshape(n, 6), np.array([x["gb_best"] for x in st], np.float32).reshape(n, 2),
                          rb if o.mode == RIGID else None, report_w(st), tr), rb


def report_w(states):
    """the (n, 7) report of msiren_align_solve_w from the states of lm_step_w"""
    return np.array([[x["accepted"], x["mean_first"], x["mean_best"], x["sums"][0], x["sums"][1], x["lam"], x["flags"]] for x in states], np.float64).reshape(len(states), 7)


def solve_result_w(maps, intensity, rigid, report, trace):
    """what msiren_align_solve_w writes -> SolveResultW"""
    angle = shift = None
    if rigid is not None:
        angle, shift = np.arctan2(rigid[:, 1], rigid[:, 0]), rigid[:, 2:4].copy()
    return SolveResultW(maps, angle, shift, report[:, 0].astype(np.int64), report[:, 1].copy(), report[:, 2].copy(), report[:, 3].astype(np.int64),
                        report[:, 5].copy(), report[:, 6].astype(np.int64), trace, intensity, report[:, 4].copy())
