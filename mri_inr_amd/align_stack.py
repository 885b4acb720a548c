"""Helpers for ``ModulatedSiren.align_stack_cost`` and ``align_stack_solve``: target slices scored against, and aligned
to, a stack that is just voxels -- what ``fuse_targets``, ``solve_volume`` and ``solve_volume_robust`` return -- instead of the stack the network
reconstructs.  The pixel is a trilinear read of the float32 stack with its analytic gradient; everything behind the pixel is section 5.16's: the
validity, (g, b), J[11], ``align_robust.robust_terms``' factors, the 80 sums, and section 5.15's grouped rigid loop around them.

This module restates msiren_align_stack_r completely, bit for bit, in elementwise numpy (every numpy operation below is one IEEE operation per
element, nothing fused): ``read_stack`` the read, ``pixel_terms`` what a pixel adds to the 80 sums, ``chunk_sums`` the one order in which the kernel
adds them, ``cost_on_host`` the call.  ``solve_on_host_s`` is ``align_robust.solve_on_host_r`` around it: the normative loop of
msiren_align_stack_solve_group_r.

The read at a point (Z, Y, X) in fp32 (``align_volume.map_points3``).  INSIDE iff 0 <= Z <= n - 1, 0 <= Y <= H - 1 and 0 <= X <= W - 1, compared in
fp32 against exact integers (a NaN fails).  Inside, in fp64 from the fp32 numbers:
    z0 = min(floor Z, n - 2),  fz = Z - z0,  az = 1 - fz      (y0, fy, ay and x0, fx, ax likewise with H, W)
    V[dz][dy][dx] = stack[z0 + dz, y0 + dy, x0 + dx]
    c[dz][dy] = (ax V[dz][dy][0]) + (fx V[dz][dy][1])        dx_[dz][dy] = V[dz][dy][1] - V[dz][dy][0]
    e[dz] = (ay c[dz][0]) + (fy c[dz][1])      ex[dz] = (ay dx_[dz][0]) + (fy dx_[dz][1])      ey[dz] = c[dz][1] - c[dz][0]
    R = f32((az e[0]) + (fz e[1]))    gX = f32((az ex[0]) + (fz ex[1]))    gY = f32((az ey[0]) + (fz ey[1]))    gZ = f32(e[1] - e[0])
Outside: NaN in all four.  A corner that is not finite is not special-cased: it reaches the values through the arithmetic (0 x NaN included), so a
pixel needs all eight corners finite -- on a stack with NaN holes a pixel counts only where its whole cell is known.  At the upper faces the last
cell is read with f = 1.  The gradient is the derivative of the interpolant inside the cell that was read."""
import numpy as np

from . import align_group as ag, align_robust as ar
from .align_volume import SUMS_VW, map_points3

CHUNK = 1024    # pixels per partial record (csrc/align.hip.h: ALIGN_CHUNK)
THREADS = 256   # threads of the workgroup that forms one
WAVE = 64
PACK = [(a, c) for a in range(11) for c in range(a, 11)]  # the upper triangle of jtj, row-major


def _stack3(stack):
    v = np.ascontiguousarray(stack, dtype=np.float32)
    if v.ndim != 3 or min(v.shape) < 2:
        raise ValueError(f"expected a stack (n, H, W) with n, H, W >= 2, got {v.shape}")
    return v


def _cell(v, length):
    """the lower corner of the cell that holds v (inside) on an axis of ``length`` voxels, the fraction inside it and its complement, fp64"""
    c = np.minimum(np.floor(v).astype(np.int64), length - 2)
    f = v.astype(np.float64) - c.astype(np.float64)
    return c, f, 1.0 - f


def read_stack(stack, points, rounded=True):
    """stack (n, H, W) float32, points (M, 3) float32 = (Z, Y, X) -> (R, gZ, gY, gX), float32 (M,) each: the rule of the module docstring.
    ``rounded`` False: the fp64 values in front of the final rounding to float32 (what the association of the rule is visible in)"""
    v = _stack3(stack)
    n, H, W = v.shape
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    Z, Y, X = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore"):
        inside = (Z >= 0) & (Z <= np.float32(n - 1)) & (Y >= 0) & (Y <= np.float32(H - 1)) & (X >= 0) & (X <= np.float32(W - 1))
    out = [np.full(len(p), np.nan, np.float32 if rounded else np.float64) for _ in range(4)]
    if not inside.any():
        return tuple(out)
    z0, fz, az = _cell(Z[inside], n)
    y0, fy, ay = _cell(Y[inside], H)
    x0, fx, ax = _cell(X[inside], W)
    with np.errstate(invalid="ignore", over="ignore"):
        e, ex, ey = [], [], []
        for dz in range(2):
            c, d = [], []
            for dy in range(2):
                v0, v1 = v[z0 + dz, y0 + dy, x0].astype(np.float64), v[z0 + dz, y0 + dy, x0 + 1].astype(np.float64)
                c.append((ax * v0) + (fx * v1))
                d.append(v1 - v0)
            e.append((ay * c[0]) + (fy * c[1]))
            ex.append((ay * d[0]) + (fy * d[1]))
            ey.append(c[1] - c[0])
        vals = ((az * e[0]) + (fz * e[1]), e[1] - e[0], (az * ey[0]) + (fz * ey[1]), (az * ex[0]) + (fz * ex[1]))
        for o, x in zip(out, vals):
            o[inside] = x.astype(o.dtype)
    return tuple(out)


def pixel_terms(R, gZ, gY, gX, target, weight, gb, s, shape):
    """One target's planes, target and weight (th tw,) float32, gb = (g, b) float32, s its scale -> (terms (th tw, 80) float64: what every pixel adds
    to the 80 sums, zeros at an invalid pixel; rweight (th tw,) float32, NaN at an invalid pixel).  Section 5.16's terms in its association."""
    th, tw = shape
    Mt = th * tw
    R, gZ, gY, gX, T, w = (np.asarray(x, np.float32).reshape(Mt) for x in (R, gZ, gY, gX, target, weight))
    g, b, s = float(np.float32(gb[0])), float(np.float32(gb[1])), float(s)
    terms, rw = np.zeros((Mt, SUMS_VW), np.float64), np.full(Mt, np.nan, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(T) & np.isfinite(R) & np.isfinite(gZ) & np.isfinite(gY) & np.isfinite(gX) & np.isfinite(w) & (w > 0)
    if not (s > 0) or not ok.any():
        return terms, rw
    px = np.nonzero(ok)[0]
    di, dj = (px // tw).astype(np.float64), (px % tw).astype(np.float64)
    R, gZ, gY, gX, T, wd = (x[ok].astype(np.float64) for x in (R, gZ, gY, gX, T, w))
    with np.errstate(invalid="ignore", over="ignore"):
        r = ((g * R) + b) - T
        gz, gy, gx = g * gZ, g * gY, g * gX
        u = (r * r) / s
        om = 1.0 / (1.0 + u)
        wl = wd * om
        wq = wl * om
        J = [gz * di, gz * dj, gz, gy * di, gy * dj, gy, gx * di, gx * dj, gx, R, np.ones_like(R)]
        wr2 = 2.0 * (wq * r)
        cols = [np.ones_like(R), wd, (wl * r) * r] + [wr2 * J[a] for a in range(11)] + [(wq * J[a]) * J[c] for a, c in PACK]
        terms[ok] = np.stack(cols, axis=1)
        rw[ok] = (om * om).astype(np.float32)
    return terms, rw


def chunk_sums(terms):
    """terms (Mt, N) float64 -> (N,): the kernel's one order.  Per chunk of 1024 pixels thread t of 256 adds its pixels lo + t, lo + t + 256, ... to
    0.0 in that order; a butterfly inside each wave of 64 (offsets 32, 16, .., 1), then the four wave totals ((w0 + w1) + w2) + w3; the chunks of the
    target in index order, starting with the first chunk's record."""
    terms = np.asarray(terms, np.float64)
    Mt, N = terms.shape
    lane = np.arange(THREADS)
    total = None
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, Mt, CHUNK):
            block = np.zeros((CHUNK, N), np.float64)
            block[:min(CHUNK, Mt - lo)] = terms[lo:lo + CHUNK]
            block = block.reshape(CHUNK // THREADS, THREADS, N)
            acc = np.zeros((THREADS, N), np.float64)
            for k in range(CHUNK // THREADS):
                acc = acc + block[k]
            o = WAVE // 2
            while o:
                acc = acc + acc[lane ^ o]
                o >>= 1
            w = acc[::WAVE]
            rec = ((w[0] + w[1]) + w[2]) + w[3]
            total = rec if total is None else total + rec
    return np.zeros(N, np.float64) if total is None else total


def cost_on_host(stack, targets, maps, scale=ar.INF, *, weights=None, intensity=None):
    """msiren_align_stack_r on the host, bit for bit -> (sums (m, 80) float64, warped (m, th, tw), wgrad (3, m, th, tw), rweight (m, th, tw)) float32"""
    v = _stack3(stack)
    t = np.ascontiguousarray(targets, dtype=np.float32)
    m, th, tw = t.shape
    mp = np.asarray(maps, np.float32).reshape(m, 9)
    w = np.ones((m, th, tw), np.float32) if weights is None else np.asarray(weights, np.float32).reshape(m, th, tw)
    gb = np.tile(np.array([1.0, 0.0], np.float32), (m, 1)) if intensity is None else np.asarray(intensity, np.float32).reshape(m, 2)
    s = ar.scales(scale, m)
    sums = np.zeros((m, SUMS_VW), np.float64)
    warped, wgrad, rweight = np.empty((m, th, tw), np.float32), np.empty((3, m, th, tw), np.float32), np.empty((m, th, tw), np.float32)
    for q in range(m):
        R, gZ, gY, gX = read_stack(v, map_points3(mp[q], (th, tw)))
        terms, rw = pixel_terms(R, gZ, gY, gX, t[q], w[q], gb[q], s[q], (th, tw))
        sums[q] = chunk_sums(terms)
        warped[q], wgrad[0, q], wgrad[1, q], wgrad[2, q], rweight[q] = (x.reshape(th, tw) for x in (R, gZ, gY, gX, rw))
    return sums, warped, wgrad, rweight


def result_on_host(stack, targets, maps, scale=ar.INF, *, weights=None, intensity=None):
    """``cost_on_host`` as the ``align_robust.AlignResultR`` that ``ModulatedSiren.align_stack_cost`` returns with every optional output"""
    return ar.unpack_r(*cost_on_host(stack, targets, maps, scale, weights=weights, intensity=intensity))


def solve_on_host_s(stack, targets, group_start, scale, *, rigid, planes, weights=None, intensity=None, options=ag.SolveOptionsG(), trace=False, cost_fn=None):
    """msiren_align_stack_solve_group_r's loop: ``align_robust.solve_on_host_r`` around ``cost_on_host`` (``cost_fn(maps, intensity, scale) -> sums``:
    another evaluation with that signature, the device's for instance).  -> (SolveResultG, the final states (groups, targets))"""
    if cost_fn is None:
        def cost_fn(maps, gb, s):
            return cost_on_host(stack, targets, maps, s, weights=weights, intensity=gb)[0]
    return ar.solve_on_host_r(cost_fn, group_start, scale, rigid=rigid, planes=planes, intensity=intensity, options=options, trace=trace)
