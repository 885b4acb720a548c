"""The slice-to-volume registration calls of ``ModulatedSiren``, from ``resample`` to ``solve_volume_robust``, ``align_stack_solve`` and
``residual_scale`` and ``leave_out_targets``: the ctypes binding of the ``msiren_resample_*``, ``msiren_align_*``, ``msiren_fuse_targets``,
``msiren_project_volume``, ``msiren_solve_volume*``, ``msiren_residual_scale`` and ``msiren_leave_out_targets`` entry points (DESIGN.md sections 5.8 to
5.20 and 5.22 to 5.24), as the mixin ``_Registration`` the model inherits.

Every public method reads the same way: check the inputs, build the options, allocate the outputs, one call into the library, wrap the
result.  The rules all of them keep:

* ``_ensure_committed()`` in front of everything that evaluates the model; ``fuse_targets``, ``project_volume``, the two volume solves and the
  two ``align_stack_*`` methods, ``residual_scale`` and ``leave_out_targets`` involve no weights of the model and only need the handle (``_ensure_handle()``).
* Outputs are filled before the call -- NaN for sampled images and volumes, 0 for sums, reports and coverage, -1 for ``stopped_at``, (1, 0)
  rows for an absent intensity, +inf for an estimated scale -- because the library may return without writing them (no targets, an empty grid, no rounds).
* An absent optional array is a null pointer (``_addr``).  For m = 0 targets the fuse, project, solve-volume and residual-scale calls take null for every
  per-target pointer (``_ptr``); the alignment calls take the address of the empty array.  The library answers the two differently.
* numpy or torch in, numpy out; a tensor in gives tensors out for the resample methods only."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _f32(x) -> np.ndarray:
    """a tensor or an array -> contiguous float32 on the host"""
    return np.ascontiguousarray(x.detach().cpu().numpy() if _is_torch(x) else x, dtype=np.float32)


def _addr(x):
    """the address of a host array, None for no array"""
    return None if x is None else x.ctypes.data


def _ptr(x, m):
    """the address of a host array for a call with m targets: None for no array and for m == 0, where the library takes no per-target pointer"""
    return x.ctypes.data if x is not None and m else None


def _optional(flag, shape, fill, dtype=np.float32):
    """an output the caller may ask for: filled with ``fill`` where ``flag`` is set, else None"""
    if not flag:
        return None
    out = np.empty(shape, dtype)
    out.fill(fill)
    return out


def _like(x, outs):
    """the outputs as tensors where the input ``x`` was one (the resample methods)"""
    if _is_torch(x):
        import torch

        outs = [torch.from_numpy(o) for o in outs]
    return outs


# ---- one checker per thing checked: each returns its argument as contiguous float32, or raises ValueError before the library is entered
def _stack(images):
    a = _f32(images)
    if a.ndim != 3:
        raise ValueError(f"expected a stack of (n, H, W) images, got {a.shape}")
    return a


def _points(points, width):
    p = _f32(points)
    if p.ndim != 2 or p.shape[1] != width:
        raise ValueError(f"expected points of shape (M, {width}), got {p.shape}")
    return p


def _targets(targets, count=None):
    """targets (m, th, tw); ``count``: the m they must have"""
    t = _f32(targets)
    if t.ndim != 3 or (count is not None and len(t) != count):
        raise ValueError(f"expected targets of shape ({'m' if count is None else count}, th, tw), got {t.shape}")
    return t


def _maps(maps, rows, width):
    """maps (rows, width); ``rows`` None: any number"""
    mp = _f32(maps)
    if mp.ndim != 2 or mp.shape[1] != width or (rows is not None and len(mp) != rows):
        raise ValueError(f"expected maps of shape ({'m' if rows is None else rows}, {width}), got {mp.shape}")
    return mp


def _exactly(x, shape, what):
    a = _f32(x)
    if a.shape != shape:
        raise ValueError(f"expected {what} of shape {shape}, got {a.shape}")
    return a


def _weights_intensity(weights, intensity, shape):
    """-> (weights or None, intensity or None) for targets of ``shape`` = (m, th, tw)"""
    w = None if weights is None else _exactly(weights, shape, "weights")
    gb = None if intensity is None else _exactly(intensity, (shape[0], 2), "intensity")
    return w, gb


def _planes(planes, m):
    """planes (m, 12) float64 = (e_i, e_j, o, c) per target"""
    pl = np.ascontiguousarray(np.asarray(planes, dtype=np.float64).reshape(-1, 12))
    if pl.shape != (m, 12):
        raise ValueError(f"expected planes of shape ({m}, 12), got {pl.shape}")
    return pl


# ---- one builder per rigid state, in fp64
def _rigid2(angle, shift):
    """angle (n,) radians, shift (n, 2) or (2,) -> the in-plane state (n, 4) = (cos, sin, shift)"""
    ang = np.atleast_1d(np.asarray(angle, dtype=np.float64))
    sh = np.broadcast_to(np.asarray(shift, dtype=np.float64), (len(ang), 2))
    return np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang), sh[:, 0], sh[:, 1]], axis=1))


def _rigid3(rotation, shift, count):
    """rotation (count, 3, 3) or (3, 3) (None: the identity), shift (count, 3) or (3,) (None: zero) -> the state (count, 12) = (Rot, shift)"""
    rot = np.broadcast_to(np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64), (count, 3, 3)).reshape(count, 9)
    sh = np.broadcast_to(np.zeros(3) if shift is None else np.asarray(shift, dtype=np.float64), (count, 3))
    return np.ascontiguousarray(np.concatenate([rot, sh], axis=1))


def _intensity_out(gb, m):
    """where a solve writes (g, b) per target: a copy of the input, (1, 0) rows without one"""
    return np.tile(np.array([1.0, 0.0], np.float32), (m, 1)) if gb is None else gb.copy()


def _steps(iterations, damping, down, up, lam_min, lam_max):
    """the Levenberg-Marquardt fields every solve's opts structure has in common"""
    return int(iterations), (float(damping), float(down), float(up), float(lam_min), float(lam_max))


# ---- what fuse_targets, project_volume and the two volume solves share
def _fuse_inputs(targets, maps, weights, intensity):
    """-> (targets (m, th, tw), maps (m, 9), weights or None, intensity or None)"""
    t = _targets(targets)
    mp = _maps(maps, len(t), 9)
    return (t, mp) + _weights_intensity(weights, intensity, t.shape)


def _thickness(thickness, spacing):
    return float(spacing if thickness is None else thickness)


def _grid(shape, m, start, coverage):
    """``shape`` = (n, H, W), the output grid of m targets -> (n, H, W) as ints, start (n, H, W) or None, and the outputs: the volume (NaN), the
    coverage (0) or None, the flags (m,) (0).  A grid without voxels is refused by the library: nothing is allocated for it here."""
    if len(shape) != 3:
        raise ValueError(f"expected shape = (n, H, W), got {shape!r}")
    n, Hh, Ww = (int(s) for s in shape)
    st = None if start is None else _exactly(start, (n, Hh, Ww), "start")
    ok = n > 0 and Hh > 0 and Ww > 0
    vol = np.full((n, Hh, Ww) if ok else (0, 0, 0), np.nan, np.float32)
    return (n, Hh, Ww), st, vol, _optional(coverage, vol.shape, 0), np.zeros(m, np.int32)


class _Registration:
    """The registration calls of ``ModulatedSiren`` (see the module docstring).  Uses the model's ``_lib``, ``_h``, ``_ensure_handle()`` and
    ``_ensure_committed()``."""

    # ---- the reconstruction read at real positions (DESIGN.md sections 5.8, 5.9) ----
    def _resample(self, images, points, grad, exact=True):
        self._ensure_committed()
        a = _f32(images)
        single = a.ndim == 2
        a = _stack(a[None] if single else a)
        p = _points(points, 2)
        n, Hh, Ww = a.shape
        M = len(p)
        outs = [np.empty(shape, dtype=np.float32) for shape in (((n, M), (2, n, M)) if grad else ((n, M),))]  # (written in full by the library)
        fn = self._lib.msiren_resample_slices_grad if grad else self._lib.msiren_resample_slices if exact else self._lib.msiren_resample_slices_native
        _lib.check(fn(self._h, _addr(a), n, Hh, Ww, _addr(p), M, *[_addr(o) for o in outs]))
        if single:
            outs = [outs[0][0]] + [o[:, 0] for o in outs[1:]]
        outs = _like(images, outs)
        return tuple(outs) if grad else outs[0]

    def resample(self, images, points, *, exact=True):
        """images (n, Hh, Ww) or (Hh, Ww), points (M, 2) -> (n, M) or (M,): the reconstruction of ``reconstruct(images)`` read at real
        positions ``points[m] = (Y, X)`` in reconstruction pixel coordinates (integer (Y, X): the centre of ``recon[Y, X]``), one point
        set for all slices -- every covering tile's network evaluated at the point, blended with the fold's weights (build-defined,
        DESIGN.md section 5.8; msiren_resample_slices).  The exact-fp32 trunk; ``exact=False``: the model's own trunk arithmetic
        (msiren_resample_slices_native; sample_mods_ragged has the details).  NaN where no tile covers the point."""
        return self._resample(images, points, False, exact)

    def resample_with_gradient(self, images, points):
        """As resample -> (values (n, M), grad (2, n, M)): grad per reconstruction pixel, grad[0] along the rows -- the weight-averaged
        analytic gradients of the covering tiles, as ``reconstruct_with_gradient`` defines it (msiren_resample_slices_grad)."""
        return self._resample(images, points, True)

    def _resample_volume(self, images, points, grad, exact=True):
        self._ensure_committed()
        a = _stack(images)
        p = _points(points, 3)
        n, Hh, Ww = a.shape
        M = len(p)
        outs = [np.full(shape, np.nan, dtype=np.float32) for shape in (((M,), (3, M)) if grad else ((M,),))]  # (n = 0: no Z is valid, no call's work)
        fn = self._lib.msiren_resample_volume_grad if grad else self._lib.msiren_resample_volume if exact else self._lib.msiren_resample_volume_native
        _lib.check(fn(self._h, _addr(a), n, Hh, Ww, _addr(p), M, *[_addr(o) for o in outs]))
        outs = _like(images, outs)
        return tuple(outs) if grad else outs[0]

    def resample_volume(self, images, points, *, exact=True):
        """images (n, Hh, Ww), points (M, 3) -> (M,): the stack read as a volume at ``points[m] = (Z, Y, X)`` -- (Y, X) as in ``resample``,
        Z in slice units (integer Z: slice Z), valid for 0 <= Z <= n - 1.  ``resample`` of the two slices either side of Z, blended
        linearly in fp32; at an integer Z the bits of ``resample(images[Z], ...)`` (build-defined, DESIGN.md section 5.9;
        msiren_resample_volume).  Two trunk evaluations per point and covering tile, whatever n is.  The exact-fp32 trunk;
        ``exact=False``: the model's own trunk arithmetic (msiren_resample_volume_native).  NaN for an invalid Z, a non-finite (Y, X) or
        a point no tile covers."""
        return self._resample_volume(images, points, False, exact)

    def resample_volume_with_gradient(self, images, points):
        """As resample_volume -> (values (M,), grad (3, M)); n >= 2.  grad[0] per slice of Z: the fp32 difference of the two slices of
        the segment that contains Z (at an interior integer the segment to its right); grad[1], grad[2] per reconstruction pixel along
        rows and columns, ``resample_with_gradient``'s planes blended like the value (msiren_resample_volume_grad)."""
        return self._resample_volume(images, points, True)

    def resample_each(self, images, points, *, exact=True):
        """images (n, Hh, Ww), points (n, M, 2) -> (n, M): every slice at its OWN point set in one call -- the volume call at integer Z,
        so out[s] is the bits of ``resample(images[s], points[s], exact=exact)``."""
        n = len(images)
        p = _f32(points)
        if p.ndim != 3 or p.shape[0] != n or p.shape[2] != 2:
            raise ValueError(f"expected points of shape ({n}, M, 2), got {p.shape}")
        M = p.shape[1]
        zyx = np.empty((n, M, 3), np.float32)
        zyx[:, :, 0] = np.arange(n, dtype=np.float32)[:, None]
        zyx[:, :, 1:] = p
        out = self._resample_volume(images, zyx.reshape(n * M, 3), False, exact)
        return out.reshape(n, M)

    # ---- slices against their own targets under in-plane maps (DESIGN.md sections 5.10 to 5.12) ----
    def _align_cost(self, images, targets, maps, warped, gradient, weighted, weights=None, intensity=None):
        """the body of align_cost and align_cost_w"""
        from . import align

        self._ensure_committed()
        a = _stack(images)
        t = _targets(targets, len(a))
        w, gb = _weights_intensity(weights, intensity, t.shape)
        n, Hh, Ww = a.shape
        th, tw = t.shape[1:]
        mp = _maps(maps, n, 6)
        sums = np.zeros((n, align.SUMS_W if weighted else align.SUMS), np.float64)
        wp = _optional(warped, (n, th, tw), np.nan)
        g = _optional(gradient, (2, n, th, tw), np.nan)
        head = (self._h, _addr(a), n, Hh, Ww, _addr(t), th, tw, _addr(mp))
        if not weighted:
            _lib.check(self._lib.msiren_align_slices(*head, _addr(sums), _addr(wp), _addr(g)))
            return align.unpack(sums, wp, g)
        _lib.check(self._lib.msiren_align_slices_w(*head, _addr(w), _addr(gb), _addr(sums), _addr(wp), _addr(g)))
        return align.unpack_w(sums, wp, g)

    def _align_solve(self, images, targets, maps, rigid, centre, steps, trace, weighted, weights=None, intensity=None, estimate_intensity=True):
        """the body of align_solve[_rigid][_w]: ``maps`` (n, 6) starts the affine mode, ``rigid`` (n, 4) the rigid one (the other is None);
        ``steps`` from _steps()"""
        from . import align

        self._ensure_committed()
        a = _stack(images)
        t = _targets(targets, len(a))
        w, gb = _weights_intensity(weights, intensity, t.shape)
        n, Hh, Ww = a.shape
        th, tw = t.shape[1:]
        mp = None if maps is None else _maps(maps, n, 6)
        if rigid is not None and rigid.shape != (n, 4):
            raise ValueError(f"expected {n} angles and shifts of shape ({n}, 2), got a state of shape {rigid.shape}")
        opts = _lib.AlignSolveWOpts if weighted else _lib.AlignSolveOpts
        mode = align.AFFINE if rigid is None else align.RIGID
        intensity_mode = (align.ESTIMATE if estimate_intensity else align.FIXED) if weighted else 0
        iterations, lm = steps
        o = opts(C.sizeof(opts), mode, iterations, intensity_mode, *lm, float(centre[0]), float(centre[1]))
        out = np.zeros((n, 6), np.float32) if mp is None else mp.copy()
        rout = None if rigid is None else rigid.copy()
        report = np.zeros((n, 7 if weighted else 6), np.float64)
        tr = _optional(trace, (max(iterations, 0), n, 11 if weighted else 8), 0, np.float64)
        head = (self._h, _addr(a), n, Hh, Ww, _addr(t), th, tw, C.byref(o), _addr(mp), _addr(rigid))
        if not weighted:
            _lib.check(self._lib.msiren_align_solve(*head, _addr(out), _addr(rout), _addr(report), _addr(tr)))
            return align.solve_result(out, rout, report, tr)
        gout = _intensity_out(gb, n)
        _lib.check(self._lib.msiren_align_solve_w(*head, _addr(w), _addr(gb), _addr(out), _addr(gout), _addr(rout), _addr(report), _addr(tr)))
        return align.solve_result_w(out, gout, rout, report, tr)

    def align_cost(self, images, targets, maps, *, warped=False, gradient=False):
        """images (n, Hh, Ww), targets (n, th, tw), maps (n, 6) -> ``align.AlignResult``: every slice read on its target's lattice under its
        own affine map (``align.map_points``: pixel (i, j) at Y = a00 i + a01 j + t0, X = a10 i + a11 j + t1 in reconstruction pixels) and
        scored against the target on the device -- ``count`` valid pixels, ``cost`` = sum (R - T)^2, ``grad`` = d cost / d map (n, 6),
        ``jtj`` (n, 6, 6) the Gauss-Newton matrix; R and its gradient are the bits of ``resample_with_gradient`` (build-defined, DESIGN.md
        section 5.10; msiren_align_slices).  A NaN target pixel, an uncovered or non-finite point is left out.  fp64 sums in a fixed order:
        the same bits run to run, alone or in a batch.  ``warped`` / ``gradient``: also return R (n, th, tw) / (gY, gX) (2, n, th, tw)."""
        return self._align_cost(images, targets, maps, warped, gradient, False)

    def align_solve(self, images, targets, maps, *, iterations=12, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, trace=False):
        """images (n, Hh, Ww), targets (n, th, tw), maps (n, 6) -> ``align.SolveResult``: every slice aligned to its target over the six
        affine parameters, on the device -- ``align_cost``'s prologue once, then ``iterations`` evaluations with a Levenberg-Marquardt step
        behind each (per slice: accept a lower mean cost and lower the damping by ``down``, reject and raise it by ``up``), no host
        synchronisation in between (build-defined; msiren_align_solve).  ``maps`` of the result is the best map of
        every slice; bit for bit what ``align.solve_on_host`` gives around ``align_cost``.  ``trace``: also the trial map, cost and count
        of every evaluation (iterations, n, 8)."""
        steps = _steps(iterations, damping, down, up, lam_min, lam_max)
        return self._align_solve(images, targets, maps, None, (0.0, 0.0), steps, trace, False)

    def align_solve_rigid(self, images, targets, angle, shift, centre, *, iterations=12, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9,
                          trace=False):
        """As ``align_solve`` over rotation and in-plane shift: slice s starts at ``align.rigid_maps(angle, shift, centre)[s]`` (angle (n,)
        radians, shift (n, 2), centre (2,) = (Y, X); cos, sin and shift are formed in fp64 here) and every trial is a rigid map about
        ``centre`` (msiren_align_solve, mode 1).  ``angle`` and ``shift`` of the result are the best state's."""
        steps = _steps(iterations, damping, down, up, lam_min, lam_max)
        return self._align_solve(images, targets, None, _rigid2(angle, shift), centre, steps, trace, False)

    def align_cost_w(self, images, targets, maps, *, weights=None, intensity=None, warped=False, gradient=False):
        """``align_cost`` with a per-pixel weight and a per-slice gain and bias -> ``align.AlignResultW``: ``weights`` (n, th, tw) or None (all
        1; a weight that is zero, negative or not finite masks its pixel), ``intensity`` (n, 2) = (g, b) or None ((1, 0)); ``cost`` = sum w (g R
        + b - T)^2 over the valid pixels, ``wsum`` their weights, ``grad`` (n, 8) and ``jtj`` (n, 8, 8) over (a00, a01, t0, a10, a11, t1, g, b)
        (build-defined; msiren_align_slices_w).  Without weights and intensity the shared entries are ``align_cost``'s
        bits.  ``warped`` / ``gradient`` return R and (gY, gX) before gain and bias."""
        return self._align_cost(images, targets, maps, warped, gradient, True, weights, intensity)

    def align_solve_w(self, images, targets, maps, *, weights=None, intensity=None, estimate_intensity=True, iterations=12, damping=1e-3, down=0.1, up=10.0,
                      lam_min=1e-9, lam_max=1e9, trace=False):
        """``align_solve`` on ``align_cost_w`` -> ``align.SolveResultW``: every pixel weighted by ``weights`` (n, th, tw), the target modelled as
        g R + b per slice from ``intensity`` (n, 2) (None: (1, 0)).  ``estimate_intensity``: (g, b) are solved for together with the map (8
        parameters); False: they stay at their inputs (6).  The accept / reject rule compares cost / wsum (build-defined, DESIGN.md section 5.12;
        msiren_align_solve_w); bit for bit what ``align.solve_on_host_w`` gives around ``align_cost_w``.  ``trace``: (iterations, n, 11)."""
        steps = _steps(iterations, damping, down, up, lam_min, lam_max)
        return self._align_solve(images, targets, maps, None, (0.0, 0.0), steps, trace, True, weights, intensity, estimate_intensity)

    def align_solve_rigid_w(self, images, targets, angle, shift, centre, *, weights=None, intensity=None, estimate_intensity=True, iterations=12, damping=1e-3, down=0.1,
                            up=10.0, lam_min=1e-9, lam_max=1e9, trace=False):
        """As ``align_solve_w`` over rotation and in-plane shift (``align_solve_rigid``'s arguments): 5 parameters with the intensity, 3 without."""
        steps = _steps(iterations, damping, down, up, lam_min, lam_max)
        return self._align_solve(images, targets, None, _rigid2(angle, shift), centre, steps, trace, True, weights, intensity, estimate_intensity)

    # ---- targets against the stack read as a volume (DESIGN.md sections 5.13 to 5.16) ----
    def _align_volume_cost(self, images, targets, maps, warped, gradient, weighted, weights=None, intensity=None, robust=False, scale=None, rweight=False):
        """the body of align_volume_cost, align_volume_cost_w and (``robust``) align_volume_cost_r"""
        from . import align_robust as ar, align_volume as av

        self._ensure_committed()
        a = _stack(images)
        t = _targets(targets)
        w, gb = _weights_intensity(weights, intensity, t.shape)
        n, Hh, Ww = a.shape
        m, th, tw = t.shape
        mp = _maps(maps, m, 9)
        s = ar.scales(scale, m) if robust else None
        sums = np.zeros((m, av.SUMS_VW if weighted else av.SUMS_V), np.float64)
        wp = _optional(warped, (m, th, tw), np.nan)
        g = _optional(gradient, (3, m, th, tw), np.nan)
        rw = _optional(rweight, (m, th, tw), np.nan)
        head = (self._h, _addr(a), n, Hh, Ww, _addr(t), m, th, tw, _addr(mp))
        if not weighted:
            _lib.check(self._lib.msiren_align_volume(*head, _addr(sums), _addr(wp), _addr(g)))
            return av.unpack_v(sums, wp, g)
        if not robust:
            _lib.check(self._lib.msiren_align_volume_w(*head, _addr(w), _addr(gb), _addr(sums), _addr(wp), _addr(g)))
            return av.unpack_vw(sums, wp, g)
        _lib.check(self._lib.msiren_align_volume_r(*head, _addr(w), _addr(gb), _addr(s), _addr(sums), _addr(wp), _addr(g), _addr(rw)))
        return ar.unpack_r(sums, wp, g, rw)

    def _align_volume_solve(self, images, targets, maps, rigid, spacing, steps, trace, weighted, weights=None, intensity=None, estimate_intensity=True):
        """the body of align_volume_solve[_rigid][_w]: ``maps`` (m, 9) starts the affine mode, ``rigid`` = (planes, rotation, shift) the rigid one
        (the other is None); ``steps`` from _steps()"""
        from . import align, align_volume as av

        self._ensure_committed()
        a = _stack(images)
        t = _targets(targets)
        w, gb = _weights_intensity(weights, intensity, t.shape)
        n, Hh, Ww = a.shape
        m, th, tw = t.shape
        mp = None if maps is None else _maps(maps, m, 9)
        pl = None if rigid is None else _planes(rigid[0], m)
        state = None if rigid is None else _rigid3(rigid[1], rigid[2], m)
        opts = _lib.AlignVolumeSolveWOpts if weighted else _lib.AlignVolumeSolveOpts
        mode = align.AFFINE if rigid is None else align.RIGID
        intensity_mode = (av.ESTIMATE if estimate_intensity else av.FIXED) if weighted else 0
        iterations, lm = steps
        o = opts(C.sizeof(opts), mode, iterations, intensity_mode, *lm, float(spacing))
        out = np.zeros((m, 9), np.float32) if mp is None else mp.copy()
        rout = None if state is None else state.copy()
        report = np.zeros((m, 7 if weighted else 6), np.float64)
        tr = _optional(trace, (max(iterations, 0), m, 14 if weighted else 11), 0, np.float64)
        head = (self._h, _addr(a), n, Hh, Ww, _addr(t), m, th, tw, C.byref(o), _addr(mp), _addr(pl), _addr(state))
        if not weighted:
            _lib.check(self._lib.msiren_align_volume_solve(*head, _addr(out), _addr(rout), _addr(report), _addr(tr)))
            return av.solve_result_v(out, rout, report, tr)
        gout = _intensity_out(gb, m)
        _lib.check(self._lib.msiren_align_volume_solve_w(*head, _addr(w), _addr(gb), _addr(out), _addr(gout), _addr(rout), _addr(report), _addr(tr)))
        return av.solve_result_vw(out, gout, rout, report, tr)

    def _align_volume_solve_group(self, images, targets, planes, spacing, groups, rotation, shift, weights, intensity, estimate_intensity, steps, trace,
                                  robust=False, scale=None):
        """the body of align_volume_solve_group and (``robust``: with the scale behind the intensity) align_volume_solve_group_robust"""
        from . import align_group as ag, align_robust as ar, align_volume as av

        self._ensure_committed()
        a = _stack(images)
        t = _targets(targets)
        w, gb = _weights_intensity(weights, intensity, t.shape)
        n, Hh, Ww = a.shape
        m, th, tw = t.shape
        pl = _planes(planes, m)
        s = ar.scales(scale, m) if robust else None
        gs = np.ascontiguousarray(ag.group_offsets(groups, m), dtype=np.int32)
        G = len(gs) - 1
        state = _rigid3(rotation, shift, G)
        iterations, lm = steps
        opts = _lib.AlignVolumeSolveGroupOpts
        o = opts(C.sizeof(opts), iterations, av.ESTIMATE if estimate_intensity else av.FIXED, 0, *lm, float(spacing))
        out = np.zeros((m, 9), np.float32)
        gout = _intensity_out(gb, m)
        rout, report, trep = state.copy(), np.zeros((G, 7), np.float64), np.zeros((m, 3), np.float64)
        tr = _optional(trace, (max(iterations, 0), G, 15), 0, np.float64)
        head = (self._h, _addr(a), n, Hh, Ww, _addr(t), m, th, tw, C.byref(o), _addr(gs), G, _addr(pl), _addr(state), _addr(w), _addr(gb))
        tail = (_addr(out), _addr(gout), _addr(rout), _addr(report), _addr(trep), _addr(tr))
        if robust:
            _lib.check(self._lib.msiren_align_volume_solve_group_r(*head, _addr(s), *tail))
        else:
            _lib.check(self._lib.msiren_align_volume_solve_group(*head, *tail))
        return ag.solve_result_g(out, gout, rout, report, trep, tr)

    def align_volume_cost(self, images, targets, maps, *, warped=False, gradient=False):
        """images (n, Hh, Ww), n >= 2, targets (m, th, tw), maps (m, 9) -> ``align_volume.AlignResultV``: every target's lattice read in the stack
        as a volume under its own 3 x 3 map (``align_volume.map_points3``: pixel (i, j) at Z = z0 i + z1 j + tz in slice units, Y = y0 i + y1 j + ty,
        X = x0 i + x1 j + tx in reconstruction pixels) and scored against the target on the device -- ``count``, ``cost`` = sum (R - T)^2, ``grad``
        (m, 9), ``jtj`` (m, 9, 9); R and its gradient are the bits of ``resample_volume_with_gradient`` (build-defined, DESIGN.md section 5.13;
        msiren_align_volume).  m is independent of n.  ``warped`` / ``gradient``: also return R (m, th, tw) / (gZ, gY, gX) (3, m, th, tw)."""
        return self._align_volume_cost(images, targets, maps, warped, gradient, False)

    def align_volume_solve(self, images, targets, maps, *, iterations=12, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, trace=False):
        """images (n, Hh, Ww), targets (m, th, tw), maps (m, 9) -> ``align_volume.SolveResultV``: every target aligned to the volume over the nine
        parameters of its map, on the device -- ``align_volume_cost``'s prologue once, then ``iterations`` evaluations with ``align_solve``'s
        Levenberg-Marquardt step behind each, no host synchronisation (build-defined; msiren_align_volume_solve).  Bit for
        bit what ``align_volume.solve_on_host_v`` gives around ``align_volume_cost``.  ``trace``: (iterations, m, 11)."""
        steps = _steps(iterations, damping, down, up, lam_min, lam_max)
        return self._align_volume_solve(images, targets, maps, None, 1.0, steps, trace, False)

    def align_volume_solve_rigid(self, images, targets, planes, spacing, *, rotation=None, shift=None, iterations=12, damping=1e-3, down=0.1, up=10.0,
                                 lam_min=1e-9, lam_max=1e9, trace=False):
        """As ``align_volume_solve`` over a rigid motion of every target's nominal plane in physical space (6 parameters): ``planes`` (m, 12)
        float64 = (e_i, e_j, o, c), the lattice's two step vectors, its origin and the rotation centre as (Z, Y, X) triples in pixel units; slices are
        ``spacing`` pixels apart.  Starts at ``rotation`` (m, 3, 3) (None: the identity) and ``shift`` (m, 3) (None: zero); every trial map is
        ``align_volume.rigid_maps3`` of the state (msiren_align_volume_solve, mode 1).  ``rotation`` and ``shift`` of the result are the best state's."""
        steps = _steps(iterations, damping, down, up, lam_min, lam_max)
        return self._align_volume_solve(images, targets, None, (planes, rotation, shift), spacing, steps, trace, False)

    def align_volume_cost_w(self, images, targets, maps, *, weights=None, intensity=None, warped=False, gradient=False):
        """``align_volume_cost`` with a per-pixel weight and a per-target gain and bias -> ``align_volume.AlignResultVW``: ``weights`` (m, th, tw)
        or None (all 1; a weight that is zero, negative or not finite masks its pixel), ``intensity`` (m, 2) = (g, b) or None ((1, 0)); ``cost`` =
        sum w (g R + b - T)^2 over the valid pixels, ``wsum`` their weights, ``grad`` (m, 11) and ``jtj`` (m, 11, 11) over the map's nine
        parameters, then g, b (build-defined; msiren_align_volume_w).  Without weights and intensity the shared entries
        are ``align_volume_cost``'s bits.  ``warped`` / ``gradient`` return R and (gZ, gY, gX) before gain and bias."""
        return self._align_volume_cost(images, targets, maps, warped, gradient, True, weights, intensity)

    def align_volume_solve_w(self, images, targets, maps, *, weights=None, intensity=None, estimate_intensity=True, iterations=12, damping=1e-3, down=0.1, up=10.0,
                             lam_min=1e-9, lam_max=1e9, trace=False):
        """``align_volume_solve`` on ``align_volume_cost_w`` -> ``align_volume.SolveResultVW``: every pixel weighted by ``weights`` (m, th, tw), the
        target modelled as g R + b per target from ``intensity`` (m, 2) (None: (1, 0)).  ``estimate_intensity``: (g, b) are solved for together
        with the map (11 parameters); False: they stay at their inputs (9).  The accept / reject rule compares cost / wsum (build-defined,
        DESIGN.md section 5.14; msiren_align_volume_solve_w); bit for bit what ``align_volume.solve_on_host_vw`` gives around
        ``align_volume_cost_w``.  ``trace``: (iterations, m, 14)."""
        steps = _steps(iterations, damping, down, up, lam_min, lam_max)
        return self._align_volume_solve(images, targets, maps, None, 1.0, steps, trace, True, weights, intensity, estimate_intensity)

    def align_volume_solve_rigid_w(self, images, targets, planes, spacing, *, rotation=None, shift=None, weights=None, intensity=None, estimate_intensity=True,
                                   iterations=12, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, trace=False):
        """As ``align_volume_solve_w`` over a rigid motion of every target's nominal plane (``align_volume_solve_rigid``'s arguments): 8 parameters
        with the intensity, 6 without."""
        steps = _steps(iterations, damping, down, up, lam_min, lam_max)
        return self._align_volume_solve(images, targets, None, (planes, rotation, shift), spacing, steps, trace, True, weights, intensity, estimate_intensity)

    def align_volume_solve_group(self, images, targets, planes, spacing, groups, *, rotation=None, shift=None, weights=None, intensity=None, estimate_intensity=True,
                                 iterations=12, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, trace=False):
        """``align_volume_solve_rigid_w`` for GROUPS of consecutive targets that moved together (stacks, interleaves): one rigid state per group, every
        target with its own plane, weights and intensity -> ``align_group.SolveResultG``.  ``groups``: the (G + 1) offsets into the targets (first 0,
        last m, strictly ascending) or a list of G group sizes.  ``rotation`` (G, 3, 3) (None: the identity) and ``shift`` (G, 3) (None: zero) are per
        group.  A group is accepted or rejected on sum cost / sum wsum over its members; with ``estimate_intensity`` every member's (g, b) is solved
        for jointly with the group's motion (6 + 2 size parameters, the 2 x 2 blocks eliminated exactly), a member without valid pixels is placed by
        the others (build-defined; msiren_align_volume_solve_group); bit for bit what ``align_group.solve_on_host_g`` gives
        around ``align_volume_cost_w``.  One PHYSICAL motion per group needs the same centre c in every member's plane (e_i, e_j, o, c): the state
        moves a point p of a member to Rot (p - c) + c + shift with that member's c; the call does not check it.  ``trace``: (iterations, G, 15)."""
        steps = _steps(iterations, damping, down, up, lam_min, lam_max)
        return self._align_volume_solve_group(images, targets, planes, spacing, groups, rotation, shift, weights, intensity, estimate_intensity, steps, trace)

    def align_volume_cost_r(self, images, targets, maps, scale, *, weights=None, intensity=None, warped=False, gradient=False, rweight=False):
        """``align_volume_cost_w`` under a robust (Geman-McClure) loss -> ``align_robust.AlignResultR``: ``scale`` a scalar or (m,), s = (c sigma)^2 in
        squared intensity units; ``cost`` = sum w r^2 / (1 + r^2 / s) over the valid pixels, ``grad`` its exact gradient, ``jtj`` the majoriser's
        Gauss-Newton matrix, ``wsum`` the plain sum of the weights (build-defined; msiren_align_volume_r).  A target whose
        scale is not > 0 has count 0; with scale +inf the sums are ``align_volume_cost_w``'s bits.  ``rweight``: (m, th, tw) float32, the factor
        1 / (1 + r^2 / s)^2 of every valid pixel (towards 0: rejected), NaN elsewhere."""
        return self._align_volume_cost(images, targets, maps, warped, gradient, True, weights, intensity, True, scale, rweight)

    def align_volume_solve_group_robust(self, images, targets, planes, spacing, groups, scale, *, rotation=None, shift=None, weights=None, intensity=None,
                                        estimate_intensity=True, iterations=12, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, trace=False):
        """``align_volume_solve_group`` on ``align_volume_cost_r``: targets whose bad pixels come without a mask -> ``align_group.SolveResultG``.
        ``scale`` a scalar or (m,), fixed for the call (``align_robust.scale_from`` gives one from a quadratic pass); every other argument, the step
        rule and the result are ``align_volume_solve_group``'s, ``cost`` and the means the robust loss (build-defined, DESIGN.md section 5.16;
        msiren_align_volume_solve_group_r); bit for bit what ``align_robust.solve_on_host_r`` gives around ``align_volume_cost_r``.  Groups of one
        target each: the robust rigid solve per target.  With scale +inf: ``align_volume_solve_group``'s bits."""
        steps = _steps(iterations, damping, down, up, lam_min, lam_max)
        return self._align_volume_solve_group(images, targets, planes, spacing, groups, rotation, shift, weights, intensity, estimate_intensity, steps, trace,
                                              True, scale)

    # ---- targets against a stack that is just voxels ----
    def align_stack_cost(self, stack, targets, maps, *, scale=float("inf"), weights=None, intensity=None, warped=False, gradient=False, rweight=False):
        """``align_volume_cost_r`` against a plain voxel ``stack`` (n, H, W), n, H, W >= 2 -- what ``fuse_targets`` and the volume solves return, NaN
        holes included -- instead of the stack the network reconstructs -> ``align_robust.AlignResultR``.  targets (m, th, tw), maps (m, 9) in the same
        convention; the pixel is a trilinear read of the stack with its analytic gradient (``align_stack.read_stack``), NaN outside the stack and
        wherever one of its eight corners is not finite; everything behind the pixel is ``align_volume_cost_r``'s.  ``scale`` +inf (the default): the
        weighted square loss.  Build-defined (msiren_align_stack_r); bit for bit what ``align_stack.cost_on_host`` gives.  No
        images and no weights of the model are involved."""
        from . import align_robust as ar, align_volume as av

        self._ensure_handle()
        a = _stack(stack)
        t = _targets(targets)
        w, gb = _weights_intensity(weights, intensity, t.shape)
        n, Hh, Ww = a.shape
        m, th, tw = t.shape
        mp = _maps(maps, m, 9)
        s = ar.scales(scale, m)
        sums = np.zeros((m, av.SUMS_VW), np.float64)
        wp = _optional(warped, (m, th, tw), np.nan)
        g = _optional(gradient, (3, m, th, tw), np.nan)
        rw = _optional(rweight, (m, th, tw), np.nan)
        _lib.check(self._lib.msiren_align_stack_r(self._h, _addr(a), n, Hh, Ww, _addr(t), m, th, tw, _addr(mp), _addr(w), _addr(gb), _addr(s), _addr(sums), _addr(wp),
                                                  _addr(g), _addr(rw)))
        return ar.unpack_r(sums, wp, g, rw)

    def align_stack_solve(self, stack, targets, planes, spacing, *, groups=None, scale=float("inf"), rotation=None, shift=None, weights=None, intensity=None,
                          estimate_intensity=True, iterations=12, damping=1e-3, down=0.1, up=10.0, lam_min=1e-9, lam_max=1e9, trace=False):
        """``align_volume_solve_group_robust`` on ``align_stack_cost``: the targets registered to a plain voxel ``stack`` under one rigid motion per
        group -> ``align_group.SolveResultG``.  ``groups`` None: every target on its own.  Every other argument, the step rule and the result are
        ``align_volume_solve_group_robust``'s (build-defined; msiren_align_stack_solve_group_r); bit for bit what
        ``align_stack.solve_on_host_s`` gives.  With ``solve_volume_robust`` on either side it is the registration step of the outer loop
        reconstruct -> register -> reconstruct, with no images and no weights of the model."""
        from . import align_group as ag, align_robust as ar, align_volume as av

        self._ensure_handle()
        a = _stack(stack)
        t = _targets(targets)
        w, gb = _weights_intensity(weights, intensity, t.shape)
        n, Hh, Ww = a.shape
        m, th, tw = t.shape
        pl = _planes(planes, m)
        s = ar.scales(scale, m)
        gs = np.ascontiguousarray(list(range(m + 1)) if groups is None else ag.group_offsets(groups, m), dtype=np.int32)  # (None: singletons)
        G = len(gs) - 1
        state = _rigid3(rotation, shift, G)
        iterations, lm = _steps(iterations, damping, down, up, lam_min, lam_max)
        opts = _lib.AlignVolumeSolveGroupOpts
        o = opts(C.sizeof(opts), iterations, av.ESTIMATE if estimate_intensity else av.FIXED, 0, *lm, float(spacing))
        out = np.zeros((m, 9), np.float32)
        gout = _intensity_out(gb, m)
        rout, report, trep = state.copy(), np.zeros((G, 7), np.float64), np.zeros((m, 3), np.float64)
        tr = _optional(trace, (max(iterations, 0), G, 15), 0, np.float64)
        _lib.check(self._lib.msiren_align_stack_solve_group_r(self._h, _addr(a), n, Hh, Ww, _addr(t), m, th, tw, C.byref(o), _addr(gs), G, _addr(pl), _addr(state), _addr(w),
                                                              _addr(gb), _addr(s), _addr(out), _addr(gout), _addr(rout), _addr(report), _addr(trep), _addr(tr)))
        return ag.solve_result_g(out, gout, rout, report, trep, tr)

    # ---- the aligned targets back on the stack's grid, and the stack back on the targets (DESIGN.md sections 5.17 to 5.20) ----
    def fuse_targets(self, targets, maps, shape, spacing, *, thickness=None, weights=None, intensity=None, min_coverage=0.0, coverage=False):
        """The aligned targets put back onto the stack's voxel grid -> ``fuse.FuseResult``: targets (m, th, tw), ``maps`` (m, 9) and ``intensity``
        (m, 2) or None exactly the ``.maps`` and ``.intensity`` of any ``SolveResultV`` / ``VW`` / ``G``, ``shape`` = (n, H, W) the output grid,
        ``spacing`` pixels per slice, ``thickness`` the half-width in pixels of the quadratic through-plane window (None: ``spacing``), ``weights``
        (m, th, tw) or None (all 1; a weight that is zero, negative or not finite, and a pixel that is not finite, leave their tap out).  Every voxel
        is the normalised sum of window x bilinear weight x pixel weight x (T - b) / g over the targets that reach it, NaN where that coverage is
        not above ``min_coverage``; ``coverage``: return it too (build-defined; msiren_fuse_targets); bit for bit what
        ``fuse.fuse_on_host`` gives.  The robust call's ``rweight`` may be multiplied into ``weights`` to keep rejected pixels out of the stack.  No
        images and no weights of the model are involved: the result can go back into ``reconstruct`` / ``align_volume_*`` as ``images``."""
        from . import fuse

        self._ensure_handle()
        t, mp, w, gb = _fuse_inputs(targets, maps, weights, intensity)
        m, th, tw = t.shape
        (n, Hh, Ww), _, vol, cov, flags = _grid(shape, m, None, coverage)
        o = _lib.FuseOpts(C.sizeof(_lib.FuseOpts), 0, float(spacing), _thickness(thickness, spacing), float(min_coverage))
        _lib.check(self._lib.msiren_fuse_targets(self._h, _ptr(t, m), m, th, tw, _ptr(mp, m), _ptr(w, m), _ptr(gb, m), C.byref(o), n, Hh, Ww, _addr(vol),
                                                 _addr(cov), _ptr(flags, m)))
        return fuse.FuseResult(vol, cov, flags)

    def project_volume(self, volume, maps, shape, spacing, *, thickness=None, intensity=None, min_coverage=0.0, targets=None, weights=None, coverage=False,
                       residual=False, stats=False):
        """The way back from ``fuse_targets`` -> ``fuse.ProjectResult``: the stack ``volume`` (n, H, W) gathered onto the lattices ``shape`` = (th, tw)
        of the m targets of ``maps`` (m, 9), with exactly the weights of the fusion (``spacing``, ``thickness``, ``intensity``, ``min_coverage`` as
        there): ``simulated`` is what each target should look like given the stack, g R + b of the normalised sum, NaN where the ``coverage`` (returned
        on request) is not above ``min_coverage``.  With ``targets`` (m, th, tw) and ``weights`` (m, th, tw) or None (all 1): ``residual`` = targets -
        simulated and ``stats`` (m, 4) = (count, sum w, sum w r, sum (w r) r) per target, on request (build-defined, DESIGN.md section 5.18;
        msiren_project_volume); bit for bit what ``fuse.project_on_host`` and ``fuse.project_stats_on_host`` give.  No images and no weights of the
        model are involved."""
        from . import fuse

        self._ensure_handle()
        vol = _f32(volume)
        if vol.ndim != 3:
            raise ValueError(f"expected volume (n, H, W), got shape {vol.shape}")
        mp = _maps(maps, None, 9)
        if len(shape) != 2:
            raise ValueError(f"expected shape = (th, tw), got {shape!r}")
        m, (th, tw) = len(mp), (int(s) for s in shape)
        if targets is None and (weights is not None or residual or stats):
            raise ValueError("weights, residual and stats need targets")
        t = None if targets is None else _exactly(targets, (m, th, tw), "targets")
        w, gb = _weights_intensity(weights, intensity, (m, th, tw))
        n, Hh, Ww = vol.shape
        o = _lib.FuseOpts(C.sizeof(_lib.FuseOpts), 0, float(spacing), _thickness(thickness, spacing), float(min_coverage))
        ok = th > 0 and tw > 0  # (the library refuses the others: nothing is allocated for them here)
        sim = np.full((m, th, tw) if ok else (m, 0, 0), np.nan, np.float32)
        cov = _optional(coverage, sim.shape, 0)
        res = _optional(residual, sim.shape, np.nan)
        st = _optional(stats, (m, 4), 0, np.float64)
        flags = np.zeros(m, np.int32)
        _lib.check(self._lib.msiren_project_volume(self._h, _ptr(vol, vol.size), n, Hh, Ww, _ptr(mp, m), _ptr(gb, m), C.byref(o), m, th, tw, _ptr(t, m),
                                                   _ptr(w, m), _ptr(sim, m), _ptr(cov, m), _ptr(res, m), _ptr(st, m), _ptr(flags, m)))
        return fuse.ProjectResult(sim, cov, res, st, flags)

    def solve_volume(self, targets, maps, shape, spacing, *, iterations, lam=0.0, thickness=None, weights=None, intensity=None, min_coverage=0.0, start=None,
                     coverage=False, history=False):
        """The stack that best explains all aligned targets at once -> ``solve_volume.SolveVolumeResult``: ``iterations`` steps of conjugate gradients,
        in one device call, on 1/2 sum w g g (tau - P x)^2 + 1/2 ``lam`` sum over the 6-neighbour edges of c (x_u - x_v)^2, with P ``project_volume``'s
        row-normalised gather, tau = (T - b) / g, and c = 1 in plane, 1 / spacing^2 through plane.  targets, maps, shape = (n, H, W), spacing,
        thickness, weights, intensity and min_coverage as in ``fuse_targets``; ``start`` (n, H, W) or None: the fusion.  The support is the finite
        voxels of the start; the volume is NaN elsewhere.  ``coverage``: the fusion's coverage too; ``history``: (iterations + 1, 2) = (<r, r>,
        <p, A p>) per iteration too.  ``stopped_at``: the iteration at which the solve broke down (rho == 0, or gamma not finite or not > 0), else -1.
        Build-defined (msiren_solve_volume); bit for bit what ``solve_volume.solve_volume_on_host`` gives.  No images and no
        weights of the model are involved."""
        from . import solve_volume as sv

        self._ensure_handle()
        t, mp, w, gb = _fuse_inputs(targets, maps, weights, intensity)
        m, th, tw = t.shape
        (n, Hh, Ww), st, vol, cov, flags = _grid(shape, m, start, coverage)
        iterations = int(iterations)
        o = _lib.SolveOpts(C.sizeof(_lib.SolveOpts), iterations, float(spacing), _thickness(thickness, spacing), float(min_coverage), float(lam))
        hist = _optional(history, (max(iterations, 0) + 1, 2), np.nan, np.float64)
        stopped = np.full(1, -1, np.int32)
        _lib.check(self._lib.msiren_solve_volume(self._h, _ptr(t, m), m, th, tw, _ptr(mp, m), _ptr(w, m), _ptr(gb, m), C.byref(o), n, Hh, Ww, _ptr(st, vol.size),
                                                 _addr(vol), _addr(cov), _addr(hist), _ptr(flags, m), _addr(stopped)))
        return sv.SolveVolumeResult(vol, cov, hist, flags, int(stopped[0]))

    def solve_volume_robust(self, targets, maps, shape, spacing, scale, *, rounds, iterations, anneal=1.0, lam=0.0, thickness=None, weights=None, intensity=None,
                            min_coverage=0.0, start=None, coverage=False, history=False, rweight=False, stats=False):
        """``solve_volume`` with outlier rejection -> ``solve_volume_robust.SolveVolumeRobustResult``: ``rounds`` reweighting rounds in one device
        call.  Each round recomputes every pixel's Geman-McClure weight omega = 1 / (1 + e^2 / s)^2 from the residual e = T - (g P x + b) of the
        current iterate and runs ``iterations`` steps of ``solve_volume``'s conjugate gradients on the reweighted normal equations, warm-started from
        x in fp64.  ``scale`` a scalar or (m,), (c sigma)^2 in squared target-intensity units as in ``align_volume_cost_r`` (+inf: the quadratic
        loss); the scale of round t is ``scale`` x ``anneal``^(rounds - 1 - t): a graduated schedule that ends on ``scale``.  Every other argument as
        in ``solve_volume``.  ``history``: (rounds, iterations + 1, 2) too; ``rweight``: the final omega per pixel (m, th, tw), NaN where the pixel
        takes no part; ``stats``: (m, 4) = (count, sum w, sum w omega, sum w om e^2) per target -- sum w omega / sum w tells the rejected slices.
        ``stopped_at`` (rounds,): per round the iteration at which it broke down, else -1.  Build-defined (DESIGN.md section 5.20;
        msiren_solve_volume_r); bit for bit what ``solve_volume_robust.solve_volume_robust_on_host`` gives.  With rounds = 1 and scale +inf:
        ``solve_volume``'s bits.  No images and no weights of the model are involved."""
        from . import align_robust as ar, solve_volume_robust as svr

        self._ensure_handle()
        t, mp, w, gb = _fuse_inputs(targets, maps, weights, intensity)
        m, th, tw = t.shape
        (n, Hh, Ww), st, vol, cov, flags = _grid(shape, m, start, coverage)
        s = ar.scales(scale, m)
        rounds, iterations = int(rounds), int(iterations)
        o = _lib.SolveROpts(C.sizeof(_lib.SolveROpts), iterations, rounds, 0, float(spacing), _thickness(thickness, spacing), float(min_coverage), float(lam),
                            float(anneal))
        nr = min(max(rounds, 0), 64)  # (the library refuses the others)
        hist = _optional(history, (nr, max(iterations, 0) + 1, 2), np.nan, np.float64)
        stopped = np.full(nr, -1, np.int32)
        rw = _optional(rweight, t.shape, np.nan)
        sts = _optional(stats, (m, 4), 0, np.float64)
        _lib.check(self._lib.msiren_solve_volume_r(self._h, _ptr(t, m), m, th, tw, _ptr(mp, m), _ptr(w, m), _ptr(gb, m), _ptr(s, m), C.byref(o), n, Hh, Ww,
                                                   _ptr(st, vol.size), _addr(vol), _addr(cov), _ptr(hist, nr), _ptr(flags, m), _ptr(stopped, nr), _ptr(rw, m),
                                                   _ptr(sts, m)))
        return svr.SolveVolumeRobustResult(vol, cov, hist, flags, stopped, rw, sts)

    # ---- the scale of the robust calls from the residuals themselves ----
    def residual_scale(self, targets, simulated=None, *, tune, weights=None, intensity=None, groups=None, quantile=0.5, centre=False, floor=0.0, stats=False):
        """The ``scale`` every robust call takes, estimated on the device from an exact order statistic of the residuals ->
        ``residual_scale.ResidualScaleResult``.  targets (m, th, tw); ``simulated`` (m, th, tw): the residual is targets - (g simulated + b) with
        ``intensity`` (m, 2) or None ((1, 0)) -- ``warped`` of the align calls with their intensity, ``simulated`` of ``project_volume`` without -- or
        None: the targets already are residuals.  A pixel counts where the residual is finite and its ``weights`` entry (None: 1) is finite and > 0.
        ``groups``: offsets or sizes of groups of consecutive targets as in ``align_stack_solve`` (None: every target on its own; ``[m]`` pools all):
        one statistic per group.  Per group the element of rank floor(quantile (count - 1)) of |e|, or with ``centre`` of |e - c| with c that element
        of the e themselves -- no interpolation -- as d; scale = max((tune d)^2, floor) for every target of the group, +inf where no pixel counts.
        ``tune`` = c ``residual_scale.MAD_TO_SIGMA`` gives (c sigma)^2.  ``stats``: (count, k, c, d) per group too.  Build-defined (DESIGN.md section
        5.23; msiren_residual_scale); bit for bit what ``residual_scale.residual_scale_on_host`` gives.  No images and no weights of the model are
        involved."""
        from . import align_group as ag, residual_scale as rs

        self._ensure_handle()
        t = _targets(targets)
        m, th, tw = t.shape
        sim = None if simulated is None else _exactly(simulated, t.shape, "simulated")
        w, gb = _weights_intensity(weights, intensity, t.shape)
        if gb is not None and sim is None:
            raise ValueError("intensity needs simulated")
        gs = None if groups is None else np.ascontiguousarray(ag.group_offsets(groups, m), dtype=np.int32)
        G = 0 if gs is None else len(gs) - 1
        o = _lib.ScaleOpts(C.sizeof(_lib.ScaleOpts), int(bool(centre)), float(quantile), float(tune), float(floor))
        scale = np.full(m, np.inf, np.float64)
        st = _optional(stats, (G if gs is not None else m, 4), 0, np.float64)
        _lib.check(self._lib.msiren_residual_scale(self._h, _ptr(t, m), _ptr(sim, m), _ptr(w, m), _ptr(gb, m), m, th, tw, C.byref(o), _addr(gs), G, _ptr(scale, m),
                                                   _ptr(st, m)))
        return rs.ResidualScaleResult(scale, st)

    # ---- every target predicted from the others ----
    def leave_out_targets(self, targets, maps, shape, spacing, *, groups=None, thickness=None, weights=None, intensity=None, min_coverage=0.0, coverage=False,
                          residual=False, stats=False, volume=False):
        """Every target as the OTHER targets predict it -> ``leave_out.LeaveOutResult``: ``simulated`` (m, th, tw) is what ``project_volume`` would read
        from the ``fuse_targets`` stack of all targets outside the target's own group, in one device call instead of one fusion and one projection per
        group.  targets, maps, shape = (n, H, W), spacing, thickness, weights, intensity and min_coverage as in ``fuse_targets``; ``groups``: offsets or
        sizes of groups of consecutive targets as in ``residual_scale`` (None: every target on its own) -- a whole group is left out at a time, as the
        slices of one acquisition are.  A voxel takes part where the coverage that is left without the group is above ``min_coverage`` and above
        ``leave_out.LEAVE_OUT_FLOOR`` of the voxel's whole coverage; ``simulated`` is NaN where no such voxel reaches the pixel.  ``coverage``: the
        pixels' coverage too; ``residual`` = targets - simulated and ``stats`` (m, 4) = (count, sum w, sum w r, sum (w r) r) as in ``project_volume``;
        ``volume``: the plain fusion of all targets and its coverage too, ``fuse_targets``' bits.  The residual is not biased towards zero as the
        residual against a stack that the target helped to build: the input for ``residual_scale``, and the score for choosing ``thickness`` and
        ``min_coverage``.  Build-defined (msiren_leave_out_targets); bit for bit what ``leave_out.leave_out_on_host`` gives.
        No images and no weights of the model are involved."""
        from . import align_group as ag, leave_out as lo

        self._ensure_handle()
        t, mp, w, gb = _fuse_inputs(targets, maps, weights, intensity)
        m, th, tw = t.shape
        (n, Hh, Ww), _, vol, vcov, flags = _grid(shape, m, None, volume)
        if not volume:
            vol = None
        gs = None if groups is None else np.ascontiguousarray(ag.group_offsets(groups, m), dtype=np.int32)
        G = 0 if gs is None else len(gs) - 1
        o = _lib.FuseOpts(C.sizeof(_lib.FuseOpts), 0, float(spacing), _thickness(thickness, spacing), float(min_coverage))
        sim = np.full(t.shape, np.nan, np.float32)
        cov = _optional(coverage, t.shape, 0)
        res = _optional(residual, t.shape, np.nan)
        st = _optional(stats, (m, 4), 0, np.float64)
        _lib.check(self._lib.msiren_leave_out_targets(self._h, _ptr(t, m), m, th, tw, _ptr(mp, m), _ptr(w, m), _ptr(gb, m), C.byref(o), _addr(gs), G, n, Hh, Ww,
                                                      _ptr(sim, m), _ptr(cov, m), _ptr(res, m), _ptr(st, m), _ptr(flags, m), _addr(vol), _addr(vcov)))
        return lo.LeaveOutResult(sim, cov, res, st, flags, vol, vcov)
