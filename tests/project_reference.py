"""An independent formulation of msiren_project_volume for tests/test_project_reference.py.  Not a test module.

Where the rule goes over the voxels and scatters each one's four bilinear taps, this one goes over the PIXELS: per target it places every voxel at
(i, j, d) on the target by solving the 3 x 3 system [a b n] (i, j, d) = v - t with the UNIT normal n (``np.linalg.solve``, as tests/fuse_reference.py
does), and per pixel (pi, pj) it sums over ALL voxels the weight k tent(i - pi) tent(j - pj) with the tent function tent(u) = max(0, 1 - |u|) and the
window k = 1 - (d / thickness)^2 of the distance itself.  No floor, no base index, no tap: the bilinear weights of the rule ARE the tent function (at
the clamped last row, fi = 1 gives the taps tent(1) = 0 and tent(0) = 1).  Nothing is shared with mri_inr_amd/fuse.py but the definition of the result.

It also reports what the comparison's bound needs: the largest condition number of the systems, the largest |(i, j, d)| that passed, how many voxels
reached a pixel at most, and which pixels have a voxel within ``edge`` of the lattice's border without being exactly on it (there the two formulations
may disagree about whether the voxel contributes at all: those pixels are left out of the comparison, and counted)."""
import collections

import numpy as np

Reference = collections.namedtuple("Reference", "simulated coverage flags cond scale reach near_edge ratio")


def project(volume, maps, shape, spacing, *, thickness=None, intensity=None, min_coverage=0.0, edge=1e-9):
    volume = np.asarray(volume, np.float32)
    n, H, W = volume.shape
    th, tw = shape
    thickness = float(spacing if thickness is None else thickness)
    mp = np.asarray(maps, np.float32).astype(np.float64).reshape(-1, 3, 3)
    m = len(mp)
    gb = np.tile([1.0, 0.0], (m, 1)) if intensity is None else np.asarray(intensity, np.float32).astype(np.float64)
    z, y, x = np.mgrid[0:n, 0:H, 0:W].astype(np.float64)
    v = np.stack([z.ravel() * spacing, y.ravel(), x.ravel()])            # (3, voxels)
    V = volume.astype(np.float64).ravel()
    finite = np.isfinite(V)
    V = np.where(finite, V, 0.0)
    flags = np.zeros(m, np.int32)
    sim, ratio, cov = np.full((m, th, tw), np.nan), np.full((m, th, tw), np.nan), np.zeros((m, th, tw))
    reach, near = np.zeros((m, th, tw), np.int64), np.zeros((m, th, tw), bool)
    cond, scale = 1.0, 1.0
    for q in range(m):
        A = mp[q].copy()
        A[0] *= spacing                                                   # Z row in pixels: columns a, b, t
        a, b = A[:, 0], A[:, 1]
        nrm = np.cross(a, b)
        if not np.isfinite(mp[q]).all() or not np.linalg.norm(nrm) ** 2 > 0 or not np.isfinite(np.linalg.norm(nrm) ** 2):
            flags[q] |= 1
        if not np.isfinite(gb[q]).all() or gb[q, 0] == 0:
            flags[q] |= 2
        if flags[q]:
            continue
        S = np.stack([a, b, nrm / np.linalg.norm(nrm)], axis=1)
        cond = max(cond, float(np.linalg.cond(S)))
        i, j, d = np.linalg.solve(S, v - A[:, 2:3])
        k = 1.0 - (d / thickness) ** 2
        seen = finite & (k > 0)
        inside = seen & (i >= 0) & (i <= th - 1) & (j >= 0) & (j <= tw - 1)
        border = seen & (((np.abs(i) > 0) & (np.abs(i) <= edge)) | ((np.abs(i - (th - 1)) > 0) & (np.abs(i - (th - 1)) <= edge))
                         | ((np.abs(j) > 0) & (np.abs(j) <= edge)) | ((np.abs(j - (tw - 1)) > 0) & (np.abs(j - (tw - 1)) <= edge)))
        if inside.any():
            scale = max(scale, float(np.abs(i[inside]).max()), float(np.abs(j[inside]).max()), float(np.abs(d[inside]).max()))
        for pi in range(th):
            ti = np.maximum(0.0, 1.0 - np.abs(i - pi))
            for pj in range(tw):
                w = ti * np.maximum(0.0, 1.0 - np.abs(j - pj))
                near[q, pi, pj] = bool((border & (w > 0)).any())
                kw = np.where(inside, k * w, 0.0)
                den = float(kw.sum())
                reach[q, pi, pj] = int((kw > 0).sum())
                cov[q, pi, pj] = den
                if den > min_coverage:
                    ratio[q, pi, pj] = float((kw * V).sum()) / den
                    sim[q, pi, pj] = gb[q, 0] * ratio[q, pi, pj] + gb[q, 1]
    return Reference(sim, cov, flags, cond, scale, int(reach.max()), near, ratio)
