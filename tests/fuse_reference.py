"""An independent formulation of msiren_fuse_targets for tests/test_fuse_reference.py.  Not a test module.

Where the rule projects the voxel onto the target's plane through the Gram matrix of (a, b) and measures the distance through the un-normalised normal
c = a x b, this one solves the 3 x 3 system [a b n] (i, j, d) = v - t with the UNIT normal n by ``np.linalg.solve``, voxel by voxel in a Python loop, and
takes the window from the distance itself: k = 1 - (d / thickness)^2.  The bilinear read is written over the four corner pixels by name.  Nothing is
shared with mri_inr_amd/fuse.py but the definition of the result.

It also reports what the comparison's bound needs: the largest condition number of the systems, the largest |(i, j, d)| that passed, how many targets
reached a voxel at most, and which voxels have a target within ``edge`` of the lattice's border without being exactly on it (there the two
formulations may disagree about whether the target contributes at all: those voxels are left out of the comparison, and counted)."""
import collections

import numpy as np

Reference = collections.namedtuple("Reference", "volume coverage flags cond scale reach near_edge")


def fuse(targets, maps, shape, spacing, *, thickness=None, weights=None, intensity=None, min_coverage=0.0, edge=1e-9):
    targets = np.asarray(targets, np.float32)
    m, th, tw = targets.shape
    n, H, W = shape
    thickness = float(spacing if thickness is None else thickness)
    w_all = np.ones(targets.shape, np.float32) if weights is None else np.asarray(weights, np.float32)
    gb = np.tile([1.0, 0.0], (m, 1)) if intensity is None else np.asarray(intensity, np.float32).astype(np.float64)
    mp = np.asarray(maps, np.float32).astype(np.float64).reshape(m, 3, 3)
    flags = np.zeros(m, np.int32)
    systems = []
    for q in range(m):
        A = mp[q].copy()
        A[0] *= spacing                      # Z row in pixels: columns a, b, t
        a, b = A[:, 0], A[:, 1]
        nrm = np.cross(a, b)
        if not np.isfinite(mp[q]).all() or not np.linalg.norm(nrm) ** 2 > 0 or not np.isfinite(np.linalg.norm(nrm) ** 2):
            flags[q] |= 1
        if not np.isfinite(gb[q]).all() or gb[q, 0] == 0:
            flags[q] |= 2
        systems.append(None if flags[q] else (np.stack([a, b, nrm / np.linalg.norm(nrm)], axis=1), A[:, 2]))
    cond = max([np.linalg.cond(s[0]) for s in systems if s is not None], default=1.0)
    num, den = np.zeros(shape), np.zeros(shape)
    reach, near = np.zeros(shape, np.int64), np.zeros(shape, bool)
    scale = 1.0
    for z in range(n):
        for y in range(H):
            for x in range(W):
                v = np.array([z * spacing, y, x], np.float64)
                for q, s in enumerate(systems):
                    if s is None:
                        continue
                    i, j, d = np.linalg.solve(s[0], v - s[1])
                    k = 1.0 - (d / thickness) ** 2
                    if not k > 0:
                        continue
                    for c, hi in ((i, th - 1), (j, tw - 1)):
                        if (0 < abs(c) <= edge) or (0 < abs(c - hi) <= edge):
                            near[z, y, x] = True
                    if not (0 <= i <= th - 1 and 0 <= j <= tw - 1):
                        continue
                    scale = max(scale, abs(i), abs(j), abs(d))
                    i0, j0 = min(int(np.floor(i)), th - 2), min(int(np.floor(j)), tw - 2)
                    fi, fj = i - i0, j - j0
                    corners = {(i0, j0): (1 - fi) * (1 - fj), (i0, j0 + 1): (1 - fi) * fj, (i0 + 1, j0): fi * (1 - fj), (i0 + 1, j0 + 1): fi * fj}
                    sn = sd = 0.0
                    for (r, c), beta in corners.items():
                        T, w = float(targets[q, r, c]), float(w_all[q, r, c])
                        if np.isfinite(T) and np.isfinite(w) and w > 0:
                            sn += beta * w * (T - gb[q, 1]) / gb[q, 0]
                            sd += beta * w
                    num[z, y, x] += k * sn
                    den[z, y, x] += k * sd
                    reach[z, y, x] += 1
    with np.errstate(all="ignore"):
        volume = np.where(den > min_coverage, num / den, np.nan)
    return Reference(volume, den, flags, float(cond), float(scale), int(reach.max()), near)
