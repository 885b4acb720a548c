"""What tools/fuse_cost.py, tools/project_cost.py and tools/solve_volume_cost.py share: the model, the workload of 64 targets of 320 x 320 on planes through
a 16 x 320 x 320 grid (slices 4 pixels apart, small tilts within +-0.01 slice per pixel, in-plane rotation within +-0.02 rad and shifts within +-2
pixels, smooth weights, a gain and bias per target), one profiled call, and the demonstration that follows a robust alignment of section 5.16's
workload (tools/align_robust_cost.py: 16 targets in 4 groups, a corrupted block left unmasked)."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, align_robust as ar, align_volume as av, synthetic as syn  # noqa: E402

N, NS, MT, SPACING = 320, 16, 64, 4.0
GRID = (NS, N, N)
C0 = 0.5 * (N - 1)


def model(committed=True):
    """the model on the device; ``committed`` False: a handle without weights, which the three calls do not need"""
    m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0,
                       use_bias=True, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                       outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda:0", activation="sine", precision="fp32")
    if committed:
        m.load_state_dict(syn.make_state_dict(seed=7, trained_like=True))
        m.to("cuda:0").eval()
    else:
        m._ensure_handle()
    return m


def workload():
    """-> (maps (MT, 9), targets, weights (MT, N, N), gb (MT, 2)) float32; the targets carry their gain and bias"""
    rng = np.random.default_rng(17)
    maps = np.zeros((MT, 9), np.float32)
    for q in range(MT):
        ang, z0, z1 = rng.uniform(-0.02, 0.02), rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)
        c, s = np.cos(ang), np.sin(ang)
        zc = -0.25 + q * (NS - 0.5) / (MT - 1)  # Z at the target's centre: -0.25 .. 15.25 slices
        maps[q] = (z0, z1, zc - (z0 + z1) * C0, c, -s, C0 - (c - s) * C0 + rng.uniform(-2, 2), s, c, C0 - (s + c) * C0 + rng.uniform(-2, 2))
    i, j = np.mgrid[0:N, 0:N]
    targets = np.stack([syn.make_slice(q % NS, N, N) for q in range(MT)]).astype(np.float32)
    weights = np.tile((0.2 + 0.8 * np.exp(-(((i - 0.5 * N) / (0.6 * N)) ** 2 + ((j - 0.5 * N) / (0.6 * N)) ** 2))).astype(np.float32), (MT, 1, 1))
    gb = np.stack([np.linspace(0.8, 1.25, MT), np.linspace(-0.05, 0.1, MT)], axis=1).astype(np.float32)
    targets = (gb[:, :1, None] * targets + gb[:, 1:, None]).astype(np.float32)
    return maps, targets, weights, gb


def profiled(m, fn, name):
    """the device ms of the one profile entry ``name`` that fn() leaves"""
    _lib.check(m._lib.msiren_profile_enable(m._h, 1))
    fn()
    m.sync()
    e = [e for e in m.profile_kernels() if e["kernel"] == name]
    _lib.check(m._lib.msiren_profile_enable(m._h, 0))
    assert len(e) == 1 and e[0]["launches"] == 1, e
    return e[0]["ms_total"]


def rotation_of(vec):
    t = np.linalg.norm(vec)
    k = vec / t
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


Aligned = collections.namedtuple("Aligned", "goal_w clean_targets open_w robust_w rw second truth inside block")
Aligned.__doc__ = """goal_w: the 16 targets with + 5 in ``block``; clean_targets: without it; open_w: the weights with nothing masking the block; robust_w:
open_w x rweight; second: the robust solve's result; truth: the maps the targets were made with; inside (n, H, W) bool: the block in the grid"""


def robust_alignment(m, weights, gb):
    """section 5.16's workload aligned: a quadratic pass, then the robust one, then its rweight"""
    DT, G, EVALS, TUNE = 16, 4, 12, 0.25
    SIZE = DT // G
    block = (slice(None), slice(100, 140), slice(120, 180))
    stack = np.stack([syn.make_slice(s, N, N) for s in range(NS)])
    planes = np.zeros((DT, 12))
    for q in range(DT):
        first = SIZE * (q // SIZE)
        zc = SPACING * (0.5 + (first + 0.5 * (SIZE - 1)) * (NS - 2.0) / (DT - 1))
        planes[q] = np.concatenate([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [SPACING * (0.5 + q * (NS - 2.0) / (DT - 1)), 0.0, 0.0], [zc, C0, C0]])
    group_start = np.arange(0, DT + 1, SIZE, dtype=np.int32)
    group_of = np.repeat(np.arange(G), SIZE)
    lin = np.linspace(-1.0, 1.0, G)
    rot_true = np.stack([rotation_of(np.deg2rad([0.1 * a, 0.1 * (0.5 - a), 0.5 * a + 0.01])) for a in lin])
    shift_true = np.stack([0.4 * lin, 0.8 * lin, -0.6 * lin], axis=1)
    truth = av.rigid_maps3(rot_true[group_of], shift_true[group_of], planes, SPACING)
    goal = m.align_volume_cost(stack, np.zeros((DT, N, N), np.float32), truth, warped=True).warped
    gbt = gb[:DT]
    goal_w = (gbt[:, :1, None] * goal + gbt[:, 1:, None]).astype(np.float32)
    goal_w[block] += 5.0
    open_w = weights[:DT].copy()
    open_w[block] = 1.0  # nothing masks the corruption
    kw = dict(weights=open_w, estimate_intensity=True, iterations=EVALS)
    quad = m.align_volume_solve_group(stack, goal_w, planes, SPACING, group_start, **kw)
    second = m.align_volume_solve_group_robust(stack, goal_w, planes, SPACING, group_start, ar.scale_from(quad, TUNE), rotation=quad.rotation, shift=quad.shift,
                                               intensity=quad.intensity, **kw)
    rw = m.align_volume_cost_r(stack, goal_w, second.maps, ar.scale_from(quad, TUNE), weights=open_w, intensity=second.intensity, rweight=True).rweight
    clean_targets = (gbt[:, :1, None] * goal + gbt[:, 1:, None]).astype(np.float32)
    inside = np.zeros(GRID, bool)
    inside[block] = True
    return Aligned(goal_w, clean_targets, open_w, open_w * np.nan_to_num(rw, nan=0.0), rw, second, truth, inside, block)


def errors(volume, clean, inside):
    """a stack against the one made from the uncorrupted targets, inside and outside the block"""
    e = np.abs(volume.astype(np.float64) - clean)
    ok = np.isfinite(e)
    return {"covered_share": round(float(ok.mean()), 4), "mean_error_outside_the_block": float(e[ok & ~inside].mean()),
            "mean_error_inside_the_block": float(e[ok & inside].mean()) if (ok & inside).any() else None, "covered_inside_the_block": int((ok & inside).sum()),
            "voxels_inside_the_block": int(inside.sum())}
