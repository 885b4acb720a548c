#!/usr/bin/env python3
"""What msiren_fuse_targets costs: 64 targets of 320 x 320 on planes through a 16 x 320 x 320 grid, slices 4 pixels apart, small
tilts (within +-0.01 slice per pixel) and in-plane motion (rotation within +-0.02 rad, shifts within +-2 pixels), thickness = spacing, smooth weights and
a gain and bias per target.

 (a) the device ms of the profile entry "fuse_kernels" (set-up and gather) for msiren_fuse_targets_dev, median and spread over the repetitions;
 (b) the share of (tile, target) pairs the tile-level cull VISITS, computed on the host from the same rule (the kernel's cull restated in numpy), beside
     the share of pairs in which some voxel contributes -- what an exact cull would visit;
 (c) the fp64 operations of the rule the kernel executes (+ - * / counted as one each: the cull's per lane of every pair, the voxel's per visited pair,
     the taps' per contributing pair) over the time, against the card's 78.6 TFLOP/s vector fp64 peak, and the bytes the taps gather (4 x 4, 8 with
     weights, per contributing pair) plus the stores against 8 TB/s: which of the two bounds the kernel;
 (d) the seconds mri_inr_amd/fuse.py: fuse_on_host takes on the same inputs, and that the device returned its bits;
 (e) a demonstration on section 5.16's workload (tools/align_robust_cost.py: 16 targets in 4 groups, a corrupted block left unmasked):
     align_volume_solve_group_robust, then fuse_targets with weights x rweight against fuse_targets with the plain weights, each without and with a
     min_coverage of 0.05 -- the fused stack's error against the fusion of the UNcorrupted targets under the same maps, inside and outside the block.
     (The fusion is normalised: a weight that is small everywhere in a voxel's neighbourhood changes nothing until min_coverage drops the voxel.)

No threshold is set: the figures go to LAB_NOTES.md section 31.  One JSON line per measurement.  Usage: python tools/fuse_cost.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, align_robust as ar, align_volume as av, fuse, synthetic as syn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
N, NS, MT, SPACING, TILE = 320, 16, 64, 4.0, 16
GRID = (NS, N, N)
PEAK_FP64, PEAK_HBM = 78.6e12, 8.0e12

m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0,
                   use_bias=True, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                   outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda:0", activation="sine", precision="fp32")
m.load_state_dict(syn.make_state_dict(seed=7, trained_like=True))
m.to("cuda:0").eval()
lib, h = m._lib, m._h

rng = np.random.default_rng(17)
maps = np.zeros((MT, 9), np.float32)
c0 = 0.5 * (N - 1)
for q in range(MT):
    ang, z0, z1 = rng.uniform(-0.02, 0.02), rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)
    c, s = np.cos(ang), np.sin(ang)
    zc = -0.25 + q * (NS - 0.5) / (MT - 1)  # Z at the target's centre: -0.25 .. 15.25 slices
    maps[q] = (z0, z1, zc - (z0 + z1) * c0, c, -s, c0 - (c - s) * c0 + rng.uniform(-2, 2), s, c, c0 - (s + c) * c0 + rng.uniform(-2, 2))
i, j = np.mgrid[0:N, 0:N]
targets = np.stack([syn.make_slice(q % NS, N, N) for q in range(MT)]).astype(np.float32)
weights = np.tile((0.2 + 0.8 * np.exp(-(((i - 0.5 * N) / (0.6 * N)) ** 2 + ((j - 0.5 * N) / (0.6 * N)) ** 2))).astype(np.float32), (MT, 1, 1))
gb = np.stack([np.linspace(0.8, 1.25, MT), np.linspace(-0.05, 0.1, MT)], axis=1).astype(np.float32)
targets = (gb[:, :1, None] * targets + gb[:, 1:, None]).astype(np.float32)


# ---- (b) the kernel's tile-level cull in numpy, and the pairs that contribute --------------------------------------------------------------------------
def visits_and_contributions():
    r = fuse.target_records(maps, gb, SPACING, SPACING)
    ty, tx = (N + TILE - 1) // TILE, (N + TILE - 1) // TILE
    yl, xl = (np.arange(ty) * TILE).astype(np.float64).reshape(1, ty, 1), (np.arange(tx) * TILE).astype(np.float64).reshape(1, 1, tx)
    yh, xh = yl + (TILE - 1), xl + (TILE - 1)
    v0 = (np.arange(NS, dtype=np.float64) * SPACING).reshape(NS, 1, 1)
    vy, vx = np.arange(N, dtype=np.float64).reshape(1, N, 1), np.arange(N, dtype=np.float64).reshape(1, 1, N)
    MARGIN = 2.0 ** -40
    window_pass = visited = needed = 0
    voxel_pairs = 0
    with np.errstate(all="ignore"):
        for q in range(MT):
            if r.flags[q]:
                continue
            a, b, c = [x[q] for x in r.a], [x[q] for x in r.b], [x[q] for x in r.c]
            p0 = v0 - r.t[0][q]
            pyl, pyh, pxl, pxh = yl - r.t[1][q], yh - r.t[1][q], xl - r.t[2][q], xh - r.t[2][q]
            pym, pxm = np.maximum(np.abs(pyl), np.abs(pyh)), np.maximum(np.abs(pxl), np.abs(pxh))

            def corners(e):
                f0 = e[0] * p0
                fy, fx = (e[1] * pyl, e[1] * pyh), (e[2] * pxl, e[2] * pxh)
                return [(f0 + y) + x for y in fy for x in fx], (np.abs(f0) + np.abs(e[1]) * pym) + np.abs(e[2]) * pxm

            k4, S = corners(c)
            margin = S * MARGIN
            lo = np.maximum(np.minimum.reduce(k4) - margin, -(np.maximum.reduce(k4) + margin))
            keep = ~(np.isfinite(sum(k4) + S) & (lo > 0) & ((lo * lo) * (1.0 - MARGIN) > r.dt[q]))
            pa4, Sa = corners(a)
            pb4, Sb = corners(b)
            i4 = [fuse.in_plane(x, y, r.G11[q], r.G12[q], r.G22[q], r.det[q])[0] for x, y in zip(pa4, pb4)]
            j4 = [fuse.in_plane(x, y, r.G11[q], r.G12[q], r.G22[q], r.det[q])[1] for x, y in zip(pa4, pb4)]
            mi = ((np.abs(r.G22[q]) * Sa + np.abs(r.G12[q]) * Sb) / r.det[q]) * MARGIN
            mj = ((np.abs(r.G11[q]) * Sb + np.abs(r.G12[q]) * Sa) / r.det[q]) * MARGIN
            out_i = (np.maximum.reduce(i4) + mi < 0) | (np.minimum.reduce(i4) - mi > N - 1)
            out_j = (np.maximum.reduce(j4) + mj < 0) | (np.minimum.reduce(j4) - mj > N - 1)
            keep2 = keep & ~(np.isfinite(sum(i4) + sum(j4) + mi + mj) & (out_i | out_j))
            window_pass += int(np.broadcast_to(keep, (NS, ty, tx)).sum())
            visited += int(keep2.sum())
            # the voxels that contribute, by the rule itself
            p1, p2 = vy - r.t[1][q], vx - r.t[2][q]
            pa = ((a[0] * p0) + (a[1] * p1)) + (a[2] * p2)
            pb = ((b[0] * p0) + (b[1] * p1)) + (b[2] * p2)
            cp = ((c[0] * p0) + (c[1] * p1)) + (c[2] * p2)
            ii, jj = fuse.in_plane(pa, pb, r.G11[q], r.G12[q], r.G22[q], r.det[q])
            on = (fuse.window(cp, r.dt[q]) > 0) & (ii >= 0) & (ii <= N - 1) & (jj >= 0) & (jj <= N - 1)
            voxel_pairs += int(on.sum())
            tiles_on = on.reshape(NS, ty, TILE, tx, TILE).any(axis=(2, 4))
            assert not (tiles_on & ~keep2).any(), "the cull dropped a pair that contributes"
            needed += int(tiles_on.sum())
    pairs = NS * ty * tx * MT
    return dict(pairs=pairs, window_pass=window_pass, visited=visited, needed=needed, contributing_voxel_pairs=voxel_pairs)


# ---- (a) the device ------------------------------------------------------------------------------------------------------------------------------------
d_t, d_m, d_w, d_gb = (m.device_array(x.shape).copy_from(x) for x in (targets, maps, weights, gb))
d_v, d_c, d_f = m.device_array(GRID), m.device_array(GRID), m.device_array((MT,))
o = _lib.FuseOpts(C.sizeof(_lib.FuseOpts), 0, SPACING, SPACING, 0.0)


def call(w=True):
    _lib.check(lib.msiren_fuse_targets_dev(h, d_t.ptr, MT, N, N, d_m.ptr, d_w.ptr if w else None, d_gb.ptr, C.byref(o), NS, N, N, d_v.ptr, d_c.ptr, d_f.ptr))


def profiled(w=True):
    _lib.check(lib.msiren_profile_enable(h, 1))
    call(w)
    m.sync()
    e = [e for e in m.profile_kernels() if e["kernel"] == "fuse_kernels"]
    _lib.check(lib.msiren_profile_enable(h, 0))
    assert len(e) == 1 and e[0]["launches"] == 1, e
    return e[0]["ms_total"]


call(), m.sync()  # warm-up: the scratch at its size
ms = {key: [profiled(w) for _ in range(reps)] for key, w in (("weighted", True), ("unweighted", False))}
call(), m.sync()
dev_volume, dev_coverage, dev_flags = d_v.numpy(), d_c.numpy(), d_f.numpy().view(np.int32)
stats = visits_and_contributions()
print(json.dumps({"cull": stats, "visited_share": round(stats["visited"] / stats["pairs"], 5), "window_pass_share": round(stats["window_pass"] / stats["pairs"], 5),
                  "needed_share": round(stats["needed"] / stats["pairs"], 5)}), flush=True)

# ---- (c) operations and bytes ----------------------------------------------------------------------------------------------------------------------------
lanes = 256
ops = lanes * (stats["pairs"] * 36 + stats["window_pass"] * 98 + stats["visited"] * 28) + stats["contributing_voxel_pairs"] * 40
out = {}
for key, v in ms.items():
    med = float(np.median(v))
    nbytes = stats["contributing_voxel_pairs"] * 16 * (2 if key == "weighted" else 1) + 2 * NS * N * N * 4
    out[key] = {"fuse_kernels_ms": round(med, 4), "ms_min_max": [round(min(v), 4), round(max(v), 4)], "fp64_ops_of_the_rule": ops, "tflops_fp64": round(ops / med / 1e9, 3),
                "share_of_fp64_peak": round(ops / med / 1e-3 / PEAK_FP64, 4), "gather_and_store_bytes": nbytes, "gbytes_per_s": round(nbytes / med / 1e6, 2),
                "share_of_hbm_peak": round(nbytes / med / 1e-3 / PEAK_HBM, 5)}
    out[key]["bound_by"] = "fp64 VALU" if out[key]["share_of_fp64_peak"] > out[key]["share_of_hbm_peak"] else "memory"
print(json.dumps({"workload": {"targets": [MT, N, N], "grid": list(GRID), "spacing": SPACING, "thickness": SPACING}, "reps": reps, **out}), flush=True)

# ---- (d) the host rule -----------------------------------------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
want = fuse.fuse_on_host(targets, maps, GRID, SPACING, weights=weights, intensity=gb)
host_s = time.perf_counter() - t0
same = bool(np.array_equal(dev_volume, want.volume, equal_nan=True) and np.array_equal(dev_coverage, want.coverage) and np.array_equal(dev_flags, want.flags))
print(json.dumps({"fuse_on_host_s": round(host_s, 2), "device_equals_host_bit_for_bit": same, "covered_share": round(float(np.isfinite(want.volume).mean()), 5),
                  "host_over_device": round(host_s * 1e3 / float(np.median(ms["weighted"])), 1)}), flush=True)

# ---- (e) robust alignment, then fusion with weights x rweight ------------------------------------------------------------------------------------------------
DT, G, EVALS, TUNE = 16, 4, 12, 0.25
SIZE = DT // G
BLOCK = (slice(None), slice(100, 140), slice(120, 180))
stack = np.stack([syn.make_slice(s, N, N) for s in range(NS)])
planes = np.zeros((DT, 12))
for q in range(DT):
    first = SIZE * (q // SIZE)
    zc = SPACING * (0.5 + (first + 0.5 * (SIZE - 1)) * (NS - 2.0) / (DT - 1))
    planes[q] = np.concatenate([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [SPACING * (0.5 + q * (NS - 2.0) / (DT - 1)), 0.0, 0.0], [zc, c0, c0]])
group_start = np.arange(0, DT + 1, SIZE, dtype=np.int32)
group_of = np.repeat(np.arange(G), SIZE)


def rotation_of(vec):
    t = np.linalg.norm(vec)
    k = vec / t
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


lin = np.linspace(-1.0, 1.0, G)
rot_true = np.stack([rotation_of(np.deg2rad([0.1 * a, 0.1 * (0.5 - a), 0.5 * a + 0.01])) for a in lin])
shift_true = np.stack([0.4 * lin, 0.8 * lin, -0.6 * lin], axis=1)
truth = av.rigid_maps3(rot_true[group_of], shift_true[group_of], planes, SPACING)
goal = m.align_volume_cost(stack, np.zeros((DT, N, N), np.float32), truth, warped=True).warped
gbt = gb[:DT]
goal_w = (gbt[:, :1, None] * goal + gbt[:, 1:, None]).astype(np.float32)
goal_w[BLOCK] += 5.0
open_w = weights[:DT].copy()
open_w[BLOCK] = 1.0  # nothing masks the corruption
kw = dict(weights=open_w, estimate_intensity=True, iterations=EVALS)
quad = m.align_volume_solve_group(stack, goal_w, planes, SPACING, group_start, **kw)
second = m.align_volume_solve_group_robust(stack, goal_w, planes, SPACING, group_start, ar.scale_from(quad, TUNE), rotation=quad.rotation, shift=quad.shift,
                                           intensity=quad.intensity, **kw)
rw = m.align_volume_cost_r(stack, goal_w, second.maps, ar.scale_from(quad, TUNE), weights=open_w, intensity=second.intensity, rweight=True).rweight
clean_targets = (gbt[:, :1, None] * goal + gbt[:, 1:, None]).astype(np.float32)
clean = m.fuse_targets(clean_targets, second.maps, GRID, SPACING, weights=open_w, intensity=second.intensity).volume.astype(np.float64)  # the targets without the + 5
MIN_COVERAGE = 0.05
inside = np.zeros(GRID, bool)
inside[BLOCK] = True


def errors(w, min_coverage):
    res = m.fuse_targets(goal_w, second.maps, GRID, SPACING, weights=w, intensity=second.intensity, min_coverage=min_coverage)
    e = np.abs(res.volume.astype(np.float64) - clean)
    ok = np.isfinite(e)
    return {"min_coverage": min_coverage, "covered_share": round(float(ok.mean()), 4), "mean_error_outside_the_block": float(e[ok & ~inside].mean()),
            "mean_error_inside_the_block": float(e[ok & inside].mean()) if (ok & inside).any() else None, "covered_inside_the_block": int((ok & inside).sum()),
            "voxels_inside_the_block": int(inside.sum())}


robust_w = open_w * np.nan_to_num(rw, nan=0.0)
print(json.dumps({"demonstration": {"largest_map_error_after_the_robust_pass": float(np.abs(second.maps.astype(np.float64) - truth).max()),
                                    "rweight_inside_the_block_max": float(np.nanmax(rw[BLOCK])), "rweight_outside_the_block_median": float(np.nanmedian(rw[:, :100])),
                                    "error_against_the_fusion_of_the_uncorrupted_targets": {
                                        "plain_weights": [errors(open_w, 0.0), errors(open_w, MIN_COVERAGE)],
                                        "weights_times_rweight": [errors(robust_w, 0.0), errors(robust_w, MIN_COVERAGE)]}}}), flush=True)
