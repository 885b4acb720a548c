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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_workload as fw  # noqa: E402
from fuse_workload import GRID, MT, N, NS, SPACING  # noqa: E402
from mri_inr_amd import _lib, fuse  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
TILE = 16
PEAK_FP64, PEAK_HBM = 78.6e12, 8.0e12

m = fw.model()
lib, h = m._lib, m._h
maps, targets, weights, gb = fw.workload()


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


call(), m.sync()  # warm-up: the scratch at its size
ms = {key: [fw.profiled(m, lambda: call(w), "fuse_kernels") for _ in range(reps)] for key, w in (("weighted", True), ("unweighted", False))}
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
al = fw.robust_alignment(m, weights, gb)
clean = m.fuse_targets(al.clean_targets, al.second.maps, GRID, SPACING, weights=al.open_w, intensity=al.second.intensity).volume.astype(np.float64)  # the targets without the + 5
MIN_COVERAGE = 0.05


def errors(w, min_coverage):
    res = m.fuse_targets(al.goal_w, al.second.maps, GRID, SPACING, weights=w, intensity=al.second.intensity, min_coverage=min_coverage)
    return {"min_coverage": min_coverage, **fw.errors(res.volume, clean, al.inside)}


print(json.dumps({"demonstration": {"largest_map_error_after_the_robust_pass": float(np.abs(al.second.maps.astype(np.float64) - al.truth).max()),
                                    "rweight_inside_the_block_max": float(np.nanmax(al.rw[al.block])), "rweight_outside_the_block_median": float(np.nanmedian(al.rw[:, :100])),
                                    "error_against_the_fusion_of_the_uncorrupted_targets": {
                                        "plain_weights": [errors(al.open_w, 0.0), errors(al.open_w, MIN_COVERAGE)],
                                        "weights_times_rweight": [errors(al.robust_w, 0.0), errors(al.robust_w, MIN_COVERAGE)]}}}), flush=True)
