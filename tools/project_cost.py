#!/usr/bin/env python3
"""What msiren_project_volume costs, on tools/fuse_cost.py's workload: a 16 x 320 x 320 stack, slices 4 pixels apart, gathered
onto 64 targets of 320 x 320 on planes through it with small tilts and in-plane motion, thickness = spacing, a gain and bias per target.

 (a) the device ms of the profile entry "project_kernels" for msiren_project_volume_dev: the set-up and the gather alone (no targets), and with the
     residual and the sums (targets and weights given) -- the difference is project_stats_kernel; median and spread over the repetitions;
 (b) the voxels the box TESTS per (voxel, pixel) pair that contributes, from project_plan.h's box restated in numpy and the rule's own pairs;
 (c) the fp64 operations the gather executes (+ - * / and compares counted as one each: 5 per tested voxel up to the window test, 14 per voxel that
     passes it, 10 per contributing pair) over the time against the card's 78.6 TFLOP/s vector fp64 peak, and the bytes it gathers (4 per voxel that
     passes the window) plus the stores against 8 TB/s;
 (d) the seconds mri_inr_amd/fuse.py: project_on_host and project_stats_on_host take on the same inputs, and that the device returned their bits;
 (e) "fuse_kernels" on the same maps and lattices as a yardstick;
 (f) the one-step demonstration on tests/fuse_cases.py's truth case at thickness = spacing, on the device: V1 = V0 + fuse(T - project(V0)), the mean
     error against the analytic volume over the covered voxels before and after.

No threshold is set: the figures go to LAB_NOTES.md section 32.  One JSON line per measurement.  Usage: python tools/project_cost.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuse_workload as fw  # noqa: E402
from fuse_workload import GRID, MT, N, NS, SPACING  # noqa: E402
from mri_inr_amd import _lib, fuse, synthetic as syn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
PEAK_FP64, PEAK_HBM = 78.6e12, 8.0e12

m = fw.model(committed=False)
lib, h = m._lib, m._h
maps, targets, weights, gb = fw.workload()
stack = np.stack([syn.make_slice(s, N, N) for s in range(NS)]).astype(np.float32)


# ---- (b) project_plan.h's box in numpy, and the pairs that contribute ------------------------------------------------------------------------------------
def tested_and_contributing():
    r = fuse.target_records(maps, gb, SPACING, SPACING)
    valid = np.isfinite(stack)
    tested = window_pass = pairs = 0
    v0 = (np.arange(NS, dtype=np.float64) * SPACING).reshape(NS, 1, 1)
    vy, vx = np.arange(N, dtype=np.float64).reshape(1, N, 1), np.arange(N, dtype=np.float64).reshape(1, 1, N)
    for q in range(MT):
        if r.flags[q]:
            continue
        s = SPACING / np.sqrt(r.det[q])
        counts = []
        for e, size in enumerate(GRID):
            R = (abs(r.a[e][q]) + abs(r.b[e][q])) + abs(r.c[e][q]) * s
            R = (R / SPACING if e == 0 else R) * (1.0 + 2.0 ** -20) + (2.0 ** -10 / SPACING if e == 0 else 2.0 ** -10)
            counts.append(min(int(np.floor(2.0 * R) + 2.0), size))
        tested += N * N * counts[0] * counts[1] * counts[2]
        taps = fuse.voxel_taps(r, q, valid, GRID, (N, N), np.float64(SPACING))
        pairs += 0 if taps is None else 4 * len(taps[1])
        cp = ((r.c[0][q] * (v0 - r.t[0][q])) + (r.c[1][q] * (vy - r.t[1][q]))) + (r.c[2][q] * (vx - r.t[2][q]))
        window_pass += int((cp * cp < r.dt[q]).sum()) * counts[1] * counts[2]  # every voxel inside the window is tested by about ny nx pixels
    return dict(tested=tested, window_pass=window_pass, contributing_pairs=pairs)


# ---- (a) the device ------------------------------------------------------------------------------------------------------------------------------------
shape = (MT, N, N)
d_v, d_m, d_gb, d_t, d_w = (m.device_array(x.shape).copy_from(x) for x in (stack, maps, gb, targets, weights))
d_s, d_c, d_r, d_st, d_f = m.device_array(shape), m.device_array(shape), m.device_array(shape), m.device_array((MT, 8)), m.device_array((MT,))
o = _lib.FuseOpts(C.sizeof(_lib.FuseOpts), 0, SPACING, SPACING, 0.0)


def call(with_targets):
    _lib.check(lib.msiren_project_volume_dev(h, d_v.ptr, NS, N, N, d_m.ptr, d_gb.ptr, C.byref(o), MT, N, N, d_t.ptr if with_targets else None, d_w.ptr if with_targets else None,
                                             d_s.ptr, d_c.ptr, d_r.ptr if with_targets else None, d_st.ptr if with_targets else None, d_f.ptr))


def fuse_call():
    _lib.check(lib.msiren_fuse_targets_dev(h, d_t.ptr, MT, N, N, d_m.ptr, d_w.ptr, d_gb.ptr, C.byref(o), NS, N, N, d_fv.ptr, d_fc.ptr, d_f.ptr))


d_fv, d_fc = m.device_array(GRID), m.device_array(GRID)
call(True), fuse_call(), m.sync()  # warm-up: the scratch at its size
ms = {"gather": [fw.profiled(m, lambda: call(False), "project_kernels") for _ in range(reps)], "gather_and_stats": [fw.profiled(m, lambda: call(True), "project_kernels") for _ in range(reps)],
      "fuse_kernels": [fw.profiled(m, fuse_call, "fuse_kernels") for _ in range(reps)]}
call(True), m.sync()
dev = fuse.ProjectResult(d_s.numpy(), d_c.numpy(), d_r.numpy(), d_st.numpy().view(np.float64), d_f.numpy().view(np.int32))
counts = tested_and_contributing()
print(json.dumps({"box": counts, "tested_per_contributing_pair": round(counts["tested"] / counts["contributing_pairs"], 3)}), flush=True)

# ---- (c) operations and bytes ----------------------------------------------------------------------------------------------------------------------------
med = {k: float(np.median(v)) for k, v in ms.items()}
ops = counts["tested"] * 5 + counts["window_pass"] * 14 + counts["contributing_pairs"] * 10
nbytes = counts["window_pass"] * 4 + 2 * MT * N * N * 4
print(json.dumps({"workload": {"targets": [MT, N, N], "grid": list(GRID), "spacing": SPACING, "thickness": SPACING}, "reps": reps,
                  "project_kernels_ms": {k: {"median": round(med[k], 4), "min_max": [round(min(v), 4), round(max(v), 4)]} for k, v in ms.items()},
                  "stats_kernel_ms": round(med["gather_and_stats"] - med["gather"], 4), "fp64_ops_of_the_gather": ops, "tflops_fp64": round(ops / med["gather"] / 1e9, 3),
                  "share_of_fp64_peak": round(ops / med["gather"] / 1e-3 / PEAK_FP64, 4), "gather_and_store_bytes": nbytes,
                  "gbytes_per_s": round(nbytes / med["gather"] / 1e6, 2), "share_of_hbm_peak": round(nbytes / med["gather"] / 1e-3 / PEAK_HBM, 5),
                  "gather_over_fuse_kernels": round(med["gather"] / med["fuse_kernels"], 2)}), flush=True)

# ---- (d) the host rule -----------------------------------------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
want = fuse.project_on_host(stack, maps, (N, N), SPACING, intensity=gb)
t1 = time.perf_counter()
res, st = fuse.project_stats_on_host(targets, want.simulated, weights)
t2 = time.perf_counter()
same = bool(np.array_equal(dev.simulated, want.simulated, equal_nan=True) and np.array_equal(dev.coverage, want.coverage) and np.array_equal(dev.flags, want.flags)
            and np.array_equal(dev.residual, res, equal_nan=True) and np.array_equal(dev.stats, st))
print(json.dumps({"project_on_host_s": round(t1 - t0, 2), "project_stats_on_host_s": round(t2 - t1, 2), "device_equals_host_bit_for_bit": same,
                  "covered_share": round(float(np.isfinite(want.simulated).mean()), 5), "host_over_device": round((t2 - t0) * 1e3 / med["gather_and_stats"], 1)}), flush=True)

# ---- (f) one back-projection step on the truth case, on the device ------------------------------------------------------------------------------------------
import fuse_cases as fc  # noqa: E402

t = fc.truth_case()
V0 = m.fuse_targets(t["targets"], t["maps"], fc.TRUTH_GRID, fc.SPACING)
P = m.project_volume(V0.volume, t["maps"], fc.TRUTH_SHAPE, fc.SPACING, targets=t["targets"], residual=True, stats=True)
D = m.fuse_targets(P.residual, t["maps"], fc.TRUTH_GRID, fc.SPACING)
V1 = V0.volume.astype(np.float64) + np.nan_to_num(D.volume.astype(np.float64), nan=0.0)
covered = np.isfinite(V0.volume)
P1 = m.project_volume(V1.astype(np.float32), t["maps"], fc.TRUTH_SHAPE, fc.SPACING, targets=t["targets"], stats=True)
rms = lambda s: float(np.sqrt(s[:, 3].sum() / s[:, 1].sum()))  # noqa: E731
print(json.dumps({"one_step": {"mean_error_before": float(np.abs(V0.volume - t["volume"])[covered].mean()), "mean_error_after": float(np.abs(V1 - t["volume"])[covered].mean()),
                               "rms_residual_before": rms(P.stats), "rms_residual_after": rms(P1.stats)}}), flush=True)
