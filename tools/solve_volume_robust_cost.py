#!/usr/bin/env python3
"""What msiren_solve_volume_r costs, on tools/fuse_workload.py's workload: 64 targets of 320 x 320 on planes through a
16 x 320 x 320 grid, slices 4 pixels apart, thickness = spacing, weights and a gain and bias per target, lambda = 0.01, scale 0.01, anneal 4.

 (a) the device ms of the profile entry "solve_volume_r_kernels" for msiren_solve_volume_r_dev with (rounds, iterations) = (1, 10), (5, 2) and (5, 0),
     without a final pass; with t(r, i) = base + r boundary + r i step: step = (t(5, 2) - t(5, 0)) / 10 and boundary = (t(5, 2) - t(1, 10)) / 4; and
     (5, 2) once more with rweight, residual and stats: the final pass; median and spread over the repetitions;
 (b) in the same run, "solve_volume_kernels" with 10 iterations, and "project_kernels" plus "fuse_kernels" on the same inputs;
 (c) what a caller pays per round boundary without the call: project_volume with the residual, the weight in numpy, then solve_volume(start=...) with 2
     iterations, five rounds: wall ms and the device ms of their profile entries per round;
 (d) on tools/solve_volume_cost.py (f)'s workload, after the robust alignment: the error of the robust solve against the solve of the uncorrupted
     targets, inside and outside the block, for several scales, beside the quadratic solve with plain weights and with weights x rweight.

No threshold is set: the figures go to LAB_NOTES.md section 35.  One JSON line per measurement.  Usage: python tools/solve_volume_robust_cost.py [reps]"""
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
from mri_inr_amd import _lib  # noqa: E402
from mri_inr_amd import solve_volume_robust as svr  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
LAM, SCALE, ANNEAL = 0.01, 0.01, 4.0

m = fw.model()  # (only the alignment of (d) needs the weights)
lib, h = m._lib, m._h
maps, targets, weights, gb = fw.workload()

# ---- (a), (b) the device -----------------------------------------------------------------------------------------------------------------------------------
shape = (MT, N, N)
d_t, d_m, d_w, d_gb = (m.device_array(x.shape).copy_from(x) for x in (targets, maps, weights, gb))
d_sc = m.device_array((2 * MT,)).copy_from(np.full(MT, SCALE, np.float64).view(np.float32))
d_v, d_c, d_f = m.device_array(GRID), m.device_array(GRID), m.device_array((MT,))
d_h, d_st = m.device_array((11, 4)), m.device_array((8,))
d_s, d_rw, d_res, d_ss = m.device_array(shape), m.device_array(shape), m.device_array(shape), m.device_array((MT, 8))
fo = _lib.FuseOpts(C.sizeof(_lib.FuseOpts), 0, SPACING, SPACING, 0.0)


def robust_call(rounds, iterations, final=False):
    o = _lib.SolveROpts(C.sizeof(_lib.SolveROpts), iterations, rounds, 0, SPACING, SPACING, 0.0, LAM, ANNEAL)
    _lib.check(lib.msiren_solve_volume_r_dev(h, d_t.ptr, MT, N, N, d_m.ptr, d_w.ptr, d_gb.ptr, d_sc.ptr, C.byref(o), NS, N, N, None, d_v.ptr, None, None, d_f.ptr, d_st.ptr,
                                             d_rw.ptr if final else None, d_res.ptr if final else None, d_ss.ptr if final else None))


def solve_call(iterations):
    o = _lib.SolveOpts(C.sizeof(_lib.SolveOpts), iterations, SPACING, SPACING, 0.0, LAM)
    _lib.check(lib.msiren_solve_volume_dev(h, d_t.ptr, MT, N, N, d_m.ptr, d_w.ptr, d_gb.ptr, C.byref(o), NS, N, N, None, d_v.ptr, None, d_h.ptr, d_f.ptr, d_st.ptr))


def fuse_call():
    _lib.check(lib.msiren_fuse_targets_dev(h, d_t.ptr, MT, N, N, d_m.ptr, d_w.ptr, d_gb.ptr, C.byref(fo), NS, N, N, d_v.ptr, d_c.ptr, d_f.ptr))


def project_call():
    _lib.check(lib.msiren_project_volume_dev(h, d_fv.ptr, NS, N, N, d_m.ptr, d_gb.ptr, C.byref(fo), MT, N, N, None, None, d_s.ptr, None, None, None, None))


fuse_call(), m.sync()
d_fv = m.device_array(GRID).copy_from(d_v.numpy())  # the fusion: what the projection reads
robust_call(5, 2, True), solve_call(10), project_call(), m.sync()  # warm-up: the scratch at its size
ms = {f"robust_{r}x{i}": [fw.profiled(m, lambda: robust_call(r, i), "solve_volume_r_kernels") for _ in range(reps)] for r, i in ((1, 10), (5, 2), (5, 0))}
ms["robust_5x2_final_pass"] = [fw.profiled(m, lambda: robust_call(5, 2, True), "solve_volume_r_kernels") for _ in range(reps)]
ms["solve_10"] = [fw.profiled(m, lambda: solve_call(10), "solve_volume_kernels") for _ in range(reps)]
ms["project_kernels"] = [fw.profiled(m, project_call, "project_kernels") for _ in range(reps)]
ms["fuse_kernels"] = [fw.profiled(m, fuse_call, "fuse_kernels") for _ in range(reps)]
med = {k: float(np.median(v)) for k, v in ms.items()}
step = (med["robust_5x2"] - med["robust_5x0"]) / 10
boundary = (med["robust_5x2"] - med["robust_1x10"]) / 4
print(json.dumps({"workload": {"targets": [MT, N, N], "grid": list(GRID), "spacing": SPACING, "thickness": SPACING, "lambda": LAM, "scale": SCALE, "anneal": ANNEAL},
                  "reps": reps, "ms": {k: {"median": round(med[k], 4), "min_max": [round(min(v), 4), round(max(v), 4)]} for k, v in ms.items()},
                  "ms_per_iteration": round(step, 4), "ms_per_round_boundary": round(boundary, 4), "boundary_over_iteration": round(boundary / step, 3),
                  "final_pass_ms": round(med["robust_5x2_final_pass"] - med["robust_5x2"], 4),
                  "one_round_of_10_over_solve_10": round(med["robust_1x10"] / med["solve_10"], 4),
                  "project_plus_fuse_ms": round(med["project_kernels"] + med["fuse_kernels"], 4)}), flush=True)

# ---- (c) five rounds driven from Python ----------------------------------------------------------------------------------------------------------------------
ROUNDS, ITER = 5, 2
factors = svr.schedule(ROUNDS, ANNEAL)
walls, devs = [], []
for _ in range(reps):
    _lib.check(lib.msiren_profile_enable(h, 1))
    t0 = time.perf_counter()
    V = m.fuse_targets(targets, maps, GRID, SPACING, weights=weights, intensity=gb).volume
    for t in range(ROUNDS):
        P = m.project_volume(V, maps, (N, N), SPACING, intensity=gb, targets=targets, weights=weights, residual=True)
        e = np.nan_to_num(P.residual.astype(np.float64), nan=0.0)
        omega = 1.0 / (1.0 + e * e / (SCALE * factors[t])) ** 2
        V = m.solve_volume(targets, maps, GRID, SPACING, iterations=ITER, lam=LAM, weights=(weights * omega).astype(np.float32), intensity=gb, start=V).volume
    walls.append(1e3 * (time.perf_counter() - t0))
    devs.append(sum(e["ms_total"] for e in m.profile_kernels() if e["kernel"] in ("project_kernels", "solve_volume_kernels")))
    _lib.check(lib.msiren_profile_enable(h, 0))
print(json.dumps({"five_rounds_of_2_from_python": {"wall_ms": {"median": round(float(np.median(walls)), 2), "min_max": [round(min(walls), 2), round(max(walls), 2)]},
                                                   "device_ms_of_project_and_solve_entries": {"median": round(float(np.median(devs)), 3),
                                                                                              "min_max": [round(min(devs), 3), round(max(devs), 3)]},
                                                   "wall_ms_per_round": round(float(np.median(walls)) / ROUNDS, 2),
                                                   "device_ms_per_round": round(float(np.median(devs)) / ROUNDS, 3),
                                                   "device_ms_per_round_boundary": round(float(np.median(devs)) / ROUNDS - ITER * step, 3),
                                                   "robust_5x2_device_ms": round(med["robust_5x2"], 3)}}), flush=True)

# ---- (d) robust alignment, then the robust solve ---------------------------------------------------------------------------------------------------------------
al = fw.robust_alignment(m, weights, gb)
TOTAL = 10
clean = m.solve_volume(al.clean_targets, al.second.maps, GRID, SPACING, weights=al.open_w, iterations=TOTAL, lam=LAM, intensity=al.second.intensity).volume.astype(np.float64)
out = {}
for name, w in (("quadratic_plain_weights", al.open_w), ("quadratic_weights_times_rweight", al.robust_w)):
    res = m.solve_volume(al.goal_w, al.second.maps, GRID, SPACING, weights=w, iterations=TOTAL, lam=LAM, intensity=al.second.intensity)
    out[name] = fw.errors(res.volume, clean, al.inside)
for scale in (1.0, 0.1, 0.01):
    for rounds, iterations in ((5, 2), (5, 3)):
        res = m.solve_volume_robust(al.goal_w, al.second.maps, GRID, SPACING, scale, rounds=rounds, iterations=iterations, anneal=ANNEAL, lam=LAM, weights=al.open_w,
                                    intensity=al.second.intensity, rweight=True, stats=True)
        part = np.isfinite(res.rweight)
        out[f"robust_scale_{scale:g}_{rounds}x{iterations}"] = {**fw.errors(res.volume, clean, al.inside), "stopped_at": res.stopped_at.tolist(),
                                                                "mean_rweight_inside_the_block": float(res.rweight[al.block][part[al.block]].mean()),
                                                                "mean_rweight": float(res.rweight[part].mean())}
print(json.dumps({"demonstration": {"lambda": LAM, "anneal": ANNEAL, "error_against_the_solve_of_the_uncorrupted_targets": out}}), flush=True)
