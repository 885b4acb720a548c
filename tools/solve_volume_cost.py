#!/usr/bin/env python3
"""What msiren_solve_volume costs, on tools/fuse_cost.py's workload: 64 targets of 320 x 320 on planes through a
16 x 320 x 320 grid, slices 4 pixels apart, small tilts and in-plane motion, thickness = spacing, weights and a gain and bias per target.

 (a) the device ms of the profile entry "solve_volume_kernels" for msiren_solve_volume_dev with 0, 1 and 10 iterations (lambda = 0.01), and so the
     cost of one iteration; median and spread over the repetitions;
 (b) in the same run, "project_kernels" (the gather alone) plus "fuse_kernels" on the same inputs: the two parent gathers an iteration is made of;
 (c) the same ten steps driven from Python with project_volume and fuse_targets (V <- V + fuse(T - project(V)), host-pointer calls): wall seconds
     and the device ms of their profile entries;
 (d) the seconds mri_inr_amd/solve_volume.py: solve_volume_on_host takes for 1 iteration on the same inputs, and that the device returned its bits;
 (e) the error curves on tests/fuse_cases.py's truth case on the device: consistent data and point samples, both thicknesses;
 (f) robust alignment followed by the solve, as tools/fuse_cost.py does for the fusion: the error against the solve of the uncorrupted targets with
     plain weights and with weights x rweight.

No threshold is set: the figures go to LAB_NOTES.md section 33.  One JSON line per measurement.  Usage: python tools/solve_volume_cost.py [reps]"""
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
from mri_inr_amd import _lib, solve_volume as sv  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
LAM = 0.01

m = fw.model()  # (only the alignment of (f) needs the weights)
lib, h = m._lib, m._h
maps, targets, weights, gb = fw.workload()

# ---- (a), (b) the device -----------------------------------------------------------------------------------------------------------------------------------
shape = (MT, N, N)
d_t, d_m, d_w, d_gb = (m.device_array(x.shape).copy_from(x) for x in (targets, maps, weights, gb))
d_v, d_c, d_f, d_st = m.device_array(GRID), m.device_array(GRID), m.device_array((MT,)), m.device_array((1,))
d_h = m.device_array((11, 4))
d_s = m.device_array(shape)
fo = _lib.FuseOpts(C.sizeof(_lib.FuseOpts), 0, SPACING, SPACING, 0.0)


def solve_call(iterations):
    o = _lib.SolveOpts(C.sizeof(_lib.SolveOpts), iterations, SPACING, SPACING, 0.0, LAM)
    _lib.check(lib.msiren_solve_volume_dev(h, d_t.ptr, MT, N, N, d_m.ptr, d_w.ptr, d_gb.ptr, C.byref(o), NS, N, N, None, d_v.ptr, d_c.ptr, d_h.ptr, d_f.ptr, d_st.ptr))


def fuse_call():
    _lib.check(lib.msiren_fuse_targets_dev(h, d_t.ptr, MT, N, N, d_m.ptr, d_w.ptr, d_gb.ptr, C.byref(fo), NS, N, N, d_v.ptr, d_c.ptr, d_f.ptr))


def project_call():
    _lib.check(lib.msiren_project_volume_dev(h, d_fv.ptr, NS, N, N, d_m.ptr, d_gb.ptr, C.byref(fo), MT, N, N, None, None, d_s.ptr, None, None, None, None))


fuse_call(), m.sync()
d_fv = m.device_array(GRID).copy_from(d_v.numpy())  # the fusion: what the projection reads
solve_call(10), project_call(), m.sync()            # warm-up: the scratch at its size
ms = {f"solve_{k}": [fw.profiled(m, lambda: solve_call(k), "solve_volume_kernels") for _ in range(reps)] for k in (0, 1, 10)}
ms["project_kernels"] = [fw.profiled(m, project_call, "project_kernels") for _ in range(reps)]
ms["fuse_kernels"] = [fw.profiled(m, fuse_call, "fuse_kernels") for _ in range(reps)]
med = {k: float(np.median(v)) for k, v in ms.items()}
per_iteration = (med["solve_10"] - med["solve_0"]) / 10
parents = med["project_kernels"] + med["fuse_kernels"]
print(json.dumps({"workload": {"targets": [MT, N, N], "grid": list(GRID), "spacing": SPACING, "thickness": SPACING, "lambda": LAM}, "reps": reps,
                  "ms": {k: {"median": round(med[k], 4), "min_max": [round(min(v), 4), round(max(v), 4)]} for k, v in ms.items()},
                  "ms_per_iteration": round(per_iteration, 4), "first_iteration_ms": round(med["solve_1"] - med["solve_0"], 4),
                  "project_plus_fuse_ms": round(parents, 4), "iteration_over_the_two_parent_gathers": round(per_iteration / parents, 3)}), flush=True)
solve_call(1), m.sync()
dev = sv.SolveVolumeResult(d_v.numpy(), d_c.numpy(), d_h.numpy().view(np.float64)[:2], d_f.numpy().view(np.int32), int(d_st.numpy().view(np.int32)[0]))

# ---- (c) ten back-projection steps driven from Python --------------------------------------------------------------------------------------------------------
_lib.check(lib.msiren_profile_enable(h, 1))
t0 = time.perf_counter()
V = m.fuse_targets(targets, maps, GRID, SPACING, weights=weights, intensity=gb).volume
for _ in range(10):
    P = m.project_volume(V, maps, (N, N), SPACING, intensity=gb, targets=targets, weights=weights, residual=True)
    res = np.where(np.isfinite(P.residual), P.residual, np.float32(0)) / gb[:, :1, None]    # the residual in the stack's intensity
    Dv = m.fuse_targets(res.astype(np.float32), maps, GRID, SPACING, weights=weights).volume
    V = (V.astype(np.float64) + np.nan_to_num(Dv.astype(np.float64), nan=0.0)).astype(np.float32)
wall = time.perf_counter() - t0
dev_ms = sum(e["ms_total"] for e in m.profile_kernels() if e["kernel"] in ("project_kernels", "fuse_kernels"))
_lib.check(lib.msiren_profile_enable(h, 0))
print(json.dumps({"ten_steps_from_python": {"wall_s": round(wall, 3), "device_ms_of_their_profile_entries": round(dev_ms, 3),
                                            "solve_10_device_ms": round(med["solve_10"], 3)}}), flush=True)

# ---- (d) the host rule -----------------------------------------------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
want = sv.solve_volume_on_host(targets, maps, GRID, SPACING, iterations=1, lam=LAM, weights=weights, intensity=gb)
host_s = time.perf_counter() - t0
same = bool(np.array_equal(dev.volume, want.volume, equal_nan=True) and np.array_equal(dev.coverage, want.coverage) and np.array_equal(dev.flags, want.flags)
            and np.array_equal(dev.history, want.history, equal_nan=True) and dev.stopped_at == want.stopped_at)
print(json.dumps({"solve_volume_on_host_s_for_1_iteration": round(host_s, 2), "device_equals_host_bit_for_bit": same, "history": want.history.tolist(),
                  "support_share": round(float(np.isfinite(want.volume).mean()), 5)}), flush=True)

# ---- (e) the error curves on the truth case, on the device -----------------------------------------------------------------------------------------------------
import fuse_cases as fc  # noqa: E402
import solve_volume_cases as sc  # noqa: E402

t = fc.truth_case()
curves = {}
for thickness in sc.THICKNESSES:
    for kind, tg in (("consistent", sc.consistent_targets(thickness)), ("point_samples", t["targets"])):
        e = []
        for k in (0, 1, 2, 3, 4, 5, 30):
            r = m.solve_volume(tg, t["maps"], fc.TRUTH_GRID, SPACING, iterations=k, thickness=thickness)
            e.append(float(np.abs(r.volume.astype(np.float64) - t["volume"])[np.isfinite(r.volume)].mean()))
        curves[f"{kind}-t{thickness:g}"] = e
print(json.dumps({"mean_error_after_0_1_2_3_4_5_30_iterations": curves}), flush=True)

# ---- (f) robust alignment, then the solve with weights x rweight -----------------------------------------------------------------------------------------------
ITER = 10
al = fw.robust_alignment(m, weights, gb)
skw = dict(iterations=ITER, lam=LAM, intensity=al.second.intensity)
clean = m.solve_volume(al.clean_targets, al.second.maps, GRID, SPACING, weights=al.open_w, **skw).volume.astype(np.float64)  # the targets without the + 5


def errors(w):
    res = m.solve_volume(al.goal_w, al.second.maps, GRID, SPACING, weights=w, **skw)
    return {**fw.errors(res.volume, clean, al.inside), "stopped_at": res.stopped_at}


print(json.dumps({"demonstration": {"iterations": ITER, "lambda": LAM, "largest_map_error_after_the_robust_pass": float(np.abs(al.second.maps.astype(np.float64) - al.truth).max()),
                                    "error_against_the_solve_of_the_uncorrupted_targets": {"plain_weights": errors(al.open_w), "weights_times_rweight": errors(al.robust_w)}}}), flush=True)
