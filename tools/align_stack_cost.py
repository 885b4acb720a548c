#!/usr/bin/env python3
"""What registering to a plain voxel stack costs on section 5.15's workload (tools/align_group_cost.py): one stream, a stack of
16 slices of 320 x 320 and 16 targets of 320 x 320 as 4 groups of 4 under one rigid motion per group, slices 4 pixels apart; from the nominal planes,
12 evaluations, the intensity estimated, scale 0.01, smooth weights in (0, 1] with a masked block.

 (a) msiren_align_stack_solve_group_r_dev (the stack read trilinearly; its targets are g_t W + b_t of its own warped planes W at the truth) against
     msiren_align_volume_solve_group_r_dev (the same slices as images of the default sine model, fp32 handle; targets from its own warped planes) on
     the same lattices in the same run.  Device ms (msiren_timer_start / _stop: HIP events around the call), the routes alternating, medians and the
     run-to-run spread;
 (b) the profile of one solve of each kind per profiled entry: "align_stack_reduce_kernels" against "align_volume_reduce_r_kernels" (and what the
     volume route spends in front of its reduce: the prologue once, bins and trunk per evaluation);
 (c) how far the stack solve ends from the truth it was given.
With ``--reduces`` only the weighted and the robust volume reduce are profiled (ms per evaluation of "align_volume_reduce_w_kernels" and
"align_volume_reduce_r_kernels"): run once per library (MSIREN_LIB) to compare two builds of them.

No threshold is set: the figures go to LAB_NOTES.md section 37.  One JSON line per measurement.  Usage: python tools/align_stack_cost.py [reps] [--reduces]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, align_volume as av, synthetic as syn  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reduces_only = "--reduces" in sys.argv
reps = int(args[0]) if args else 7
N, NS, MT, G, EVALS, SPACING, SCALE = 320, 16, 16, 4, 12, 4.0, 0.01
SIZE = MT // G
BLOCK = (slice(None), slice(100, 140), slice(120, 180))

m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0,
                   use_bias=True, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                   outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda:0", activation="sine", precision="fp32")
m.load_state_dict(syn.make_state_dict(seed=7, trained_like=True))
m.to("cuda:0").eval()
lib, h = m._lib, m._h

stack = np.stack([syn.make_slice(s, N, N) for s in range(NS)])
planes = np.zeros((MT, 12))
for q in range(MT):
    o = np.array([SPACING * (0.5 + q * (NS - 2.0) / (MT - 1)), 0.0, 0.0])  # nominal planes at Z = 0.5 .. 14.5 slices
    first = SIZE * (q // SIZE)
    zc = SPACING * (0.5 + (first + 0.5 * (SIZE - 1)) * (NS - 2.0) / (MT - 1))  # the group's centre: the middle of its planes
    planes[q] = np.concatenate([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], o, [zc, (N - 1) / 2, (N - 1) / 2]])
group_start = np.arange(0, MT + 1, SIZE, dtype=np.int32)
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
gb_truth = np.stack([np.linspace(0.8, 1.25, MT), np.linspace(-0.05, 0.1, MT)], axis=1).astype(np.float32)
i, j = np.mgrid[0:N, 0:N]
weights = np.tile((0.2 + 0.8 * np.exp(-(((i - 0.5 * N) / (0.6 * N)) ** 2 + ((j - 0.5 * N) / (0.6 * N)) ** 2))).astype(np.float32), (MT, 1, 1))
weights[BLOCK] = 0.0


def targets_of(warped):
    t = gb_truth[:, :1, None] * np.nan_to_num(warped, nan=0.0) + gb_truth[:, 1:, None]
    t[BLOCK] += 5.0
    return t.astype(np.float32)


blank = np.zeros((MT, N, N), np.float32)
goal_volume = targets_of(m.align_volume_cost(stack, blank, truth, warped=True).warped)
goal_stack = blank if reduces_only else targets_of(m.align_stack_cost(stack, blank, truth, warped=True).warped)
rigid_g = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (G, 1))
scale = np.full(MT, SCALE, np.float64)
cg = _lib.AlignVolumeSolveGroupOpts(C.sizeof(_lib.AlignVolumeSolveGroupOpts), EVALS, av.ESTIMATE, 0, 1e-3, 0.1, 10.0, 1e-9, 1e9, SPACING)

d_i, d_tv, d_ts, d_w = (m.device_array(x.shape).copy_from(x) for x in (stack, goal_volume, goal_stack, weights))
d_p = m.device_array((MT, 24)).copy_from(planes.view(np.float32))
d_rg = m.device_array((G, 24)).copy_from(rigid_g.view(np.float32))
d_s = m.device_array((MT, 2)).copy_from(scale.view(np.float32).reshape(MT, 2))
d_out, d_gout, d_gr, d_grep, d_trep = m.device_array((MT, 9)), m.device_array((MT, 2)), m.device_array((G, 24)), m.device_array((G, 14)), m.device_array((MT, 6))
ms = C.c_float()


def timed(fn):
    _lib.check(lib.msiren_timer_start(h))
    fn()
    _lib.check(lib.msiren_timer_stop(h, C.byref(ms)))
    return ms.value


def solve_volume_w():
    return timed(lambda: _lib.check(lib.msiren_align_volume_solve_group_dev(h, d_i.ptr, NS, N, N, d_tv.ptr, MT, N, N, C.byref(cg), group_start.ctypes.data, G, d_p.ptr,
                                                                            d_rg.ptr, d_w.ptr, None, d_out.ptr, d_gout.ptr, d_gr.ptr, d_grep.ptr, d_trep.ptr, None)))


def solve_volume_r():
    return timed(lambda: _lib.check(lib.msiren_align_volume_solve_group_r_dev(h, d_i.ptr, NS, N, N, d_tv.ptr, MT, N, N, C.byref(cg), group_start.ctypes.data, G, d_p.ptr,
                                                                              d_rg.ptr, d_w.ptr, None, d_s.ptr, d_out.ptr, d_gout.ptr, d_gr.ptr, d_grep.ptr, d_trep.ptr,
                                                                              None)))


def solve_stack():
    return timed(lambda: _lib.check(lib.msiren_align_stack_solve_group_r_dev(h, d_i.ptr, NS, N, N, d_ts.ptr, MT, N, N, C.byref(cg), group_start.ctypes.data, G, d_p.ptr,
                                                                             d_rg.ptr, d_w.ptr, None, d_s.ptr, d_out.ptr, d_gout.ptr, d_gr.ptr, d_grep.ptr, d_trep.ptr,
                                                                             None)))


def wall(fn):
    m.sync()
    t0 = time.perf_counter()
    dev = fn()
    m.sync()
    return dev, 1e3 * (time.perf_counter() - t0)


def profiled(fn):
    _lib.check(lib.msiren_profile_enable(h, 1))
    dev, wall_ms = wall(fn)
    p = {e["kernel"]: (e["launches"], round(e["ms_total"], 4)) for e in m.profile_kernels()}
    _lib.check(lib.msiren_profile_enable(h, 0))
    return {"launches_and_ms_total": p, "profiled_ms": round(sum(v[1] for v in p.values()), 4), "device_ms": round(dev, 3), "wall_ms": round(wall_ms, 3),
            "ms_per_evaluation": {k: round(v[1] / v[0], 5) for k, v in p.items() if v[0] == EVALS}}


if reduces_only:
    solve_volume_w(), solve_volume_r()  # warm-up
    w, r = [], []
    for _ in range(reps):  # the two reduces alternate
        w.append(profiled(solve_volume_w)["ms_per_evaluation"]["align_volume_reduce_w_kernels"])
        r.append(profiled(solve_volume_r)["ms_per_evaluation"]["align_volume_reduce_r_kernels"])
    print(json.dumps({"library": _lib.LIB_PATH, "reps": reps, "reduce_w_ms_per_evaluation": {"median": float(np.median(w)), "min_max": [min(w), max(w)]},
                      "reduce_r_ms_per_evaluation": {"median": float(np.median(r)), "min_max": [min(r), max(r)]}}), flush=True)
    sys.exit(0)

ROUTES = {"align_stack_solve_group_r_dev": solve_stack, "align_volume_solve_group_r_dev": solve_volume_r}
for fn in ROUTES.values():  # warm-up: every workspace at its size
    fn()
t = {k: [] for k in ROUTES}
for _ in range(reps):  # the routes alternate
    for k, fn in ROUTES.items():
        t[k].append(wall(fn))
med = {k: {"device_ms": round(float(np.median([x[0] for x in v])), 3), "wall_ms": round(float(np.median([x[1] for x in v])), 3),
           "device_ms_min_max": [round(float(min(x[0] for x in v)), 3), round(float(max(x[0] for x in v)), 3)]} for k, v in t.items()}

per_eval = {"align_stack_reduce_kernels": [], "align_volume_reduce_r_kernels": []}
prof = {}
for _ in range(reps):  # the routes alternate here too: the per-evaluation figure of the two reduces, median and spread
    for name, fn in ROUTES.items():
        prof[name] = profiled(fn)
        for k in per_eval:
            if k in prof[name]["ms_per_evaluation"]:
                per_eval[k].append(prof[name]["ms_per_evaluation"][k])
for name in ROUTES:
    print(json.dumps({"profile_of": name, **prof[name]}), flush=True)

res = m.align_stack_solve(stack, goal_stack, planes, SPACING, groups=group_start, scale=SCALE, weights=weights, estimate_intensity=True, iterations=EVALS)
s, v = med["align_stack_solve_group_r_dev"], med["align_volume_solve_group_r_dev"]
summary = {k: {"median": round(float(np.median(x)), 5), "min_max": [min(x), max(x)]} for k, x in per_eval.items()}
print(json.dumps({"workload": {"stack": [NS, N, N], "targets": [MT, N, N], "groups": [SIZE] * G, "scale": SCALE}, "evaluations": EVALS, "reps": reps, "routes": med,
                  "stack_over_volume_device_ms": round(s["device_ms"] / v["device_ms"], 4), "ms_per_evaluation": summary,
                  "stack_reduce_over_volume_reduce_r": round(summary["align_stack_reduce_kernels"]["median"] / summary["align_volume_reduce_r_kernels"]["median"], 4),
                  "stack_solve": {"largest_map_error": float(np.abs(res.maps.astype(np.float64) - truth).max()),
                                  "largest_gain_bias_error": float(np.abs(res.intensity.astype(np.float64) - gb_truth).max()),
                                  "accepted_steps_per_group": res.accepted.tolist(), "flags": res.flags.tolist()}}), flush=True)
