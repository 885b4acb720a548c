#!/usr/bin/env python3
"""What the robust reduce costs in the grouped volume alignment, section 5.15's workload (tools/align_group_cost.py): default
sine model, fp32 handle, one stream, a stack of 16 slices of 320 x 320 and 16 targets of 320 x 320 as 4 groups of 4 under one rigid motion per group,
slices 4 pixels apart; from the nominal planes, 12 evaluations, the intensity estimated.  The targets are g_t W + b_t of the device's own warped
planes W at the truth, corrupted by + 5 inside a block, with smooth weights in (0, 1].

 (a) msiren_align_volume_solve_group_dev against msiren_align_volume_solve_group_r_dev (scale 0.01) on the SAME inputs, the block masked by the
     weights in both, so both reduce the same pixels: the pipeline is the same, only the reduce kernel differs (two fp64 divisions and a handful of
     multiplications more per pixel).  Device ms (msiren_timer_start / _stop: HIP events around the call), the routes alternating, medians and the
     run-to-run spread;
 (b) the profile of one solve of each kind per profiled entry: "align_volume_reduce_w_kernels" against "align_volume_reduce_r_kernels";
 (c) what the loss is for: the block NOT masked (its weights 1): the quadratic solve; the robust solve (scale 0.01) from the same nominal start, where
     the gains start 0.25 off and a scale that tight rejects most of the image; and the robust solve as a second pass, from the quadratic pass's state
     with align_robust.scale_from(that pass, 0.25) as its scale.  The largest |map - truth| and |(g, b) - truth| of each.

No threshold is set: the figures go to LAB_NOTES.md section 29.  One JSON line per measurement.  Usage: python tools/align_robust_cost.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, align_robust as ar, align_volume as av, synthetic as syn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N, NS, MT, G, EVALS, SPACING, SCALE, TUNE = 320, 16, 16, 4, 12, 4.0, 0.01, 0.25
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
goal = m.align_volume_cost(stack, np.zeros((MT, N, N), np.float32), truth, warped=True).warped
gb_truth = np.stack([np.linspace(0.8, 1.25, MT), np.linspace(-0.05, 0.1, MT)], axis=1).astype(np.float32)
i, j = np.mgrid[0:N, 0:N]
open_w = np.tile((0.2 + 0.8 * np.exp(-(((i - 0.5 * N) / (0.6 * N)) ** 2 + ((j - 0.5 * N) / (0.6 * N)) ** 2))).astype(np.float32), (MT, 1, 1))
open_w[BLOCK] = 1.0      # (c): nothing masks the corruption
masked_w = open_w.copy()
masked_w[BLOCK] = 0.0    # (a), (b): section 5.15's weights
goal_w = (gb_truth[:, :1, None] * goal + gb_truth[:, 1:, None]).astype(np.float32)
goal_w[BLOCK] += 5.0
identity = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
rigid_g = np.tile(identity, (G, 1))
scale = np.full(MT, SCALE, np.float64)
cg = _lib.AlignVolumeSolveGroupOpts(C.sizeof(_lib.AlignVolumeSolveGroupOpts), EVALS, av.ESTIMATE, 0, 1e-3, 0.1, 10.0, 1e-9, 1e9, SPACING)

d_i, d_tw, d_w = (m.device_array(x.shape).copy_from(x) for x in (stack, goal_w, masked_w))
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


def solve_group():
    return timed(lambda: _lib.check(lib.msiren_align_volume_solve_group_dev(h, d_i.ptr, NS, N, N, d_tw.ptr, MT, N, N, C.byref(cg), group_start.ctypes.data, G, d_p.ptr,
                                                                            d_rg.ptr, d_w.ptr, None, d_out.ptr, d_gout.ptr, d_gr.ptr, d_grep.ptr, d_trep.ptr, None)))


def solve_group_r():
    return timed(lambda: _lib.check(lib.msiren_align_volume_solve_group_r_dev(h, d_i.ptr, NS, N, N, d_tw.ptr, MT, N, N, C.byref(cg), group_start.ctypes.data, G, d_p.ptr,
                                                                              d_rg.ptr, d_w.ptr, None, d_s.ptr, d_out.ptr, d_gout.ptr, d_gr.ptr, d_grep.ptr, d_trep.ptr,
                                                                              None)))


def wall(fn):
    m.sync()
    t0 = time.perf_counter()
    dev = fn()
    m.sync()
    return dev, 1e3 * (time.perf_counter() - t0)


ROUTES = {"align_volume_solve_group_dev": solve_group, "align_volume_solve_group_r_dev": solve_group_r}
for fn in ROUTES.values():  # warm-up: every workspace at its size
    fn()
t = {k: [] for k in ROUTES}
for _ in range(reps):  # the routes alternate
    for k, fn in ROUTES.items():
        t[k].append(wall(fn))
med = {k: {"device_ms": round(float(np.median([x[0] for x in v])), 3), "wall_ms": round(float(np.median([x[1] for x in v])), 3),
           "device_ms_min_max": [round(float(min(x[0] for x in v)), 3), round(float(max(x[0] for x in v)), 3)]} for k, v in t.items()}

prof = {}
for name, fn in ROUTES.items():
    _lib.check(lib.msiren_profile_enable(h, 1))
    dev, wall_ms = wall(fn)
    p = {e["kernel"]: (e["launches"], round(e["ms_total"], 4)) for e in m.profile_kernels()}
    _lib.check(lib.msiren_profile_enable(h, 0))
    prof[name] = {"launches_and_ms_total": p, "profiled_ms": round(sum(v[1] for v in p.values()), 4), "device_ms": round(dev, 3), "wall_ms": round(wall_ms, 3),
                  "ms_per_evaluation": {k: round(v[1] / v[0], 5) for k, v in p.items() if v[0] == EVALS}}
    print(json.dumps({"profile_of": name, **prof[name]}), flush=True)

# (c) the block not masked: the quadratic solve, the robust solve from the same nominal start, and the robust solve as a second pass -- from the
# quadratic pass's state, with the scale that pass gives (align_robust.scale_from)
kw = dict(weights=open_w, estimate_intensity=True, iterations=EVALS)
quad = m.align_volume_solve_group(stack, goal_w, planes, SPACING, group_start, **kw)
rob = m.align_volume_solve_group_robust(stack, goal_w, planes, SPACING, group_start, SCALE, **kw)
second_scale = ar.scale_from(quad, TUNE)
second = m.align_volume_solve_group_robust(stack, goal_w, planes, SPACING, group_start, second_scale, rotation=quad.rotation, shift=quad.shift, intensity=quad.intensity,
                                           **kw)


def report(res):
    return {"largest_map_error": float(np.abs(res.maps.astype(np.float64) - truth).max()),
            "largest_gain_bias_error": float(np.abs(res.intensity.astype(np.float64) - gb_truth).max()), "accepted_steps_per_group": res.accepted.tolist(),
            "flags": res.flags.tolist()}


a, r = med["align_volume_solve_group_dev"], med["align_volume_solve_group_r_dev"]
w_ms = prof["align_volume_solve_group_dev"]["ms_per_evaluation"]["align_volume_reduce_w_kernels"]
r_ms = prof["align_volume_solve_group_r_dev"]["ms_per_evaluation"]["align_volume_reduce_r_kernels"]
print(json.dumps({"workload": {"stack": [NS, N, N], "targets": [MT, N, N], "groups": [SIZE] * G, "scale": SCALE}, "evaluations": EVALS, "reps": reps, "routes": med,
                  "robust_minus_weighted_device_ms": round(r["device_ms"] - a["device_ms"], 3),
                  "weighted_device_spread_ms": round(a["device_ms_min_max"][1] - a["device_ms_min_max"][0], 3),
                  "reduce_w_ms_per_evaluation": w_ms, "reduce_r_ms_per_evaluation": r_ms, "reduce_r_over_w": round(r_ms / w_ms, 4),
                  "unmasked_block": {"quadratic_from_the_nominal_planes": report(quad), "robust_from_the_nominal_planes": report(rob),
                                     "robust_second_pass": {"tune": TUNE, "scale_min_max": [float(second_scale.min()), float(second_scale.max())], **report(second)}}}),
      flush=True)
