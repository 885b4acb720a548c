#!/usr/bin/env python3
"""What the grouped step stage costs in the volume alignment, section 5.13's workload: default sine model, fp32 handle, one
stream, a stack of 16 slices of 320 x 320 and 16 targets of 320 x 320 on planes through it, slices 4 pixels apart, as 4 groups of 4 under one rigid
motion per group (the members of a group share their centre); from the nominal planes, 12 evaluations, the intensity estimated.  The targets are
g_t W + b_t of the device's own warped planes W at the truth, with smooth weights in (0, 1] and a masked block that is corrupted in the target.

 (a) msiren_align_volume_solve_w_dev (rigid, every target alone) against msiren_align_volume_solve_group_dev on the same inputs: the pipeline is the
     same, only the step stage differs.  Device ms (msiren_timer_start / _stop: HIP events around the call) and wall ms, the routes alternating,
     medians and the run-to-run spread;
 (b) the host loop: 12 msiren_align_volume_w calls on host pointers with align_group.lm_step_g in Python between them, wall ms;
 (c) the profile of one solve of each kind per profiled entry: "align_volume_step_w_kernel" against "align_group_step_kernels".

The claims: the grouped call's device time stays within (a)'s run-to-run spread plus the new step stage's own profiled time, and the grouped call is
faster than (b) in wall time.  One JSON line per measurement.  Usage: python tools/align_group_cost.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, align, align_group as ag, align_volume as av, synthetic as syn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N, NS, MT, G, EVALS, SPACING = 320, 16, 16, 4, 12, 4.0
SIZE = MT // G

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
weights = np.tile((0.2 + 0.8 * np.exp(-(((i - 0.5 * N) / (0.6 * N)) ** 2 + ((j - 0.5 * N) / (0.6 * N)) ** 2))).astype(np.float32), (MT, 1, 1))
weights[:, 100:140, 120:180] = 0.0
goal_w = (gb_truth[:, :1, None] * goal + gb_truth[:, 1:, None]).astype(np.float32)
goal_w[:, 100:140, 120:180] += 5.0
start = av.rigid_maps3(np.eye(3), np.zeros(3), planes, SPACING)
identity = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
rigid_t, rigid_g = np.tile(identity, (MT, 1)), np.tile(identity, (G, 1))
cw = _lib.AlignVolumeSolveWOpts(C.sizeof(_lib.AlignVolumeSolveWOpts), align.RIGID, EVALS, av.ESTIMATE, 1e-3, 0.1, 10.0, 1e-9, 1e9, SPACING)
cg = _lib.AlignVolumeSolveGroupOpts(C.sizeof(_lib.AlignVolumeSolveGroupOpts), EVALS, av.ESTIMATE, 0, 1e-3, 0.1, 10.0, 1e-9, 1e9, SPACING)

d_i, d_tw, d_m, d_w = (m.device_array(x.shape).copy_from(x) for x in (stack, goal_w, start, weights))
d_p = m.device_array((MT, 24)).copy_from(planes.view(np.float32))
d_rt, d_rg = m.device_array((MT, 24)).copy_from(rigid_t.view(np.float32)), m.device_array((G, 24)).copy_from(rigid_g.view(np.float32))
d_out, d_gout, d_rout, d_repw = m.device_array((MT, 9)), m.device_array((MT, 2)), m.device_array((MT, 24)), m.device_array((MT, 14))
d_gr, d_grep, d_trep = m.device_array((G, 24)), m.device_array((G, 14)), m.device_array((MT, 6))
ms = C.c_float()


def timed(fn):
    _lib.check(lib.msiren_timer_start(h))
    fn()
    _lib.check(lib.msiren_timer_stop(h, C.byref(ms)))
    return ms.value


def solve_w():
    return timed(lambda: _lib.check(lib.msiren_align_volume_solve_w_dev(h, d_i.ptr, NS, N, N, d_tw.ptr, MT, N, N, C.byref(cw), d_m.ptr, d_p.ptr, d_rt.ptr, d_w.ptr, None,
                                                                        d_out.ptr, d_gout.ptr, d_rout.ptr, d_repw.ptr, None)))


def solve_group():
    return timed(lambda: _lib.check(lib.msiren_align_volume_solve_group_dev(h, d_i.ptr, NS, N, N, d_tw.ptr, MT, N, N, C.byref(cg), group_start.ctypes.data, G, d_p.ptr,
                                                                            d_rg.ptr, d_w.ptr, None, d_out.ptr, d_gout.ptr, d_gr.ptr, d_grep.ptr, d_trep.ptr, None)))


def host_loop():
    """(b): the round trip the grouped call removes"""
    def cost_fn(maps, gb):
        r = m.align_volume_cost_w(stack, goal_w, maps, weights=weights, intensity=gb)
        iu = np.triu_indices(11)
        return np.concatenate([r.count[:, None].astype(np.float64), r.wsum[:, None], r.cost[:, None], r.grad, r.jtj[:, iu[0], iu[1]]], axis=1)

    return ag.solve_on_host_g(cost_fn, group_start, rigid=rigid_g, planes=planes, intensity=None,
                              options=ag.SolveOptionsG(iterations=EVALS, spacing=SPACING, intensity_mode=av.ESTIMATE))[0]


def wall(fn):
    m.sync()
    t0 = time.perf_counter()
    dev = fn()
    m.sync()
    return dev, 1e3 * (time.perf_counter() - t0)


ROUTES = {"align_volume_solve_w_dev": solve_w, "align_volume_solve_group_dev": solve_group}
for fn in ROUTES.values():  # warm-up: every workspace at its size
    fn()
t = {k: [] for k in ROUTES}
for _ in range(reps):  # the routes alternate
    for k, fn in ROUTES.items():
        t[k].append(wall(fn))
med = {k: {"device_ms": round(float(np.median([x[0] for x in v])), 3), "wall_ms": round(float(np.median([x[1] for x in v])), 3),
           "device_ms_min_max": [round(float(min(x[0] for x in v)), 3), round(float(max(x[0] for x in v)), 3)]} for k, v in t.items()}
host_loop()  # warm-up
host_ms, host = [], None
for _ in range(max(1, min(reps, 3))):
    m.sync()
    t0 = time.perf_counter()
    host = host_loop()
    host_ms.append(1e3 * (time.perf_counter() - t0))
solve_group()
m.sync()
maps, gb, grep = d_out.numpy(), d_gout.numpy(), d_grep.numpy().view(np.float64)

prof = {}
for name, fn in ROUTES.items():
    _lib.check(lib.msiren_profile_enable(h, 1))
    dev, wall_ms = wall(fn)
    p = {e["kernel"]: (e["launches"], round(e["ms_total"], 4)) for e in m.profile_kernels()}
    _lib.check(lib.msiren_profile_enable(h, 0))
    per_eval = {k: round(v[1] / v[0], 5) for k, v in p.items() if v[0] == EVALS}
    prof[name] = {"launches_and_ms_total": p, "profiled_ms": round(sum(v[1] for v in p.values()), 4), "device_ms": round(dev, 3), "wall_ms": round(wall_ms, 3),
                  "ms_per_evaluation": per_eval}
    print(json.dumps({"profile_of": name, **prof[name]}), flush=True)

a, g = med["align_volume_solve_w_dev"], med["align_volume_solve_group_dev"]
spread = a["device_ms_min_max"][1] - a["device_ms_min_max"][0]
step_ms = prof["align_volume_solve_group_dev"]["launches_and_ms_total"]["align_group_step_kernels"][1]
print(json.dumps({"workload": {"stack": [NS, N, N], "targets": [MT, N, N], "groups": [SIZE] * G}, "evaluations": EVALS, "reps": reps, "routes": med,
                  "host_loop_wall_ms": {"median": round(float(np.median(host_ms)), 3), "min_max": [round(min(host_ms), 3), round(max(host_ms), 3)]},
                  "group_minus_solve_w_device_ms": round(g["device_ms"] - a["device_ms"], 3), "solve_w_device_spread_ms": round(spread, 3),
                  "group_step_stage_profiled_ms": step_ms,
                  "solve_w_step_stage_profiled_ms": prof["align_volume_solve_w_dev"]["launches_and_ms_total"]["align_volume_step_w_kernel"][1],
                  "claim_device_within_spread_plus_step_stage": bool(g["device_ms"] <= a["device_ms"] + spread + step_ms),
                  "claim_faster_than_the_host_loop_in_wall_time": bool(g["wall_ms"] < float(np.median(host_ms))),
                  "device_equals_host_loop": bool(np.array_equal(maps, host.maps) and np.array_equal(gb, host.intensity) and
                                                  np.array_equal(grep[:, 0], host.accepted.astype(np.float64))),
                  "largest_map_error": float(np.abs(maps.astype(np.float64) - truth).max()),
                  "largest_gain_bias_error": float(np.abs(gb.astype(np.float64) - gb_truth).max()),
                  "accepted_steps_per_group": grep[:, 0].astype(int).tolist(), "flags": grep[:, 6].astype(int).tolist()}), flush=True)
