#!/usr/bin/env python3
"""What the per-pixel weight and the per-target gain and bias cost in the volume alignment, tools/align_volume_cost.py's
workload: default sine model, fp32 handle, one stream, a stack of 16 slices of 320 x 320 and 16 targets of 320 x 320 on tilted planes through it,
slices 4 pixels apart; from the nominal planes, 8 evaluations.  The weighted targets are g_t W + b_t of the device's own warped planes W at the
truth, with smooth weights in (0, 1] and a masked block that is corrupted in the target.

 (a) one evaluation: msiren_align_volume_dev (56 sums) against msiren_align_volume_w_dev (80 sums) without weights and intensity on the same
     targets, and with them on the weighted targets, the routes alternating: device ms (msiren_timer_start / _stop: HIP events around the call)
     and wall ms, medians;
 (b) msiren_align_volume_solve_dev against msiren_align_volume_solve_w_dev (intensity fixed / estimated), the same way;
 (c) the profile of one solve of each kind per step: "align_volume_reduce_kernels" / "align_volume_step_kernel" against
     "align_volume_reduce_w_kernels" / "align_volume_step_w_kernel", device and wall ms per profiled step, and the trunk's share of an evaluation.

One JSON line per measurement.  Usage: python tools/align_volume_w_cost.py [reps] [mode: 0 affine, 1 rigid]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, align, align_volume as av, synthetic as syn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
mode = int(sys.argv[2]) if len(sys.argv) > 2 else align.RIGID
N, NS, MT, EVALS, SPACING = 320, 16, 16, 8, 4.0

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
    planes[q] = np.concatenate([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], o, o + np.array([0.0, (N - 1) / 2, (N - 1) / 2])])


def rotation_of(vec):
    t = np.linalg.norm(vec)
    k = vec / t
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


lin = np.linspace(-1.0, 1.0, MT)
rot_true = np.stack([rotation_of(np.deg2rad([0.1 * a, 0.1 * (0.5 - a), 0.5 * a + 0.01])) for a in lin])  # tilts of up to 0.4 slices across the lattice
shift_true = np.stack([0.4 * lin, 0.8 * lin, -0.6 * lin], axis=1)
truth = av.rigid_maps3(rot_true, shift_true, planes, SPACING)
goal = m.align_volume_cost(stack, np.zeros((MT, N, N), np.float32), truth, warped=True).warped
gb_truth = np.stack([np.linspace(0.8, 1.25, MT), np.linspace(-0.05, 0.1, MT)], axis=1).astype(np.float32)
i, j = np.mgrid[0:N, 0:N]
weights = np.tile((0.2 + 0.8 * np.exp(-(((i - 0.5 * N) / (0.6 * N)) ** 2 + ((j - 0.5 * N) / (0.6 * N)) ** 2))).astype(np.float32), (MT, 1, 1))
weights[:, 100:140, 120:180] = 0.0
goal_w = (gb_truth[:, :1, None] * goal + gb_truth[:, 1:, None]).astype(np.float32)
goal_w[:, 100:140, 120:180] += 5.0
start = av.rigid_maps3(np.eye(3), np.zeros(3), planes, SPACING)
rigid = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (MT, 1))
o = av.SolveOptionsV(mode=mode, iterations=EVALS, spacing=SPACING)
co = _lib.AlignVolumeSolveOpts(C.sizeof(_lib.AlignVolumeSolveOpts), mode, EVALS, 0, o.damping, o.down, o.up, o.lam_min, o.lam_max, SPACING)
cw = {est: _lib.AlignVolumeSolveWOpts(C.sizeof(_lib.AlignVolumeSolveWOpts), mode, EVALS, est, o.damping, o.down, o.up, o.lam_min, o.lam_max, SPACING)
      for est in (av.FIXED, av.ESTIMATE)}

d_i, d_t, d_tw, d_m, d_w, d_gb = (m.device_array(x.shape).copy_from(x) for x in (stack, goal, goal_w, start, weights, gb_truth))
d_r, d_p = m.device_array((MT, 24)).copy_from(rigid.view(np.float32)), m.device_array((MT, 24)).copy_from(planes.view(np.float32))
d_s, d_sw = m.device_array((MT, 2 * av.SUMS_V)), m.device_array((MT, 2 * av.SUMS_VW))
d_out, d_gout, d_rout, d_rep, d_repw = m.device_array((MT, 9)), m.device_array((MT, 2)), m.device_array((MT, 24)), m.device_array((MT, 12)), m.device_array((MT, 14))
ms = C.c_float()


def timed(fn):
    _lib.check(lib.msiren_timer_start(h))
    fn()
    _lib.check(lib.msiren_timer_stop(h, C.byref(ms)))
    return ms.value


def plain_cost():
    return timed(lambda: _lib.check(lib.msiren_align_volume_dev(h, d_i.ptr, NS, N, N, d_t.ptr, MT, N, N, d_m.ptr, d_s.ptr, None, None)))


def weighted_cost(with_weights):
    if with_weights:
        return timed(lambda: _lib.check(lib.msiren_align_volume_w_dev(h, d_i.ptr, NS, N, N, d_tw.ptr, MT, N, N, d_m.ptr, d_w.ptr, d_gb.ptr, d_sw.ptr, None, None)))
    return timed(lambda: _lib.check(lib.msiren_align_volume_w_dev(h, d_i.ptr, NS, N, N, d_t.ptr, MT, N, N, d_m.ptr, None, None, d_sw.ptr, None, None)))


def plain_solve():
    return timed(lambda: _lib.check(lib.msiren_align_volume_solve_dev(h, d_i.ptr, NS, N, N, d_t.ptr, MT, N, N, C.byref(co), d_m.ptr, d_p.ptr, d_r.ptr, d_out.ptr, d_rout.ptr,
                                                                      d_rep.ptr, None)))


def weighted_solve(est):
    gb = None if est == av.ESTIMATE else d_gb.ptr  # estimated from (1, 0); fixed at the truth
    return timed(lambda: _lib.check(lib.msiren_align_volume_solve_w_dev(h, d_i.ptr, NS, N, N, d_tw.ptr, MT, N, N, C.byref(cw[est]), d_m.ptr, d_p.ptr, d_r.ptr, d_w.ptr, gb,
                                                                        d_out.ptr, d_gout.ptr, d_rout.ptr, d_repw.ptr, None)))


def wall(fn):
    m.sync()
    t0 = time.perf_counter()
    dev = fn()
    m.sync()
    return dev, 1e3 * (time.perf_counter() - t0)


ROUTES = {"align_volume_dev": plain_cost, "align_volume_w_dev_no_weights_no_intensity": lambda: weighted_cost(False), "align_volume_w_dev": lambda: weighted_cost(True),
          "align_volume_solve_dev": plain_solve, "align_volume_solve_w_dev_fixed": lambda: weighted_solve(av.FIXED),
          "align_volume_solve_w_dev_estimate": lambda: weighted_solve(av.ESTIMATE)}
for fn in ROUTES.values():  # warm-up: every workspace at its size
    fn()
t = {k: [] for k in ROUTES}
for _ in range(reps):  # the routes alternate
    for k, fn in ROUTES.items():
        t[k].append(wall(fn))
med = {k: {"device_ms": round(float(np.median([x[0] for x in v])), 3), "wall_ms": round(float(np.median([x[1] for x in v])), 3),
           "device_ms_min_max": [round(float(min(x[0] for x in v)), 3), round(float(max(x[0] for x in v)), 3)]} for k, v in t.items()}
plain_cost()
weighted_cost(False)
m.sync()
s56, s80 = d_s.numpy().view(np.float64), d_sw.numpy().view(np.float64)
shared = [0, 2] + list(range(3, 12)) + [14 + q for q, (a, b) in enumerate((a, b) for a in range(11) for b in range(a, 11)) if b < 9]
weighted_solve(av.ESTIMATE)
m.sync()
maps, gb, rep = d_out.numpy(), d_gout.numpy(), d_repw.numpy().view(np.float64)
plain_solve()
m.sync()
ratio = lambda a, b: round(med[a]["device_ms"] / med[b]["device_ms"], 4)  # noqa: E731
print(json.dumps({"workload": {"stack": [NS, N, N], "targets": [MT, N, N]}, "evaluations": EVALS, "mode": "rigid" if mode else "affine", "reps": reps, "routes": med,
                  "volume_w_no_weights_over_volume": ratio("align_volume_w_dev_no_weights_no_intensity", "align_volume_dev"),
                  "volume_w_over_volume": ratio("align_volume_w_dev", "align_volume_dev"),
                  "solve_w_fixed_over_solve": ratio("align_volume_solve_w_dev_fixed", "align_volume_solve_dev"),
                  "solve_w_estimate_over_solve": ratio("align_volume_solve_w_dev_estimate", "align_volume_solve_dev"),
                  "no_weights_no_intensity_shared_sums_same_bits": bool(np.array_equal(s80[:, shared], s56)),
                  "estimate": {"largest_map_error": float(np.abs(maps.astype(np.float64) - truth).max()),
                               "median_map_error": float(np.median(np.abs(maps.astype(np.float64) - truth).max(axis=1))),
                               "largest_gain_bias_error": float(np.abs(gb.astype(np.float64) - gb_truth).max()),
                               "accepted_steps_per_target": rep[:, 0].astype(int).tolist(), "flags": rep[:, 6].astype(int).tolist()},
                  "plain_on_plain_targets_largest_map_error": float(np.abs(d_out.numpy().astype(np.float64) - truth).max())}), flush=True)

for name, fn in (("align_volume_solve_dev", plain_solve), ("align_volume_solve_w_dev_estimate", lambda: weighted_solve(av.ESTIMATE)),
                 ("align_volume_dev", plain_cost), ("align_volume_w_dev_no_weights_no_intensity", lambda: weighted_cost(False)), ("align_volume_w_dev", lambda: weighted_cost(True))):
    _lib.check(lib.msiren_profile_enable(h, 1))
    dev, wall_ms = wall(fn)
    prof = {e["kernel"]: (e["launches"], round(e["ms_total"], 4)) for e in m.profile_kernels()}
    _lib.check(lib.msiren_profile_enable(h, 0))
    total = sum(v[1] for v in prof.values())
    evals = EVALS if "solve" in name else 1
    per_eval = {k: round(v[1] / v[0], 5) for k, v in prof.items() if v[0] == evals and ("align" in k or "ragged" in k)}
    trunk = sum(v for k, v in per_eval.items() if "trunk" in k)
    print(json.dumps({"profile_of": name, "launches_and_ms_total": prof, "profiled_ms": round(total, 4), "device_ms": round(dev, 3), "wall_ms": round(wall_ms, 3),
                      "ms_per_evaluation": per_eval, "trunk_share_of_an_evaluation": round(trunk / max(sum(per_eval.values()), 1e-30), 4)}), flush=True)
