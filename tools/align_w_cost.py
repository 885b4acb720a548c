#!/usr/bin/env python3
"""What the per-pixel weight and the per-slice gain and bias cost, tools/align_solve_cost.py's workload: default sine
model, fp32 handle, one stream, 16 slices of 320 x 320 against 320 x 320 targets under a known small rigid map; from the identity, 8
evaluations.  The weighted targets are g_t W + b_t with smooth weights in (0, 1] and a masked block that is corrupted in the target.

 (a) msiren_align_solve_dev (29 sums) against msiren_align_solve_w_dev (47 sums, intensity fixed / estimated), the routes alternating:
     device ms (msiren_timer_start / _stop: HIP events around the call) and wall ms, medians;
 (b) one evaluation: msiren_align_slices_dev against msiren_align_slices_w_dev, the same way;
 (c) the profile of one solve of each kind per step: "align_reduce_kernels" / "align_step_kernel" against "align_reduce_w_kernels" /
     "align_step_w_kernel", and the trunk's share of an evaluation.

One JSON line per measurement.  Usage: python tools/align_w_cost.py [reps] [mode: 0 affine, 1 rigid]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, align, synthetic as syn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
mode = int(sys.argv[2]) if len(sys.argv) > 2 else align.RIGID
N, NS, EVALS = 320, 16, 8

m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0,
                   use_bias=True, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                   outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda:0", activation="sine", precision="fp32")
m.load_state_dict(syn.make_state_dict(seed=7, trained_like=True))
m.to("cuda:0").eval()
lib, h = m._lib, m._h

stack = np.stack([syn.make_slice(s, N, N) for s in range(NS)])
centre = ((N - 1) / 2, (N - 1) / 2)
truth = align.rigid_maps(np.deg2rad(np.linspace(-1.0, 1.0, NS)), np.stack([np.linspace(-0.8, 0.8, NS), np.linspace(0.6, -0.6, NS)], axis=1), centre)
goal = m.align_cost(stack, np.zeros((NS, N, N), np.float32), truth, warped=True).warped
gb_truth = np.stack([np.linspace(0.8, 1.25, NS), np.linspace(-0.05, 0.1, NS)], axis=1).astype(np.float32)
i, j = np.mgrid[0:N, 0:N]
weights = np.tile((0.2 + 0.8 * np.exp(-(((i - 0.5 * N) / (0.6 * N)) ** 2 + ((j - 0.5 * N) / (0.6 * N)) ** 2))).astype(np.float32), (NS, 1, 1))
weights[:, 100:140, 120:180] = 0.0
goal_w = (gb_truth[:, :1, None] * goal + gb_truth[:, 1:, None]).astype(np.float32)
goal_w[:, 100:140, 120:180] += 5.0
start = np.tile(np.asarray(align.IDENTITY, np.float32), (NS, 1))
rigid = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (NS, 1))
o = align.SolveOptions(mode=mode, iterations=EVALS, centre=centre)
co = _lib.AlignSolveOpts(C.sizeof(_lib.AlignSolveOpts), mode, EVALS, 0, o.damping, o.down, o.up, o.lam_min, o.lam_max, centre[0], centre[1])
cw = {est: _lib.AlignSolveWOpts(C.sizeof(_lib.AlignSolveWOpts), mode, EVALS, est, o.damping, o.down, o.up, o.lam_min, o.lam_max, centre[0], centre[1])
      for est in (align.FIXED, align.ESTIMATE)}

d_i, d_t, d_tw, d_m, d_w, d_gb = (m.device_array(x.shape).copy_from(x) for x in (stack, goal, goal_w, start, weights, gb_truth))
d_r = m.device_array((NS, 8)).copy_from(rigid.view(np.float32))
d_s, d_sw = m.device_array((NS, 2 * align.SUMS)), m.device_array((NS, 2 * align.SUMS_W))
d_out, d_gout, d_rout, d_rep, d_repw = m.device_array((NS, 6)), m.device_array((NS, 2)), m.device_array((NS, 8)), m.device_array((NS, 12)), m.device_array((NS, 14))
ms = C.c_float()


def timed(fn):
    _lib.check(lib.msiren_timer_start(h))
    fn()
    _lib.check(lib.msiren_timer_stop(h, C.byref(ms)))
    return ms.value


def plain_solve():
    return timed(lambda: _lib.check(lib.msiren_align_solve_dev(h, d_i.ptr, NS, N, N, d_t.ptr, N, N, C.byref(co), d_m.ptr, d_r.ptr, d_out.ptr, d_rout.ptr, d_rep.ptr, None)))


def weighted_solve(est):
    gb = None if est == align.ESTIMATE else d_gb.ptr  # estimated from (1, 0); fixed at the truth
    return timed(lambda: _lib.check(lib.msiren_align_solve_w_dev(h, d_i.ptr, NS, N, N, d_tw.ptr, N, N, C.byref(cw[est]), d_m.ptr, d_r.ptr, d_w.ptr, gb, d_out.ptr, d_gout.ptr,
                                                                 d_rout.ptr, d_repw.ptr, None)))


def plain_cost():
    return timed(lambda: _lib.check(lib.msiren_align_slices_dev(h, d_i.ptr, NS, N, N, d_t.ptr, N, N, d_m.ptr, d_s.ptr, None, None)))


def weighted_cost():
    return timed(lambda: _lib.check(lib.msiren_align_slices_w_dev(h, d_i.ptr, NS, N, N, d_tw.ptr, N, N, d_m.ptr, d_w.ptr, d_gb.ptr, d_sw.ptr, None, None)))


def wall(fn):
    m.sync()
    t0 = time.perf_counter()
    dev = fn()
    m.sync()
    return dev, 1e3 * (time.perf_counter() - t0)


ROUTES = {"align_solve_dev": plain_solve, "align_solve_w_dev_fixed": lambda: weighted_solve(align.FIXED), "align_solve_w_dev_estimate": lambda: weighted_solve(align.ESTIMATE),
          "align_slices_dev": plain_cost, "align_slices_w_dev": weighted_cost}
for fn in ROUTES.values():  # warm-up: every workspace at its size
    fn()
t = {k: [] for k in ROUTES}
for _ in range(reps):  # the routes alternate
    for k, fn in ROUTES.items():
        t[k].append(wall(fn))
med = {k: {"device_ms": round(float(np.median([x[0] for x in v])), 3), "wall_ms": round(float(np.median([x[1] for x in v])), 3),
           "device_ms_min_max": [round(float(min(x[0] for x in v)), 3), round(float(max(x[0] for x in v)), 3)]} for k, v in t.items()}
weighted_solve(align.ESTIMATE)
m.sync()
maps, gb, rep = d_out.numpy(), d_gout.numpy(), d_repw.numpy().view(np.float64)
plain_solve()
m.sync()
print(json.dumps({"workload": [NS, N, N], "evaluations": EVALS, "mode": "rigid" if mode else "affine", "reps": reps, "routes": med,
                  "solve_w_estimate_over_solve": round(med["align_solve_w_dev_estimate"]["device_ms"] / med["align_solve_dev"]["device_ms"], 4),
                  "solve_w_fixed_over_solve": round(med["align_solve_w_dev_fixed"]["device_ms"] / med["align_solve_dev"]["device_ms"], 4),
                  "slices_w_over_slices": round(med["align_slices_w_dev"]["device_ms"] / med["align_slices_dev"]["device_ms"], 4),
                  "estimate": {"largest_map_error": float(np.abs(maps.astype(np.float64) - truth).max()), "largest_gain_bias_error": float(np.abs(gb.astype(np.float64) - gb_truth).max()),
                               "accepted_steps_per_slice": rep[:, 0].astype(int).tolist(), "flags": rep[:, 6].astype(int).tolist()},
                  "plain_on_plain_targets_largest_map_error": float(np.abs(d_out.numpy().astype(np.float64) - truth).max())}), flush=True)

for name, fn in (("align_solve_dev", plain_solve), ("align_solve_w_dev_estimate", lambda: weighted_solve(align.ESTIMATE))):
    _lib.check(lib.msiren_profile_enable(h, 1))
    fn()
    m.sync()
    prof = {e["kernel"]: (e["launches"], round(e["ms_total"], 4)) for e in m.profile_kernels()}
    _lib.check(lib.msiren_profile_enable(h, 0))
    total = sum(v[1] for v in prof.values())
    per_eval = {k: round(v[1] / v[0], 5) for k, v in prof.items() if v[0] == EVALS}
    trunk = sum(v for k, v in per_eval.items() if "trunk" in k)
    print(json.dumps({"profile_of": name, "launches_and_ms_total": prof, "profiled_ms": round(total, 4), "ms_per_evaluation": per_eval,
                      "trunk_share_of_an_evaluation": round(trunk / max(sum(per_eval.values()), 1e-30), 4)}), flush=True)
