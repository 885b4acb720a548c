#!/usr/bin/env python3
"""What scoring slices under affine maps costs, default sine model, fp32 handle, one stream: 16 slices of
320 x 320 against 320 x 320 targets, every slice under its own small rigid map.

1. model.align_cost (msiren_align_slices: one synchronous host call, 29 doubles per slice come back) against the same quantities by hand:
   the (n M, 3) points built on the host, model.resample_volume_with_gradient at integer Z (uploads the points, evaluates two slices per
   point, downloads value and three planes), the chain rule and the sums in numpy.  Host wall clock around synchronous calls, `reps` calls
   behind a warm-up; the two routes alternate.
2. msiren_align_slices_dev alone: device time from msiren_timer_start / _stop (HIP events), and per profiled step with the share of the two
   reduce kernels.
3. A Gauss-Newton demonstration: the target is the call's own `warped` under a known small rigid map; from the identity, cost and the largest
   parameter error per iteration.
One JSON line per measurement.  Usage: python tools/align_cost.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, align, synthetic as syn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
N, NS = 320, 16

m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0,
                   use_bias=True, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                   outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda:0", activation="sine", precision="fp32")
m.load_state_dict(syn.make_state_dict(seed=7, trained_like=True))
m.to("cuda:0").eval()
lib, h = m._lib, m._h

stack = np.stack([syn.make_slice(s, N, N) for s in range(NS)])
rng = np.random.default_rng(0)
centre = ((N - 1) / 2, (N - 1) / 2)
maps = align.rigid_maps(np.deg2rad(rng.uniform(-2, 2, NS)), rng.uniform(-1.5, 1.5, (NS, 2)), centre)
ii, jj = np.mgrid[0:N, 0:N]
targets = np.stack([0.5 + 0.4 * np.sin(0.021 * ii + 0.5 * s) * np.cos(0.017 * jj) for s in range(NS)]).astype(np.float32)
M = N * N


def by_hand():
    """the sums of align_cost without the call; returns them and the seconds of each part"""
    t0 = time.perf_counter()
    zyx = np.empty((NS, M, 3), np.float32)
    for s in range(NS):
        zyx[s, :, 0] = s
        zyx[s, :, 1:] = align.map_points(maps[s], (N, N))
    t1 = time.perf_counter()
    val, grad = m.resample_volume_with_gradient(stack, zyx.reshape(NS * M, 3))
    t2 = time.perf_counter()
    R, gY, gX = (x.reshape(NS, M).astype(np.float64) for x in (val, grad[1], grad[2]))
    T = targets.reshape(NS, M).astype(np.float64)
    ok = np.isfinite(T) & np.isfinite(R) & np.isfinite(gY) & np.isfinite(gX)
    i, j = ii.reshape(M).astype(np.float64), jj.reshape(M).astype(np.float64)
    sums = np.zeros((NS, align.SUMS))
    for s in range(NS):
        k = ok[s]
        r = R[s, k] - T[s, k]
        J = np.stack([gY[s, k] * i[k], gY[s, k] * j[k], gY[s, k], gX[s, k] * i[k], gX[s, k] * j[k], gX[s, k]])
        sums[s, 0], sums[s, 1], sums[s, 2:8] = k.sum(), r @ r, 2.0 * (J @ r)
        sums[s, 8:] = (J @ J.T)[np.triu_indices(6)]
    t3 = time.perf_counter()
    return sums, (t1 - t0, t2 - t1, t3 - t2)


res = m.align_cost(stack, targets, maps)     # warm-up of both routes, and the agreement of what they compute
hand, _ = by_hand()
res = m.align_cost(stack, targets, maps)
got = np.concatenate([res.count[:, None], res.cost[:, None], res.grad, res.jtj[:, np.triu_indices(6)[0], np.triu_indices(6)[1]]], axis=1)
agree = float(np.max(np.abs(got - hand) / np.maximum(np.abs(hand), 1e-300)))
t_call, t_hand = [], []
for _ in range(reps):
    t0 = time.perf_counter()
    m.align_cost(stack, targets, maps)
    t_call.append(time.perf_counter() - t0)
    t_hand.append(by_hand()[1])
t_hand = np.array(t_hand)
print(json.dumps({"workload": [NS, N, N], "targets": [N, N], "reps": reps, "valid_pixels": int(res.count.sum()),
                  "largest_relative_difference_call_vs_by_hand": agree,
                  "align_cost_host_call_ms": {"median": round(1e3 * float(np.median(t_call)), 3), "min": round(1e3 * min(t_call), 3), "max": round(1e3 * max(t_call), 3)},
                  "by_hand_ms": {"median": round(1e3 * float(np.median(t_hand.sum(axis=1))), 3), "min": round(1e3 * float(t_hand.sum(axis=1).min()), 3),
                                 "max": round(1e3 * float(t_hand.sum(axis=1).max()), 3),
                                 "points_on_host": round(1e3 * float(np.median(t_hand[:, 0])), 3),
                                 "resample_volume_with_gradient": round(1e3 * float(np.median(t_hand[:, 1])), 3),
                                 "host_sums": round(1e3 * float(np.median(t_hand[:, 2])), 3)},
                  "bytes_up_by_hand": int(NS * M * 12 + stack.nbytes), "bytes_down_by_hand": int(NS * M * 16),
                  "bytes_up_call": int(stack.nbytes + targets.nbytes + maps.nbytes), "bytes_down_call": int(NS * align.SUMS * 8)}), flush=True)

# the _dev form: device time and steps
d_i, d_t, d_m = (m.device_array(x.shape).copy_from(x) for x in (stack, targets, maps))
d_s = m.device_array((NS, 2 * align.SUMS))


def dev_call():
    _lib.check(lib.msiren_align_slices_dev(h, d_i.ptr, NS, N, N, d_t.ptr, N, N, d_m.ptr, d_s.ptr, None, None))


t_end = time.perf_counter() + 0.4
while time.perf_counter() < t_end:
    dev_call()
m.sync()
_lib.check(lib.msiren_timer_start(h))
for _ in range(reps):
    dev_call()
ms = C.c_float()
_lib.check(lib.msiren_timer_stop(h, C.byref(ms)))
m.sync()
_lib.check(lib.msiren_profile_enable(h, 1))
for _ in range(reps):
    dev_call()
m.sync()
per = {e["kernel"]: round(e["ms_total"] / e["launches"], 4) for e in m.profile_kernels()}
_lib.check(lib.msiren_profile_enable(h, 0))
total = sum(per.values())
print(json.dumps({"call": "msiren_align_slices_dev", "device_ms_per_call": round(ms.value / reps, 4), "steps_ms": per,
                  "reduce_share_of_profiled_steps": round(per.get("align_reduce_kernels", 0.0) / total, 4) if total else None}), flush=True)

# Gauss-Newton from the identity towards a known rigid map
truth = align.rigid_maps(np.deg2rad(np.linspace(-1.0, 1.0, NS)), np.stack([np.linspace(-0.8, 0.8, NS), np.linspace(0.6, -0.6, NS)], axis=1), centre)
goal = m.align_cost(stack, np.zeros_like(targets), truth, warped=True).warped
cur = np.tile(np.asarray(align.IDENTITY, np.float32), (NS, 1))
for it in range(8):
    r = m.align_cost(stack, goal, cur)
    print(json.dumps({"gauss_newton_iteration": it, "cost_sum": float(r.cost.sum()), "cost_max": float(r.cost.max()),
                      "largest_parameter_error": float(np.abs(cur.astype(np.float64) - truth).max()), "valid_pixels": int(r.count.sum())}), flush=True)
    cur = (cur.astype(np.float64) + align.gauss_newton_step(r, damping=1e-3)).astype(np.float32)
