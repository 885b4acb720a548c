#!/usr/bin/env python3
"""What scoring and aligning target slices against a volume on the device costs: default sine model, fp32 handle, one
stream, a stack of 16 slices of 320 x 320 and 16 targets of 320 x 320 on tilted planes through it (a rotation by a vector of up to 0.5 degrees
about the lattice's centre and a shift below a pixel, slices 4 pixels apart); the targets are the device's own warped planes at the truth.

 (a) one cost call, msiren_align_volume_dev, against the same sums by hand: the points built on the host, model.resample_volume_with_gradient
     (12 bytes per pixel up, 16 down), the chain rule and the 56 sums in numpy;
 (b) the solve, msiren_align_volume_solve_dev (one call, 8 evaluations), against 8 x msiren_align_volume_dev with a sync, 448 bytes per target
     down, align_volume.lm_step_v on the host and 36 bytes per target up in between -- the same trajectory, bit for bit;
 (c) the profile of one cost call and one solve per step;
 (d) the 2-D msiren_align_slices_dev on the same lattices (the in-plane six of the truth, target s against slice s): the volume call's trunk sees
     twice the entries.

Device ms: msiren_timer_start / _stop (HIP events) around each device call, summed; wall ms: the host's clock around the whole route.  One JSON
line per measurement.  Usage: python tools/align_volume_cost.py [reps] [mode: 0 affine, 1 rigid]"""
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
start = av.rigid_maps3(np.eye(3), np.zeros(3), planes, SPACING)
rigid = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (MT, 1))
o = av.SolveOptionsV(mode=mode, iterations=EVALS, spacing=SPACING)
co = _lib.AlignVolumeSolveOpts(C.sizeof(_lib.AlignVolumeSolveOpts), mode, EVALS, 0, o.damping, o.down, o.up, o.lam_min, o.lam_max, SPACING)

d_i, d_t, d_m = (m.device_array(x.shape).copy_from(x) for x in (stack, goal, start))
d_r, d_p = m.device_array((MT, 24)).copy_from(rigid.view(np.float32)), m.device_array((MT, 24)).copy_from(planes.view(np.float32))
d_cur, d_s = m.device_array((MT, 9)), m.device_array((MT, 2 * av.SUMS_V))
d_out, d_rout, d_rep = m.device_array((MT, 9)), m.device_array((MT, 24)), m.device_array((MT, 12))
d_m2, d_s2 = m.device_array((NS, 6)).copy_from(np.ascontiguousarray(truth[:, 3:])), m.device_array((NS, 2 * align.SUMS))
ms = C.c_float()


def timed(fn):
    _lib.check(lib.msiren_timer_start(h))
    fn()
    _lib.check(lib.msiren_timer_stop(h, C.byref(ms)))
    return ms.value


def cost_call(d_maps=d_m):
    return timed(lambda: _lib.check(lib.msiren_align_volume_dev(h, d_i.ptr, NS, N, N, d_t.ptr, MT, N, N, d_maps.ptr, d_s.ptr, None, None)))


def cost_by_hand():
    """(a): the loop body the call replaces -> sums (MT, 56)"""
    i = np.repeat(np.arange(N), N).astype(np.float64)
    j = np.tile(np.arange(N), N).astype(np.float64)
    out = np.zeros((MT, av.SUMS_V))
    pts = np.concatenate([av.map_points3(start[q], (N, N)) for q in range(MT)])
    val, grad = m.resample_volume_with_gradient(stack, pts)
    for q in range(MT):
        sl = slice(q * N * N, (q + 1) * N * N)
        R, gZ, gY, gX, T = (x.astype(np.float64) for x in (val[sl], grad[0, sl], grad[1, sl], grad[2, sl], goal[q].ravel()))
        ok = np.isfinite(R) & np.isfinite(gZ) & np.isfinite(gY) & np.isfinite(gX) & np.isfinite(T)
        r = (R - T)[ok]
        J = np.stack([gZ * i, gZ * j, gZ, gY * i, gY * j, gY, gX * i, gX * j, gX], axis=1)[ok]
        H = J.T @ J
        out[q] = np.concatenate([[ok.sum(), r @ r], 2.0 * (r @ J), H[np.triu_indices(9)]])
    return out


def on_device():
    """(b) one call -> (device ms, maps)"""
    dev = timed(lambda: _lib.check(lib.msiren_align_volume_solve_dev(h, d_i.ptr, NS, N, N, d_t.ptr, MT, N, N, C.byref(co), d_m.ptr, d_p.ptr, d_r.ptr, d_out.ptr,
                                                                     d_rout.ptr, d_rep.ptr, None)))
    return dev, d_out.numpy()


def dev_calls_host_steps():
    """(b) the cost call in a host loop -> (device ms, maps)"""
    st = [av.lm_init_v(o, start[q], rigid[q], planes[q]) for q in range(MT)]
    dev = 0.0
    for k in range(EVALS):
        d_cur.copy_from(np.array([x["trial"] for x in st], np.float32))
        dev += cost_call(d_cur)
        sums = d_s.numpy().view(np.float64)
        for q in range(MT):
            av.lm_step_v(st[q], sums[q], k, o)
    return dev, np.array([x["best"] for x in st], np.float32)


def cost_2d():
    return timed(lambda: _lib.check(lib.msiren_align_slices_dev(h, d_i.ptr, NS, N, N, d_t.ptr, N, N, d_m2.ptr, d_s2.ptr, None, None)))


def wall(fn):
    m.sync()
    t0 = time.perf_counter()
    out = fn()
    m.sync()
    return 1e3 * (time.perf_counter() - t0), out


for fn in (cost_call, cost_by_hand, on_device, dev_calls_host_steps, cost_2d):  # warm-up: every workspace at its size
    fn()
t = {k: [] for k in ("cost", "hand", "solve", "loop", "cost2d")}
for _ in range(reps):  # the routes alternate
    w, dev = wall(cost_call)
    t["cost"].append((dev, w))
    w, by_hand = wall(cost_by_hand)
    t["hand"].append((float("nan"), w))
    w, (dev, maps_i) = wall(on_device)
    t["solve"].append((dev, w))
    w, (dev, maps_ii) = wall(dev_calls_host_steps)
    t["loop"].append((dev, w))
    w, dev = wall(cost_2d)
    t["cost2d"].append((dev, w))
med = {k: [round(float(np.median([x[j] for x in v])), 3) for j in (0, 1)] for k, v in t.items()}
cost_call()
sums = d_s.numpy().view(np.float64)
scale = np.maximum(np.abs(sums), 1e-300)
err = lambda maps: float(np.abs(maps.astype(np.float64) - truth).max())  # noqa: E731
rep = d_rep.numpy().view(np.float64)  # of the last one-call solve: accepted, mean_first, mean_best, count, lam, flags
print(json.dumps({"workload": {"stack": [NS, N, N], "targets": [MT, N, N]}, "reps": reps,
                  "a_align_volume_dev": {"device_ms": med["cost"][0], "wall_ms": med["cost"][1]},
                  "a_by_hand_host_points_resample_volume_grad_numpy": {"wall_ms": med["hand"][1], "counts_equal": bool(np.array_equal(by_hand[:, 0], sums[:, 0])),
                                                                       "largest_relative_difference_of_a_sum": float((np.abs(by_hand - sums) / scale)[:, 1:].max())},
                  "d_align_slices_dev_same_lattices": {"device_ms": med["cost2d"][0], "wall_ms": med["cost2d"][1],
                                                       "volume_over_2d_device": round(med["cost"][0] / med["cost2d"][0], 4)}}), flush=True)
print(json.dumps({"evaluations": EVALS, "mode": "rigid" if mode else "affine",
                  "b_align_volume_solve_dev": {"device_ms": med["solve"][0], "wall_ms": med["solve"][1], "largest_map_error": err(maps_i),
                                               "median_map_error": float(np.median(np.abs(maps_i.astype(np.float64) - truth).max(axis=1))),
                                               "start_map_error": err(start), "accepted_steps_per_target": rep[:, 0].astype(int).tolist(),
                                               "flags": rep[:, 5].astype(int).tolist()},
                  "b_align_volume_dev_and_host_steps": {"device_ms": med["loop"][0], "wall_ms": med["loop"][1], "largest_map_error": err(maps_ii),
                                                        "same_bits_as_the_one_call_solve": bool(np.array_equal(maps_i, maps_ii))},
                  "device_ms_loop_minus_solve": round(med["loop"][0] - med["solve"][0], 3)}), flush=True)

for name, fn in (("align_volume_dev", cost_call), ("align_volume_solve_dev", on_device), ("align_slices_dev", cost_2d)):  # (c)
    _lib.check(lib.msiren_profile_enable(h, 1))
    fn()
    m.sync()
    prof = {e["kernel"]: (e["launches"], round(e["ms_total"], 4)) for e in m.profile_kernels()}
    _lib.check(lib.msiren_profile_enable(h, 0))
    total = sum(v[1] for v in prof.values())
    print(json.dumps({"profile_of": name, "launches_and_ms_total": prof, "profiled_ms": round(total, 4)}), flush=True)
