#!/usr/bin/env python3
"""What aligning slices on the device saves, tools/align_cost.py's workload: default sine model, fp32 handle, one
stream, 16 slices of 320 x 320 against 320 x 320 targets that are the slices' own warped planes under a known small rigid map; from the
identity, 8 evaluations, three ways:

 (i)   msiren_align_solve_dev: the prologue once, the step on the device, no host synchronisation inside the call;
 (ii)  8 x msiren_align_slices_dev with a sync, 232 bytes per slice down, align.lm_step on the host and 24 bytes per slice up in between --
       the same trajectory, bit for bit;
 (iii) the README loop on host pointers: model.align_cost + align.gauss_newton_step (images and targets uploaded every iteration).

Device ms: msiren_timer_start / _stop (HIP events) around each device call, summed -- the host's work between the calls of (ii) is not in
it; wall ms: the host's clock around the whole loop.  The slice prologue has no profile entry of its own: what seven more of them (and
seven more calls) cost is the device time of (ii) minus that of (i).  Then the profile of (i) and (ii) per step.  One JSON line per
measurement.  Usage: python tools/align_solve_cost.py [reps] [mode: 0 affine, 1 rigid]"""
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
start = np.tile(np.asarray(align.IDENTITY, np.float32), (NS, 1))
rigid = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (NS, 1))
o = align.SolveOptions(mode=mode, iterations=EVALS, centre=centre)
co = _lib.AlignSolveOpts(C.sizeof(_lib.AlignSolveOpts), mode, EVALS, 0, o.damping, o.down, o.up, o.lam_min, o.lam_max, centre[0], centre[1])

d_i, d_t, d_m = (m.device_array(x.shape).copy_from(x) for x in (stack, goal, start))
d_r = m.device_array((NS, 8)).copy_from(rigid.view(np.float32))
d_cur, d_s = m.device_array((NS, 6)), m.device_array((NS, 2 * align.SUMS))
d_out, d_rout, d_rep = m.device_array((NS, 6)), m.device_array((NS, 8)), m.device_array((NS, 12))
ms = C.c_float()


def timed(fn):
    _lib.check(lib.msiren_timer_start(h))
    fn()
    _lib.check(lib.msiren_timer_stop(h, C.byref(ms)))
    return ms.value


def on_device():
    """(i) -> (device ms, maps)"""
    dev = timed(lambda: _lib.check(lib.msiren_align_solve_dev(h, d_i.ptr, NS, N, N, d_t.ptr, N, N, C.byref(co), d_m.ptr, d_r.ptr, d_out.ptr, d_rout.ptr, d_rep.ptr, None)))
    return dev, d_out.numpy()


def dev_calls_host_steps():
    """(ii) -> (device ms, maps)"""
    st = [align.lm_init(o, start[s], rigid[s]) for s in range(NS)]
    dev = 0.0
    for k in range(EVALS):
        d_cur.copy_from(np.array([x["trial"] for x in st], np.float32))
        dev += timed(lambda: _lib.check(lib.msiren_align_slices_dev(h, d_i.ptr, NS, N, N, d_t.ptr, N, N, d_cur.ptr, d_s.ptr, None, None)))
        sums = d_s.numpy().view(np.float64)
        for s in range(NS):
            align.lm_step(st[s], sums[s], k, o)
    return dev, np.array([x["best"] for x in st], np.float32)


def readme_loop():
    """(iii) -> maps"""
    cur = start.copy()
    for _ in range(EVALS):
        r = m.align_cost(stack, goal, cur)
        cur = (cur + align.gauss_newton_step(r, damping=1e-3)).astype(np.float32)
    return cur


def wall(fn):
    m.sync()
    t0 = time.perf_counter()
    out = fn()
    m.sync()
    return 1e3 * (time.perf_counter() - t0), out


for fn in (on_device, dev_calls_host_steps, readme_loop):  # warm-up: every workspace at its size
    fn()
t = {"i": [], "ii": [], "iii": []}
for _ in range(reps):  # the three alternate
    w, (dev, maps_i) = wall(on_device)
    t["i"].append((dev, w))
    w, (dev, maps_ii) = wall(dev_calls_host_steps)
    t["ii"].append((dev, w))
    w, maps_iii = wall(readme_loop)
    t["iii"].append((float("nan"), w))
med = {k: [round(float(np.median([x[j] for x in v])), 3) for j in (0, 1)] for k, v in t.items()}
err = lambda maps: float(np.abs(maps.astype(np.float64) - truth).max())  # noqa: E731
rep = d_rep.numpy().view(np.float64)  # of the last (i): accepted, mean_first, mean_best, count, lam, flags
ratio = rep[:, 2] / rep[:, 1]
print(json.dumps({"workload": [NS, N, N], "evaluations": EVALS, "mode": "rigid" if mode else "affine", "reps": reps,
                  "i_align_solve_dev": {"device_ms": med["i"][0], "wall_ms": med["i"][1], "largest_parameter_error": err(maps_i),
                                        "median_parameter_error": float(np.median(np.abs(maps_i.astype(np.float64) - truth).max(axis=1))),
                                        "accepted_steps_per_slice": rep[:, 0].astype(int).tolist(),
                                        "mean_best_over_mean_first": {"min": float(ratio.min()), "median": float(np.median(ratio)), "max": float(ratio.max())}},
                  "ii_align_slices_dev_and_host_steps": {"device_ms": med["ii"][0], "wall_ms": med["ii"][1], "largest_parameter_error": err(maps_ii),
                                                         "same_bits_as_i": bool(np.array_equal(maps_i, maps_ii))},
                  "iii_readme_loop_host_pointers": {"wall_ms": med["iii"][1], "largest_parameter_error": err(maps_iii)},
                  "device_ms_ii_minus_i": round(med["ii"][0] - med["i"][0], 3), "share_of_ii": round((med["ii"][0] - med["i"][0]) / med["ii"][0], 4)}), flush=True)

PER_EVAL = ("align_bin_kernels", "align_reduce_kernels", "align_step_kernel")
for name, fn in (("i", on_device), ("ii", dev_calls_host_steps)):
    _lib.check(lib.msiren_profile_enable(h, 1))
    fn()
    m.sync()
    prof = {e["kernel"]: (e["launches"], round(e["ms_total"], 4)) for e in m.profile_kernels()}
    _lib.check(lib.msiren_profile_enable(h, 0))
    total = sum(v[1] for v in prof.values())
    print(json.dumps({"profile_of": name, "launches_and_ms_total": prof, "profiled_ms": round(total, 4)}), flush=True)
