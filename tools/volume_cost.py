#!/usr/bin/env python3
"""What reading a stack of slices as a volume costs, default sine model, one stream, `reps` timed calls behind a
0.4 s warm-up, device time from msiren_timer_start / _stop (HIP events): a 16-slice 320 x 320 stack read on an oblique 320 x 320 plane --
Z running 0 ... 15 across the plane's rows, rotated by 10 degrees in plane (102 400 points) -- through msiren_resample_volume_dev and
msiren_resample_volume_native_dev on an fp32 and an f16x3 handle, total and per profiled step, against the route without the volume call:
msiren_resample_slices_dev of all 16 slices at the plane's (Y, X) (the interpolation along Z on the host not counted).
Then the bin step alone next to resample_bin_kernels: the same 102 400 points at integer Z on ONE slice through both calls.
One JSON line per measurement.  Usage: python tools/volume_cost.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, plane_points, synthetic as syn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
N, NS = 320, 16


def build(prec):
    m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0,
                       use_bias=True, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                       outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda:0", activation="sine", precision=prec)
    m.load_state_dict(syn.make_state_dict(seed=7, trained_like=True))
    m.to("cuda:0").eval()
    return m


def timed(m, call):
    t_end = time.perf_counter() + 0.4
    while time.perf_counter() < t_end:
        call()
    m.sync()
    _lib.check(m._lib.msiren_timer_start(m._h))
    for _ in range(reps):
        call()
    ms = C.c_float()
    _lib.check(m._lib.msiren_timer_stop(m._h, C.byref(ms)))
    return ms.value / reps


def steps(m, call):
    m.sync()
    _lib.check(m._lib.msiren_profile_enable(m._h, 1))
    for _ in range(reps):
        call()
    m.sync()
    per = {e["kernel"]: round(e["ms_total"] / e["launches"], 4) for e in m.profile_kernels()}
    _lib.check(m._lib.msiren_profile_enable(m._h, 0))
    return per


stack = np.stack([syn.make_slice(s, N, N) for s in range(NS)])
a, c = np.deg2rad(10.0), (N - 1) / 2
u = np.array([(NS - 1) / (N - 1), np.cos(a), np.sin(a)])   # one row down the plane: Z from 0 to 15 over the 320 rows
v = np.array([0.0, -np.sin(a), np.cos(a)])
origin = np.array([0.0, c, c]) - c * (u * [0, 1, 1]) - c * v
pts = plane_points(origin, u, v, (N, N))
M = len(pts)
yx = np.ascontiguousarray(pts[:, 1:])
flat = np.ascontiguousarray(np.concatenate([np.zeros((M, 1), np.float32), yx], axis=1))  # integer Z on one slice

for prec in ("fp32", "f16x3"):
    m = build(prec)
    lib, h = m._lib, m._h
    d_i, d_p, d_yx, d_f = (m.device_array(x.shape).copy_from(x) for x in (stack, pts, yx, flat))
    d_v, d_all = m.device_array((M,)), m.device_array((NS, M))
    calls = {
        "volume": lambda: _lib.check(lib.msiren_resample_volume_dev(h, d_i.ptr, NS, N, N, d_p.ptr, M, d_v.ptr)),
        "volume_native": lambda: _lib.check(lib.msiren_resample_volume_native_dev(h, d_i.ptr, NS, N, N, d_p.ptr, M, d_v.ptr)),
        "all_slices": lambda: _lib.check(lib.msiren_resample_slices_dev(h, d_i.ptr, NS, N, N, d_yx.ptr, M, d_all.ptr)),
        "all_slices_native": lambda: _lib.check(lib.msiren_resample_slices_native_dev(h, d_i.ptr, NS, N, N, d_yx.ptr, M, d_all.ptr)),
        "one_slice_volume": lambda: _lib.check(lib.msiren_resample_volume_dev(h, d_i.ptr, 1, N, N, d_f.ptr, M, d_v.ptr)),
        "one_slice_resample": lambda: _lib.check(lib.msiren_resample_slices_dev(h, d_i.ptr, 1, N, N, d_yx.ptr, M, d_v.ptr)),
    }
    ms = {k: round(timed(m, f), 4) for k, f in calls.items()}
    per = {k: steps(m, f) for k, f in calls.items()}
    calls["volume"]()
    m.sync()
    covered = int(np.isfinite(d_v.numpy()).sum())
    print(json.dumps({"handle": prec, "stack": [NS, N, N], "points": M, "points_covered": covered, "rotation_deg": 10, "call_ms": ms,
                      "all_slices_over_volume": round(ms["all_slices"] / ms["volume"], 3),
                      "all_slices_native_over_volume_native": round(ms["all_slices_native"] / ms["volume_native"], 3)}), flush=True)
    for k in ("volume", "volume_native", "all_slices", "all_slices_native"):
        print(json.dumps({"handle": prec, "call": k, "steps_ms": per[k]}), flush=True)
    print(json.dumps({"handle": prec, "call": "bin step, 102 400 points at integer Z on one slice",
                      "resample_volume_bin_kernels_ms": per["one_slice_volume"].get("resample_volume_bin_kernels"),
                      "resample_bin_kernels_ms": per["one_slice_resample"].get("resample_bin_kernels"),
                      "one_slice_volume_ms": ms["one_slice_volume"], "one_slice_resample_ms": ms["one_slice_resample"]}), flush=True)
    del m
