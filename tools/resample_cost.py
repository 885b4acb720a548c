#!/usr/bin/env python3
"""What reading the reconstruction at arbitrary points costs, default sine model on an fp32 handle, one stream,
`reps` timed calls behind a 0.4 s warm-up, device time from msiren_timer_start / _stop (HIP events): a 320 x 320 slice rotated by 10
degrees about its centre (102 400 points) through msiren_resample_slices_dev / _grad_dev, against msiren_reconstruct_slices_dev /
_grad_dev of the same slice -- the work is about the native number of (tile, coordinate) evaluations, so the fp32 handle's slice time is
the yardstick.  Then one profiled call of each form: the share of binning and blend (the profile's event pairs).
Then the same call on an f16x3 handle (the default precision): msiren_resample_slices_dev (exact: siren_trunk_f32_ragged_kernel) against
msiren_resample_slices_native_dev (siren_trunk_f16x3n_ragged_kernel + its conditional exact-fp32 launch), total and per profiled step, and
the native call on a slice whose upper half is black -- what the inactive units of the dropped tiles cost.
One JSON line per measurement.  Usage: python tools/resample_cost.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, synthetic as syn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0,
                   use_bias=True, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                   outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda:0", activation="sine", precision="fp32")
m.load_state_dict(syn.make_state_dict(seed=7, trained_like=True))
m.to("cuda:0").eval()
lib, h = m._lib, m._h


def timed(call, m=m):
    lib, h = m._lib, m._h
    t_end = time.perf_counter() + 0.4
    while time.perf_counter() < t_end:
        call()
    m.sync()
    _lib.check(lib.msiren_timer_start(h))
    for _ in range(reps):
        call()
    ms = C.c_float()
    _lib.check(lib.msiren_timer_stop(h, C.byref(ms)))
    return ms.value / reps


N = 320
img = syn.make_slice(0, N, N)[None]
yy, xx = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(N, dtype=np.float64), indexing="ij")
a, c = np.deg2rad(10.0), (N - 1) / 2
pts = np.stack([c + (yy - c) * np.cos(a) - (xx - c) * np.sin(a), c + (yy - c) * np.sin(a) + (xx - c) * np.cos(a)], -1).reshape(-1, 2).astype(np.float32)
M = len(pts)
d_i, d_p = m.device_array(img.shape).copy_from(img), m.device_array(pts.shape).copy_from(pts)
d_r, d_gr = m.device_array((1, N, N)), m.device_array((2, 1, N, N))
d_v, d_g = m.device_array((1, M)), m.device_array((2, 1, M))

calls = {
    "reconstruct": lambda: _lib.check(lib.msiren_reconstruct_slices_dev(h, d_i.ptr, 1, N, N, d_r.ptr)),
    "reconstruct_grad": lambda: _lib.check(lib.msiren_reconstruct_slices_grad_dev(h, d_i.ptr, 1, N, N, 16, d_r.ptr, d_gr.ptr)),
    "resample": lambda: _lib.check(lib.msiren_resample_slices_dev(h, d_i.ptr, 1, N, N, d_p.ptr, M, d_v.ptr)),
    "resample_grad": lambda: _lib.check(lib.msiren_resample_slices_grad_dev(h, d_i.ptr, 1, N, N, d_p.ptr, M, d_v.ptr, d_g.ptr)),
}
ms = {k: timed(f) for k, f in calls.items()}
covered = int(np.isfinite(d_v.numpy()).sum())
print(json.dumps({"call": "resample vs reconstruct", "slice": [N, N], "points": M, "points_covered": covered, "rotation_deg": 10,
                  "reconstruct_ms": round(ms["reconstruct"], 4), "resample_ms": round(ms["resample"], 4),
                  "ratio": round(ms["resample"] / ms["reconstruct"], 3)}), flush=True)
print(json.dumps({"call": "resample_grad vs reconstruct_grad", "reconstruct_grad_ms": round(ms["reconstruct_grad"], 4),
                  "resample_grad_ms": round(ms["resample_grad"], 4), "ratio": round(ms["resample_grad"] / ms["reconstruct_grad"], 3)}), flush=True)

for name in ("resample", "resample_grad"):
    m.sync()
    _lib.check(lib.msiren_profile_enable(h, 1))
    for _ in range(reps):
        calls[name]()
    entries = m.profile_kernels()
    _lib.check(lib.msiren_profile_enable(h, 0))
    per = {e["kernel"]: e["ms_total"] / e["launches"] for e in entries}
    total = sum(per.values())
    print(json.dumps({"call": name + " (profiled steps; the prologue's launches are not among them)",
                      "ms_per_call": {k: round(v, 4) for k, v in per.items()},
                      "bin_share_of_steps": round(per.get("resample_bin_kernels", 0.0) / total, 3),
                      "blend_share_of_steps": round(per.get("resample_blend_kernel", 0.0) / total, 3),
                      "bin_and_blend_share_of_call": round((per.get("resample_bin_kernels", 0.0) + per.get("resample_blend_kernel", 0.0)) / ms[name], 3)}),
          flush=True)


# ---- the default precision: exact against native (LAB_NOTES.md section 19) -----------------------------------------
m16 = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0,
                     use_bias=True, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                     outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda:0", activation="sine", precision="f16x3")
m16.load_state_dict(syn.make_state_dict(seed=7, trained_like=True))
m16.to("cuda:0").eval()
masked = img.copy()
masked[0, :N // 2] = 0.0
e_i, e_k, e_p = m16.device_array(img.shape).copy_from(img), m16.device_array(img.shape).copy_from(masked), m16.device_array(pts.shape).copy_from(pts)
e_v = m16.device_array((1, M))
calls16 = {
    "exact": lambda: _lib.check(m16._lib.msiren_resample_slices_dev(m16._h, e_i.ptr, 1, N, N, e_p.ptr, M, e_v.ptr)),
    "native": lambda: _lib.check(m16._lib.msiren_resample_slices_native_dev(m16._h, e_i.ptr, 1, N, N, e_p.ptr, M, e_v.ptr)),
    "exact_masked": lambda: _lib.check(m16._lib.msiren_resample_slices_dev(m16._h, e_k.ptr, 1, N, N, e_p.ptr, M, e_v.ptr)),
    "native_masked": lambda: _lib.check(m16._lib.msiren_resample_slices_native_dev(m16._h, e_k.ptr, 1, N, N, e_p.ptr, M, e_v.ptr)),
}
ms16 = {k: timed(f, m16) for k, f in calls16.items()}
steps = {}
for name, call in calls16.items():
    m16.sync()
    _lib.check(m16._lib.msiren_profile_enable(m16._h, 1))
    for _ in range(reps):
        call()
    m16.sync()
    steps[name] = {e["kernel"]: round(e["ms_total"] / e["launches"], 4) for e in m16.profile_kernels()}
    _lib.check(m16._lib.msiren_profile_enable(m16._h, 0))


def trunk_ms(per):
    return next(v for k, v in per.items() if k.startswith("siren_trunk_f32_ragged_kernel") or k.startswith("siren_trunk_f16x3n_ragged_kernel"))


for tag in ("", "_masked"):
    ex, na = steps["exact" + tag], steps["native" + tag]
    print(json.dumps({"call": "f16x3 handle, resample exact vs native" + (" (upper half of the slice black)" if tag else ""), "points": M,
                      "exact_ms": round(ms16["exact" + tag], 4), "native_ms": round(ms16["native" + tag], 4),
                      "call_ratio_exact_over_native": round(ms16["exact" + tag] / ms16["native" + tag], 3),
                      "exact_steps_ms": ex, "native_steps_ms": na,
                      "trunk_ratio_exact_over_native": round(trunk_ms(ex) / trunk_ms(na), 3)}), flush=True)

# two streams: consecutive calls alternate, so a call's conditional exact-fp32 launch (68 KB of LDS) meets the other stream's native trunk
_lib.check(m16._lib.msiren_set_streams(m16._h, 2))
ms2 = {k: timed(calls16[k], m16) for k in ("exact", "native")}
_lib.check(m16._lib.msiren_set_streams(m16._h, 1))
print(json.dumps({"call": "f16x3 handle, two streams, back-to-back calls", "exact_ms": round(ms2["exact"], 4), "native_ms": round(ms2["native"], 4),
                  "call_ratio_exact_over_native": round(ms2["exact"] / ms2["native"], 3)}), flush=True)
