#!/usr/bin/env python3
"""What scoring a 320 x 320 slice costs, host against device, for 1 and 64 slices:
  host       metrics.calculate_psnr / _ssim / _nrmse (fp64 numpy / scipy) on one pair, ms per slice
  device     msiren_score_images_dev on n pairs already in HBM, device time per call from msiren_timer_start / _stop
  old / new  wall time per slice of the evaluation step of one slice: reconstruct_from_patches + patches_to_image + the host
             metrics by hand (the path before scoring moved to the device) against harness.metrics_error (scores on the device)
One JSON line per slice count.  Usage: python tools/score_cost.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, harness, metrics, synthetic as syn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0,
                   use_bias=True, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                   outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda:0", activation="sine")
m.load_state_dict(syn.make_state_dict(seed=7, trained_like=True))
m.to("cuda:0").eval()
harness.bind(m)
lib, h = m._lib, m._h
HW = 320


def wall(fn, n):
    fn()  # warm-up: code objects, workspaces
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


for n in (1, 64):
    full_imgs = np.stack([syn.make_slice(k, HW, HW, brain_mask=True) for k in range(n)])
    under_imgs = ((full_imgs + np.roll(full_imgs, 1, 2) + np.roll(full_imgs, -1, 2)) / np.float32(3)).astype(np.float32)
    full_t, info = harness.image_to_patches(full_imgs, 32, 16)
    under_t, _ = harness.image_to_patches(under_imgs, 32, 16)
    per = full_t.shape[0] // n
    rec = harness.reconstruct_from_patches(m, under_t, info)
    full = harness.patches_to_image(full_t, info, 32, 16)

    host_ms = wall(lambda: (metrics.calculate_psnr(full[0], rec[0]), metrics.calculate_ssim(full[0], rec[0]),
                            metrics.calculate_nrmse(full[0], rec[0])), reps) * 1e3

    d_full = m.device_array(full.shape).copy_from(full)
    d_rec = m.device_array(rec.shape).copy_from(rec)
    d_s = m.device_array((n, 6))
    for _ in range(3):
        _lib.check(lib.msiren_score_images_dev(h, d_full.ptr, d_rec.ptr, n, HW, HW, d_s.ptr))
    calls = 200
    _lib.check(lib.msiren_timer_start(h))
    for _ in range(calls):
        _lib.check(lib.msiren_score_images_dev(h, d_full.ptr, d_rec.ptr, n, HW, HW, d_s.ptr))
    ms = C.c_float()
    _lib.check(lib.msiren_timer_stop(h, C.byref(ms)))
    dev_us = ms.value / calls * 1e3

    # the evaluation step of each slice in turn, tiles already on the device (as the driver hands them over)
    d_full_t = [m.device_array((per, 32, 32)).copy_from(full_t[k * per:(k + 1) * per]) for k in range(n)]
    d_under_t = [m.device_array((per, 32, 32)).copy_from(under_t[k * per:(k + 1) * per]) for k in range(n)]
    one = [info[0]]

    def old():
        for k in range(n):
            r = harness.reconstruct_from_patches(m, d_under_t[k], one).numpy()[0]
            f = harness.patches_to_image(d_full_t[k], one, 32, 16).numpy()[0]
            metrics.calculate_psnr(f, r), metrics.calculate_ssim(f, r), metrics.calculate_nrmse(f, r)

    def new():
        for k in range(n):
            harness.metrics_error(m, d_full_t[k], d_under_t[k], one, "cuda", 32, 16, 24)

    r_old = max(1, reps // n)
    old_ms = wall(old, r_old) * 1e3 / n
    new_ms = wall(new, max(3, reps * 4 // n)) * 1e3 / n
    print(json.dumps({"slices": n, "size": [HW, HW], "host_metrics_ms_per_slice": round(host_ms, 3),
                      "score_images_dev_us_per_call": round(dev_us, 2), "score_images_dev_us_per_slice": round(dev_us / n, 3),
                      "metrics_error_old_ms_per_slice": round(old_ms, 3), "metrics_error_new_ms_per_slice": round(new_ms, 3),
                      "speedup": round(old_ms / new_ms, 1)}), flush=True)
