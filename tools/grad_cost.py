#!/usr/bin/env python3
"""What the model's spatial gradient costs, default sine model on an fp32 handle, one stream, `reps` timed calls
behind a 0.4 s warm-up, device time from msiren_timer_start / _stop (HIP events):
  trunk   msiren_sample_grad_mods_dev against msiren_sample_mods_dev, 400 patches x 576 coordinates (one 320 x 320 slice's worth): the jet
          kernel issues 3 x the fp32 trunk's MFMAs at one workgroup per CU where the fp32 trunk runs two -- the ratio is recorded against 3
  slice   msiren_reconstruct_slices_grad_dev against msiren_reconstruct_slices_dev on one 320 x 320 slice (prologue + trunk + 3 folds
          against prologue + trunk + 1 fold)
One JSON line per measurement.  Usage: python tools/grad_cost.py [reps]"""
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


def timed(call):
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


B, Q = 400, 576
mods = syn.make_mods(1, 5, B, 256)
coords = np.random.default_rng(0).uniform(-1.0, 1.0, size=(Q, 2)).astype(np.float32)
d_m, d_c = m.device_array(mods.shape).copy_from(mods), m.device_array(coords.shape).copy_from(coords)
d_v, d_g = m.device_array((B, Q)), m.device_array((2, B, Q))
ms_v = timed(lambda: _lib.check(lib.msiren_sample_mods_dev(h, d_c.ptr, Q, d_m.ptr, B, d_v.ptr)))
trunk = m.last_trunk_kernel()
ms_g = timed(lambda: _lib.check(lib.msiren_sample_grad_mods_dev(h, d_c.ptr, Q, d_m.ptr, B, d_v.ptr, d_g.ptr)))
print(json.dumps({"call": "sample_mods_grad vs sample_mods", "patches": B, "coords_per_patch": Q, "value_ms": round(ms_v, 4),
                  "value_and_grad_ms": round(ms_g, 4), "ratio": round(ms_g / ms_v, 3), "ratio_over_3": round(ms_g / ms_v / 3, 3),
                  "value_trunk": trunk}), flush=True)

img = syn.make_slice(0, 320, 320)[None]
d_i, d_r, d_gr = m.device_array(img.shape).copy_from(img), m.device_array((1, 320, 320)), m.device_array((2, 1, 320, 320))
ms_r = timed(lambda: _lib.check(lib.msiren_reconstruct_slices_dev(h, d_i.ptr, 1, 320, 320, d_r.ptr)))
ms_rg = timed(lambda: _lib.check(lib.msiren_reconstruct_slices_grad_dev(h, d_i.ptr, 1, 320, 320, 16, d_r.ptr, d_gr.ptr)))
print(json.dumps({"call": "reconstruct_slices_grad vs reconstruct_slices", "slice": [320, 320], "recon_ms": round(ms_r, 4),
                  "recon_and_grad_ms": round(ms_rg, 4), "ratio": round(ms_rg / ms_r, 3)}), flush=True)
