#!/usr/bin/env python3
"""What evaluating the model off its own grid costs, default sine f16x3 model, the 400 tiles of one 320 x 320
slice, one stream, `reps` timed calls behind a 0.4 s warm-up, device time from msiren_timer_start / _stop:
  calls      msiren_forward_tiles_dev (the model's own 576 coordinates) against msiren_sample_tiles_dev on the x2 lattice (2 304), the x3
             lattice (5 184) and 2 304 scattered caller coordinates: ms per call and Mcoord/s (the same trunk over the same kind of units:
             the rates should agree within run-to-run noise; a lattice below 0.9 of the native rate points at its table against the L2)
  table      layer0_table_kernel alone (the profile's event pair around it) for Q = 576, 2 304, 5 184, and its share of a 400-tile call
  commit     msiren_commit_weights on the same handle: the host loop that builds the committed table (and packs every weight)
One JSON line per measurement.  Usage: python tools/sample_cost.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mri_inr_amd import ModulatedSiren, _lib, harness, synthetic as syn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0,
                   use_bias=True, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                   outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda:0", activation="sine")
m.load_state_dict(syn.make_state_dict(seed=7, trained_like=True))
m.to("cuda:0").eval()
harness.bind(m)
lib, h = m._lib, m._h

tiles, _ = harness.image_to_patches(syn.make_slice(0, 320, 320)[None], 32, 16)
B = tiles.shape[0]
d_tiles = m.device_array(tiles.shape).copy_from(tiles)
sets = {"native": None, "lattice_x2": m.upsampled_grid(32), "lattice_x3": m.upsampled_grid(48),
        "scattered_2304": np.random.default_rng(0).uniform(-1.0, 1.0, size=(2304, 2)).astype(np.float32)}


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


call_ms, native_rate = {}, None
for name, coords in sets.items():
    Q = 576 if coords is None else coords.shape[0]
    d_out = m.device_array((B, Q))
    if coords is None:
        ms = timed(lambda: _lib.check(lib.msiren_forward_tiles_dev(h, d_tiles.ptr, B, d_out.ptr)))
    else:
        d_c = m.device_array(coords.shape).copy_from(coords)
        ms = timed(lambda: _lib.check(lib.msiren_sample_tiles_dev(h, d_c.ptr, Q, d_tiles.ptr, B, d_out.ptr)))
    rate = B * Q / ms / 1e3
    native_rate = native_rate or rate
    call_ms[Q] = ms
    print(json.dumps({"call": name, "tiles": B, "coords_per_tile": Q, "ms_per_call": round(ms, 4), "mcoord_per_s": round(rate, 1),
                      "of_native": round(rate / native_rate, 3), "table_mb": round(Q * 1024 / 2**20, 2) if coords is not None else None,
                      "trunk": m.last_trunk_kernel()}), flush=True)

mods = syn.make_mods(1, 5, 1, 256)
d_mods, d_o1 = m.device_array(mods.shape).copy_from(mods), m.device_array((1, 5184))
for Q in (576, 2304, 5184):
    c = np.random.default_rng(Q).uniform(-1.0, 1.0, size=(Q, 2)).astype(np.float32)
    d_c = m.device_array(c.shape).copy_from(c)
    for _ in range(5):
        _lib.check(lib.msiren_sample_mods_dev(h, d_c.ptr, Q, d_mods.ptr, 1, d_o1.ptr))
    _lib.check(lib.msiren_profile_enable(h, 1))
    for _ in range(reps):
        _lib.check(lib.msiren_sample_mods_dev(h, d_c.ptr, Q, d_mods.ptr, 1, d_o1.ptr))
    rows = [r for r in m.profile_kernels() if r["kernel"] == "layer0_table_kernel"]
    _lib.check(lib.msiren_profile_enable(h, 0))
    us = rows[0]["ms_total"] / rows[0]["launches"] * 1e3
    share = us / 1e3 / call_ms[Q] if Q in call_ms else None
    print(json.dumps({"layer0_table_kernel": True, "Q": Q, "us_per_launch": round(us, 2), "launches": rows[0]["launches"],
                      "share_of_400_tile_call": round(share, 4) if share else None}), flush=True)

t = []
for _ in range(5):
    t0 = time.perf_counter()
    _lib.check(lib.msiren_commit_weights(h))
    t.append(time.perf_counter() - t0)
print(json.dumps({"msiren_commit_weights_ms": round(float(np.median(t)) * 1e3, 2)}), flush=True)
