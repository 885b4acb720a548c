"""What msiren_leave_out_targets costs (LAB_NOTES.md section 42) on section 5.17's workload (tools/fuse_workload.py: 64 targets of
320 x 320 against a 16 x 320 x 320 stack), for singletons and for 4 groups of 16, one JSON line per figure, all in one run:
 (a) the device ms of the profile entry "leave_out_kernels", median of 5, with the residual and the stats;
 (b) beside it "fuse_kernels" of all targets and "project_kernels" of all targets with the residual and the stats: the call should cost about two
     projections;
 (c) what it replaces: per group one fuse_targets of the targets outside it and one project_volume of its own -- the wall time of the G + G calls and the
     device time of their profile entries -- and how far the two predictions are apart (the chain rounds its stack to float32);
 (d) the wall time of the numpy restatement leave_out_on_host, and that the device has its bits;
 (e) the table of the issue on the device: tests/fuse_cases.py's truth case thinned to every 4th target, + 0.5 on a 20 x 20 block of one target, the mean
     |residual| inside and outside the block for the self-residual project_volume(fuse_targets(all)) and for the left-out residual, at two thicknesses.

    python tools/leave_out_cost.py [reps]"""
import json
import os
import sys
import time

import numpy as np

import fuse_workload as fw
from mri_inr_amd import _lib, leave_out as lo

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import fuse_cases as fc  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
m = fw.model(committed=False)
maps, targets, weights, gb = fw.workload()
KW = dict(weights=weights, intensity=gb)


def stats_of(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


fused = m.fuse_targets(targets, maps, fw.GRID, fw.SPACING, **KW)
fuse_ms = [fw.profiled(m, lambda: m.fuse_targets(targets, maps, fw.GRID, fw.SPACING, **KW), "fuse_kernels") for _ in range(reps)]
project_ms = [fw.profiled(m, lambda: m.project_volume(fused.volume, maps, (fw.N, fw.N), fw.SPACING, intensity=gb, targets=targets, weights=weights, residual=True,
                                                      stats=True), "project_kernels") for _ in range(reps)]
print(json.dumps({"figure": "fuse_kernels, all targets", **stats_of(fuse_ms)}), flush=True)
print(json.dumps({"figure": "project_kernels, all targets, residual and stats", **stats_of(project_ms)}), flush=True)

for name, groups in (("singletons", None), ("4 groups of 16", [16] * 4)):
    call = lambda: m.leave_out_targets(targets, maps, fw.GRID, fw.SPACING, groups=groups, residual=True, stats=True, **KW)  # noqa: E731
    ms = [fw.profiled(m, call, "leave_out_kernels") for _ in range(reps)]
    got = m.leave_out_targets(targets, maps, fw.GRID, fw.SPACING, groups=groups, coverage=True, residual=True, stats=True, volume=True, **KW)
    # (c) the chain it replaces
    offsets = lo.segments(groups, fw.MT)
    sim = np.full(targets.shape, np.nan, np.float32)
    _lib.check(m._lib.msiren_profile_enable(m._h, 1))
    t0 = time.perf_counter()
    for a, b in zip(offsets[:-1], offsets[1:]):
        rest = np.ones(fw.MT, bool)
        rest[a:b] = False
        stack = m.fuse_targets(targets[rest], maps[rest], fw.GRID, fw.SPACING, weights=weights[rest], intensity=gb[rest])
        sim[a:b] = m.project_volume(stack.volume, maps[a:b], (fw.N, fw.N), fw.SPACING, intensity=gb[a:b], targets=targets[a:b], weights=weights[a:b], residual=True,
                                    stats=True).simulated
    m.sync()
    chain_wall = (time.perf_counter() - t0) * 1e3
    chain_dev = {e["kernel"]: (e["launches"], e["ms_total"]) for e in m.profile_kernels()}
    _lib.check(m._lib.msiren_profile_enable(m._h, 0))
    both = np.isfinite(sim) & np.isfinite(got.simulated)
    t0 = time.perf_counter()
    call()
    call_wall = (time.perf_counter() - t0) * 1e3
    # (d) the restatement
    t0 = time.perf_counter()
    want = lo.leave_out_on_host(targets, maps, fw.GRID, fw.SPACING, groups=groups, **KW)
    host_s = time.perf_counter() - t0
    same = all(np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes() for g, w in zip(got, want))
    med = float(np.median(ms))
    print(json.dumps({"figure": "leave_out_kernels", "groups": name, **stats_of(ms), "over_project": round(med / float(np.median(project_ms)), 3),
                      "over_fuse_plus_project": round(med / float(np.median(project_ms) + np.median(fuse_ms)), 3), "call_wall_ms": round(call_wall, 2),
                      "chain_calls": 2 * (len(offsets) - 1), "chain_wall_ms": round(chain_wall, 1),
                      "chain_device_ms": round(sum(v[1] for v in chain_dev.values()), 3), "chain_entries": {k: [v[0], round(v[1], 3)] for k, v in chain_dev.items()},
                      "pixels_predicted": int(np.isfinite(got.simulated).sum()), "pixels": int(got.simulated.size),
                      "finite_masks_differ": int((np.isfinite(sim) != np.isfinite(got.simulated)).sum()),
                      "max_abs_difference_to_the_chain": float(np.abs(sim.astype(np.float64) - got.simulated)[both].max()),
                      "leave_out_on_host_s": round(host_s, 2), "device_has_the_restatements_bits": bool(same)}), flush=True)

# (e) the table
t = fc.truth_case()
T, mp = t["targets"][::4].copy(), t["maps"][::4]
T[2, 10:30, 10:30] += np.float32(0.5)
block = np.zeros(T.shape, bool)
block[2, 10:30, 10:30] = True
for thickness in (fc.SPACING, fc.SPACING / 2):
    f = m.fuse_targets(T, mp, fc.TRUTH_GRID, fc.SPACING, thickness=thickness)
    own = np.abs(m.project_volume(f.volume, mp, T.shape[1:], fc.SPACING, thickness=thickness, targets=T, residual=True).residual)
    left = np.abs(m.leave_out_targets(T, mp, fc.TRUTH_GRID, fc.SPACING, thickness=thickness, residual=True).residual)
    ok = np.isfinite(own) & np.isfinite(left)
    print(json.dumps({"figure": "mean |residual|", "thickness": thickness, "self_in_the_block": round(float(own[ok & block].mean()), 4),
                      "self_elsewhere": round(float(own[ok & ~block].mean()), 4), "left_out_in_the_block": round(float(left[ok & block].mean()), 4),
                      "left_out_elsewhere": round(float(left[ok & ~block].mean()), 4), "pixels": int(ok.sum())}), flush=True)
