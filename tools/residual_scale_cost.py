"""What msiren_residual_scale costs (LAB_NOTES.md section 39) on section 5.17's workload (tools/fuse_workload.py: 64 targets of 320 x 320
against a 16 x 320 x 320 stack), one JSON line per figure:
 (a) the device ms of the profile entry "residual_scale_kernels", median of 7, for both centres and for singletons, 16 groups of 4 and everything pooled,
     on the residual that msiren_project_volume leaves;
 (b) in the same run the device ms of "project_kernels" with the residual -- the call it follows -- and the host route it replaces: the residual copied
     back and np.partition per segment (wall ms);
 (c) bytes read per pass over device time: one selection reads targets and writes keys once, then reads the keys three times more (centre = 1: and once
     more to turn them, then three times again), against the card's copy bandwidth.

    python tools/residual_scale_cost.py [reps]"""
import json
import sys
import time

import numpy as np

import fuse_workload as fw
from mri_inr_amd import residual_scale as rs

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
m = fw.model(committed=False)
maps, targets, weights, gb = fw.workload()
TUNE = 6 * rs.MAD_TO_SIGMA
fused = m.fuse_targets(targets, maps, fw.GRID, fw.SPACING, weights=weights, intensity=gb)


def project():
    return m.project_volume(fused.volume, maps, (fw.N, fw.N), fw.SPACING, intensity=gb, targets=targets, weights=weights, residual=True)


residual = project().residual
pixels = residual.size
GROUPINGS = (("singletons", None), ("16 groups of 4", [4] * 16), ("pooled", [fw.MT]))
project_ms = [fw.profiled(m, project, "project_kernels") for _ in range(reps)]
print(json.dumps({"figure": "project_kernels with the residual", "ms_median": round(float(np.median(project_ms)), 4), "ms_min": round(min(project_ms), 4),
                  "ms_max": round(max(project_ms), 4), "pixels": pixels}), flush=True)
for centre in (False, True):
    for name, groups in GROUPINGS:
        kw = dict(tune=TUNE, weights=weights, groups=groups, centre=centre)
        ms = [fw.profiled(m, lambda: m.residual_scale(residual, **kw), "residual_scale_kernels") for _ in range(reps)]
        med = float(np.median(ms))
        # per pixel: the first pass reads residual and weight and writes the key (12 bytes), every other pass reads the key (4), the turn reads and writes it (8)
        moved = pixels * ((12 + 3 * 4) + ((8 + 3 * 4) if centre else 0))
        got = m.residual_scale(residual, stats=True, **kw)
        t0 = time.perf_counter()
        back = residual.copy()  # (stands for the copy back to the host: the array is on the host already; the partition is what is timed)
        offsets = rs.segments(groups, fw.MT)
        for lo, hi in zip(offsets[:-1], offsets[1:]):
            e = back[lo:hi][rs.pixel_counts(back[lo:hi], weights[lo:hi])]
            k = rs.rank(0.5, len(e))
            c = np.partition(e, k)[k] if centre else np.float32(0)
            np.partition(np.abs(e - c), k)[k]
        host_ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"figure": "residual_scale_kernels", "centre": int(centre), "segments": name, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
                          "ms_max": round(max(ms), 4), "over_project": round(med / float(np.median(project_ms)), 3), "bytes_moved": moved,
                          "gb_per_s": round(moved / (med * 1e-3) / 1e9, 1), "host_partition_wall_ms": round(host_ms, 2),
                          "scale_min": float(got.scale.min()), "scale_max": float(got.scale.max()), "count_total": int(got.stats[:, 0].sum())}), flush=True)
