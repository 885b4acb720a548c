"""The registration binding's own rules, checked on a host without a device: what every public method from ``resample`` to
``solve_volume_robust`` hands to the library, and what it returns when the library writes nothing.

A ``ModulatedSiren`` is built without a handle and given a recording stand-in for the library: every ``msiren_*`` attribute is a function
that records its arguments and returns 0.  Per call the record holds the function's name, the number of arguments (checked against
``_lib.PROTOTYPES``), every scalar, the bytes of the opts structure, and a label per pointer: ``null``, ``in:<name>`` where it is the address
of one of the caller's arrays (the inputs are contiguous and of the final dtype, so what the binding forwards without a copy keeps its address:
a swap of targets and weights shows), ``out:<field>`` where it is the address of an array of the result, else ``fresh``.  Host arrays the binding
builds itself (rigid states, group offsets, scales, ``resample_each``'s points) are read through their pointer and recorded by value.  The
result is recorded field by field -- type, shape, dtype, values: the stand-in writes nothing, so the values are the binding's pre-fill.
``commits``: whether the model's weights were pushed and committed in front of the call.  A refusal is recorded as the exception's type, and
the test asserts that the library was not entered.

The expectations are ``tests/golden/binding_calls.json``.  That file was written by this module's recorder (``python
tests/test_binding_calls.py --write <file>``) from the binding as it stood in commit d321e11, before the family moved out of ``model.py``;
it is not regenerated when the binding is restructured -- a binding that disagrees with it has changed what the library is given.  Its entry
``public`` holds the signature and the docstring's digest of every method: nothing a caller sees moved with the code."""

import ctypes as C
import hashlib
import inspect
import json
import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN_FILE = os.path.join(REPO, "tests", "golden", "binding_calls.json")

# pairwise distinct sizes: a swapped pair of dimensions shows in the scalars
N, HH, WW, M, TH, TW, G, NP = 3, 7, 5, 4, 3, 2, 2, 6
KW = dict(dim_in=2, dim_hidden=64, dim_out=1, num_layers=3, latent_dim=32, w0=1.0, w0_initial=30.0, use_bias=True, dropout=0.1, modulate=True,
          encoder_type="custom", encoder_path=None, outer_patch_size=32, inner_patch_size=16, siren_patch_size=12, device="cpu", activation="sine")
WEIGHT_CALLS = ("msiren_set_tensor", "msiren_commit_weights")

# host arrays the binding builds itself: function -> {argument index: (dtype, element count from the call's arguments)}
_RIGID2 = {10: (np.float64, lambda a: 4 * a[2])}
_RIGID3 = {12: (np.float64, lambda a: 12 * a[6])}
_POINTS3 = {5: (np.float32, lambda a: 3 * a[6])}
_GROUP = {10: (np.int32, lambda a: a[11] + 1), 13: (np.float64, lambda a: 12 * a[11])}
BUILT = {
    "msiren_resample_volume": _POINTS3, "msiren_resample_volume_native": _POINTS3,
    "msiren_align_solve": _RIGID2, "msiren_align_solve_w": _RIGID2,
    "msiren_align_volume_solve": _RIGID3, "msiren_align_volume_solve_w": _RIGID3,
    "msiren_align_volume_solve_group": _GROUP,
    "msiren_align_volume_solve_group_r": {**_GROUP, 16: (np.float64, lambda a: a[6])},
    "msiren_align_volume_r": {12: (np.float64, lambda a: a[6])},
    "msiren_solve_volume_r": {8: (np.float64, lambda a: a[2])},
}


class Recorder:
    """stands in for the loaded library: every attribute is a function that records its arguments and returns 0.  The arguments are taken
    apart inside the call, where the arrays the binding built are alive"""

    def __init__(self):
        self.names, self.calls = [], []

    def __getattr__(self, name):
        def fn(*args):
            self.names.append(name)
            if name not in WEIGHT_CALLS:
                self.calls.append((name, _arguments(name, args)))
            return 0
        return fn


def _ramp(shape, dtype=np.float32, step=0.25, first=1.0):
    return np.ascontiguousarray((first + step * np.arange(int(np.prod(shape)))).reshape(shape), dtype=dtype)


def inputs():
    """the caller's arrays, by the name a pointer to them is labelled with"""
    rot = np.zeros((M, 3, 3))
    rot[:, 0, 0], rot[:, 1, 2], rot[:, 2, 1] = 1.0, -1.0, 1.0  # (a quarter turn about Z: not the identity)
    return dict(
        images=_ramp((N, HH, WW)), points2=_ramp((NP, 2)), points3=_ramp((NP, 3)), points_each=_ramp((N, NP, 2)),
        targets2=_ramp((N, TH, TW)), weights2=_ramp((N, TH, TW), step=0.5), intensity2=_ramp((N, 2), first=2.0), maps2=_ramp((N, 6)),
        angle=_ramp((N,), np.float64, 0.5, 0.0), shift2=_ramp((N, 2), np.float64),
        targets=_ramp((M, TH, TW)), weights=_ramp((M, TH, TW), step=0.5), intensity=_ramp((M, 2), first=2.0), maps=_ramp((M, 9)),
        planes=_ramp((M, 12), np.float64), rotation=rot, shift3=_ramp((M, 3), np.float64), rotation_g=np.ascontiguousarray(rot[:G]),
        shift_g=_ramp((G, 3), np.float64), scales=_ramp((M,), np.float64, 1.0, 3.0),
        volume=_ramp((N, HH, WW), step=0.125), start=_ramp((N, HH, WW), step=0.375),
        targets0=np.zeros((0, TH, TW), np.float32), maps0=np.zeros((0, 9), np.float32), weights0=np.zeros((0, TH, TW), np.float32),
        intensity0=np.zeros((0, 2), np.float32), scales0=np.zeros(0, np.float64), start0=np.zeros((0, 4, 4), np.float32),
        volume0=np.zeros((0, HH, WW), np.float32))


def _t(a):
    import torch

    return torch.from_numpy(a)


GRID = (N, HH, WW)


def cases():
    """(id, call(m, x)): every public method of the family, its options off and on"""
    c = []

    def add(name, fn):
        c.append((name, fn))

    # ---- resample, resample_volume, resample_each
    add("resample", lambda m, x: m.resample(x["images"], x["points2"]))
    add("resample-native", lambda m, x: m.resample(x["images"], x["points2"], exact=False))
    add("resample-single", lambda m, x: m.resample(x["images"][0], x["points2"]))
    add("resample-torch", lambda m, x: m.resample(_t(x["images"]), _t(x["points2"])))
    add("resample-float64-in", lambda m, x: m.resample(x["images"].astype(np.float64), x["points2"].tolist()))
    add("resample_with_gradient", lambda m, x: m.resample_with_gradient(x["images"], x["points2"]))
    add("resample_with_gradient-single", lambda m, x: m.resample_with_gradient(x["images"][1], x["points2"]))
    add("resample_with_gradient-torch", lambda m, x: m.resample_with_gradient(_t(x["images"]), x["points2"]))
    add("resample_volume", lambda m, x: m.resample_volume(x["images"], x["points3"]))
    add("resample_volume-native", lambda m, x: m.resample_volume(x["images"], x["points3"], exact=False))
    add("resample_volume-torch", lambda m, x: m.resample_volume(_t(x["images"]), _t(x["points3"])))
    add("resample_volume_with_gradient", lambda m, x: m.resample_volume_with_gradient(x["images"], x["points3"]))
    add("resample_volume_with_gradient-torch", lambda m, x: m.resample_volume_with_gradient(_t(x["images"]), x["points3"]))
    add("resample_each", lambda m, x: m.resample_each(x["images"], x["points_each"]))
    add("resample_each-native", lambda m, x: m.resample_each(x["images"], x["points_each"], exact=False))
    add("resample_each-torch", lambda m, x: m.resample_each(_t(x["images"]), _t(x["points_each"])))
    add("refuse-resample-images-4d", lambda m, x: m.resample(x["images"][None], x["points2"]))
    add("refuse-resample-images-1d", lambda m, x: m.resample(x["images"][0, 0], x["points2"]))
    add("refuse-resample-points-width", lambda m, x: m.resample(x["images"], x["points3"]))
    add("refuse-resample-points-rank", lambda m, x: m.resample(x["images"], x["points_each"]))
    add("refuse-resample_with_gradient-points", lambda m, x: m.resample_with_gradient(x["images"], x["points3"]))
    add("refuse-resample_volume-images-2d", lambda m, x: m.resample_volume(x["images"][0], x["points3"]))
    add("refuse-resample_volume-points-width", lambda m, x: m.resample_volume(x["images"], x["points2"]))
    add("refuse-resample_volume_with_gradient-images", lambda m, x: m.resample_volume_with_gradient(x["images"][None], x["points3"]))
    add("refuse-resample_each-points-rank", lambda m, x: m.resample_each(x["images"], x["points2"]))
    add("refuse-resample_each-points-count", lambda m, x: m.resample_each(x["images"], x["points_each"][:2]))
    add("refuse-resample_each-points-width", lambda m, x: m.resample_each(x["images"], np.zeros((N, NP, 3), np.float32)))

    # ---- align_cost, align_solve, align_solve_rigid and their weighted forms: n slices, n targets
    add("align_cost", lambda m, x: m.align_cost(x["images"], x["targets2"], x["maps2"]))
    add("align_cost-warped", lambda m, x: m.align_cost(x["images"], x["targets2"], x["maps2"], warped=True))
    add("align_cost-gradient", lambda m, x: m.align_cost(x["images"], x["targets2"], x["maps2"], gradient=True))
    add("align_cost-warped-gradient-torch", lambda m, x: m.align_cost(_t(x["images"]), _t(x["targets2"]), _t(x["maps2"]), warped=True, gradient=True))
    add("refuse-align_cost-images", lambda m, x: m.align_cost(x["images"][0], x["targets2"], x["maps2"]))
    add("refuse-align_cost-targets-rank", lambda m, x: m.align_cost(x["images"], x["targets2"][0], x["maps2"]))
    add("refuse-align_cost-targets-count", lambda m, x: m.align_cost(x["images"], x["targets"], x["maps2"]))
    add("refuse-align_cost-maps-width", lambda m, x: m.align_cost(x["images"], x["targets2"], x["maps"][:N]))
    add("refuse-align_cost-maps-rows", lambda m, x: m.align_cost(x["images"], x["targets2"], x["maps2"][:2]))
    add("align_solve", lambda m, x: m.align_solve(x["images"], x["targets2"], x["maps2"]))
    add("align_solve-options-trace", lambda m, x: m.align_solve(x["images"], x["targets2"], x["maps2"], iterations=5, damping=0.5, down=0.25, up=4.0, lam_min=1e-3,
                                                              lam_max=1e3, trace=True))
    add("align_solve-no-iterations-trace", lambda m, x: m.align_solve(x["images"], x["targets2"], x["maps2"], iterations=0, trace=True))
    add("align_solve-negative-iterations-trace", lambda m, x: m.align_solve(x["images"], x["targets2"], x["maps2"], iterations=-2, trace=True))
    add("align_solve-torch", lambda m, x: m.align_solve(_t(x["images"]), _t(x["targets2"]), _t(x["maps2"])))
    add("refuse-align_solve-images", lambda m, x: m.align_solve(x["images"][None], x["targets2"], x["maps2"]))
    add("refuse-align_solve-targets", lambda m, x: m.align_solve(x["images"], x["targets"], x["maps2"]))
    add("refuse-align_solve-maps", lambda m, x: m.align_solve(x["images"], x["targets2"], x["maps"][:N]))
    add("align_solve_rigid", lambda m, x: m.align_solve_rigid(x["images"], x["targets2"], x["angle"], x["shift2"], (3.0, 2.0)))
    add("align_solve_rigid-one-shift-trace", lambda m, x: m.align_solve_rigid(x["images"], x["targets2"], x["angle"], (0.5, -1.5), (3.0, 2.0), iterations=4, trace=True))
    add("refuse-align_solve_rigid-angle-count", lambda m, x: m.align_solve_rigid(x["images"], x["targets2"], x["angle"][:2], x["shift2"][:2], (3.0, 2.0)))
    add("refuse-align_solve_rigid-one-angle", lambda m, x: m.align_solve_rigid(x["images"], x["targets2"], 0.25, (0.0, 0.0), (3.0, 2.0)))
    add("refuse-align_solve_rigid-targets", lambda m, x: m.align_solve_rigid(x["images"], x["targets2"][0], x["angle"], x["shift2"], (3.0, 2.0)))
    add("align_cost_w", lambda m, x: m.align_cost_w(x["images"], x["targets2"], x["maps2"]))
    add("align_cost_w-weights", lambda m, x: m.align_cost_w(x["images"], x["targets2"], x["maps2"], weights=x["weights2"]))
    add("align_cost_w-intensity-warped", lambda m, x: m.align_cost_w(x["images"], x["targets2"], x["maps2"], intensity=x["intensity2"], warped=True))
    add("align_cost_w-all", lambda m, x: m.align_cost_w(x["images"], x["targets2"], x["maps2"], weights=x["weights2"], intensity=x["intensity2"], warped=True,
                                                         gradient=True))
    add("refuse-align_cost_w-images", lambda m, x: m.align_cost_w(x["images"][0], x["targets2"], x["maps2"]))
    add("refuse-align_cost_w-targets", lambda m, x: m.align_cost_w(x["images"], x["targets"], x["maps2"]))
    add("refuse-align_cost_w-weights", lambda m, x: m.align_cost_w(x["images"], x["targets2"], x["maps2"], weights=x["weights"]))
    add("refuse-align_cost_w-intensity", lambda m, x: m.align_cost_w(x["images"], x["targets2"], x["maps2"], intensity=x["intensity"]))
    add("refuse-align_cost_w-maps", lambda m, x: m.align_cost_w(x["images"], x["targets2"], x["maps"][:N]))
    add("align_solve_w", lambda m, x: m.align_solve_w(x["images"], x["targets2"], x["maps2"]))
    add("align_solve_w-weights-intensity-trace", lambda m, x: m.align_solve_w(x["images"], x["targets2"], x["maps2"], weights=x["weights2"], intensity=x["intensity2"],
                                                                            iterations=3, trace=True))
    add("align_solve_w-fixed-intensity", lambda m, x: m.align_solve_w(x["images"], x["targets2"], x["maps2"], intensity=x["intensity2"], estimate_intensity=False,
                                                                    damping=0.5, down=0.25, up=4.0, lam_min=1e-3, lam_max=1e3))
    add("refuse-align_solve_w-weights", lambda m, x: m.align_solve_w(x["images"], x["targets2"], x["maps2"], weights=x["weights2"][:, :2]))
    add("refuse-align_solve_w-intensity", lambda m, x: m.align_solve_w(x["images"], x["targets2"], x["maps2"], intensity=x["intensity2"][:, :1]))
    add("refuse-align_solve_w-maps", lambda m, x: m.align_solve_w(x["images"], x["targets2"], x["maps2"][:2]))
    add("align_solve_rigid_w", lambda m, x: m.align_solve_rigid_w(x["images"], x["targets2"], x["angle"], x["shift2"], (3.0, 2.0)))
    add("align_solve_rigid_w-all", lambda m, x: m.align_solve_rigid_w(x["images"], x["targets2"], x["angle"], x["shift2"], (3.0, 2.0), weights=x["weights2"],
                                                                    intensity=x["intensity2"], estimate_intensity=False, iterations=2, trace=True))
    add("refuse-align_solve_rigid_w-angle-count", lambda m, x: m.align_solve_rigid_w(x["images"], x["targets2"], x["angle"][:2], (0.0, 0.0), (3.0, 2.0)))
    add("refuse-align_solve_rigid_w-weights", lambda m, x: m.align_solve_rigid_w(x["images"], x["targets2"], x["angle"], x["shift2"], (3.0, 2.0), weights=x["weights"]))

    # ---- the volume alignment: n slices, m targets
    add("align_volume_cost", lambda m, x: m.align_volume_cost(x["images"], x["targets"], x["maps"]))
    add("align_volume_cost-warped", lambda m, x: m.align_volume_cost(x["images"], x["targets"], x["maps"], warped=True))
    add("align_volume_cost-gradient-torch", lambda m, x: m.align_volume_cost(_t(x["images"]), _t(x["targets"]), _t(x["maps"]), gradient=True))
    add("refuse-align_volume_cost-images", lambda m, x: m.align_volume_cost(x["images"][0], x["targets"], x["maps"]))
    add("refuse-align_volume_cost-targets", lambda m, x: m.align_volume_cost(x["images"], x["targets"][0], x["maps"]))
    add("refuse-align_volume_cost-maps-width", lambda m, x: m.align_volume_cost(x["images"], x["targets"], x["maps"][:, :6]))
    add("refuse-align_volume_cost-maps-rows", lambda m, x: m.align_volume_cost(x["images"], x["targets"], x["maps"][:N]))
    add("align_volume_solve", lambda m, x: m.align_volume_solve(x["images"], x["targets"], x["maps"]))
    add("align_volume_solve-options-trace", lambda m, x: m.align_volume_solve(x["images"], x["targets"], x["maps"], iterations=5, damping=0.5, down=0.25, up=4.0,
                                                                            lam_min=1e-3, lam_max=1e3, trace=True))
    add("align_volume_solve-negative-iterations-trace", lambda m, x: m.align_volume_solve(x["images"], x["targets"], x["maps"], iterations=-1, trace=True))
    add("refuse-align_volume_solve-images", lambda m, x: m.align_volume_solve(x["images"][0], x["targets"], x["maps"]))
    add("refuse-align_volume_solve-targets", lambda m, x: m.align_volume_solve(x["images"], x["targets"][None], x["maps"]))
    add("refuse-align_volume_solve-maps", lambda m, x: m.align_volume_solve(x["images"], x["targets"], x["maps2"]))
    add("align_volume_solve_rigid", lambda m, x: m.align_volume_solve_rigid(x["images"], x["targets"], x["planes"], 2.5))
    add("align_volume_solve_rigid-state-trace", lambda m, x: m.align_volume_solve_rigid(x["images"], x["targets"], x["planes"], 2.5, rotation=x["rotation"],
                                                                                      shift=x["shift3"], iterations=3, trace=True))
    add("align_volume_solve_rigid-one-state", lambda m, x: m.align_volume_solve_rigid(x["images"], x["targets"], x["planes"].reshape(M, 4, 3), 2.5,
                                                                                    rotation=x["rotation"][0], shift=(0.5, 1.5, -2.0)))
    add("refuse-align_volume_solve_rigid-planes", lambda m, x: m.align_volume_solve_rigid(x["images"], x["targets"], x["planes"][:N], 2.5))
    add("refuse-align_volume_solve_rigid-rotation", lambda m, x: m.align_volume_solve_rigid(x["images"], x["targets"], x["planes"], 2.5, rotation=x["rotation"][:N]))
    add("refuse-align_volume_solve_rigid-shift", lambda m, x: m.align_volume_solve_rigid(x["images"], x["targets"], x["planes"], 2.5, shift=x["shift3"][:N]))
    add("refuse-align_volume_solve_rigid-images", lambda m, x: m.align_volume_solve_rigid(x["images"][0], x["targets"], x["planes"], 2.5))
    add("align_volume_cost_w", lambda m, x: m.align_volume_cost_w(x["images"], x["targets"], x["maps"]))
    add("align_volume_cost_w-weights-gradient", lambda m, x: m.align_volume_cost_w(x["images"], x["targets"], x["maps"], weights=x["weights"], gradient=True))
    add("align_volume_cost_w-all", lambda m, x: m.align_volume_cost_w(x["images"], x["targets"], x["maps"], weights=x["weights"], intensity=x["intensity"], warped=True,
                                                                    gradient=True))
    add("refuse-align_volume_cost_w-images", lambda m, x: m.align_volume_cost_w(x["images"][0], x["targets"], x["maps"]))
    add("refuse-align_volume_cost_w-targets", lambda m, x: m.align_volume_cost_w(x["images"], x["targets"][0], x["maps"]))
    add("refuse-align_volume_cost_w-weights", lambda m, x: m.align_volume_cost_w(x["images"], x["targets"], x["maps"], weights=x["weights2"]))
    add("refuse-align_volume_cost_w-intensity", lambda m, x: m.align_volume_cost_w(x["images"], x["targets"], x["maps"], intensity=x["intensity2"]))
    add("refuse-align_volume_cost_w-maps", lambda m, x: m.align_volume_cost_w(x["images"], x["targets"], x["maps2"]))
    add("align_volume_solve_w", lambda m, x: m.align_volume_solve_w(x["images"], x["targets"], x["maps"]))
    add("align_volume_solve_w-all-trace", lambda m, x: m.align_volume_solve_w(x["images"], x["targets"], x["maps"], weights=x["weights"], intensity=x["intensity"],
                                                                            estimate_intensity=False, iterations=3, damping=0.5, down=0.25, up=4.0, lam_min=1e-3,
                                                                            lam_max=1e3, trace=True))
    add("refuse-align_volume_solve_w-weights", lambda m, x: m.align_volume_solve_w(x["images"], x["targets"], x["maps"], weights=x["weights2"]))
    add("refuse-align_volume_solve_w-intensity", lambda m, x: m.align_volume_solve_w(x["images"], x["targets"], x["maps"], intensity=x["intensity2"]))
    add("refuse-align_volume_solve_w-maps", lambda m, x: m.align_volume_solve_w(x["images"], x["targets"], x["maps"][:, :6]))
    add("align_volume_solve_rigid_w", lambda m, x: m.align_volume_solve_rigid_w(x["images"], x["targets"], x["planes"], 2.5))
    add("align_volume_solve_rigid_w-all-trace", lambda m, x: m.align_volume_solve_rigid_w(x["images"], x["targets"], x["planes"], 2.5, rotation=x["rotation"],
                                                                                        shift=x["shift3"], weights=x["weights"], intensity=x["intensity"],
                                                                                        estimate_intensity=False, iterations=2, trace=True))
    add("refuse-align_volume_solve_rigid_w-planes", lambda m, x: m.align_volume_solve_rigid_w(x["images"], x["targets"], x["planes"][:N], 2.5))
    add("refuse-align_volume_solve_rigid_w-rotation", lambda m, x: m.align_volume_solve_rigid_w(x["images"], x["targets"], x["planes"], 2.5, rotation=x["rotation"][:N]))
    add("refuse-align_volume_solve_rigid_w-weights", lambda m, x: m.align_volume_solve_rigid_w(x["images"], x["targets"], x["planes"], 2.5, weights=x["weights2"]))

    # ---- groups of targets, the robust loss
    add("align_volume_solve_group-offsets", lambda m, x: m.align_volume_solve_group(x["images"], x["targets"], x["planes"], 2.5, [0, 1, M]))
    add("align_volume_solve_group-sizes", lambda m, x: m.align_volume_solve_group(x["images"], x["targets"], x["planes"], 2.5, [3, 1]))
    add("align_volume_solve_group-all-trace", lambda m, x: m.align_volume_solve_group(x["images"], x["targets"], x["planes"], 2.5, [0, 1, M], rotation=x["rotation_g"],
                                                                                    shift=x["shift_g"], weights=x["weights"], intensity=x["intensity"],
                                                                                    estimate_intensity=False, iterations=3, damping=0.5, down=0.25, up=4.0,
                                                                                    lam_min=1e-3, lam_max=1e3, trace=True))
    add("refuse-align_volume_solve_group-planes", lambda m, x: m.align_volume_solve_group(x["images"], x["targets"], x["planes"][:N], 2.5, [0, 1, M]))
    add("refuse-align_volume_solve_group-groups", lambda m, x: m.align_volume_solve_group(x["images"], x["targets"], x["planes"], 2.5, [0, 1, M + 1]))
    add("refuse-align_volume_solve_group-rotation", lambda m, x: m.align_volume_solve_group(x["images"], x["targets"], x["planes"], 2.5, [0, 1, M], rotation=x["rotation"]))
    add("refuse-align_volume_solve_group-weights", lambda m, x: m.align_volume_solve_group(x["images"], x["targets"], x["planes"], 2.5, [0, 1, M], weights=x["weights2"]))
    add("refuse-align_volume_solve_group-intensity", lambda m, x: m.align_volume_solve_group(x["images"], x["targets"], x["planes"], 2.5, [0, 1, M],
                                                                                           intensity=x["intensity2"]))
    add("refuse-align_volume_solve_group-images", lambda m, x: m.align_volume_solve_group(x["images"][0], x["targets"], x["planes"], 2.5, [0, 1, M]))
    add("refuse-align_volume_solve_group-targets", lambda m, x: m.align_volume_solve_group(x["images"], x["targets"][0], x["planes"], 2.5, [0, 1, M]))
    add("align_volume_cost_r-one-scale", lambda m, x: m.align_volume_cost_r(x["images"], x["targets"], x["maps"], 4.0))
    add("align_volume_cost_r-scales-rweight", lambda m, x: m.align_volume_cost_r(x["images"], x["targets"], x["maps"], x["scales"], rweight=True))
    add("align_volume_cost_r-all", lambda m, x: m.align_volume_cost_r(x["images"], x["targets"], x["maps"], x["scales"], weights=x["weights"], intensity=x["intensity"],
                                                                    warped=True, gradient=True, rweight=True))
    add("refuse-align_volume_cost_r-scale", lambda m, x: m.align_volume_cost_r(x["images"], x["targets"], x["maps"], x["scales"][:N]))
    add("refuse-align_volume_cost_r-maps", lambda m, x: m.align_volume_cost_r(x["images"], x["targets"], x["maps2"], 4.0))
    add("refuse-align_volume_cost_r-weights", lambda m, x: m.align_volume_cost_r(x["images"], x["targets"], x["maps"], 4.0, weights=x["weights2"]))
    add("refuse-align_volume_cost_r-images", lambda m, x: m.align_volume_cost_r(x["images"][0], x["targets"], x["maps"], 4.0))
    add("align_volume_solve_group_robust-offsets", lambda m, x: m.align_volume_solve_group_robust(x["images"], x["targets"], x["planes"], 2.5, [0, 1, M], 4.0))
    add("align_volume_solve_group_robust-sizes-scales", lambda m, x: m.align_volume_solve_group_robust(x["images"], x["targets"], x["planes"], 2.5, [3, 1], x["scales"]))
    add("align_volume_solve_group_robust-all-trace",
        lambda m, x: m.align_volume_solve_group_robust(x["images"], x["targets"], x["planes"], 2.5, [0, 1, M], x["scales"], rotation=x["rotation_g"], shift=x["shift_g"],
                                                       weights=x["weights"], intensity=x["intensity"], estimate_intensity=False, iterations=3, damping=0.5, down=0.25,
                                                       up=4.0, lam_min=1e-3, lam_max=1e3, trace=True))
    add("refuse-align_volume_solve_group_robust-planes", lambda m, x: m.align_volume_solve_group_robust(x["images"], x["targets"], x["planes"][:N], 2.5, [0, 1, M], 4.0))
    add("refuse-align_volume_solve_group_robust-scale", lambda m, x: m.align_volume_solve_group_robust(x["images"], x["targets"], x["planes"], 2.5, [0, 1, M],
                                                                                                     x["scales"][:N]))
    add("refuse-align_volume_solve_group_robust-groups", lambda m, x: m.align_volume_solve_group_robust(x["images"], x["targets"], x["planes"], 2.5, [2, 1], 4.0))
    add("refuse-align_volume_solve_group_robust-shift", lambda m, x: m.align_volume_solve_group_robust(x["images"], x["targets"], x["planes"], 2.5, [0, 1, M], 4.0,
                                                                                                     shift=x["shift3"]))
    add("refuse-align_volume_solve_group_robust-intensity", lambda m, x: m.align_volume_solve_group_robust(x["images"], x["targets"], x["planes"], 2.5, [0, 1, M], 4.0,
                                                                                                         intensity=x["intensity2"]))

    # ---- fuse_targets, project_volume, solve_volume, solve_volume_robust: no images, no weights of the model
    add("fuse_targets", lambda m, x: m.fuse_targets(x["targets"], x["maps"], GRID, 2.5))
    add("fuse_targets-all", lambda m, x: m.fuse_targets(x["targets"], x["maps"], GRID, 2.5, thickness=1.5, weights=x["weights"], intensity=x["intensity"],
                                                      min_coverage=0.125, coverage=True))
    add("fuse_targets-torch", lambda m, x: m.fuse_targets(_t(x["targets"]), _t(x["maps"]), list(GRID), 2.5, weights=_t(x["weights"])))
    add("fuse_targets-no-targets", lambda m, x: m.fuse_targets(x["targets0"], x["maps0"], GRID, 2.5, weights=x["weights0"], intensity=x["intensity0"], coverage=True))
    add("fuse_targets-empty-grid", lambda m, x: m.fuse_targets(x["targets"], x["maps"], (0, 4, 4), 2.5, coverage=True))
    add("fuse_targets-negative-grid", lambda m, x: m.fuse_targets(x["targets"], x["maps"], (N, -1, WW), 2.5))
    add("refuse-fuse_targets-targets", lambda m, x: m.fuse_targets(x["targets"][0], x["maps"], GRID, 2.5))
    add("refuse-fuse_targets-maps-width", lambda m, x: m.fuse_targets(x["targets"], x["maps"][:, :6], GRID, 2.5))
    add("refuse-fuse_targets-maps-rows", lambda m, x: m.fuse_targets(x["targets"], x["maps"][:N], GRID, 2.5))
    add("refuse-fuse_targets-weights", lambda m, x: m.fuse_targets(x["targets"], x["maps"], GRID, 2.5, weights=x["weights2"]))
    add("refuse-fuse_targets-intensity", lambda m, x: m.fuse_targets(x["targets"], x["maps"], GRID, 2.5, intensity=x["intensity2"]))
    add("refuse-fuse_targets-shape", lambda m, x: m.fuse_targets(x["targets"], x["maps"], (HH, WW), 2.5))
    add("project_volume", lambda m, x: m.project_volume(x["volume"], x["maps"], (TH, TW), 2.5))
    add("project_volume-options", lambda m, x: m.project_volume(x["volume"], x["maps"], (TH, TW), 2.5, thickness=1.5, intensity=x["intensity"], min_coverage=0.125,
                                                              coverage=True))
    add("project_volume-targets", lambda m, x: m.project_volume(x["volume"], x["maps"], (TH, TW), 2.5, targets=x["targets"], residual=True))
    add("project_volume-all", lambda m, x: m.project_volume(x["volume"], x["maps"], (TH, TW), 2.5, thickness=1.5, intensity=x["intensity"], targets=x["targets"],
                                                          weights=x["weights"], coverage=True, residual=True, stats=True))
    add("project_volume-targets-only", lambda m, x: m.project_volume(x["volume"], x["maps"], (TH, TW), 2.5, targets=x["targets"], weights=x["weights"]))
    add("project_volume-torch", lambda m, x: m.project_volume(_t(x["volume"]), _t(x["maps"]), [TH, TW], 2.5, targets=_t(x["targets"]), stats=True))
    add("project_volume-no-targets", lambda m, x: m.project_volume(x["volume"], x["maps0"], (TH, TW), 2.5, intensity=x["intensity0"], targets=x["targets0"],
                                                                 weights=x["weights0"], coverage=True, residual=True, stats=True))
    add("project_volume-empty-lattice", lambda m, x: m.project_volume(x["volume"], x["maps"], (0, TW), 2.5, coverage=True))
    add("project_volume-empty-volume", lambda m, x: m.project_volume(x["volume0"], x["maps"], (TH, TW), 2.5))
    add("refuse-project_volume-volume", lambda m, x: m.project_volume(x["volume"][0], x["maps"], (TH, TW), 2.5))
    add("refuse-project_volume-maps-width", lambda m, x: m.project_volume(x["volume"], x["maps2"], (TH, TW), 2.5))
    add("refuse-project_volume-maps-rank", lambda m, x: m.project_volume(x["volume"], x["maps"][0], (TH, TW), 2.5))
    add("refuse-project_volume-shape", lambda m, x: m.project_volume(x["volume"], x["maps"], (M, TH, TW), 2.5))
    add("refuse-project_volume-weights-alone", lambda m, x: m.project_volume(x["volume"], x["maps"], (TH, TW), 2.5, weights=x["weights"]))
    add("refuse-project_volume-residual-alone", lambda m, x: m.project_volume(x["volume"], x["maps"], (TH, TW), 2.5, residual=True))
    add("refuse-project_volume-stats-alone", lambda m, x: m.project_volume(x["volume"], x["maps"], (TH, TW), 2.5, stats=True))
    add("refuse-project_volume-targets", lambda m, x: m.project_volume(x["volume"], x["maps"], (TH, TW), 2.5, targets=x["targets2"]))
    add("refuse-project_volume-weights", lambda m, x: m.project_volume(x["volume"], x["maps"], (TH, TW), 2.5, targets=x["targets"], weights=x["weights2"]))
    add("refuse-project_volume-intensity", lambda m, x: m.project_volume(x["volume"], x["maps"], (TH, TW), 2.5, intensity=x["intensity2"]))
    add("solve_volume", lambda m, x: m.solve_volume(x["targets"], x["maps"], GRID, 2.5, iterations=5))
    add("solve_volume-all", lambda m, x: m.solve_volume(x["targets"], x["maps"], GRID, 2.5, iterations=5, lam=0.75, thickness=1.5, weights=x["weights"],
                                                      intensity=x["intensity"], min_coverage=0.125, start=x["start"], coverage=True, history=True))
    add("solve_volume-negative-iterations-history", lambda m, x: m.solve_volume(x["targets"], x["maps"], GRID, 2.5, iterations=-3, history=True))
    add("solve_volume-no-targets", lambda m, x: m.solve_volume(x["targets0"], x["maps0"], GRID, 2.5, iterations=2, weights=x["weights0"], intensity=x["intensity0"],
                                                             start=x["start"], history=True))
    add("solve_volume-empty-grid", lambda m, x: m.solve_volume(x["targets"], x["maps"], (0, 4, 4), 2.5, iterations=2, start=x["start0"], coverage=True))
    add("refuse-solve_volume-start", lambda m, x: m.solve_volume(x["targets"], x["maps"], GRID, 2.5, iterations=2, start=x["start"][:2]))
    add("refuse-solve_volume-shape", lambda m, x: m.solve_volume(x["targets"], x["maps"], (HH, WW), 2.5, iterations=2))
    add("refuse-solve_volume-targets", lambda m, x: m.solve_volume(x["targets"][0], x["maps"], GRID, 2.5, iterations=2))
    add("refuse-solve_volume-maps", lambda m, x: m.solve_volume(x["targets"], x["maps2"], GRID, 2.5, iterations=2))
    add("refuse-solve_volume-weights", lambda m, x: m.solve_volume(x["targets"], x["maps"], GRID, 2.5, iterations=2, weights=x["weights2"]))
    add("refuse-solve_volume-intensity", lambda m, x: m.solve_volume(x["targets"], x["maps"], GRID, 2.5, iterations=2, intensity=x["intensity2"]))
    add("solve_volume_robust-one-scale", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], GRID, 2.5, 4.0, rounds=2, iterations=5))
    add("solve_volume_robust-all", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], GRID, 2.5, x["scales"], rounds=3, iterations=5, anneal=1.5, lam=0.75,
                                                                    thickness=1.5, weights=x["weights"], intensity=x["intensity"], min_coverage=0.125, start=x["start"],
                                                                    coverage=True, history=True, rweight=True, stats=True))
    add("solve_volume_robust-no-rounds", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], GRID, 2.5, 4.0, rounds=0, iterations=2, history=True))
    add("solve_volume_robust-negative-rounds", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], GRID, 2.5, 4.0, rounds=-1, iterations=2, history=True))
    add("solve_volume_robust-64-rounds", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], GRID, 2.5, 4.0, rounds=64, iterations=1, history=True))
    add("solve_volume_robust-65-rounds", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], GRID, 2.5, 4.0, rounds=65, iterations=1, history=True))
    add("solve_volume_robust-negative-iterations", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], GRID, 2.5, 4.0, rounds=2, iterations=-2, history=True))
    add("solve_volume_robust-no-targets", lambda m, x: m.solve_volume_robust(x["targets0"], x["maps0"], GRID, 2.5, x["scales0"], rounds=2, iterations=2,
                                                                           weights=x["weights0"], intensity=x["intensity0"], history=True, rweight=True, stats=True))
    add("solve_volume_robust-empty-grid", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], (N, HH, 0), 2.5, 4.0, rounds=2, iterations=2, coverage=True))
    add("refuse-solve_volume_robust-start", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], GRID, 2.5, 4.0, rounds=2, iterations=2, start=x["start"][:2]))
    add("refuse-solve_volume_robust-shape", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], (N, HH, WW, 1), 2.5, 4.0, rounds=2, iterations=2))
    add("refuse-solve_volume_robust-scale", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], GRID, 2.5, x["scales"][:N], rounds=2, iterations=2))
    add("refuse-solve_volume_robust-targets", lambda m, x: m.solve_volume_robust(x["targets"][0], x["maps"], GRID, 2.5, 4.0, rounds=2, iterations=2))
    add("refuse-solve_volume_robust-maps", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"][:N], GRID, 2.5, 4.0, rounds=2, iterations=2))
    add("refuse-solve_volume_robust-weights", lambda m, x: m.solve_volume_robust(x["targets"], x["maps"], GRID, 2.5, 4.0, rounds=2, iterations=2, weights=x["weights2"]))
    return c


# ------------------------------------------------------------------------------------------------------------------------ the recorder
def _number(v):
    """a float as JSON holds it: the number itself, or the name of a value JSON has no literal for"""
    v = float(v)
    return v if math.isfinite(v) else repr(v)


def _array(a, values=True):
    out = {"type": "ndarray", "dtype": str(a.dtype), "shape": list(a.shape)}
    if not values:
        return out
    flat = a.reshape(-1)
    vals = [_number(v) if a.dtype.kind == "f" else int(v) for v in flat.tolist()]
    if vals and all(v == vals[0] for v in vals):
        out["fill"] = vals[0]  # (one value throughout: the pre-fill)
    else:
        out["values"] = vals
    return out


def _is_torch(v):
    return type(v).__module__.split(".")[0] == "torch"


def _value(v, values=True):
    """a result, or a field of one, as JSON; ``values`` False: an array's type, shape and dtype only"""
    if v is None or isinstance(v, (bool, str)):
        return v
    if _is_torch(v):
        return dict(_array(v.numpy(), values), type="torch.Tensor")
    if isinstance(v, np.ndarray):
        return _array(v, values)
    if isinstance(v, tuple) and hasattr(v, "_fields"):
        return {"type": type(v).__name__, "fields": {k: _value(x, values) for k, x in zip(v._fields, v)}}
    if isinstance(v, (tuple, list)):
        return {"type": type(v).__name__, "items": [_value(x, values) for x in v]}
    if isinstance(v, (int, np.integer)):
        return {"type": type(v).__name__, "value": int(v)}
    if isinstance(v, (float, np.floating)):
        return {"type": type(v).__name__, "value": _number(v)}
    raise TypeError(f"unexpected {type(v)} in a result")


def _addresses(v, path, out):
    """address -> "out:<field>" for every array of a result"""
    if _is_torch(v):
        out.setdefault(v.data_ptr(), "out:" + path)
    elif isinstance(v, np.ndarray):
        out.setdefault(v.ctypes.data, "out:" + path)
    elif isinstance(v, tuple):
        names = v._fields if hasattr(v, "_fields") else range(len(v))
        for k, x in zip(names, v):
            _addresses(x, f"{path}.{k}" if path else str(k), out)


def _arguments(name, args):
    """the arguments of one recorded call, pointers still as addresses; built host arrays read while they are alive"""
    from mri_inr_amd import _lib

    _, argtypes = _lib.PROTOTYPES[name]
    assert len(args) == len(argtypes), f"{name} takes {len(argtypes)} arguments, was given {len(args)}"
    out = []
    for i, (a, ty) in enumerate(zip(args, argtypes)):
        if i == 0:
            assert isinstance(a, C.c_void_p) and a.value == 1, f"{name}: the first argument is the handle"
            out.append("handle")
        elif ty is C.c_void_p:
            assert a is None or (isinstance(a, int) and not isinstance(a, bool)), f"{name} argument {i}: expected an address or None, got {a!r}"
            built = BUILT.get(name, {}).get(i)
            read = None
            if a is not None and built is not None:
                dtype, count = built[0], int(built[1](args))
                read = _array(np.ctypeslib.as_array((np.ctypeslib.as_ctypes_type(dtype) * count).from_address(a)).copy()) if count else None
            out.append({"address": a, "read": read})
        elif isinstance(getattr(ty, "_type_", None), type) and issubclass(ty._type_, C.Structure):
            o = a._obj
            assert type(o) is ty._type_, f"{name} argument {i}: expected {ty._type_.__name__}, got {type(o).__name__}"
            out.append({"opts": type(o).__name__, "bytes": bytes(o).hex()})
        else:
            assert isinstance(a, (int, np.integer)) and not isinstance(a, bool), f"{name} argument {i}: expected an integer, got {a!r}"
            out.append(int(a))
    return out


def prefilled(name):
    """whether the outputs of a case are filled before the call: all but those of ``resample`` and ``resample_with_gradient``, which the library
    writes in full (NaN where no tile covers a point)"""
    return not name.startswith(("resample-", "resample_with_gradient")) and name != "resample"


def record(name, fn):
    """one case -> its record"""
    from mri_inr_amd import ModulatedSiren

    x = inputs()
    named = {(v.ctypes.data): "in:" + k for k, v in x.items() if v.size}
    m, lib = ModulatedSiren(**KW), Recorder()
    m._lib, m._h, m._committed = lib, C.c_void_p(1), False
    try:
        result = fn(m, x)
    except ValueError:
        lib = m._lib = Recorder()
        m._committed = True  # (a refusal: once more with the weights in place -- nothing at all may reach the library)
        with pytest.raises(ValueError):
            fn(m, x)
        return {"raises": "ValueError", "calls": list(lib.names)}  # (a copy: the model's end is not part of the case)
    outs = {}
    _addresses(result if isinstance(result, tuple) else (result,), "", outs)
    calls = []
    for function, args in lib.calls:
        labelled = []
        for a in args:
            if isinstance(a, dict) and "address" in a:
                p = a["address"]
                label = "null" if p is None else named.get(p) or outs.get(p) or "fresh"
                a = label if a["read"] is None or label != "fresh" else {"pointer": label, "holds": a["read"]}
            labelled.append(a)
        calls.append({"function": function, "arguments": labelled})
    return {"commits": "msiren_commit_weights" in lib.names, "calls": calls, "result": _value(result, prefilled(name))}


PUBLIC = ("resample", "resample_with_gradient", "resample_volume", "resample_volume_with_gradient", "resample_each", "align_cost", "align_solve",
          "align_solve_rigid", "align_cost_w", "align_solve_w", "align_solve_rigid_w", "align_volume_cost", "align_volume_solve", "align_volume_solve_rigid",
          "align_volume_cost_w", "align_volume_solve_w", "align_volume_solve_rigid_w", "align_volume_solve_group", "align_volume_cost_r",
          "align_volume_solve_group_robust", "fuse_targets", "project_volume", "solve_volume", "solve_volume_robust")


def public():
    """what a caller sees of every method of the family on ``ModulatedSiren``: the signature with its defaults, and the docstring (as its digest)"""
    from mri_inr_amd import ModulatedSiren

    return {name: {"signature": str(inspect.signature(getattr(ModulatedSiren, name))),
                   "doc_sha256": hashlib.sha256(getattr(ModulatedSiren, name).__doc__.encode()).hexdigest()} for name in PUBLIC}


def record_all():
    return dict({name: record(name, fn) for name, fn in cases()}, public=public())


def _same(got, want, where):
    """equal, floats to 1e-12 relative (the angle of a rigid state passes through the host's cos, sin and arctan2)"""
    if isinstance(want, float) and isinstance(got, float):
        assert math.isclose(got, want, rel_tol=1e-12, abs_tol=0.0), f"{where}: {got!r} != {want!r}"
    elif isinstance(want, dict) and isinstance(got, dict):
        assert sorted(got) == sorted(want), f"{where}: keys {sorted(got)} != {sorted(want)}"
        for k in want:
            _same(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, list) and isinstance(got, list):
        assert len(got) == len(want), f"{where}: {len(got)} entries != {len(want)}"
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{where}[{i}]")
    else:
        assert type(got) is type(want) and got == want, f"{where}: {got!r} != {want!r}"


def _expected():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


CASES = cases()


@pytest.fixture(scope="module")
def expected():
    return _expected()


def test_the_golden_file_and_the_cases_name_each_other():
    assert sorted(_expected()) == sorted([name for name, _ in CASES] + ["public"])
    assert len(set(name for name, _ in CASES)) == len(CASES)
    used = "\n".join(inspect.getsource(fn) for _, fn in CASES)
    assert all(f"m.{name}(" in used for name in PUBLIC)


def test_nothing_public_changed(expected):
    assert public() == expected["public"]


@pytest.mark.parametrize("name,fn", CASES, ids=[name for name, _ in CASES])
def test_binding_call(name, fn, expected):
    got = json.loads(json.dumps(record(name, fn)))
    want = expected[name]
    if name.startswith("refuse-"):
        assert want == {"raises": "ValueError", "calls": []}
    _same(got, want, name)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--write", "usage: test_binding_calls.py --write <file>"
    with open(sys.argv[2], "w") as f:
        json.dump(record_all(), f, indent=0, sort_keys=True)
        f.write("\n")
