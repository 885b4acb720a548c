"""The stack, models, lattices, maps and targets of tests/test_gpu_align.py, with their fp64 reference and the
gate.  Not a test module; no GPU needed: tests/test_align_reference.py checks on the CPU that the reference's own fp32 variant sits inside
half the cap and that the gate rejects every seeded mutant.

The stack is tests/volume_cases.py's: n = 4 slices of 40 x 40 (3 x 3 tiles each, covered over [-4, 51]), slice 1 with its upper row of tiles
black, slice 3 black.  One kind of map per slice: 0 the identity plus a fractional offset, 1 a rotation by 7 degrees about the lattice's
centre (moved onto the image's), 2 an anisotropic scale that sends part of the lattice outside every cover, 3 a small shear on the black
slice.  Every product a i is zero or a normal fp32 number (no map entry below 1e-3 in magnitude but the identity's zeros).

The gate (section 5.7's construction, on the sums): an error is measured per sum against the sum of the magnitudes of its terms; the
reference's own distance D is the largest such error of its perturbed-fp32 variant over the case's slices and sums; every sum of the
device has to lie within min(4 D, 1e-4) of the reference on that scale, and the count has to be exact.
"""
import functools

import numpy as np

import align_reference as ar
import volume_cases as vc
from mri_inr_amd import align
from mri_inr_amd import synthetic as syn
from oracle import siren_oracle as orc

FACTOR, CAP = 4.0, 1e-4
N, HW = vc.N, 40
MODELS = {"sine5": dict(L=5, act="sine"), "morlet3": dict(L=3, act="morlet")}
LATTICES = ((19, 23), (47, 45))  # one ragged chunk; chunks of 1024, 1024, 67


@functools.lru_cache(maxsize=None)
def state_dict(model):
    return vc.full_sd() if model == "sine5" else syn.make_state_dict(seed=7, num_layers=MODELS[model]["L"], trained_like=True)


def maps(shape):
    th, tw = shape
    centre = ((th - 1) / 2, (tw - 1) / 2)
    rot = align.rigid_maps(np.deg2rad(7.0), (19.3 - centre[0], 20.6 - centre[1]), centre)[0]
    return np.array([[1.0, 0.0, 0.37, 0.0, 1.0, 1.61],
                     rot,
                     [1.37, 0.013, -7.3, -0.021, 0.81, 2.2],
                     [0.9, 0.1, 3.3, -0.1, 0.9, 5.2]], np.float32)


def targets(shape):
    """smooth images in [0.1, 0.9]; a block of NaN pixels (a mask) in the first one"""
    th, tw = shape
    i, j = np.mgrid[0:th, 0:tw]
    t = np.stack([0.5 + 0.4 * np.sin(0.21 * i + 0.5 * s) * np.cos(0.17 * j - 0.3 * s) for s in range(N)]).astype(np.float32)
    t[0, 3:6, 4:9] = np.nan
    return t


@functools.lru_cache(maxsize=None)
def stack_mods(model, dtype_name):
    """volume_cases.stack_mods for the model: per slice the modulations of its tiles (rows of black tiles zero, never read) and its black tiles"""
    dtype, L, sd = np.dtype(dtype_name).type, MODELS[model]["L"], state_dict(model)
    mods, black = [], []
    for img in vc.images():
        patches, info = orc.image_to_patches(img, vc.O, vc.I)
        kept, blk, _ = orc.filter_and_remember_black_patches(patches)
        assert info == (vc.NV, vc.NH)
        m = np.zeros((L, vc.NPT, 256), dtype)
        if len(blk) < vc.NPT:
            z = orc.encoder_forward(sd, kept, dtype=dtype)
            m[:, [t for t in range(vc.NPT) if t not in blk]] = orc.modulator_forward(sd, z, num_layers=L, dtype=dtype)
        mods.append(m)
        black.append(list(blk))
    return mods, black


def reference(model, shape, dtype=np.float64, perturbed=False):
    mods, black = stack_mods(model, np.dtype(dtype).name)
    return ar.align_of_stack(state_dict(model), mods, black, maps(shape), targets(shape), vc.NV, vc.NH, vc.S, vc.I, num_layers=MODELS[model]["L"],
                             activation=MODELS[model]["act"], dtype=dtype, perturbed=perturbed)


def scaled_errors(sums, ref, mags):
    """|sums - ref| / magnitudes per sum; 0 where both are zero, inf where a sum without terms is not zero"""
    err = np.abs(np.asarray(sums, np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(mags > 0, err / mags, np.where(err == 0, 0.0, np.inf))


@functools.lru_cache(maxsize=None)
def data(model, shape):
    """one case: maps, targets, the fp64 reference (sums, magnitudes, planes), the reference's own distance D and the gate"""
    sums, mags, planes = reference(model, shape)
    s32, _, _ = reference(model, shape, np.float32, perturbed=True)
    assert np.array_equal(s32[:, 0], sums[:, 0])  # the same pixels are valid
    D = float(scaled_errors(s32, sums, mags).max())
    return dict(maps=maps(shape), targets=targets(shape), sums=sums, mags=mags, planes=planes, variant=s32, D=D, gate=min(FACTOR * D, CAP))


def accepts(d, sums):
    """the gate of case ``d`` on device sums (n, 29): the count exact, every other sum within the gate on its scale"""
    sums = np.asarray(sums, np.float64)
    return bool(np.array_equal(sums[:, 0], d["sums"][:, 0]) and (scaled_errors(sums, d["sums"], d["mags"]) <= d["gate"]).all())
