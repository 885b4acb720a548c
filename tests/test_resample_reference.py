"""tests/resample_reference.py on the CPU: the semantics of msiren_resample_slices*  against the oracle's fold."""
import math

import numpy as np

import resample_reference as rr
from mri_inr_amd import synthetic as syn
from oracle import siren_oracle as orc

O, I, S = 32, 16, 24
PAD = (S - I) // 2
NV = NH = 3


def integer_pixels():
    return np.stack(np.meshgrid(np.arange(NV * I), np.arange(NH * I), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)


def test_blend_of_given_tiles_at_integer_pixels_is_the_weighted_fold():
    """measured for the issue: 1.8e-7 absolute on values in [-1, 1] (the oracle folds in fp32)"""
    tiles = np.random.default_rng(0).uniform(-1, 1, size=(NV * NH, S, S)).astype(np.float32)
    want = orc.patches_to_image_weighted_average(tiles, (NV, NH), S, I)

    def tile_values(t, ty, tx):
        assert np.all(ty == np.round(ty)) and np.all(tx == np.round(tx))
        return tiles[t, ty.astype(int), tx.astype(int)][None]

    got = rr.blend(integer_pixels(), NV, NH, S, I, tile_values)[0].reshape(NV * I, NH * I)
    err = np.abs(got - want).max()
    print("blend vs weighted fold: max abs", err)
    assert err <= 1e-6
    # black tiles contribute zeros with their weight, as reintegrate_black_patches + fold
    black = [0, 4]
    zeroed = tiles.copy()
    zeroed[black] = 0
    got = rr.blend(integer_pixels(), NV, NH, S, I, tile_values, black)[0].reshape(NV * I, NH * I)
    assert np.abs(got - orc.patches_to_image_weighted_average(zeroed, (NV, NH), S, I)).max() <= 1e-6


def test_cover_count_never_exceeds_ceil_s_over_i_squared():
    rng = np.random.default_rng(1)
    for s, i, n in ((24, 16, 3), (24, 16, 20), (32, 16, 5), (24, 8, 6), (20, 16, 4), (16, 16, 3)):
        ka = math.ceil(s / i)
        pad = (s - i) // 2
        edges = [np.float32(v * i - pad + d) for v in range(n) for d in (0, s - 1)]
        ys = np.concatenate([rng.uniform(-pad - 2, n * i + pad + 2, 2000).astype(np.float32), np.arange(-pad - 1, n * i + pad + 1, dtype=np.float32),
                             edges, [np.nextafter(e, np.float32(np.inf)) for e in edges], [np.nextafter(e, np.float32(-np.inf)) for e in edges]])
        counts = [len(rr.covering(y, n, s, i)) for y in ys]
        assert max(counts) == ka, (s, i, max(counts))
        pts = np.stack([ys[:500], ys[500:1000]], 1)
        assert max(len(c) for c in rr.covers(pts, n, n, s, i)) <= ka * ka


def test_cover_is_closed_at_both_ends():
    for v in range(NV):
        lo, hi = np.float32(v * I - PAD), np.float32(v * I - PAD + S - 1)
        assert v in rr.covering(lo, NV, S, I) and v in rr.covering(hi, NV, S, I)
        assert v not in rr.covering(np.nextafter(lo, np.float32(-np.inf)), NV, S, I)
        assert v in rr.covering(np.nextafter(lo, np.float32(np.inf)), NV, S, I)
        assert v in rr.covering(np.nextafter(hi, np.float32(-np.inf)), NV, S, I)
        assert v not in rr.covering(np.nextafter(hi, np.float32(np.inf)), NV, S, I)
    assert rr.covering(np.float32("nan"), NV, S, I) == [] and rr.covering(np.float32("inf"), NV, S, I) == []
    out = rr.blend(np.array([[np.nan, 3.0], [-4.5, 3.0], [3.0, 52.0]], np.float32), NV, NH, S, I, lambda t, ty, tx: np.ones((1, len(ty))))
    assert np.isnan(out).all()


def test_reference_at_integer_pixels_meets_the_oracles_reconstruction():
    """Both in fp64 arithmetic on the same fp32 inputs; what differs is the local coordinate (float32(-1 + ty 2 / (S - 1)) against the
    oracle's linspace_f32, up to one ulp of a coordinate) and the fold's fp32 sums.  Measured: max 3.0e-06, rms 3.2e-07 of max|recon| --
    inside the project's 1e-4 / 1e-5 norm by a factor of 30 and more; asserted at a fifth of the norm."""
    sd = syn.make_state_dict(seed=7, trained_like=True)
    img = syn.make_slice(2, 40, 40)
    img[:, :24] = 0.0  # the left column of tiles sees nothing but black
    patches, info = orc.image_to_patches(img, O, I)
    kept, black, shape = orc.filter_and_remember_black_patches(patches)
    assert info == (NV, NH) and 0 < len(black) < NV * NH
    want = orc.reconstruct_slice(sd, img, num_layers=5, dtype=np.float64)
    z = orc.encoder_forward(sd, kept, dtype=np.float64)
    mods = np.zeros((5, NV * NH, 256))
    mods[:, [t for t in range(NV * NH) if t not in black]] = orc.modulator_forward(sd, z, num_layers=5, dtype=np.float64)
    got, _ = rr.resample(sd, mods, black, integer_pixels(), NV, NH, S, I, num_layers=5)
    got = got.reshape(NV * I, NH * I)
    scale = np.abs(want).max()
    em, er = np.abs(got - want).max() / scale, np.sqrt(np.mean((got - want) ** 2)) / scale
    print(f"reference vs oracle reconstruction: max {em:.2e} rms {er:.2e} of max|recon| {scale:.3f}")
    assert em <= 2e-5 and er <= 2e-6
