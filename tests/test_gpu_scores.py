"""PSNR / SSIM / NRMSE on the device (msiren_score_images(_dev), mri_inr_amd/csrc/scores.hip.h; harness.score_images and
metrics_error) against the host definitions they restate: mri_inr_amd/metrics.py and the explicit-window SSIM of
oracle/ssim_windows.py.  Both sides work in fp64 and differ only in summation order, so the bounds are tight: |dPSNR| <= 1e-9 dB,
relative dNRMSE <= 1e-12, |dSSIM| <= 1e-9 (the bound tests/test_host_logic.py demands between metrics.py and ssim_by_windows)."""

import numpy as np
import pytest

from conftest import load_golden
from mri_inr_amd import ModulatedSiren, _lib, harness, metrics, synthetic as syn
from oracle.ssim_windows import ssim_by_windows

pytestmark = pytest.mark.gpu

PSNR_TOL, NRMSE_RTOL, SSIM_TOL = 1e-9, 1e-12, 1e-9


@pytest.fixture(scope="module")
def model():
    m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=5, latent_dim=256, w0=1.0, w0_initial=30.0,
                       use_bias=True, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                       outer_patch_size=32, inner_patch_size=16, siren_patch_size=24, device="cuda", activation="sine")
    m.load_state_dict(syn.make_state_dict(seed=7, trained_like=True))
    m.to("cuda").eval()
    harness.bind(m)
    return m


def host_scores(o, p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([metrics.calculate_psnr(o, p), metrics.calculate_ssim(o, p), metrics.calculate_nrmse(o, p)])


def assert_close(dev, o, p):
    ref = host_scores(o, p)
    assert abs(dev[0] - ref[0]) <= PSNR_TOL, (dev, ref)
    assert abs(dev[1] - ref[1]) <= SSIM_TOL, (dev, ref)
    assert abs(dev[2] - ref[2]) <= NRMSE_RTOL * abs(ref[2]), (dev, ref)
    assert abs(dev[1] - ssim_by_windows(o, p, metrics.calculate_data_range(o, p))) <= SSIM_TOL


def noisy(img, seed, sigma=0.05):
    return (img + sigma * np.random.default_rng(seed).standard_normal(img.shape)).astype(np.float32)


def test_scores_match_host_metrics_synthetic_and_ragged(model):
    pairs = []
    for k in range(3):   # 320 x 320 brain-masked: large exact-zero regions in the original
        full = syn.make_slice(k, 320, 320, brain_mask=True)
        pairs.append((full, noisy(full, k)))
    for hh, ww in [(80, 64), (208, 144), (7, 7), (7, 40), (33, 7), (39, 71)]:
        full = syn.make_slice(hh + ww, hh, ww)
        pairs.append((full, noisy(full, hh * ww, sigma=0.3) - np.float32(0.2)))   # negative predictions
    for o, p in pairs:
        assert (p < 0).any()
        got = harness.score_images(o, p)
        assert got.shape == (1, 3) and got.dtype == np.float64
        assert_close(got[0], o, p)
        d_got = harness.score_images(model.device_array(o.shape).copy_from(o), model.device_array(p.shape).copy_from(p))
        assert np.array_equal(d_got, got)   # the host form and the _dev form: same bits


def test_scores_of_model_reconstructions(model):
    for hh, ww in [(320, 320), (200, 136), (80, 64)]:
        img = syn.make_slice(hh, hh, ww, brain_mask=True)
        tiles, info = harness.image_to_patches(img[None], 32, 16)
        rec = harness.reconstruct_from_patches(model, tiles, info)[0]
        full = harness.patches_to_image(tiles, info, 32, 16)[0]
        assert_close(harness.score_images(full, rec)[0], full, rec)


def test_offset_images_against_explicit_windows(model):
    """Values around m = 1e3 with noise sigma = 1: every SSIM variance is a difference of two terms of size m^2, so it carries an
    absolute rounding error of a few eps * m^2 on either side (eps = 2^-53; metrics.py's running sums are the less exact side here).
    S moves by that over (vx + vy + C2) ~ sigma^2: |dS| <= 8 eps m^2 / sigma^2 ~ 9e-10 against ssim_by_windows."""
    rng = np.random.default_rng(5)
    o = (1000.0 + rng.standard_normal((96, 80))).astype(np.float32)
    p = (o + 0.3 * rng.standard_normal(o.shape)).astype(np.float32)
    got = harness.score_images(o, p)[0]
    bound = 8 * 2.0 ** -53 * 1000.0 ** 2
    assert abs(got[1] - ssim_by_windows(o, p, metrics.calculate_data_range(o, p))) <= bound
    ref = host_scores(o, p)
    assert abs(got[0] - ref[0]) <= PSNR_TOL and abs(got[2] - ref[2]) <= NRMSE_RTOL * ref[2]


def test_degenerate_pairs_give_the_host_ieee_values(model):
    img = syn.make_slice(3, 48, 40, brain_mask=True)
    assert np.array_equal(harness.score_images(img, img)[0], [np.inf, 1.0, 0.0])
    zero = np.zeros_like(img)
    const = np.full((48, 40), 0.5, np.float32)
    for o, p in [(zero, img), (zero, zero), (const, const), (const, np.full_like(const, 0.75))]:
        got, ref = harness.score_images(o, p)[0], host_scores(o, p)
        np.testing.assert_equal(np.isfinite(got), np.isfinite(ref))
        np.testing.assert_equal(got[~np.isfinite(got)], ref[~np.isfinite(ref)])   # inf / nan where the host has them (sign included)
        np.testing.assert_allclose(got[np.isfinite(got)], ref[np.isfinite(ref)], rtol=1e-12, atol=SSIM_TOL)
    assert np.isinf(harness.score_images(zero, img)[0, 2])                    # NRMSE over an all-zero original
    np.testing.assert_equal(harness.score_images(const, const)[0], [np.nan, np.nan, 0.0])   # dr = 0: 0/0 in PSNR and SSIM


def mixed_batch(n, hh=64, ww=72):
    o = np.stack([syn.make_slice(k, hh, ww, brain_mask=(k % 2 == 0)) for k in range(n)])
    p = np.stack([noisy(o[k], k, sigma=0.01 * (1 + k % 7)) for k in range(n)])
    p[3] = o[3]                          # identical
    o[5] = 0.0                           # all-zero original
    o[6] = p[6] = np.float32(0.25)       # constant pair
    p[7] -= np.float32(0.5)              # negative predictions
    return o, p


def test_deterministic_and_batch_invariant(model):
    o, p = mixed_batch(64)
    d_o = model.device_array(o.shape).copy_from(o)
    d_p = model.device_array(p.shape).copy_from(p)
    batch = harness.score_images(d_o, d_p)
    alone = np.concatenate([harness.score_images(o[k], p[k]) for k in range(len(o))])
    again = harness.score_images(d_o, d_p)
    assert np.array_equal(batch.view(np.uint64), alone.view(np.uint64))
    assert np.array_equal(batch.view(np.uint64), again.view(np.uint64))
    for k in (0, 1, 7, 20):
        assert_close(batch[k], o[k], p[k])


@pytest.mark.parametrize("streams", [1, 2, 3])
def test_score_dev_is_ordered_behind_reconstruct_dev(model, streams):
    """msiren_reconstruct_tiles_dev, then msiren_score_images_dev with no sync in between: the scores see the reconstruction."""
    lib, h = model._lib, model._h
    n = 8
    imgs = np.stack([syn.make_slice(20 + k, 320, 320, brain_mask=True) for k in range(n)])
    tiles, info = harness.image_to_patches(imgs, 32, 16)
    nv, nh = info[0]
    full = harness.patches_to_image(tiles, info, 32, 16)
    d_t = model.device_array(tiles.shape).copy_from(tiles)
    d_full = model.device_array(full.shape).copy_from(full)
    d_rec = model.device_array(full.shape)
    d_s = model.device_array((n, 6))
    _lib.check(lib.msiren_set_streams(h, streams))
    try:
        results = []
        for _ in range(2 * streams):
            d_rec.copy_from(np.zeros(full.shape, np.float32))      # what an unordered score call would read
            _lib.check(lib.msiren_reconstruct_tiles_dev(h, d_t.ptr, n, nv, nh, d_rec.ptr))
            _lib.check(lib.msiren_score_images_dev(h, d_full.ptr, d_rec.ptr, n, 320, 320, d_s.ptr))
            model.sync()
            results.append(d_s.numpy().view(np.float64).copy())
        synced = harness.score_images(d_full, d_rec)
        host = np.empty((n, 3))
        rec = d_rec.numpy()
        _lib.check(lib.msiren_score_images(h, full.ctypes.data, rec.ctypes.data, n, 320, 320, host.ctypes.data))
    finally:
        _lib.check(lib.msiren_set_streams(h, 1))
    for r in results:
        assert np.array_equal(r.view(np.uint64), synced.view(np.uint64))
    assert np.array_equal(host.view(np.uint64), synced.view(np.uint64))
    assert_close(synced[0], full[0], rec[0])


def test_score_argument_errors(model):
    lib, h = model._lib, model._h
    img = np.ones((6, 32), np.float32)
    out = np.empty(3)
    for hh, ww in [(6, 32), (32, 6)]:
        assert lib.msiren_score_images(h, img.ctypes.data, img.ctypes.data, 1, hh, ww, out.ctypes.data) == _lib.E_INVALID
        assert b"7x7" in lib.msiren_last_error()
    d = model.device_array((8, 8))
    d_s = model.device_array((1, 6))
    assert lib.msiren_score_images_dev(h, None, d.ptr, 1, 8, 8, d_s.ptr) == _lib.E_INVALID
    assert b"null" in lib.msiren_last_error()
    assert lib.msiren_score_images_dev(h, d.ptr, d.ptr, 1, 8, 8, None) == _lib.E_INVALID
    assert lib.msiren_score_images_dev(h, d.ptr, d.ptr, -1, 8, 8, d_s.ptr) == _lib.E_INVALID
    assert b"n_images" in lib.msiren_last_error()
    assert lib.msiren_score_images_dev(None, d.ptr, d.ptr, 1, 8, 8, d_s.ptr) == _lib.E_INVALID
    assert lib.msiren_score_images_dev(h, None, None, 0, 8, 8, None) == 0
    assert lib.msiren_score_images(h, None, None, 0, 8, 8, None) == 0
    with pytest.raises(ValueError):
        harness.score_images(np.ones((6, 6), np.float32), np.ones((6, 6), np.float32))
    with pytest.raises(ValueError):
        harness.score_images(np.ones((8, 8), np.float32), np.ones((8, 9), np.float32))


def test_metrics_error_scores_on_the_device(model):
    """metrics_error (error.py:200-271) returns the host metrics of the images it reconstructs and folds -- the golden slice of
    tests/test_gpu_parity.py and synthetic ones, square and ragged."""
    g = load_golden("slice_recon.npz")
    golden_img = syn.make_slice(0, 160, 128, brain_mask=True)
    cases = [(golden_img, golden_img), (syn.make_slice(11, 320, 320, brain_mask=True), None), (syn.make_slice(12, 200, 136), None)]
    for full_img, under_img in cases:
        if under_img is None:
            under_img = ((full_img + np.roll(full_img, 1, 1) + np.roll(full_img, -1, 1)) / np.float32(3)).astype(np.float32)
        full_t, info = harness.image_to_patches(full_img[None], 32, 16)
        under_t, _ = harness.image_to_patches(under_img[None], 32, 16)
        got = harness.metrics_error(model, full_t, under_t, info, "cuda", 32, 16, 24)
        assert isinstance(got, tuple) and len(got) == 3 and all(isinstance(v, float) for v in got)
        rec = harness.reconstruct_from_patches(model, under_t, info)[0]
        full = harness.patches_to_image(full_t, info, 32, 16)[0]
        assert_close(np.array(got), full, rec)
    # the golden reconstruction of that slice (the reference's own model output) scored against the slice
    assert_close(harness.score_images(golden_img, g["image"][0])[0], golden_img, g["image"][0])
