"""The exact-fp32 prologue's five kernels (mri_inr_amd/csrc/encoder_modulator.hip.h) against tests/fp32_prologue_reference.py, element
by element, on the cases of tests/fp32_prologue_cases.py: every fp32 handle runs them, and every 16-bit handle off the preset shapes.

Per case: the latent against the end-to-end reference with its running bound; every Modulator layer in isolation, from the inputs the
device itself read (its own mods[l - 1] and z), on the device's own latent and on a seeded normal draw: |got - ref| <= bound on EVERY
element, zeros where the reference has them; msiren_last_prologue_kernel is "" (the per-layer launches ran); the one-call form
msiren_encode_modulate_tiles returns the bits of the two halves.  The largest |got - ref| / bound per case and stage is printed
(`FP32GATE` lines; LAB_NOTES.md section 41 holds a run's) -- reported, never a gate.

Then what the cases cannot reach through those calls: the device-side row count (`plan[0]` of the masked slice pipeline) through
`reconstruct` against the step-by-step chain, bit for bit; rows that are not finite; the shape msiren_create refuses.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import fp32_prologue_cases as fc
import fp32_prologue_reference as fr
from mri_inr_amd import ModulatedSiren, _lib, harness, synthetic as syn

pytestmark = pytest.mark.gpu


def build(mo: fc.Model, S=fc.S, device="cuda"):
    return ModulatedSiren(dim_in=2, dim_hidden=mo.H, dim_out=1, num_layers=mo.L, latent_dim=mo.Z, w0=1.0, w0_initial=30.0, use_bias=True,
                          dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None, outer_patch_size=32, inner_patch_size=16,
                          siren_patch_size=S, device=device, activation="sine", precision=mo.precision)


@functools.lru_cache(maxsize=2)
def model(mo: fc.Model, S=fc.S):
    m = build(mo, S)
    sd = fc.state_dict(mo) if S == fc.S else dict(fc.state_dict(mo), grid=syn.make_grid(S))
    m.load_state_dict(sd)
    m.to("cuda").eval()
    return m


def gate(tag, got, ref, bound):
    assert got.dtype == np.float32 and np.isfinite(got).all(), tag
    r = fr.ratio(got, ref, bound)
    i = np.unravel_index(np.argmax(r), r.shape)
    print(f"FP32GATE {tag}: worst |got - ref| / bound {r[i]:.3g} at {tuple(int(k) for k in i)}")
    assert r[i] <= 1.0, (tag, i, float(got[i]), float(ref[i]), float(bound[i]))
    return float(r[i])


@pytest.mark.parametrize("c", fc.CASES, ids=lambda c: c.id)
def test_every_element_within_the_bound(c):
    mo, sd, t = c.model, fc.state_dict(c.model), fc.tiles(c)
    m = model(mo)
    z = m.encoder(t)
    assert m.last_prologue_kernel() == "" and z.shape == (c.B, mo.Z)
    zr, ze = fr.encoder(sd, t)
    gate(f"{c.id} latent [{c.conv12} / {c.conv3} / {c.fc}]", z, zr, ze)
    for name, zz in (("own", z), ("normal", fc.normal_latent(c))):
        mods = m.modulator(zz)
        assert m.last_prologue_kernel() == "" and len(mods) == mo.L
        h = None
        for l in range(mo.L):
            ref = fr.modulator_layer(sd, l, h, zz)
            gate(f"{c.id} {name} layer {l} [{c.mod}]", mods[l], ref.out, ref.bound)
            assert fr.misplaced_zeros(mods[l], ref) == 0, (name, l)
            h = mods[l]
    # the launches forward(tiles) makes in front of its trunk, in one call: the same kernels, the same bits
    mods1, z1 = m.encode_modulate(t, return_latent=True)
    assert m.last_prologue_kernel() == "" and np.array_equal(z1, z) and np.array_equal(mods1, np.stack(m.modulator(z)))


# ---- the device-side row count ---------------------------------------------------------------------------------------------------------
S_FOLD = 16   # (the fold needs siren_patch_size >= inner_patch_size)


@pytest.mark.parametrize("mo,n,hw", [(fc.M_100, 2, (96, 80)), (fc.M_256, 2, (96, 80)), (fc.M_256, 12, (160, 160))],
                         ids=["100-24-3-valu", "256-128-3-16x16", "256-128-3-tile"])
def test_reconstruct_same_bits_as_step_by_step(mo, n, hw):
    """`reconstruct` hands the number of non-black tiles over on the device (plan[0]): the encoder, conv3, Linear(64, Z) and every
    Modulator layer launch on the upper bound and stop at a count they read themselves.  The step-by-step chain's model call knows
    its batch on the host.  2 slices of 96 x 80: 60 tiles (the VALU kernels under a plan for the first time; the 16 x 16 kernel);
    12 slices of 160 x 160: 1 200 tiles, fewer kept -- the tile kernel with count < B."""
    m = model(mo, S_FOLD)
    harness.bind(m)
    imgs = np.stack([syn.make_slice(k, *hw, brain_mask=True) for k in range(n)])
    imgs[1] = 0.0
    rec = m.reconstruct(imgs)
    assert m.last_prologue_kernel() == "" and np.isfinite(rec).all() and rec[0].std() > 0 and not rec[1].any()
    tiles, info = harness.image_to_patches(imgs, 32, 16)
    kept, black, shape = harness.filter_and_remember_black_patches(tiles)
    per = info[0][0] * info[0][1]
    assert tiles.shape[0] == n * per and per <= len(black) < tiles.shape[0] - 1
    if n == 12:
        assert tiles.shape[0] == 1200 and len(black) > 100
    full = harness.reintegrate_black_patches(m(kept), black, shape)
    assert np.array_equal(harness.patches_to_image_weighted_average(full, info, S_FOLD, 16, "cuda"), rec)
    assert np.array_equal(m.reconstruct(imgs[0]), rec[0])
    assert not m.reconstruct(np.zeros((2,) + hw, np.float32)).any()      # a count of zero
    assert np.array_equal(m.reconstruct(imgs), rec)


# ---- rows that are not finite ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mo", [fc.M_256, fc.M_100], ids=lambda mo: mo.id)
def test_non_finite_tiles_stay_in_their_rows(mo):
    m = model(mo)
    clean = fc.make_tiles(37, 77)
    dirty = clean.copy()
    dirty[5], dirty[20] = np.nan, np.inf
    bad = np.zeros(37, bool)
    bad[[5, 20]] = True
    z0, z1 = m.encoder(clean), m.encoder(dirty)
    assert np.isfinite(z0).all() and not np.isfinite(z1[bad]).any()
    assert np.array_equal(z1[~bad], z0[~bad])
    m0, m1 = np.stack(m.modulator(z0)), np.stack(m.modulator(z1))
    assert np.isfinite(m0).all() and not np.isfinite(m1[:, bad]).any()
    assert np.array_equal(m1[:, ~bad], m0[:, ~bad])
    m2, z2 = m.encode_modulate(dirty, return_latent=True)
    assert np.array_equal(z2, z1, equal_nan=True) and np.array_equal(m2, m1, equal_nan=True)


# ---- the shape msiren_create refuses -----------------------------------------------------------------------------------------------------
def test_create_refuses_a_valu_modulator_past_64_kb_of_lds():
    """H % 16 || Z % 16 runs modulator_layer_kernel with 8 192 + 32 K bytes of LDS in a plain launch: K = (L > 1 ? H : 0) + Z <= 1792.
    (500, 1300, 2) would need 65 792 bytes (tests/test_dispatch.py pins the count): refused at msiren_create with MSIREN_E_INVALID, naming
    latent_dim; nothing is launched to find out.  (500, 1292, 2), exactly 65 536, is created."""
    lib = _lib.load()
    cfg = build(fc.Model(500, 1300, 2), device="cpu")._config()   # (no handle yet: the configuration alone)
    h = C.c_void_p()
    assert lib.msiren_create(C.byref(cfg), C.byref(h)) == _lib.E_INVALID and not h.value
    assert "latent_dim" in _lib.last_error() and "1792" in _lib.last_error(), _lib.last_error()
    with pytest.raises(ValueError, match="latent_dim"):
        build(fc.Model(500, 1300, 2))
    ok = build(fc.Model(500, 1292, 2))
    assert ok._h is not None and ok.profile_kernels() == []
    for mo in (fc.Model(500, 1300, 1), fc.Model(496, 1312, 2)):   # one layer: K = Z; multiples of 16: the MFMA kernels
        assert build(mo)._h is not None
