"""The model's spatial gradient on the GPU: model.sample_mods_grad / sample_grad / reconstruct_with_gradient, i.e.
msiren_sample_grad_* and msiren_reconstruct_slices_grad on siren_trunk_f32_jet_kernel.

Values: the bits of an fp32 handle's sample_mods (np.array_equal).  Gradients: against the fp64 forward-mode reference
(tests/grad_reference.py), per case within 4 x the distance of the reference's own perturbed fp32 variant from it, capped at the project's
parity norm -- the gate tests/test_grad_reference.py keeps at most half way to the smallest seeded error.  Where a call runs the prologue
first (tiles in), the fp32 variant runs the oracle's prologue in fp32 as well: the floor is that of the chain the call evaluates.
"""
import functools

import numpy as np
import pytest

import grad_reference as gr
from mri_inr_amd import ModulatedSiren, _lib, synthetic as syn
from oracle import siren_oracle as orc

pytestmark = pytest.mark.gpu


def build(sd, *, H=256, L=5, act="sine", prec="fp32", use_bias=True, strict=False, **kw):
    m = ModulatedSiren(dim_in=2, dim_hidden=H, dim_out=1, num_layers=L, latent_dim=256, w0=1.0, w0_initial=30.0, use_bias=use_bias,
                       dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None, outer_patch_size=32, inner_patch_size=16,
                       siren_patch_size=24, device="cuda", activation=act, precision=prec, **kw)
    m.load_state_dict(sd, strict=strict)
    m.to("cuda")
    m.eval()
    return m


@functools.lru_cache(maxsize=None)
def case_model(case, prec="fp32"):
    return build(gr.case_state_dict(case), H=case.H, L=case.L, act=case.act, prec=prec, use_bias=case.use_bias)


@functools.lru_cache(maxsize=None)
def full_sd():
    return syn.make_state_dict(seed=7, trained_like=True)


@functools.lru_cache(maxsize=None)
def full_model(prec="fp32"):
    return build(full_sd(), prec=prec, strict=True)


def case_by_name(name):
    return next(c for c in gr.CASES if c.name == name)


def check_grad(got, ref, gates, what):
    assert got.shape == ref.shape and got.dtype == np.float32, (got.shape, ref.shape, got.dtype)
    assert np.isfinite(got).all(), what
    em, er = gr.distances(got, ref)
    print(f"{what}: max|grad| {np.abs(ref).max():.1f}  nerr {em:.2e} (gate {gates[0]:.2e})  rms {er:.2e} (gate {gates[1]:.2e})")
    assert em <= gates[0] and er <= gates[1], (what, em, er, gates)


# ---- 1. the values are the fp32 trunk's bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in gr.CASES if c.H in (256, 128)], ids=str)
def test_values_are_the_fp32_trunks_bits(case):
    m = case_model(case)
    for Q, B in gr.SIZES:
        mods, coords = gr.case_inputs(case, Q, B)
        val, grad = m.sample_mods_grad(mods, coords)
        assert val.shape == (B, Q) and grad.shape == (2, B, Q)
        assert np.array_equal(val, m.sample_mods(mods, coords)), (Q, B)
        assert "f32_kernel" in m.last_trunk_kernel()  # (the gradient call does not rename the last trunk)


@pytest.mark.parametrize("name", ["H256-sine-L5", "H256-morlet-L5", "H256-sine-L2"])
def test_split_fp16_handle_returns_the_fp32_handles_bits(name):
    case = case_by_name(name)
    m32, m16 = case_model(case), case_model(case, "f16x3")
    for Q, B in ((77, 9), (33, 1)):
        mods, coords = gr.case_inputs(case, Q, B)
        v32, g32 = m32.sample_mods_grad(mods, coords)
        v16, g16 = m16.sample_mods_grad(mods, coords)
        assert np.array_equal(v16, v32) and np.array_equal(g16, g32), (Q, B)


# ---- 2. gradients against the fp64 reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gr.CASES, ids=str)
def test_gradients_vs_reference(case):
    m = case_model(case)
    for Q, B in gr.SIZES:
        d = gr.case_data(case, Q, B)
        _, grad = m.sample_mods_grad(d["mods"], d["coords"])
        check_grad(np.asarray(grad), d["grad"], d["gate"], f"{case} Q={Q} B={B}")


def prologue(sd, tiles, dtype):
    z = orc.encoder_forward(sd, tiles, dtype=dtype)
    return orc.modulator_forward(sd, z, num_layers=5, dtype=dtype)


def test_gradients_from_tiles_vs_reference():
    sd, m = full_sd(), full_model()
    tiles = np.random.default_rng(5).random((17, 32, 32), dtype=np.float32)
    coords = np.random.default_rng(3).uniform(-1.2, 1.2, size=(77, 2)).astype(np.float32)
    _, ref = gr.value_and_grad(sd, prologue(sd, tiles, np.float64), coords, num_layers=5)
    _, g32 = gr.value_and_grad(sd, prologue(sd, tiles, np.float32), coords, num_layers=5, dtype=np.float32, perturbed=True)
    fm, fr = gr.distances(g32, ref)
    val, grad = m.sample_grad(tiles, coords)
    assert np.array_equal(val, m.sample(tiles, coords))
    check_grad(np.asarray(grad), ref, (min(gr.FACTOR * fm, gr.CAP_MAX), min(gr.FACTOR * fr, gr.CAP_RMS)), "17 tiles Q=77")


# ---- 3. locality, bit for bit ---------------------------------------------------------------------------------------------------
def test_locality():
    case = case_by_name("H256-sine-L5")
    m = case_model(case)
    mods, coords = gr.case_inputs(case, 77, 9)
    val, grad = (np.array(a) for a in m.sample_mods_grad(mods, coords))
    v32, g32 = m.sample_mods_grad(mods, coords[:32])
    assert np.array_equal(grad[:, :, :32], g32) and np.array_equal(val[:, :32], v32)          # a coordinate does not see the set around it
    for b in (0, 4, 8):
        v1, g1 = m.sample_mods_grad(mods[:, b:b + 1], coords)
        assert np.array_equal(grad[:, b:b + 1], g1) and np.array_equal(val[b:b + 1], v1), b    # a patch does not see the batch around it
    d_m, d_c = m.device_array(mods.shape).copy_from(mods), m.device_array(coords.shape).copy_from(coords)
    try:
        for n in (1, 2, 3):                                                                     # 1 / 2 / 3 streams, the _dev form
            _lib.check(m._lib.msiren_set_streams(m._h, n))
            for _ in range(n + 1):
                dv, dg = m.sample_mods_grad(d_m, d_c)
                assert np.array_equal(dv.numpy(), val) and np.array_equal(dg.numpy(), grad), n  # ... which is the host form's result
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))
    # out = NULL: the gradient alone, unchanged (host and _dev form)
    g = np.empty((2, 9, 77), np.float32)
    _lib.check(m._lib.msiren_sample_grad_mods(m._h, coords.ctypes.data, 77, mods.ctypes.data, 9, None, g.ctypes.data))
    assert np.array_equal(g, grad)
    d_g = m.device_array((2, 9, 77))
    _lib.check(m._lib.msiren_sample_grad_mods_dev(m._h, d_c.ptr, 77, d_m.ptr, 9, None, d_g.ptr))
    m.sync()
    assert np.array_equal(d_g.numpy(), grad)
    m.pin_outputs(False)                                                                        # pageable outputs
    try:
        v, g = m.sample_mods_grad(mods, coords)
        assert np.array_equal(v, val) and np.array_equal(g, grad)
    finally:
        m.pin_outputs(True)
    assert m.sample_mods_grad(mods[:, :0], coords)[1].shape == (2, 0, 77)                       # B = 0 does nothing


# ---- 4. a non-finite coordinate -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["H256-sine-L5", "H128-morlet-L2"])
def test_nonfinite_coordinate_stays_where_it_is(name):
    case = case_by_name(name)
    m = case_model(case)
    mods, coords = gr.case_inputs(case, 77, 9)
    coords = coords[:40]
    bad = coords.copy()
    bad[17, 1] = np.nan
    val, grad = (np.array(a) for a in m.sample_mods_grad(mods, coords))
    bval, bgrad = m.sample_mods_grad(mods, bad)
    assert not np.isfinite(bval[:, 17]).any() and not np.isfinite(bgrad[:, :, 17]).any()
    keep = np.arange(40) != 17
    assert np.array_equal(bval[:, keep], val[:, keep]) and np.array_equal(bgrad[:, :, keep], grad[:, :, keep])


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def profile_on(m):
    _lib.check(m._lib.msiren_profile_enable(m._h, 1))


def test_refusals_launch_nothing():
    coords = np.random.default_rng(1).uniform(-1, 1, size=(10, 2)).astype(np.float32)
    sd512 = syn.make_state_dict(seed=3, dim_hidden=512, num_layers=3, with_encoder=False)
    sd512 = {k: v for k, v in sd512.items() if not k.startswith("modulator")}
    wide = build(sd512, H=512, L=3)
    case = case_by_name("H256-sine-L2")
    res = build(gr.case_state_dict(case), L=2, residual=True)
    for m, H, L, word in ((wide, 512, 3, "256"), (res, 256, 2, "residual")):
        profile_on(m)
        mods = syn.make_mods(2, L, 2, H)
        with pytest.raises(ValueError, match=word):
            m.sample_mods_grad(mods, coords)
        d_m, d_c, d_g = m.device_array(mods.shape).copy_from(mods), m.device_array(coords.shape).copy_from(coords), m.device_array((2, 2, 10))
        assert m._lib.msiren_sample_grad_mods_dev(m._h, d_c.ptr, 10, d_m.ptr, 2, None, d_g.ptr) == _lib.E_INVALID
        d_i, d_r = m.device_array((1, 64, 48)), m.device_array((2, 1, 64, 48))
        assert m._lib.msiren_reconstruct_slices_grad_dev(m._h, d_i.ptr, 1, 64, 48, 16, None, d_r.ptr) == _lib.E_INVALID
        assert word in _lib.last_error()
        m.sync()
        assert m.profile_kernels() == []
        assert m.sample_mods(mods, coords).shape == (2, 10)  # the handle stays usable
    m = case_model(case)
    profile_on(m)
    try:
        mods = syn.make_mods(2, 2, 2, 256)
        big = np.zeros((65537, 2), np.float32)
        d_m, d_c = m.device_array(mods.shape).copy_from(mods), m.device_array(big.shape).copy_from(big)
        d_v, d_g = m.device_array((2, 10)), m.device_array((2, 2, 10))
        v, g = np.empty((2, 10), np.float32), np.empty((2, 2, 10), np.float32)
        for Q in (0, 65537):
            assert m._lib.msiren_sample_grad_mods(m._h, big.ctypes.data, Q, mods.ctypes.data, 2, v.ctypes.data, g.ctypes.data) == _lib.E_INVALID
            assert m._lib.msiren_sample_grad_mods_dev(m._h, d_c.ptr, Q, d_m.ptr, 2, d_v.ptr, d_g.ptr) == _lib.E_INVALID
            assert str(Q) in _lib.last_error()
            with pytest.raises(ValueError):
                m.sample_mods_grad(mods, big[:Q])
        assert m._lib.msiren_sample_grad_mods_dev(m._h, d_c.ptr + 4, 10, d_m.ptr, 2, d_v.ptr, d_g.ptr) == _lib.E_INVALID  # misaligned pairs
        assert "aligned" in _lib.last_error()
        m.sync()
        assert m.profile_kernels() == []
    finally:
        _lib.check(m._lib.msiren_profile_enable(m._h, 0))


# ---- 6. the slice form -----------------------------------------------------------------------------------------------------------
def banded_image():
    img = syn.make_slice(4, 64, 48)
    img[:40] = 0.0  # the two upper rows of tiles see nothing but black: the filter drops them
    return img


@pytest.mark.parametrize("stride", [16, 32])
def test_slice_form(stride):
    sd, m = full_sd(), full_model()
    img = banded_image()
    S, I = 24, 16
    T = S * stride // I
    patches, info = orc.image_to_patches(img, 32, 16)
    kept, black, shape = orc.filter_and_remember_black_patches(patches)
    assert shape[0] == 12 and 0 < len(black) < 12, (shape, len(black))
    recon, grad = m.reconstruct_with_gradient(img, out_stride=stride)
    assert recon.shape == (4 * stride, 3 * stride) and grad.shape == (2, 4 * stride, 3 * stride)
    assert np.array_equal(recon, m.reconstruct(img, out_stride=stride))
    # the lattice: out_stride = inner_patch_size is the model's own grid (as for reconstruct), another stride its upsampled lattice
    lattice = np.asarray(m.grid, dtype=np.float32) if stride == I else m.upsampled_grid(stride)
    gscale = np.float32((2.0 / (S - 1)) / (stride / I))
    _, tg = m.sample_grad(patches, lattice)
    planes = np.array(tg) * gscale
    planes[:, np.asarray(black, dtype=np.int64)] = 0.0
    d_r = m.device_array((1, 4 * stride, 3 * stride))
    for k in range(2):
        d_t = m.device_array((12, T, T)).copy_from(np.ascontiguousarray(planes[k]).reshape(12, T, T))
        _lib.check(m._lib.msiren_weighted_fold_scaled_dev(m._h, d_t.ptr, 1, 4, 3, stride, d_r.ptr))
        m.sync()
        assert np.array_equal(grad[k], d_r.numpy()[0]), k
    # _dev form, recon = NULL
    d_i, d_g = m.device_array((1, 64, 48)).copy_from(img[None]), m.device_array((2, 1, 4 * stride, 3 * stride))
    _lib.check(m._lib.msiren_reconstruct_slices_grad_dev(m._h, d_i.ptr, 1, 64, 48, stride, None, d_g.ptr))
    m.sync()
    assert np.array_equal(d_g.numpy()[:, 0], grad)

    # against the fp64 reference, folded with the oracle's fold; the floor: the same chain in fp32, perturbed
    def chain(dtype, **kw):
        _, g = gr.value_and_grad(sd, prologue(sd, kept, dtype), lattice, num_layers=5, dtype=dtype, **kw)
        g = (g * dtype(gscale)).reshape(2, -1, T, T)
        return np.stack([orc.patches_to_image_weighted_average(orc.reintegrate_black_patches(g[k], black, (shape[0], T, T)), info, T, stride)
                         for k in range(2)])

    ref, g32 = chain(np.float64), chain(np.float32, perturbed=True)
    fm, fr = gr.distances(g32, ref)
    check_grad(np.asarray(grad), ref, (min(gr.FACTOR * fm, gr.CAP_MAX), min(gr.FACTOR * fr, gr.CAP_RMS)), f"slice form I'={stride}")


# ---- 7. the profile entry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kernel", [("H256-sine-L5", "siren_trunk_f32_jet_kernel<256,0>"), ("H128-morlet-L2", "siren_trunk_f32_jet_kernel<128,1>"),
                                         ("H200-sine-L5", "siren_trunk_f32_jet_kernel<256,0>")])
def test_profile_entry(name, kernel):
    case = case_by_name(name)
    m = case_model(case)
    mods, coords = gr.case_inputs(case, 33, 9)
    profile_on(m)
    try:
        m.sample_mods_grad(mods, coords)
        entries = m.profile_kernels()
        assert [e["kernel"] for e in entries] == [kernel], entries
        assert entries[0]["launches"] == 1 and entries[0]["coords"] == 9 * 33, entries
    finally:
        _lib.check(m._lib.msiren_profile_enable(m._h, 0))
