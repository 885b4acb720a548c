"""One coordinate set per patch on the GPU: model.sample_mods_ragged / sample_mods_ragged_grad, i.e.
msiren_sample_ragged_* on siren_trunk_f32_ragged_kernel / siren_trunk_f32_jet_ragged_kernel.

No tolerance anywhere: a coordinate's column of the trunk never sees its neighbours, so every patch's slice of the output has to be the
BITS of an fp32 handle's sample_mods (sample_mods_grad) of that patch alone at its own coordinates.
"""
import functools

import numpy as np
import pytest

import grad_reference as gr
from mri_inr_amd import ModulatedSiren, _lib, synthetic as syn

pytestmark = pytest.mark.gpu

# patches without coordinates at both ends; 63 / 64 / 65 around the value kernel's chunk, 130 = two chunks and a ragged third
COUNTS = [0, 1, 63, 64, 65, 130, 0]
# ... and 31 / 32 / 33 around the jet's
COUNTS_JET = [0, 1, 31, 32, 33, 130, 0]

CASES = {
    "H256-sine-L5": gr.Case("H256-sine-L5", 256, 5, "sine"),
    "H128-morlet-L3": gr.Case("H128-morlet-L3", 128, 3, "morlet"),
    "H256-sine-L1": gr.Case("H256-sine-L1", 256, 1, "sine"),
}


def build(sd, *, H=256, L=5, act="sine", prec="fp32", **kw):
    m = ModulatedSiren(dim_in=2, dim_hidden=H, dim_out=1, num_layers=L, latent_dim=256, w0=1.0, w0_initial=30.0, use_bias=True,
                       dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None, outer_patch_size=32, inner_patch_size=16,
                       siren_patch_size=24, device="cuda", activation=act, precision=prec, **kw)
    m.load_state_dict(sd, strict=False)
    m.to("cuda")
    m.eval()
    return m


@functools.lru_cache(maxsize=None)
def case_model(name, prec="fp32"):
    c = CASES[name]
    return build(gr.case_state_dict(c), H=c.H, L=c.L, act=c.act, prec=prec)


@functools.lru_cache(maxsize=None)
def wide_residual_model():
    sd = syn.make_state_dict(seed=3, dim_hidden=512, num_layers=3, with_encoder=False)
    return build({k: v for k, v in sd.items() if not k.startswith("modulator")}, H=512, L=3, residual=True)


def inputs(H, L, counts, seed=11):
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    coords = np.random.default_rng(seed).uniform(-1.2, 1.2, size=(int(offsets[-1]), 2)).astype(np.float32)
    return syn.make_mods(2, L, len(counts), H), coords, offsets


def profile_on(m):
    _lib.check(m._lib.msiren_profile_enable(m._h, 1))


def profile_off(m):
    _lib.check(m._lib.msiren_profile_enable(m._h, 0))


def check_values_patch_by_patch(m, mods, coords, offsets, out):
    assert out.shape == (len(coords),) and out.dtype == np.float32
    for b in range(mods.shape[1]):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi > lo:
            assert np.array_equal(out[lo:hi], m.sample_mods(mods[:, b:b + 1], coords[lo:hi])[0]), (b, lo, hi)


# ---- 1. every patch's slice is the fp32 trunk's bits ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("counts", [COUNTS, COUNTS_JET], ids=["chunk64", "chunk32"])
def test_values_are_the_fp32_trunks_bits(name, counts):
    m, c = case_model(name), CASES[name]
    mods, coords, offsets = inputs(c.H, c.L, counts)
    check_values_patch_by_patch(m, mods, coords, offsets, np.asarray(m.sample_mods_ragged(mods, coords, offsets)))
    assert "f32_kernel" in m.last_trunk_kernel()  # (the ragged call does not rename the last trunk)


def test_values_wide_residual():
    m = wide_residual_model()
    mods, coords, offsets = inputs(512, 3, COUNTS)
    check_values_patch_by_patch(m, mods, coords, offsets, np.asarray(m.sample_mods_ragged(mods, coords, offsets)))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("counts", [COUNTS, COUNTS_JET], ids=["chunk64", "chunk32"])
def test_value_and_gradient_are_the_jets_bits(name, counts):
    m, c = case_model(name), CASES[name]
    mods, coords, offsets = inputs(c.H, c.L, counts)
    val, grad = (np.asarray(a) for a in m.sample_mods_ragged_grad(mods, coords, offsets))
    assert val.shape == (len(coords),) and grad.shape == (2, len(coords))
    assert np.array_equal(val, m.sample_mods_ragged(mods, coords, offsets))
    for b in range(len(counts)):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi > lo:
            v, g = m.sample_mods_grad(mods[:, b:b + 1], coords[lo:hi])
            assert np.array_equal(val[lo:hi], v[0]) and np.array_equal(grad[:, lo:hi], g[:, 0]), (b, lo, hi)


# ---- 2. every patch given the same set: the shared-set call ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_same_set_for_every_patch_is_sample_mods(name):
    m, c = case_model(name), CASES[name]
    B, Q = 5, 70
    mods = syn.make_mods(2, c.L, B, c.H)
    shared = np.random.default_rng(4).uniform(-1.2, 1.2, size=(Q, 2)).astype(np.float32)
    coords, offsets = np.tile(shared, (B, 1)), np.arange(B + 1, dtype=np.int32) * Q
    assert np.array_equal(np.asarray(m.sample_mods_ragged(mods, coords, offsets)).reshape(B, Q), m.sample_mods(mods, shared))
    val, grad = m.sample_mods_ragged_grad(mods, coords, offsets)
    v, g = m.sample_mods_grad(mods, shared)
    assert np.array_equal(np.asarray(val).reshape(B, Q), v) and np.array_equal(np.asarray(grad).reshape(2, B, Q), g)


# ---- 3. always exact fp32 ------------------------------------------------------------------------------------------------------------
def test_split_fp16_handle_returns_the_fp32_handles_bits():
    m32, m16 = case_model("H256-sine-L5"), case_model("H256-sine-L5", "f16x3")
    mods, coords, offsets = inputs(256, 5, COUNTS)
    assert np.array_equal(m16.sample_mods_ragged(mods, coords, offsets), m32.sample_mods_ragged(mods, coords, offsets))
    (v16, g16), (v32, g32) = m16.sample_mods_ragged_grad(mods, coords, offsets), m32.sample_mods_ragged_grad(mods, coords, offsets)
    assert np.array_equal(v16, v32) and np.array_equal(g16, g32)


# ---- 4. the device form, other callers' types ------------------------------------------------------------------------------------
def test_device_form_and_null_value_output():
    m = case_model("H256-sine-L5")
    mods, coords, offsets = inputs(256, 5, COUNTS)
    T, B = len(coords), len(COUNTS)
    val, grad = (np.array(a) for a in m.sample_mods_ragged_grad(mods, coords, offsets))
    d_m, d_c = m.device_array(mods.shape).copy_from(mods), m.device_array(coords.shape).copy_from(coords)
    try:
        for n in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, n))
            for _ in range(n + 1):
                dv, dg = m.sample_mods_ragged_grad(d_m, d_c, offsets)
                assert np.array_equal(dv.numpy(), val) and np.array_equal(dg.numpy(), grad), n
                assert np.array_equal(m.sample_mods_ragged(d_m, d_c, offsets).numpy(), val), n
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))
    g = np.empty((2, T), np.float32)  # out = NULL: the gradient alone, unchanged
    _lib.check(m._lib.msiren_sample_ragged_grad_mods(m._h, coords.ctypes.data, offsets.ctypes.data, mods.ctypes.data, B, T, None, g.ctypes.data))
    assert np.array_equal(g, grad)
    assert np.array_equal(m.sample_mods_ragged(mods, coords, offsets.astype(np.int64).tolist()), val)  # offsets as a plain list


# ---- 5. a non-finite coordinate ----------------------------------------------------------------------------------------------------
def test_nonfinite_coordinate_spoils_only_itself():
    m = case_model("H128-morlet-L3")
    mods, coords, offsets = inputs(128, 3, COUNTS)
    val, grad = (np.array(a) for a in m.sample_mods_ragged_grad(mods, coords, offsets))
    bad = coords.copy()
    at = int(offsets[3]) + 17  # inside the 64-coordinate patch
    bad[at, 1], bad[at + 1, 0] = np.nan, np.inf
    bval, bgrad = (np.asarray(a) for a in m.sample_mods_ragged_grad(mods, bad, offsets))
    bout = np.asarray(m.sample_mods_ragged(mods, bad, offsets))
    keep = np.ones(len(coords), bool)
    keep[at:at + 2] = False
    assert not np.isfinite(bval[~keep]).any() and not np.isfinite(bgrad[:, ~keep]).any() and not np.isfinite(bout[~keep]).any()
    assert np.array_equal(bval[keep], val[keep]) and np.array_equal(bgrad[:, keep], grad[:, keep]) and np.array_equal(bout[keep], val[keep])


# ---- 6. nothing to do, and refusals ------------------------------------------------------------------------------------------------
def test_empty_calls_launch_nothing():
    m = case_model("H256-sine-L5")
    profile_on(m)
    try:
        mods = syn.make_mods(2, 5, 3, 256)
        none = np.zeros((0, 2), np.float32)
        assert m.sample_mods_ragged(mods, none, np.zeros(4, np.int32)).shape == (0,)               # T = 0
        v, g = m.sample_mods_ragged_grad(mods[:, :0], none, np.zeros(1, np.int32))                   # B = 0
        assert v.shape == (0,) and g.shape == (2, 0)
        d_m = m.device_array(mods.shape).copy_from(mods)
        assert m.sample_mods_ragged(d_m, none, np.zeros(4, np.int32)).shape == (0,)
        assert m._lib.msiren_sample_ragged_mods_dev(m._h, d_m.ptr, d_m.ptr, d_m.ptr, 3, 0, d_m.ptr) == 0
        for fn in (m._lib.msiren_sample_ragged_mods, m._lib.msiren_sample_ragged_mods_dev):
            assert fn(m._h, None, None, None, 0, 0, None) == 0
            assert fn(m._h, None, None, None, 3, 0, None) == 0
        m.sync()
        assert m.profile_kernels() == []
    finally:
        profile_off(m)


def test_malformed_offsets_are_value_errors():
    m = case_model("H256-sine-L5")
    mods, coords, offsets = inputs(256, 5, [3, 4, 5])
    T = len(coords)
    out = np.empty(T, np.float32)
    profile_on(m)
    try:
        for bad in ([1, 3, 7, 12], [0, 3, 7, 11], [0, 3, 7, 13], [0, 8, 7, 12], [0, -1, 7, 12]):
            o = np.asarray(bad, np.int32)
            assert m._lib.msiren_sample_ragged_mods(m._h, coords.ctypes.data, o.ctypes.data, mods.ctypes.data, 3, T, out.ctypes.data) == _lib.E_INVALID, bad
            assert "offsets" in _lib.last_error()
            with pytest.raises(ValueError, match="offsets"):
                m.sample_mods_ragged(mods, coords, o)
            with pytest.raises(ValueError, match="offsets"):
                m.sample_mods_ragged_grad(mods, coords, o)
        with pytest.raises(ValueError, match="offsets"):
            m.sample_mods_ragged(mods, coords, offsets[:-1])                                          # B entries instead of B + 1
        with pytest.raises(ValueError, match="offsets"):
            m.sample_mods_ragged(mods, coords, offsets.astype(np.float32))
        with pytest.raises(ValueError):
            m.sample_mods_ragged(mods, coords.reshape(-1), offsets)
        big = 1 << 30                                                                                # an index would leave 32 bits
        assert m._lib.msiren_sample_ragged_mods(m._h, coords.ctypes.data, offsets.ctypes.data, mods.ctypes.data, 3, big, out.ctypes.data) == _lib.E_INVALID
        d_m, d_c, d_o = m.device_array(mods.shape).copy_from(mods), m.device_array(coords.shape).copy_from(coords), m.device_array((T,))
        assert m._lib.msiren_sample_ragged_mods_dev(m._h, d_c.ptr, d_o.ptr, d_m.ptr, 3, big, d_o.ptr) == _lib.E_INVALID
        m.sync()
        assert m.profile_kernels() == []
        assert np.asarray(m.sample_mods_ragged(mods, coords, offsets)).shape == (T,)                 # the handle stays usable
    finally:
        profile_off(m)


def test_gradient_form_refuses_wide_and_residual_models():
    wide = wide_residual_model()
    res = build(gr.case_state_dict(gr.Case("H256-sine-L2", 256, 2, "sine")), L=2, residual=True)
    sd512 = syn.make_state_dict(seed=3, dim_hidden=512, num_layers=3, with_encoder=False)
    plain512 = build({k: v for k, v in sd512.items() if not k.startswith("modulator")}, H=512, L=3)
    for m, H, L, word in ((plain512, 512, 3, "256"), (res, 256, 2, "residual"), (wide, 512, 3, "256|residual")):
        mods, coords, offsets = inputs(H, L, [3, 4, 5])
        profile_on(m)
        try:
            with pytest.raises(ValueError, match=word):
                m.sample_mods_ragged_grad(mods, coords, offsets)
            d_m, d_c = m.device_array(mods.shape).copy_from(mods), m.device_array(coords.shape).copy_from(coords)
            with pytest.raises(ValueError, match=word):
                m.sample_mods_ragged_grad(d_m, d_c, offsets)
            m.sync()
            assert m.profile_kernels() == []
        finally:
            profile_off(m)
        check_values_patch_by_patch(m, mods, coords, offsets, np.asarray(m.sample_mods_ragged(mods, coords, offsets)))  # the value form runs


# ---- 7. the profile entry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kernels", [("H256-sine-L5", ("siren_trunk_f32_ragged_kernel<256,0,0>", "siren_trunk_f32_jet_ragged_kernel<256,0>")),
                                          ("H128-morlet-L3", ("siren_trunk_f32_ragged_kernel<128,1,0>", "siren_trunk_f32_jet_ragged_kernel<128,1>"))])
def test_profile_entry(name, kernels):
    m, c = case_model(name), CASES[name]
    mods, coords, offsets = inputs(c.H, c.L, COUNTS)
    profile_on(m)
    try:
        m.sample_mods_ragged(mods, coords, offsets)
        m.sample_mods_ragged_grad(mods, coords, offsets)
        entries = m.profile_kernels()
        assert [e["kernel"] for e in entries] == list(kernels), entries
        assert all(e["launches"] == 1 and e["coords"] == len(coords) for e in entries), entries
    finally:
        profile_off(m)
