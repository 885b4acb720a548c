"""The representation off its own grid: model.sample / sample_mods at caller-chosen coordinates and the slice
pipeline at another output stride, against the fp64 oracle evaluated at the same coordinates (``sd["grid"] = coords``).

Gate: the project's (tests/conftest.py, test_gpu_parity.check): max|a - ref| / max|ref| <= 1e-4 and RMS <= 1e-5 against the fp64
oracle; the H = 512 16-bit handles keep the tolerance of test_config5_16bit_trunk_vs_own_oracle.  The fp32 oracle alone sits at
4.5e-6 .. 6.9e-6 of the fp64 one on these lattices, so the gate is the arithmetic's, not the lattice's.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import nerr, rms
from mri_inr_amd import ModulatedSiren, _lib, harness, synthetic as syn
from oracle import siren_oracle as orc

pytestmark = pytest.mark.gpu

TOL, RMS_TOL = 1e-4, 1e-5
L = 5


def make_model(sd, *, H=256, L=5, Z=256, act="sine", encoder_type="custom", strict=True, **kw):
    m = ModulatedSiren(dim_in=2, dim_hidden=H, dim_out=1, num_layers=L, latent_dim=Z, w0=1.0, w0_initial=30.0, use_bias=True,
                       dropout=0.1, modulate=True, encoder_type=encoder_type, encoder_path=None, outer_patch_size=32,
                       inner_patch_size=16, siren_patch_size=24, device="cuda", activation=act, **kw)
    m.load_state_dict({k: v for k, v in sd.items() if k in m.state_dict()} if not strict else sd, strict=strict)
    m.to("cuda")
    m.eval()
    return m


def check(out, ref, tol=TOL, rtol=RMS_TOL, what=""):
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert out.dtype == np.float32
    assert np.isfinite(out).all()
    e, r = nerr(out, ref), rms(out, ref)
    print(f"{what}: nerr {e:.3e} rms {r:.3e}")
    assert e <= tol and r <= rtol, (what, e, r)
    return e


def ref_mods(sd, mods, coords, *, num_layers=L, act="sine", chunk=8):
    """fp64 oracle at `coords`, a few patches at a time (a x3 lattice is 5 184 coordinates x 256 features x 8 bytes per patch)."""
    sdg = dict(sd)
    sdg["grid"] = np.asarray(coords, dtype=np.float32)
    mods = np.asarray(mods)
    return np.concatenate([orc.siren_forward(sdg, mods[:, i:i + chunk], num_layers=num_layers, activation=act, dtype=np.float64)
                           for i in range(0, mods.shape[1], chunk)])


def ref_tiles(sd, tiles, coords, *, act="sine"):
    z = orc.encoder_forward(sd, tiles, dtype=np.float64)
    mods = orc.modulator_forward(sd, z, num_layers=L, dtype=np.float64)
    return ref_mods(sd, mods, coords, act=act)


def scattered(Q, seed=3):
    return np.random.default_rng(seed).uniform(-1.2, 1.2, size=(Q, 2)).astype(np.float32)


def range_events(m):
    n = C.c_int64()
    _lib.check(m._lib.msiren_range_events(m._h, C.byref(n)))
    return n.value


@pytest.fixture(scope="module")
def sd():
    return syn.make_state_dict(seed=7, trained_like=True)


@pytest.fixture(scope="module")
def m16(sd):
    return make_model(sd, precision="f16x3")


@pytest.fixture(scope="module")
def m32(sd):
    return make_model(sd, precision="fp32")


@pytest.fixture(scope="module")
def tiles48():
    return np.random.default_rng(5).random((48, 32, 32), dtype=np.float32)


# ---- 1. scattered coordinates --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("act", ["sine", "morlet"])
def test_scattered_coordinates_vs_oracle(act, prec):
    sd = syn.make_state_dict(seed=7, trained_like=True)
    m = make_model(sd, act=act, precision=prec)
    mods = syn.make_mods(2, L, 9, 256)
    for Q in (77, 1, 33):
        coords = scattered(Q, seed=Q)
        out = m.sample_mods(mods, coords)
        assert out.shape == (9, Q)
        check(out, ref_mods(sd, mods, coords, act=act), what=f"scattered {prec} {act} Q={Q}")


def test_largest_coordinate_set(sd, m16, m32):
    """Q = 65 536, the bound: 2 048 units per patch, a 64 MB table -- the index arithmetic of the trunks at its largest P."""
    coords = scattered(65536, seed=8)
    mods = syn.make_mods(3, L, 3, 256)
    ref = ref_mods(sd, mods, coords, chunk=1)
    for m in (m16, m32):
        out = m.sample_mods(mods, coords)
        check(out, ref, what=f"Q=65536 {m.precision}")
        assert np.array_equal(out[:, :77], m.sample_mods(mods, coords[:77]))  # a coordinate's value does not depend on the set around it


# ---- 2. lattices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [8, 32, 48])
def test_lattices_vs_oracle_and_the_scaled_pipelines_trunk_step(sd, m16, tiles48, stride):
    grid = m16.upsampled_grid(stride)
    T = 24 * stride // 16
    assert grid.shape == (T * T, 2)
    out = m16.sample(tiles48, grid)
    ref = ref_tiles(sd, tiles48, grid)
    check(out, ref, what=f"lattice I'={stride} B=48")
    small = m16.sample(tiles48[:3], grid)
    if stride == 8:
        assert "f16x3h" in m16.last_trunk_kernel(), m16.last_trunk_kernel()  # 3 x 5 units: the half-unit instance
    check(small, ref[:3], what=f"lattice I'={stride} B=3")
    # the scaled pipeline = tiling -> this trunk step -> fold: its reconstruction of 6 x 8 non-black tiles is the fold of `out`
    d_t = m16.device_array(out.shape).copy_from(out)
    d_r = m16.device_array((1, 6 * stride, 8 * stride))
    _lib.check(m16._lib.msiren_weighted_fold_scaled_dev(m16._h, d_t.ptr, 1, 6, 8, stride, d_r.ptr))
    m16.sync()
    pipe = harness.reconstruct_from_patches(m16, tiles48, [(6, 8)], out_stride=stride)
    assert pipe.shape == (1, 6 * stride, 8 * stride)
    assert np.array_equal(pipe, d_r.numpy())


# ---- 3. the x3 lattice contains the native grid --------------------------------------------------------------------------------
def test_x3_lattice_contains_the_native_grid(m16, m32, tiles48):
    for m in (m16, m32):
        x3 = m.sample(tiles48, m.upsampled_grid(48)).reshape(48, 72, 72)[:, 1::3, 1::3]
        native = m(tiles48)
        e = nerr(x3, native)
        print(f"x3[1::3, 1::3] vs native ({m.precision}): nerr {e:.3e}")
        assert e <= 1e-4, e


# ---- 4. the model's own grid ---------------------------------------------------------------------------------------------------
def test_own_grid(sd, m16, m32, tiles48):
    assert np.array_equal(m32.sample(tiles48, m32.grid).reshape(48, 24, 24), m32(tiles48))  # same kernel, same coordinates
    out = m16.sample(tiles48, m16.grid)
    check(out, ref_tiles(sd, tiles48, m16.grid), what="own grid f16x3")
    native = m16(tiles48).reshape(48, -1)
    differing = int((out != native).sum())
    print(f"own grid, f16x3: device-built against committed layer-0 table: max|diff| {np.abs(out - native).max():.3e}, "
          f"{differing} of {out.size} outputs differ")


# ---- 5. invariance, bit for bit ------------------------------------------------------------------------------------------------
def test_invariance(m16, m32, tiles48):
    coords = scattered(333, seed=9)
    for m in (m16, m32):
        a = np.array(m.sample(tiles48, coords))
        assert np.array_equal(a, m.sample(tiles48, coords))                      # the same call twice
        for k in (1, 7, 29):
            assert np.array_equal(a[:k], m.sample(tiles48[:k], coords)), k       # a batch against its pieces
        d_t = m.device_array(tiles48.shape).copy_from(tiles48)
        d_c = m.device_array(coords.shape).copy_from(coords)
        for n in (1, 2, 3):                                                      # 1 / 2 / 3 streams, the _dev form
            _lib.check(m._lib.msiren_set_streams(m._h, n))
            outs = [m.sample(d_t, d_c) for _ in range(n + 1)]
            for o in outs:
                assert o.shape == (48, 333) and np.array_equal(o.numpy(), a), n  # ... and the host-pointer form against it
        _lib.check(m._lib.msiren_set_streams(m._h, 1))
        assert np.array_equal(m.sample(tiles48, d_c), a)                         # coordinates as numpy against a DeviceArray
        assert np.array_equal(m.sample(d_t, coords).numpy(), a)
        pt, pc = m.pinned_empty(tiles48.shape), m.pinned_empty(coords.shape)     # page-locked against pageable caller buffers
        pt[...] = tiles48
        pc[...] = coords
        assert np.array_equal(m.sample(pt, pc), a)
        m.pin_outputs(False)
        try:
            assert np.array_equal(m.sample(tiles48, coords), a) and np.array_equal(m.sample(pt, coords), a)
        finally:
            m.pin_outputs(True)


def test_two_coordinate_sets_alternate_on_two_streams(m16, tiles48):
    m = m16
    ca, cb = scattered(500, seed=1), scattered(123, seed=2)
    want = {0: np.array(m.sample(tiles48, ca)), 1: np.array(m.sample(tiles48, cb))}
    d_t = m.device_array(tiles48.shape).copy_from(tiles48)
    d_c = [m.device_array(ca.shape).copy_from(ca), m.device_array(cb.shape).copy_from(cb)]
    _lib.check(m._lib.msiren_set_streams(m._h, 2))
    try:
        outs = [m.device_array((48, (500, 123)[i % 2])) for i in range(6)]
        for i, o in enumerate(outs):  # A B A B A B back to back, no sync: each stream's table is rebuilt in stream order
            _lib.check(m._lib.msiren_sample_tiles_dev(m._h, d_c[i % 2].ptr, d_c[i % 2].shape[0], d_t.ptr, 48, o.ptr))
        # and with the sets swapped between the streams (three calls shift the rotation by one)
        more = [m.device_array((48, (123, 500)[i % 2])) for i in range(3)]
        for i, o in enumerate(more):
            _lib.check(m._lib.msiren_sample_tiles_dev(m._h, d_c[(i + 1) % 2].ptr, d_c[(i + 1) % 2].shape[0], d_t.ptr, 48, o.ptr))
        m.sync()
        for i, o in enumerate(outs):
            assert np.array_equal(o.numpy(), want[i % 2]), i
        for i, o in enumerate(more):
            assert np.array_equal(o.numpy(), want[(i + 1) % 2]), i
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))


# ---- 6. domain guard -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", [1e5, 3e7])
def test_domain_guard_reruns_at_the_calls_coordinates(mod):
    """The recipe of test_f16x3_domain_identical_to_fp32_outside_it (tests/test_gpu_ws.py): modulations beyond what fp16 carries."""
    B = 40
    sd = syn.make_state_dict(seed=11, with_encoder=False)
    sd = {k: v for k, v in sd.items() if not k.startswith("modulator")}
    m = make_model(sd, encoder_type="other", strict=False, precision="f16x3")
    f = make_model(sd, encoder_type="other", strict=False, precision="fp32")
    mods = (syn.make_mods(5, L, B, 256) * np.float32(mod)).astype(np.float32)
    for Q in (77, 640):
        coords = scattered(Q, seed=4)
        want = f.sample_mods(mods, coords)
        assert np.isfinite(want).all()
        e0 = range_events(m)
        got = m.sample_mods(mods, coords)                                       # host form: the flag is read on the host (HostCheck)
        assert range_events(m) > e0, "the recipe no longer leaves the fp16 domain"
        assert np.array_equal(got, want)
        d_m, d_c = m.device_array(mods.shape).copy_from(mods), m.device_array(coords.shape).copy_from(coords)
        for n in (1, 2):                                                         # _dev form: the conditional launch on the stream
            _lib.check(m._lib.msiren_set_streams(m._h, n))
            assert np.array_equal(m.sample_mods(d_m, d_c).numpy(), want), n
        _lib.check(m._lib.msiren_set_streams(m._h, 1))
        inside = syn.make_mods(6, L, 7, 256)                                     # an in-domain call afterwards is the trunk's own
        check(m.sample_mods(inside, coords), ref_mods(sd, inside, coords), what=f"in-domain after flagged Q={Q}")


# ---- 7. a non-finite coordinate ------------------------------------------------------------------------------------------------
def test_nonfinite_coordinate_stays_where_it_is(m16, m32, tiles48):
    coords = scattered(40, seed=6)
    bad = coords.copy()
    bad[17, 1] = np.nan
    for m in (m16, m32):
        for B in (48, 5):
            clean, out = np.array(m.sample(tiles48[:B], coords)), np.array(m.sample(tiles48[:B], bad))
            assert not np.isfinite(out[:, 17]).any()
            keep = np.arange(40) != 17
            assert np.array_equal(out[:, keep], clean[:, keep]), (m.precision, B)


# ---- 8. the scaled pipeline ----------------------------------------------------------------------------------------------------
def oracle_scaled(sd, img, stride):
    T = 24 * stride // 16
    patches, info = orc.image_to_patches(np.asarray(img, dtype=np.float32), 32, 16)
    kept, black, shape = orc.filter_and_remember_black_patches(patches)
    lin = lattice_formula(stride)
    grid = np.stack(np.meshgrid(lin, lin, indexing="ij"), axis=-1).reshape(-1, 2)
    rec = ref_tiles(sd, kept, grid).reshape(-1, T, T).astype(np.float32)
    rec = orc.reintegrate_black_patches(rec, black, shape)
    return orc.patches_to_image_weighted_average(rec, info, T, stride), len(black), shape[0]


def lattice_formula(stride, S=24, I=16):
    d = np.float64(2.0) / np.float64(S - 1)
    r = np.float64(stride) / np.float64(I)
    j = np.arange(S * stride // I, dtype=np.float64)
    return ((np.float64(-1.0) - d / np.float64(2.0)) + (d / r) * (j + np.float64(0.5))).astype(np.float32)


@pytest.mark.parametrize("stride", [8, 32, 48])
def test_scaled_reconstruction_vs_oracle_chain(sd, m16, m32, stride):
    img = syn.make_slice(3, 128, 112, brain_mask=True)
    ref, nblack, ntiles = oracle_scaled(sd, img, stride)
    assert (ntiles, nblack) == (56, 8)
    assert np.array_equal(m16.upsampled_grid(stride)[:24 * stride // 16, 1], lattice_formula(stride))
    for m in (m16, m32):
        out = m.reconstruct(img, out_stride=stride)
        assert out.shape == (8 * stride, 7 * stride)
        check(out, ref, what=f"scaled recon I'={stride} {m.precision}")


def test_scaled_reconstruction_ragged_image_and_batches(sd, m16):
    img = syn.make_slice(4, 70, 50)
    for stride in (8, 32):
        ref, _, _ = oracle_scaled(sd, img, stride)
        out = m16.reconstruct(img, out_stride=stride)
        assert out.shape == (5 * stride, 4 * stride)
        check(out, ref, what=f"scaled recon 70x50 I'={stride}")
    imgs = np.stack([syn.make_slice(k, 128, 112, brain_mask=True) for k in (3, 5, 6)])
    batch = np.array(m16.reconstruct(imgs, out_stride=32))
    assert batch.shape == (3, 256, 224)
    for k in range(3):
        assert np.array_equal(batch[k], m16.reconstruct(imgs[k], out_stride=32)), k
    # the *_dev form on two streams
    d_i = m16.device_array(imgs.shape).copy_from(imgs)
    _lib.check(m16._lib.msiren_set_streams(m16._h, 2))
    try:
        outs = [m16.device_array(batch.shape) for _ in range(3)]
        for o in outs:
            _lib.check(m16._lib.msiren_reconstruct_slices_scaled_dev(m16._h, d_i.ptr, 3, 128, 112, 32, o.ptr))
        m16.sync()
        for o in outs:
            assert np.array_equal(o.numpy(), batch)
    finally:
        _lib.check(m16._lib.msiren_set_streams(m16._h, 1))


@pytest.mark.parametrize("stride", [8, 32, 48])
def test_scaled_fold_alone_vs_oracle_fold(m16, stride):
    T, nV, nH = 24 * stride // 16, 3, 4
    tiles = np.random.default_rng(stride).standard_normal((2 * nV * nH, T, T)).astype(np.float32)
    d_t = m16.device_array(tiles.shape).copy_from(tiles)
    d_r = m16.device_array((2, nV * stride, nH * stride))
    _lib.check(m16._lib.msiren_weighted_fold_scaled_dev(m16._h, d_t.ptr, 2, nV, nH, stride, d_r.ptr))
    m16.sync()
    got = d_r.numpy()
    for s in range(2):
        ref = orc.patches_to_image_weighted_average(tiles[s * nV * nH:(s + 1) * nV * nH], (nV, nH), T, stride)
        e = nerr(got[s], ref)
        print(f"scaled fold I'={stride}: nerr {e:.3e}")
        assert e < 1e-6, e


# ---- 9. out_stride = I is the existing path -----------------------------------------------------------------------------------
def test_native_stride_is_the_existing_path(m16, m32):
    img = syn.make_slice(3, 128, 112, brain_mask=True)
    for m in (m16, m32):
        assert np.array_equal(m.reconstruct(img, out_stride=16), m.reconstruct(img))
        patches, info = orc.image_to_patches(img, 32, 16)
        assert np.array_equal(harness.reconstruct_from_patches(m, patches, [info], out_stride=16),
                              harness.reconstruct_from_patches(m, patches, [info]))


# ---- 10. re-commit -------------------------------------------------------------------------------------------------------------
def test_recommit_drops_the_kept_tables(sd):
    m = make_model(sd, precision="f16x3")
    img = syn.make_slice(4, 70, 50)
    first = np.array(m.reconstruct(img, out_stride=32))
    check(first, oracle_scaled(sd, img, 32)[0], what="before re-commit")
    sd2 = syn.make_state_dict(seed=8, trained_like=True)
    m.load_state_dict(sd2)
    second = np.array(m.reconstruct(img, out_stride=32))
    check(second, oracle_scaled(sd2, img, 32)[0], what="after re-commit")
    assert not np.array_equal(first, second)


# ---- 11. errors ----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable(sd, m16, tiles48):
    m, tiles = m16, tiles48[:4]
    good = scattered(10)
    with pytest.raises(ValueError):
        m.sample(tiles, np.zeros((0, 2), np.float32))
    with pytest.raises(ValueError):
        m.sample(tiles, np.zeros((65537, 2), np.float32))
    with pytest.raises(ValueError):
        m.sample(tiles, np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError):
        m.reconstruct(syn.make_slice(4, 70, 50), out_stride=6)
    # the library's own checks (the Python layer raises before it gets there)
    d_t, d_c = m.device_array(tiles.shape).copy_from(tiles), m.device_array((65537, 2))
    d_o = m.device_array((4, 10))
    out = np.empty((4, 10), np.float32)
    for Q in (0, 65537):
        assert m._lib.msiren_sample_tiles(m._h, good.ctypes.data, Q, tiles.ctypes.data, 4, out.ctypes.data) == _lib.E_INVALID
        assert m._lib.msiren_sample_tiles_dev(m._h, d_c.ptr, Q, d_t.ptr, 4, d_o.ptr) == _lib.E_INVALID
        assert str(Q) in _lib.last_error()
    d_i = m.device_array((1, 70, 50))
    assert m._lib.msiren_reconstruct_slices_scaled_dev(m._h, d_i.ptr, 1, 70, 50, 6, d_o.ptr) == _lib.E_INVALID
    assert all(s in _lib.last_error() for s in ("6", "24", "16")), _lib.last_error()
    m.sync()
    # B = 0 and n = 0 do nothing
    assert m.sample(tiles[:0], good).shape == (0, 10)
    assert m._lib.msiren_reconstruct_slices_scaled_dev(m._h, None, 0, 70, 50, 32, None) == 0
    check(m.sample(tiles, good), ref_tiles(sd, tiles, good), what="after the errors")


def test_net_still_refuses_foreign_coordinates(m16):
    mods = syn.make_mods(2, L, 2, 256)
    with pytest.raises(ValueError, match="sample_mods"):
        m16.net(scattered(576).reshape(1, 576, 2).repeat(2, 0), mods)


# ---- 12. H = 512 ---------------------------------------------------------------------------------------------------------------
def test_h512_bf16_handle_vs_own_oracle():
    H, L3, Z, B = 512, 3, 128, 9
    sd = syn.make_state_dict(seed=21, dim_hidden=H, num_layers=L3, latent_dim=Z, with_encoder=False)
    sd = {k: v for k, v in sd.items() if not k.startswith("modulator")}
    m = make_model(sd, H=H, L=L3, Z=Z, strict=False, precision="bf16")
    mods = syn.make_mods(8, L3, B, H, lo=0.1, hi=0.6)
    coords = scattered(100, seed=12)
    out = m.sample_mods(mods, coords)
    assert "x1w" in m.last_trunk_kernel()
    ref = ref_mods(sd, mods, coords, num_layers=L3)
    e = nerr(out, ref)
    print(f"bf16 H=512 L=3 Q=100: nerr {e:.3e}")
    assert np.isfinite(out).all() and e <= 6e-2, e
    assert np.array_equal(out, m.sample_mods(mods, coords))
