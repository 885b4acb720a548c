"""Geometry and lattice of an output stride (msiren_upsampled_geometry / msiren_upsampled_lattice): handle-free,
no device.  S' = S I'/I, pad' = (S' - I')/2, lin'[j] = (-1 - d/2) + (d/r)(j + 1/2) with d = 2/(S-1), r = I'/I in fp64, rounded once."""
import ctypes as C
import os

import numpy as np
import pytest

from mri_inr_amd import ModulatedSiren, _lib
from oracle import siren_oracle as orc


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def geometry(lib, S, I, stride):
    tile, pad = C.c_int32(-1), C.c_int32(-1)
    rc = lib.msiren_upsampled_geometry(S, I, stride, C.byref(tile), C.byref(pad))
    return rc, tile.value, pad.value


def lattice(lib, S, I, stride):
    rc, tile, _ = geometry(lib, S, I, stride)
    assert rc == 0
    lin = np.full(tile, np.nan, dtype=np.float32)
    assert lib.msiren_upsampled_lattice(S, I, stride, lin.ctypes.data) == 0
    return lin


def formula(S, I, stride):
    """Section 1 of the definition, each fp64 operation rounded on its own, one rounding to fp32."""
    d = np.float64(2.0) / np.float64(S - 1)
    r = np.float64(stride) / np.float64(I)
    tile = S * stride // I
    j = np.arange(tile, dtype=np.float64)
    return ((np.float64(-1.0) - d / np.float64(2.0)) + (d / r) * (j + np.float64(0.5))).astype(np.float32)


@pytest.mark.parametrize("stride,tile,pad", [(32, 48, 8), (48, 72, 12), (8, 12, 2), (16, 24, 4)])
def test_geometry(lib, stride, tile, pad):
    assert geometry(lib, 24, 16, stride) == (0, tile, pad)


@pytest.mark.parametrize("stride", [2, 6])
def test_geometry_rejects_fractional_tile_or_padding(lib, stride):
    rc, _, _ = geometry(lib, 24, 16, stride)
    assert rc == _lib.E_INVALID
    msg = lib.msiren_last_error().decode()
    assert str(stride) in msg and "24" in msg and "16" in msg, msg
    assert lib.msiren_upsampled_lattice(24, 16, stride, np.zeros(64, np.float32).ctypes.data) == _lib.E_INVALID


@pytest.mark.parametrize("stride", [8, 16, 32, 48])
def test_lattice_is_the_formula_bit_for_bit(lib, stride):
    got, want = lattice(lib, 24, 16, stride), formula(24, 16, stride)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("stride", [4, 8, 12, 16, 20, 24, 32, 48, 64])
def test_lattice_is_symmetric_about_zero(lib, stride):
    lin = lattice(lib, 24, 16, stride)
    assert np.array_equal(lin, -lin[::-1])


def test_x3_lattice_contains_the_native_grid(lib):
    lin = lattice(lib, 24, 16, 48)
    native = orc.linspace_f32(-1, 1, 24)
    assert lin.shape == (72,)
    assert np.abs(lin[1::3].astype(np.float64) - np.asarray(native, dtype=np.float64)).max() <= 1.2e-7
    assert abs(abs(float(lin[0])) - 1.029) < 1e-3  # the end points lie slightly outside +-1


def test_upsampled_grid_has_ij_order():
    m = ModulatedSiren(2, 256, 1, 5, 256, 1.0, 30.0, True, 0.1, True, "custom", None, 32, 16, 24, "cpu", "sine")
    lib_ = _lib.load()
    for stride in (8, 32, 48):
        g = m.upsampled_grid(stride)
        lin = lattice(lib_, 24, 16, stride)
        T = len(lin)
        assert g.shape == (T * T, 2) and g.dtype == np.float32
        want = np.stack(np.meshgrid(lin, lin, indexing="ij"), axis=-1).reshape(-1, 2)
        assert np.array_equal(g, want)
        assert np.array_equal(g[:T, 0], np.full(T, lin[0])) and np.array_equal(g[:T, 1], lin)  # column 0 = row coordinate
    with pytest.raises(ValueError):
        m.upsampled_grid(6)
