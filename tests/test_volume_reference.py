"""tests/volume_reference.py, tests/volume_cases.py and mri_inr_amd.volume.plane_points on the CPU: the semantics of msiren_resample_volume*
 against tests/resample_reference.py slice by slice."""
import numpy as np
import pytest

import resample_reference as rr
import volume_cases as vc
import volume_reference as vr
from mri_inr_amd import plane_points


def slice_reference(s, yx):
    mods, black = vc.stack_mods("float64")
    return rr.resample(vc.full_sd(), mods[s], black[s], yx, vc.NV, vc.NH, vc.S, vc.I, num_layers=vc.L)


def test_integer_z_is_the_slice_exactly():
    yx = np.random.default_rng(0).uniform(vc.LO, vc.HI, size=(12, 2)).astype(np.float32)
    for s in range(vc.N):
        pts = np.concatenate([np.full((len(yx), 1), s, np.float32), yx], axis=1)
        val, grad = vc.reference(pts)
        want_v, want_g = slice_reference(s, yx)
        assert np.array_equal(val, want_v) and np.array_equal(grad[1:], want_g), s
        lo, hi = min(s, vc.N - 2), min(s, vc.N - 2) + 1  # the segment that contains Z; at an interior integer the one to its right
        assert np.array_equal(grad[0], slice_reference(hi, yx)[0] - slice_reference(lo, yx)[0]), s
    one, none = vr.volume(lambda s, p: slice_reference(2, p), np.concatenate([np.zeros((len(yx), 1), np.float32), yx], axis=1), 1)
    assert np.array_equal(one, slice_reference(2, yx)[0]) and none is None  # n = 1: the value alone


def test_linear_between_slices_and_the_z_slope_is_a_central_difference():
    rng = np.random.default_rng(1)
    yx = rng.uniform(0.0, 40.0, size=(10, 2)).astype(np.float32)
    for seg in range(vc.N - 1):
        z = (seg + rng.integers(8, 57, len(yx)) / 64.0).astype(np.float32)  # (multiples of 1 / 64: Z +- h is exact in fp32)
        h = np.float32(1 / 16)
        val, grad = vc.reference(np.column_stack([z, yx]))
        up, _ = vc.reference(np.column_stack([z + h, yx]))
        dn, _ = vc.reference(np.column_stack([z - h, yx]))
        r0, r1 = slice_reference(seg, yx)[0], slice_reference(seg + 1, yx)[0]
        f = z.astype(np.float64) - seg
        assert np.abs(val - ((1 - f) * r0 + f * r1)).max() <= 1e-12
        assert np.abs(grad[0] - (up - dn) / (2 * float(h))).max() <= 1e-12 * 16
        g0, g1 = slice_reference(seg, yx)[1], slice_reference(seg + 1, yx)[1]
        assert np.abs(grad[1:] - ((1 - f) * g0 + f * g1)).max() <= 1e-12


def test_nan_rules():
    below, above = np.nextafter(np.float32(0), np.float32(-np.inf)), np.nextafter(np.float32(vc.N - 1), np.float32(np.inf))
    pts = np.array([[below, 20, 20], [above, 20, 20], [np.nan, 20, 20], [1.5, -10, 5], [1.5, np.nan, 5], [1.5, 20, 20], [0, 20, 20], [vc.N - 1, 20, 20]], np.float32)
    val, grad = vc.reference(pts)
    assert np.isnan(val[:5]).all() and np.isnan(grad[:, :5]).all()
    assert np.isfinite(val[5:]).all() and np.isfinite(grad[:, 5:]).all()
    z0, f = vr.pairs(pts, vc.N)
    assert z0.tolist() == [-1, -1, -1, 1, 1, 1, 0, vc.N - 2] and f[5:].tolist() == [0.5, 0.0, 1.0]
    assert vr.slices_read(pts, vc.N, value_form=True)[5:] == [[1, 2], [0], [vc.N - 1]] and vr.slices_read(pts, vc.N)[6:] == [[0, 1], [vc.N - 2, vc.N - 1]]


def test_a_draw_exists_and_its_bins_are_what_the_manifest_says():
    d = vc.data()
    pts, parts = d["points"], d["parts"]
    print("points", len(pts), "draw", d["draw"], "floor", d["floor"], "gate", d["gate"])
    assert 300 <= len(pts) <= 400 and pts.dtype == np.float32 and pts.shape[1] == 3
    assert d["black"] == [[], [0, 1, 2], [], list(range(vc.NPT))]
    inv = parts["invalid"]
    assert inv.stop == len(pts) and (~d["finite"]).sum() == inv.stop - inv.start and not d["finite"][inv].any()
    assert np.isnan(d["grad"][:, inv]).all() and np.isfinite(d["grad"][:, :inv.start]).all()
    for value_form in (True, False):
        counts = vc.bin_counts(pts, value_form)
        print("value form" if value_form else "gradient form", counts.reshape(vc.N, vc.NPT).tolist())
        assert counts[vc.PILE_BIN] > 128 and all(counts[b] == 0 for b in vc.EMPTY_BINS), counts
        assert (np.delete(counts, vc.EMPTY_BINS) > 0).sum() >= 30
    z = pts[:inv.start, 0]
    f = z - np.floor(z)
    for seg in range(vc.N - 1):  # integer and fractional Z in every segment, the ends of the stack exactly
        assert ((z > seg) & (z < seg + 1)).sum() >= 5 and (z == seg).sum() >= 2
    assert (z == vc.N - 1).sum() >= 2 and ((f != 0) & (f * 64 == np.floor(f * 64))).sum() >= 10
    w = pts[parts["window"]]
    assert len(w) == 144 and np.all(w == np.round(w)) and len(set(w[:, 0])) == 1
    # a point under the black slice alone, under black tiles alone, and next to the black slice
    b = parts["black"]
    assert np.all(d["value"][b][:4] == 0) and np.all(d["grad"][1:, b][:, :4] == 0) and np.all(d["value"][b][4:] != 0)


def test_plane_points():
    p = plane_points((1.0, 2.0, 3.0), (0.5, 1.0, 0.0), (0.0, 0.0, 2.0), (3, 4))
    assert p.shape == (12, 3) and p.dtype == np.float32
    assert p[0].tolist() == [1.0, 2.0, 3.0] and p[1].tolist() == [1.0, 2.0, 5.0] and p[4].tolist() == [1.5, 3.0, 3.0] and p[11].tolist() == [2.0, 4.0, 9.0]
    # formed in fp64, rounded once
    o, u, v = np.array([0.1, 0.2, 0.3]), np.array([1 / 3, 1 / 7, 1 / 9]), np.array([1 / 11, 1 / 13, 1 / 17])
    q = plane_points(o, u, v, (5, 6))
    want = np.array([o + i * u + j * v for i in range(5) for j in range(6)]).astype(np.float32)
    assert np.array_equal(q, want)
    assert plane_points(o, u, v, (0, 6)).shape == (0, 3)
    with pytest.raises(ValueError):
        plane_points((0, 0), u, v, (2, 2))
