"""CPU checks of tests/geometry_cases.py (no GPU): the geometries are what its table says, the black tiles are where its docstring says, the points
reach every cover count, leave one bin empty and pile one past 128 entries, and the gates of tests/test_gpu_geometry.py reject the transpositions and
truncations a kernel could make unnoticed on a 3 x 3 square slice with KA = 2 (MUTANTS), each evaluated with the fp64 reference itself.  The
reference's own floors per geometry are printed.
"""
import numpy as np
import pytest

import align_cases as ac
import geometry_cases as gcs
import resample_reference as rr
from mri_inr_amd import align, align_volume as av
from oracle import siren_oracle as orc

GEOS = list(gcs.GEOMETRIES)
TABLE = {"rect": (16, 24, 4, 2, (40, 72), (3, 5)), "ka3": (8, 24, 8, 3, (40, 56), (5, 7)), "ka4": (8, 32, 12, 4, (40, 56), (5, 7)),
         "ka1": (32, 32, 0, 1, (40, 72), (2, 3))}


@pytest.mark.parametrize("name", GEOS)
def test_tile_grid_pad_ka_and_black_tiles(name):
    geo = gcs.GEOMETRIES[name]
    I, S, pad, KA, hw, tiles = TABLE[name]
    assert (geo.I, geo.S, geo.pad, geo.KA, (geo.height, geo.width), (geo.nV, geo.nH)) == (I, S, pad, KA, hw, tiles)
    assert geo.nV != geo.nH and geo.K == KA * KA and gcs.EXPECTED[name] == dict(pad=pad, KA=KA)
    img = gcs.images(name)
    assert img.shape == (gcs.N,) + hw
    found = []
    for s in range(gcs.N):
        patches, info = orc.image_to_patches(img[s], gcs.O, I)
        assert info == tiles  # what the oracle's tiling returns, not the table
        found.append(orc.filter_and_remember_black_patches(patches)[1])
    # slice 0 none, slice 1 its tile COLUMN 0, slice 2 its tile ROW 0: each the other's transpose, and different because nV != nH
    assert found == gcs.black_tiles(geo) == [[], [v * geo.nH for v in range(geo.nV)], list(range(geo.nH))]
    assert found == gcs.stack_mods(name, "sine5", "float64")[1]
    assert sorted(h * geo.nV + v for v in range(geo.nV) for h in range(geo.nH) if v * geo.nH + h in found[1]) != found[1]


@pytest.mark.parametrize("name", GEOS)
def test_points_are_what_the_cases_say(name):
    geo, d = gcs.GEOMETRIES[name], gcs.data(name)
    pts, parts = d["points"], d["parts"]
    per_tile, per_point = gcs.per_tile_counts(name, pts)
    print(f"{name}: M {len(pts)} draw {d['draw']} covers per tile {per_tile.tolist()}")
    print(f"{name}: floor of the values {d['value_floor'][0]:.2e} / {d['value_floor'][1]:.2e}, of the gradients {d['floor'][0]:.2e} / {d['floor'][1]:.2e}, "
          f"gate {d['gate'][0]:.2e} / {d['gate'][1]:.2e}")
    assert 300 <= len(pts) <= 380
    assert max(per_point) == geo.KA ** 2
    want = {a * b for a in range(1, geo.KA + 1) for b in range(1, geo.KA + 1)}
    inside = set(np.array(per_point)[:parts["outside"].start].tolist())
    assert inside == (want | {0} if name == "ka1" else want), inside
    assert per_tile[gcs.tile(geo, *gcs.EMPTY)] == 0 and (np.delete(per_tile, gcs.tile(geo, *gcs.EMPTY)) > 0).all()
    assert per_tile[gcs.tile(geo, *geo.pile)] > 128
    # windows: integer pixels inside the reconstruction, across a seam of their axis, at the far end of the other
    wy, wx = pts[parts["window_y"]], pts[parts["window_x"]]
    for w in (wy, wx):
        assert np.array_equal(w, np.round(w)) and (w >= 0).all() and (w[:, 0] < geo.nV * geo.I).all() and (w[:, 1] < geo.nH * geo.I).all()
    assert wy[:, 0].min() < geo.I <= wy[:, 0].max() and wy[:, 1].min() >= (geo.nH - 1) * geo.I
    assert wx[:, 1].min() < (geo.nH - 1) * geo.I <= wx[:, 1].max() and wx[:, 0].min() >= (geo.nV - 1) * geo.I
    # every exact cover edge of both axes, and the corners of the last tile row and the last tile column
    ends_y = {float(v * geo.I - geo.pad + e) for v in range(geo.nV) for e in (0, geo.S - 1)}
    ends_x = {float(h * geo.I - geo.pad + e) for h in range(geo.nH) for e in (0, geo.S - 1)}
    edges, corners = pts[parts["edges"]], pts[parts["corners"]]
    assert ends_y <= set(edges[:, 0].tolist()) and ends_x <= set(edges[:, 1].tolist())
    last_row, last_col = gcs.tile(geo, geo.nV - 1, 0), gcs.tile(geo, 0, geo.nH - 1)
    cov = rr.covers(corners, geo.nV, geo.nH, geo.S, geo.I)
    assert all(last_row in [t for t, _, _ in lst] for lst in cov[:4]) and all(last_col in [t for t, _, _ in lst] for lst in cov[4:]) and last_row != last_col
    # outside, inf and NaN are NaN; on ka1 so are the points strictly between two covers
    assert not d["finite"][parts["outside"]].any() and d["finite"][:parts["between"].start].sum() >= 280
    if name == "ka1":
        assert len(pts[parts["between"]]) == 4 and not d["finite"][parts["between"]].any()
        assert np.isfinite(pts[parts["between"]]).all() and (pts[parts["between"]] > geo.lo).all()
    else:
        assert d["finite"][:parts["outside"].start].all()
    # a point under black tiles only is zero in the reference, and only in its slice
    only_col0 = d["finite"] & (pts[:, 1] < geo.I - geo.pad)
    only_row0 = d["finite"] & (pts[:, 0] < geo.I - geo.pad)
    assert only_col0.sum() >= 3 and only_row0.sum() >= 3
    assert not d["value"][1, only_col0].any() and d["value"][0, only_col0].all() and d["value"][2, only_col0 & ~only_row0].all()
    assert not d["value"][2, only_row0].any() and d["value"][0, only_row0].all() and d["value"][1, only_row0 & ~only_col0].all()


@pytest.mark.parametrize("name", GEOS)
def test_volume_points_are_what_the_cases_say(name):
    geo, d = gcs.GEOMETRIES[name], gcs.data3(name)
    pts, parts = d["points"], d["parts"]
    print(f"{name}: M {len(pts)} draw {d['draw']} floor of the values {d['value_floor'][0]:.2e} / {d['value_floor'][1]:.2e}, of grad[1:] {d['floor'][0]:.2e} / "
          f"{d['floor'][1]:.2e}, gate {d['gate'][0]:.2e} / {d['gate'][1]:.2e}")
    z = pts[:parts["invalid_z"].start, 0]
    assert {0.0, 0.5, 1.0, 1.5, 2.0} <= set(z.tolist()) and ((z != np.round(2 * z) / 2) & np.isfinite(z)).sum() >= 30
    assert not d["finite"][parts["invalid_z"]].any() and np.isnan(d["grad"][:, parts["invalid_z"]]).all()
    for value_form in (True, False):
        counts = gcs.bin_counts3(name, pts, value_form)
        empty = [s * geo.NPt + gcs.tile(geo, *gcs.EMPTY) for s in range(gcs.N)]
        assert not counts[empty].any() and counts[1 * geo.NPt + gcs.tile(geo, *geo.pile)] > 128
    assert d["black"] == gcs.black_tiles(geo)


@pytest.mark.parametrize("name,mutant", [(g, m) for g in GEOS for m in gcs.MUTANTS if gcs.mutant_applies(g, m)])
def test_the_gate_rejects_every_mutant(name, mutant):
    d = gcs.data(name)
    why = gcs.outside_the_gate(d, *gcs.mutant_slices(name, mutant, d["points"]))
    print(f"{name} {mutant}: {why}")
    assert why is not None


@pytest.mark.parametrize("name", GEOS)
def test_the_mutants_apply_where_they_can_differ_and_none_is_the_reference(name):
    applied = {m for m in gcs.MUTANTS if gcs.mutant_applies(name, m)}
    assert applied >= {"tiles_h_nV_v", "cover_nV_nH_exchanged", "black_transposed"}
    assert ("slots_truncated" in applied) == (name in ("ka3", "ka4")) and ("pad_4" in applied) == (name != "rect")
    d = gcs.data(name)
    assert gcs.outside_the_gate(d, *gcs.mutant_slices(name, None, d["points"])) is None  # the construction without a mutant is inside the gate


@pytest.mark.parametrize("name", GEOS)
def test_the_lattices_lie_across_the_long_axis(name):
    geo, shape = gcs.GEOMETRIES[name], (19, 23)
    cols2, cols3 = set(), set()
    for row in gcs.maps2(name, shape):
        cols2 |= {t % geo.nH for lst in rr.covers(align.map_points(row, shape), geo.nV, geo.nH, geo.S, geo.I) for t, _, _ in lst}
    for row in gcs.maps3(name, shape):
        cols3 |= {t % geo.nH for lst in rr.covers(av.map_points3(row, shape)[:, 1:], geo.nV, geo.nH, geo.S, geo.I) for t, _, _ in lst}
    want = {3, 4} if name == "rect" else {geo.nH - 2, geo.nH - 1}
    assert want <= cols2 and want <= cols3 and 0 not in cols2 | cols3, (cols2, cols3)
    assert gcs.maps2(name, shape).shape == (gcs.N, 6) and gcs.maps3(name, shape).shape == (gcs.M3, 9) and gcs.targets3(shape).shape == (gcs.M3,) + shape


def test_the_sums_gates_of_one_lattice_case():
    """the alignment cases build and their gates sit inside the cap (ka1: the cheapest; the GPU tests build the others)"""
    d2, d3 = gcs.align_data("ka1", "sine5", (19, 23)), gcs.align_volume_data("ka1", "sine5", (19, 23))
    for fam, d in list(d2.items()) + list(d3.items()):
        print(f"ka1 {fam}: counts {d['sums'][:, 0].astype(int).tolist()} D {d['D']:.2e} gate {d['gate']:.2e}")
        assert 0 < d["gate"] < ac.CAP and gcs.accepts(d, d["variant"]) and (d["sums"][:, 0] > 0).any()
    assert 0 < d2["plain"]["sums"][:, 0].min() < 19 * 23 and d3["r"]["sums"][2, 0] == 0  # uncovered pixels; a NaN scale scores nothing
