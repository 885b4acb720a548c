"""msiren_fuse_targets on the CPU (no GPU needed): the normative restatement mri_inr_amd/fuse.py: fuse_on_host against the
independent formulation of tests/fuse_reference.py, the properties the rule promises, how close the fused stack is to the truth, seeded mutants of the
rule, and fuse_plan.h (what the call refuses, its tiling and scratch) in a stand-alone compiled host program.  Cases: tests/fuse_cases.py.

The bound of the comparison.  Both formulations place a voxel at (i, j, d) on a target; with kappa the largest condition number of the 3 x 3 systems
[a b n] (measured by the reference), s the largest |(i, j, d)| that passed and u = 2^-53, either one is within delta = 64 kappa^2 u s of the exact
coordinates (the Gram route squares the condition number; 64 covers the handful of operations of both).  Where k > 0, |d| <= thickness, so the window
k = 1 - d^2 / thickness^2 moves by at most 2 delta / thickness; the four bilinear weights move by at most 2 delta per axis in sum.  One target's k sd
therefore moves by at most wmax E, E = delta (2 / thickness + 4) + 16 u, its k sn by at most wmax vmax E (vmax the largest |(T - b) / g|), and with R
targets reaching a voxel at most
    |coverage - reference| <= R wmax E + 2^-24 coverage                              (the second term: the result is float32)
    |volume - reference|   <= R wmax E (vmax + |volume|) / coverage + 2^-24 |volume|
Two kinds of voxel are left out and counted: where a target is within 1e-9 of the lattice's border without being exactly on it (the two may disagree
about whether it contributes at all), and where the reference's coverage is below R wmax E (the same for the window's edge: NaN or not is undecided)."""
import functools
import os
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

import fuse_cases as fc
import fuse_reference as fr
from mri_inr_amd import fuse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def same_result(a, b):
    return same(a.volume, b.volume) and same(a.coverage, b.coverage) and np.array_equal(a.flags, b.flags)


def case_args(name, grid, thickness, plain=False):
    d = fc.identity() if name == "identity" else fc.planes()
    kw = dict(thickness=thickness)
    if not plain and "weights" in d:
        kw.update(weights=d["weights"], intensity=d["intensity"])
    return (d["targets"], d["maps"], grid, fc.SPACING), kw


@functools.lru_cache(maxsize=None)
def reference(name, grid, thickness, plain=False):
    args, kw = case_args(name, grid, thickness, plain)
    return fr.fuse(*args, **kw)


def compare(got, ref, args, kw):
    """-> (agrees, the largest error over its bound, voxels left out)"""
    targets, thickness = np.asarray(args[0], np.float64), float(kw["thickness"])
    w = np.asarray(kw["weights"], np.float64) if "weights" in kw else np.ones(1)
    gb = np.asarray(kw["intensity"], np.float64) if "intensity" in kw else np.array([[1.0, 0.0]])
    ok = ref.flags == 0
    wmax = np.nanmax(np.where(np.isfinite(w), w, 0.0))
    gbk = gb[ok] if len(gb) > 1 else gb
    with np.errstate(all="ignore"):
        vmax = np.nanmax(np.abs((targets[ok] - gbk[:, 1, None, None]) / gbk[:, 0, None, None]))
    delta = 64.0 * ref.cond ** 2 * U * ref.scale
    E = delta * (2.0 / thickness + 4.0) + 16.0 * U
    floor = max(ref.reach, 1) * wmax * E
    use = ~ref.near_edge & ~((ref.coverage > 0) & (ref.coverage <= floor))
    if not np.array_equal(got.flags, ref.flags):
        return False, np.inf, int((~use).sum())
    if not np.array_equal(np.isnan(got.volume)[use], np.isnan(ref.volume)[use]):
        return False, np.inf, int((~use).sum())
    cov_err = np.abs(got.coverage.astype(np.float64) - ref.coverage)
    cov_bound = floor + 2.0 ** -24 * ref.coverage
    seen = use & np.isfinite(ref.volume)
    vol_err = np.abs(got.volume.astype(np.float64) - ref.volume)[seen]
    vol_bound = (floor * (vmax + np.abs(ref.volume)) / ref.coverage + 2.0 ** -24 * np.abs(ref.volume))[seen]
    worst = max(float((cov_err / cov_bound.clip(1e-300))[use].max()), float((vol_err / vol_bound).max()) if seen.any() else 0.0)
    return worst <= 1.0, worst, int((~use).sum())


CASES = [("planes", g, t, False) for g in fc.GRIDS for t in fc.THICKNESSES] + [("planes", fc.GRIDS[0], fc.SPACING, True)]


@pytest.mark.parametrize("name,grid,thickness,plain", CASES)
def test_the_host_rule_agrees_with_the_independent_formulation(name, grid, thickness, plain):
    args, kw = case_args(name, grid, thickness, plain)
    got, ref = fuse.fuse_on_host(*args, **kw), reference(name, grid, thickness, plain)
    ok, worst, left_out = compare(got, ref, args, kw)
    print(f"{name} {grid} thickness {thickness} plain {plain}: condition {ref.cond:.9f}, largest coordinate {ref.scale:.2f}, at most {ref.reach} targets per voxel, "
          f"largest error / bound {worst:.3f}, {left_out} voxels left out, {int(np.isfinite(got.volume).sum())} covered")
    assert ok and left_out <= 0.01 * got.volume.size
    assert got.flags.tolist() == [0] * fc.M_PLANES + [fuse.DEGENERATE, fuse.BAD_INTENSITY if not plain else 0]
    assert got.volume.dtype == np.float32 and got.coverage.dtype == np.float32 and got.flags.dtype == np.int32
    assert np.isfinite(got.volume).sum() > 500 and np.isnan(got.volume[-1]).all() and not got.coverage[-1].any()  # the last slice: no target reaches it


def test_identity_returns_the_targets_bits():
    d = fc.identity()
    res = fuse.fuse_on_host(d["targets"], d["maps"], fc.IDENTITY_GRID, fc.SPACING)
    assert same(res.volume, d["targets"]) and (res.coverage == 1.0).all() and not res.flags.any()
    ones = np.ones_like(d["targets"])
    assert same_result(res, fuse.fuse_on_host(d["targets"], d["maps"], fc.IDENTITY_GRID, fc.SPACING, thickness=fc.SPACING, weights=ones, intensity=[[1, 0]] * 3))


@pytest.mark.parametrize("g,b", [(4.0, -2.0), (0.5, 8.0), (-2.0, 0.25)])
def test_gain_and_bias_that_are_powers_of_two_are_inverted_exactly(g, b):
    """with targets on a dyadic grid g T + b is exact in float32, and so is ((double)T' - b) / g: every bit of the plain fusion comes back"""
    d = fc.planes()
    t = (np.round(np.nan_to_num(d["targets"], nan=0.0) * 64) / 64).astype(np.float32)
    t[fc.NAN_PIXEL_AT] = np.nan
    scaled = (np.float32(g) * t + np.float32(b)).astype(np.float32)
    assert np.array_equal(((scaled.astype(np.float64) - b) / g), t.astype(np.float64), equal_nan=True)
    for grid in fc.GRIDS:
        plain = fuse.fuse_on_host(t[:fc.M_PLANES], d["maps"][:fc.M_PLANES], grid, fc.SPACING, weights=d["weights"][:fc.M_PLANES])
        got = fuse.fuse_on_host(scaled[:fc.M_PLANES], d["maps"][:fc.M_PLANES], grid, fc.SPACING, weights=d["weights"][:fc.M_PLANES], intensity=[[g, b]] * fc.M_PLANES)
        assert same_result(got, plain) and np.isfinite(got.volume).sum() > 500


def test_flagged_zero_weight_and_outside_targets_change_no_bit_when_appended():
    d, o = fc.planes(), fc.outside_target()
    n = fc.M_PLANES
    grid = fc.GRIDS[1]
    base = fuse.fuse_on_host(d["targets"][:n], d["maps"][:n], grid, fc.SPACING, weights=d["weights"][:n], intensity=d["intensity"][:n])
    full = fuse.fuse_on_host(d["targets"], d["maps"], grid, fc.SPACING, weights=d["weights"], intensity=d["intensity"])  # + the degenerate map and the gain 0
    assert same(full.volume, base.volume) and same(full.coverage, base.coverage) and full.flags[n:].tolist() == [fuse.DEGENERATE, fuse.BAD_INTENSITY]
    extra = [(o["targets"], o["maps"], o["weights"], o["intensity"]),                                                           # outside
             (d["targets"][:1], d["maps"][:1], np.zeros((1,) + fc.SHAPE, np.float32), d["intensity"][:1]),                      # weight 0 everywhere
             (d["targets"][:1], d["maps"][:1], d["weights"][:1], np.array([[np.nan, 0.0]], np.float32)),                        # gain NaN
             (d["targets"][:1], np.full((1, 9), np.inf, np.float32), d["weights"][:1], d["intensity"][:1])]                     # a map that is not finite
    for t, mp, w, gb in extra:
        for front in (False, True):
            order = (lambda a, b: np.concatenate([b, a])) if front else (lambda a, b: np.concatenate([a, b]))
            got = fuse.fuse_on_host(order(d["targets"][:n], t), order(d["maps"][:n], mp), grid, fc.SPACING, weights=order(d["weights"][:n], w),
                                    intensity=order(d["intensity"][:n], gb))
            assert same(got.volume, base.volume) and same(got.coverage, base.coverage)


def test_min_coverage_only_turns_values_into_nan():
    d = fc.planes()
    grid = fc.GRIDS[0]
    base = fuse.fuse_on_host(d["targets"], d["maps"], grid, fc.SPACING, weights=d["weights"], intensity=d["intensity"])
    for mc in (1e-3, 0.25, 1.0, 1e9):
        got = fuse.fuse_on_host(d["targets"], d["maps"], grid, fc.SPACING, weights=d["weights"], intensity=d["intensity"], min_coverage=mc)
        keep = base.coverage.astype(np.float64) > mc  # (float32 of den > mc where den > mc, up to the rounding of den: none of these sits on a threshold)
        assert same(got.coverage, base.coverage) and np.array_equal(got.flags, base.flags)
        assert np.array_equal(np.isfinite(got.volume), keep & np.isfinite(base.volume)) and same(got.volume[keep], base.volume[keep])
        if mc == 0.25:
            assert 0 < np.isfinite(got.volume).sum() < np.isfinite(base.volume).sum()


@pytest.mark.parametrize("thickness", fc.THICKNESSES)
def test_closeness_to_the_truth(thickness):
    t = fc.truth_case()
    res = fuse.fuse_on_host(t["targets"], t["maps"], fc.TRUTH_GRID, fc.SPACING, thickness=thickness)
    covered = np.isfinite(res.volume)
    err = np.abs(res.volume.astype(np.float64) - t["volume"])[covered]
    share, worst, mean = fc.TRUTH_ERRORS[thickness]
    print(f"thickness {thickness}: covered {covered.mean():.6f}, max error {err.max():.6f} (recorded {worst:.6f}), mean error {err.mean():.6f} (recorded {mean:.6f})")
    assert not res.flags.any() and covered.mean() >= fc.TRUTH_COVERED
    assert abs(covered.mean() - share) <= 0.02 * share and abs(err.max() - worst) <= 0.02 * worst and abs(err.mean() - mean) <= 0.02 * mean


def test_graze_cases_sit_on_the_edges_they_claim():
    """the graze case (the GPU's test of the cull) on the host: at shift 0 and thickness 4 the window's edge and the lattice's border are hit exactly"""
    d = fc.graze(0)
    r = fuse.target_records(d["maps"], None, fc.SPACING, 4.0)
    assert r.det[0] == 25.0 / 16 and r.dt[0] == 25.0 and (r.c[0][0], r.c[1][0], r.c[2][0]) == (1.0, -0.75, 0.0) and not r.flags.any()
    cp = (1.0 * (2 * 4.0 - r.t[0][0])) + (-0.75 * (31.0 - r.t[1][0]))
    assert cp == 5.0 and fuse.window(np.float64(cp), r.dt[0]) == 0.0
    seen = {}
    for shift in fc.GRAZE_SHIFTS:
        for thickness in fc.GRAZE_THICKNESSES:
            g = fc.graze(shift)
            for q in range(3):
                seen[shift, thickness, q] = fuse.fuse_on_host(g["targets"][q:q + 1], g["maps"][q:q + 1], fc.GRIDS[0], fc.SPACING, thickness=thickness).coverage
    # target 0, z = 2, row y = 31: outside at the edge, inside one ulp of the thickness (or of ty) further
    assert not seen[0, 4.0, 0][2, 31].any() and not seen[0, fc.GRAZE_THICKNESSES[0], 0][2, 31].any() and seen[0, fc.GRAZE_THICKNESSES[2], 0][2, 31, :23].all()
    assert not seen[0, 4.0, 0][2, 16:31].any() and {bool(seen[s, 4.0, 0][2, 31, 0]) for s in (-1, 1)} == {False, True}
    # target 1: i = 18 at y = 16 and j = 22 at x = 16 exactly -- inside; one ulp further out: outside
    assert seen[0, 4.0, 1][2, 16, :17].all() and seen[0, 4.0, 1][2, :17, 16].all() and not seen[0, 4.0, 1][2, 17:].any() and not seen[0, 4.0, 1][2, :, 17:].any()
    assert {bool(seen[s, 4.0, 1][2, 16, 0]) for s in (-1, 1)} == {False, True}
    # target 2: i = 0 at y = 15 and j = 0 at x = 31
    assert seen[0, 4.0, 2][1, 15, 31:].all() and not seen[0, 4.0, 2][1, :15].any() and not seen[0, 4.0, 2][1, :, :31].any()
    assert {bool(seen[s, 4.0, 2][1, 15, 31]) for s in (-1, 1)} == {False, True}


# ---- seeded mutants of the rule ------------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "window_in_abs_d": ("window", lambda cp, dt: 1.0 - (np.abs(cp) / np.sqrt(dt))),
    "w_missing_from_bw": ("tap_weight", lambda beta, w: beta),
    "b_subtracted_after_the_division": ("tap_value", lambda T, bias, g: (T / g) - bias),
    "i_and_j_swapped": ("in_plane", lambda pa, pb, G11, G12, G22, det: (((G11 * pb) - (G12 * pa)) / det, ((G22 * pa) - (G12 * pb)) / det)),
    "spacing_not_applied_to_the_z_row": ("z_row", lambda x, spacing: x),
    "floor_without_the_clamp": ("base_index", lambda i, size: np.floor(i)),
    "an_invalid_tap_counted": ("tap_valid", lambda T, w: np.ones(np.shape(T), bool)),
}
MUTANT_CASES = [("planes", fc.GRIDS[0], fc.SPACING, False), ("identity", fc.IDENTITY_GRID, fc.SPACING, False)]


def rejected(name, grid, thickness, plain):
    args, kw = case_args(name, grid, thickness, plain)
    try:
        got = fuse.fuse_on_host(*args, **kw)
    except IndexError:  # a read outside the target: what the clamp is there to prevent
        return True
    return not compare(got, reference(name, grid, thickness, plain), args, kw)[0]


def test_the_comparison_accepts_the_rule_on_the_mutants_cases():
    assert not any(rejected(*c) for c in MUTANT_CASES)


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_comparison_rejects_every_seeded_mutant(mutant, monkeypatch):
    attr, wrong = MUTANTS[mutant]
    monkeypatch.setattr(fuse, attr, wrong)
    caught = [c[0] for c in MUTANT_CASES if rejected(*c)]
    print(f"{mutant}: rejected on {caught}")
    assert caught, mutant


# ---- fuse_plan.h ---------------------------------------------------------------------------------------------------------------------------------------
PROG = textwrap.dedent(r"""
    #include <cmath>
    #include <cstdio>
    #include <cstdlib>
    #include <cstring>
    #include <initializer_list>
    #include <limits>
    #include "fuse_plan.h"
    using namespace msiren;

    #define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
    static char msg[256];
    static float buf[64];
    static FuseArgs good(const msiren_fuse_opts* o) { return FuseArgs{buf, 3, 19, 23, buf, nullptr, nullptr, o, 4, 40, 40, buf, nullptr, nullptr, true}; }
    static bool refused(const FuseArgs& a, const char* word) {
        msg[0] = 0;
        if (fuse_check(a, msg, sizeof msg)) return false;
        if (!std::strstr(msg, word)) { std::printf("'%s' does not name '%s'\n", msg, word); return false; }
        return true;
    }

    int main() {
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        msiren_fuse_opts o{(int32_t)sizeof(msiren_fuse_opts), 0, 4.0, 4.0, 0.0};
        CHECK(sizeof(msiren_fuse_opts) == 32);
        CHECK(fuse_check(good(&o), msg, sizeof msg));
        { msiren_fuse_opts b = o; b.struct_size = 24; CHECK(refused(good(&b), "struct_size")); b.struct_size = 40; CHECK(refused(good(&b), "struct_size")); }
        for (double bad : {0.0, -1.0, nan, inf, -inf}) {
            msiren_fuse_opts b = o; b.spacing = bad; CHECK(refused(good(&b), "spacing"));
            b = o; b.thickness = bad; CHECK(refused(good(&b), "thickness"));
        }
        for (double bad : {-1e-300, nan, -inf}) { msiren_fuse_opts b = o; b.min_coverage = bad; CHECK(refused(good(&b), "min_coverage")); }
        { msiren_fuse_opts b = o; b.min_coverage = inf; CHECK(fuse_check(good(&b), msg, sizeof msg)); b.min_coverage = 0.5; CHECK(fuse_check(good(&b), msg, sizeof msg)); }
        { FuseArgs a = good(&o); a.th = 1; CHECK(refused(a, "th")); a = good(&o); a.tw = 1; CHECK(refused(a, "tw")); a.tw = 2; a.th = 2; CHECK(fuse_check(a, msg, sizeof msg)); }
        { FuseArgs a = good(&o); a.n = 0; CHECK(refused(a, "n_slices")); a = good(&o); a.H = 0; CHECK(refused(a, "height")); a = good(&o); a.W = -3; CHECK(refused(a, "width")); }
        { FuseArgs a = good(&o); a.m = -1; CHECK(refused(a, "m_targets")); }
        // the two products flip exactly at 2^30
        { FuseArgs a = good(&o); a.n = 1 << 10, a.H = 1 << 10, a.W = 1 << 10; CHECK(refused(a, "n_slices height width")); a.W = (1 << 10) - 1; CHECK(fuse_check(a, msg, sizeof msg));
          a = good(&o); a.n = (int64_t)1 << 62; CHECK(refused(a, "n_slices height width")); a.n = 1, a.H = a.W = 0x7fffffff; CHECK(refused(a, "n_slices height width")); }
        { FuseArgs a = good(&o); a.m = 1 << 12, a.th = 1 << 9, a.tw = 1 << 9; CHECK(refused(a, "m_targets th tw")); a.m = (1 << 12) - 1; CHECK(fuse_check(a, msg, sizeof msg));
          a.m = (int64_t)1 << 61; CHECK(refused(a, "m_targets th tw")); }
        { FuseArgs a = good(&o); a.targets = nullptr; CHECK(refused(a, "targets")); a = good(&o); a.maps = nullptr; CHECK(refused(a, "maps"));
          a = good(&o); a.volume = nullptr; CHECK(refused(a, "volume")); a = good(nullptr); CHECK(refused(a, "opts")); }
        // misaligned device pointers are named; host pointers are not checked
        {
            const char* names[] = {"targets", "maps", "weights", "intensity", "volume", "coverage", "flags"};
            for (int k = 0; k < 7; ++k) {
                FuseArgs a = good(&o);
                const void* odd = (const char*)buf + 2;
                const void** slot[] = {&a.targets, &a.maps, &a.weights, &a.intensity, &a.volume, &a.coverage, &a.flags};
                *slot[k] = odd;
                CHECK(refused(a, names[k]) && std::strstr(msg, "aligned"));
                a.device = false;
                CHECK(fuse_check(a, msg, sizeof msg));
            }
        }
        // m = 0 is valid without targets, maps, opts and volume; a grid is still needed, and opts that are given are still checked
        { FuseArgs a = good(nullptr); a.m = 0, a.targets = a.maps = a.volume = nullptr, a.th = a.tw = 0; CHECK(fuse_check(a, msg, sizeof msg)); a.n = 0; CHECK(refused(a, "n_slices"));
          msiren_fuse_opts b = o; b.spacing = 0; a = good(&b); a.m = 0; CHECK(refused(a, "spacing")); }
        // tiling and scratch
        CHECK(kFuseTile == 16 && kFuseRecord == 20 && FUSE_FLAGS == kFuseRecord - 1 && FUSE_C + 3 == FUSE_GAIN);
        CHECK(fuse_tiles_y(40) == 3 && fuse_tiles_x(37) == 3 && fuse_tiles_x(48) == 3 && fuse_tiles_x(49) == 4 && fuse_tiles_y(1) == 1 && fuse_tiles(5, 37, 45) == 45);
        CHECK(fuse_tiles(1, 0x7fffffff, 1) == 0x8000000 && fuse_tiles(kFuseLimit - 1, 1, 1) == kFuseLimit - 1);
        CHECK(fuse_layout(0).total == 0 && fuse_layout(1).total == 160 && fuse_layout(64).total == 64 * 160 && fuse_layout(7).records == 0 && fuse_layout(7).total % 8 == 0);
        std::puts("ok");
        return 0;
    }
""")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_fuse_plan(tmp_path):
    src, exe = tmp_path / "fuse_plan.cpp", tmp_path / "fuse_plan"
    src.write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mri_inr_amd", "csrc"), str(src), "-o", str(exe)], check=True, capture_output=True,
                   text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
