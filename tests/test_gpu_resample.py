"""The reconstruction at arbitrary points on the GPU: model.resample / resample_with_gradient, i.e.
msiren_resample_slices* -- slice prologue, points binned by tile, the ragged exact-fp32 trunks, blend.

Values against the fp64 reference (tests/resample_reference.py) within the project's norm (max <= 1e-4 of max|ref|,
rms <= 1e-5); gradients within tests/test_gpu_grad.py's gate, 4 x the reference's own perturbed-fp32 floor capped at that norm; what
must not depend on order, batch or run is compared bit for bit.
"""
import functools

import numpy as np
import pytest

import grad_reference as gr
import resample_reference as rr
from mri_inr_amd import ModulatedSiren, _lib, synthetic as syn
from oracle import siren_oracle as orc

pytestmark = pytest.mark.gpu

O, I, S = 32, 16, 24
PAD = (S - I) // 2
NV = NH = 3
LO, HI = float(-PAD), float(NV * I - 1 + PAD)  # the cover of the whole slice: [-4, 51]
NORM_MAX, NORM_RMS = 1e-4, 1e-5


def build(sd, prec="fp32", act="sine", L=5):
    m = ModulatedSiren(dim_in=2, dim_hidden=256, dim_out=1, num_layers=L, latent_dim=256, w0=1.0, w0_initial=30.0, use_bias=True,
                       dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None, outer_patch_size=O, inner_patch_size=I,
                       siren_patch_size=S, device="cuda", activation=act, precision=prec)
    m.load_state_dict(sd, strict=True)
    m.to("cuda")
    m.eval()
    return m


@functools.lru_cache(maxsize=None)
def full_sd(L=5):
    return syn.make_state_dict(seed=7, num_layers=L, trained_like=True)


@functools.lru_cache(maxsize=None)
def model(prec="fp32", act="sine", L=5):
    """(tests/test_gpu_coordset_cases.py runs the same slices on a second model: Morlet, L = 3)"""
    return build(full_sd(L), prec, act, L)


@functools.lru_cache(maxsize=None)
def images():
    img = np.stack([syn.make_slice(3, 40, 40), syn.make_slice(4, 40, 40)])
    img[1, :24] = 0.0  # the upper row of tiles of the second slice sees nothing but black: the plan drops it
    return img


def in_last_tile(p):
    return (p[:, 0] >= 2 * I - PAD) & (p[:, 1] >= 2 * I - PAD)


def make_points(draw):
    """M ~ 300: the integer pixels of a 12 x 12 window across the seam of tiles 0 and 1; real points over the slice's cover; the exact
    cover edges; points outside; a NaN point; a pile inside tile (1, 1) alone, which with the window's makes that tile's set span
    three chunks of 64; tile (2, 2) left without a point (whatever falls into its cover is drawn again / left out)."""
    rng = np.random.default_rng(100 + draw)
    window = np.stack(np.meshgrid(np.arange(10, 22), np.arange(10, 22), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    real = rng.uniform(LO, HI, size=(400, 2)).astype(np.float32)
    real = real[~in_last_tile(real)][:80]
    pile = rng.uniform(20.0, 27.0, size=(40, 2)).astype(np.float32)
    ends = [float(v * I - PAD + d) for v in range(NV) for d in (0, S - 1)]  # -4, 19, 12, 35, 28, 51
    edges = np.array([[e, 20.5] for e in ends] + [[20.5, e] for e in ends] + [[-4, -4], [51, 5], [19, 19], [12, 12], [35, 12]], np.float32)
    edges = edges[~in_last_tile(edges)]
    below, above = np.nextafter(np.float32(LO), np.float32(-np.inf)), np.nextafter(np.float32(HI), np.float32(np.inf))
    outside = np.array([[below, 10], [10, above], [-10, 5], [5, 100], [np.inf, 3], [np.nan, 7.5]], np.float32)
    pts = np.concatenate([window, real, pile, edges, outside])
    return pts, dict(window=slice(0, len(window)), outside=slice(len(pts) - len(outside), len(pts)))


def prologue(sd, tiles, dtype, L=5):
    z = orc.encoder_forward(sd, tiles, dtype=dtype)
    return orc.modulator_forward(sd, z, num_layers=L, dtype=dtype)


def reference_slice(img, pts, dtype, act="sine", L=5, **kw):
    sd = full_sd(L)
    patches, info = orc.image_to_patches(img, O, I)
    kept, black, _ = orc.filter_and_remember_black_patches(patches)
    assert info == (NV, NH)
    mods = np.zeros((L, NV * NH, 256), dtype)
    mods[:, [t for t in range(NV * NH) if t not in black]] = prologue(sd, kept, dtype, L)
    val, grad = rr.resample(sd, mods, black, pts, NV, NH, S, I, num_layers=L, activation=act, dtype=dtype, **kw)
    return val, grad, black


@functools.lru_cache(maxsize=None)
def data(act="sine", L=5):
    """The points (the first draw at which the reference's gradient ALONE sits inside the caps, as grad_reference.case_data draws), the
    fp64 reference of both slices and the gradient gate: 4 x the distance of the same chain in perturbed fp32, capped at the norm."""
    for draw in range(16):
        pts, parts = make_points(draw)
        ref = [reference_slice(img, pts, np.float64, act, L) for img in images()]
        f32 = [reference_slice(img, pts, np.float32, act, L, perturbed=True) for img in images()]
        val, grad = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref], axis=1)
        g32 = np.stack([r[1] for r in f32], axis=1)
        ok = np.isfinite(val[0])
        fm, fr = gr.distances(g32[:, :, ok], grad[:, :, ok])
        if gr.FACTOR * fm <= gr.CAP_MAX and gr.FACTOR * fr <= gr.CAP_RMS:
            break
    return dict(points=pts, parts=parts, value=val, grad=grad, finite=ok, black=[r[2] for r in ref], draw=draw,
                gate=(min(gr.FACTOR * fm, gr.CAP_MAX), min(gr.FACTOR * fr, gr.CAP_RMS)))


@functools.lru_cache(maxsize=None)
def gpu_result():
    m = model()
    val, grad = m.resample_with_gradient(images(), data()["points"])
    return np.array(val), np.array(grad)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_points_are_what_the_test_says():
    d = data()
    pts = d["points"]
    cov = rr.covers(pts, NV, NH, S, I)
    per_tile = np.bincount([t for lst in cov for t, _, _ in lst], minlength=NV * NH)
    print("points", len(pts), "draw", d["draw"], "covers per tile", per_tile.tolist(), "gate", d["gate"])
    assert 250 <= len(pts) <= 350 and per_tile[4] > 128 and per_tile[8] == 0 and (per_tile[:8] > 0).all()
    assert max(len(lst) for lst in cov) == 4 and (~d["finite"]).sum() == 6
    assert d["black"][0] == [] and d["black"][1] == [0, 1, 2]


def test_values_vs_reference():
    d = data()
    val, _ = gpu_result()
    ok = d["finite"]
    assert val.shape == (2, len(d["points"])) and val.dtype == np.float32
    em, er = gr.distances(val[:, ok], d["value"][:, ok])
    print(f"values: max {em:.2e} rms {er:.2e} (norm {NORM_MAX:.0e} / {NORM_RMS:.0e})")
    assert em <= NORM_MAX and er <= NORM_RMS
    assert np.array_equal(val, model().resample(images(), d["points"]), equal_nan=True)  # the value form gives the same bits


def test_gradients_vs_reference():
    d = data()
    _, grad = gpu_result()
    ok = d["finite"]
    assert grad.shape == (2, 2, len(d["points"]))
    em, er = gr.distances(grad[:, :, ok], d["grad"][:, :, ok])
    print(f"gradients: max|grad| {np.abs(d['grad'][:, :, ok]).max():.3f} nerr {em:.2e} (gate {d['gate'][0]:.2e}) rms {er:.2e} (gate {d['gate'][1]:.2e})")
    assert em <= d["gate"][0] and er <= d["gate"][1]


def test_integer_pixels_are_the_fp32_reconstruction():
    d = data()
    val, grad = gpu_result()
    m = model()
    recon, rgrad = m.reconstruct_with_gradient(images())
    assert np.array_equal(recon, m.reconstruct(images()))
    w = d["points"][d["parts"]["window"]].astype(int)
    for got, ref, what in ((val[:, d["parts"]["window"]], recon[:, w[:, 0], w[:, 1]], "values"),
                           (grad[:, :, d["parts"]["window"]], rgrad[:, :, w[:, 0], w[:, 1]], "gradients")):
        em, er = gr.distances(got, ref)
        print(f"integer pixels, {what}: max {em:.2e} rms {er:.2e}")
        assert em <= NORM_MAX and er <= NORM_RMS, what


def test_outside_and_nan_points_are_nan_and_touch_nothing_else():
    d = data()
    val, grad = gpu_result()
    out = d["parts"]["outside"]
    assert np.isnan(val[:, out]).all() and np.isnan(grad[:, :, out]).all()
    assert np.isfinite(np.delete(val, np.arange(out.start, out.stop), axis=1)).all()
    inside = d["points"][:out.start]
    v2, g2 = model().resample_with_gradient(images(), inside)  # the same call without them: the other points' bits
    assert np.array_equal(bits(v2), bits(val[:, :out.start])) and np.array_equal(bits(g2), bits(grad[:, :, :out.start]))


def test_point_under_black_tiles_only_is_zero():
    d = data()
    val, grad = gpu_result()
    pts = d["points"]
    only_top = np.isfinite(pts).all(1) & (pts[:, 0] >= LO) & (pts[:, 0] < 2 * I - PAD - I) & (pts[:, 1] >= LO) & (pts[:, 1] <= HI)  # rows of tiles 0 alone
    assert only_top.sum() >= 5
    assert np.all(val[1, only_top] == 0) and np.all(grad[:, 1, only_top] == 0)
    assert np.all(val[0, only_top] != 0)


def test_permutation_batch_and_rerun_bit_for_bit():
    d = data()
    val, grad = gpu_result()
    m = model()
    perm = np.random.default_rng(9).permutation(len(d["points"]))
    vp, gp = m.resample_with_gradient(images(), d["points"][perm])
    assert np.array_equal(bits(vp), bits(val[:, perm])) and np.array_equal(bits(gp), bits(grad[:, :, perm]))
    assert np.array_equal(bits(m.resample(images(), d["points"][perm])), bits(val[:, perm]))
    for s in range(2):  # a slice alone (2-D and 3-D input) is the slice in the batch
        v1, g1 = m.resample_with_gradient(images()[s], d["points"])
        assert v1.shape == val[s].shape and g1.shape == grad[:, s].shape
        assert np.array_equal(bits(v1), bits(val[s])) and np.array_equal(bits(g1), bits(grad[:, s])), s
    v2, g2 = m.resample_with_gradient(images(), d["points"])
    assert np.array_equal(bits(v2), bits(val)) and np.array_equal(bits(g2), bits(grad))


def test_split_fp16_handle_runs_its_own_prologue_and_the_fp32_trunk():
    d = data()
    val16 = model("f16x3").resample(images(), d["points"])
    ok = d["finite"]
    em, er = gr.distances(val16[:, ok], d["value"][:, ok])
    print(f"f16x3 handle: max {em:.2e} rms {er:.2e}")
    assert em <= NORM_MAX and er <= NORM_RMS and np.isnan(val16[:, ~ok]).all()


def test_device_form_single_point_and_null_value_output():
    d = data()
    val, grad = gpu_result()
    m = model()
    one = d["points"][37:38]
    v1, g1 = m.resample_with_gradient(images(), one)  # M = 1
    assert np.array_equal(bits(v1), bits(val[:, 37:38])) and np.array_equal(bits(g1), bits(grad[:, :, 37:38]))
    img, pts = images(), d["points"]
    M = len(pts)
    d_i, d_p = m.device_array(img.shape).copy_from(img), m.device_array(pts.shape).copy_from(pts)
    d_v, d_g = m.device_array((2, M)), m.device_array((2, 2, M))
    _lib.check(m._lib.msiren_resample_slices_grad_dev(m._h, d_i.ptr, 2, 40, 40, d_p.ptr, M, None, d_g.ptr))
    _lib.check(m._lib.msiren_resample_slices_dev(m._h, d_i.ptr, 2, 40, 40, d_p.ptr, M, d_v.ptr))
    m.sync()
    assert np.array_equal(bits(d_g.numpy()), bits(grad)) and np.array_equal(bits(d_v.numpy()), bits(val))
    assert m.resample(img[:0], pts).shape == (0, M) and m.resample(img, pts[:0]).shape == (2, 0)  # nothing to do


def test_refusals_launch_nothing():
    m = model()
    img = images()
    _lib.check(m._lib.msiren_profile_enable(m._h, 1))
    try:
        out = np.empty(4, np.float32)
        for M in (1 << 26, 1 << 40):  # 8 M K >= 2^31
            assert m._lib.msiren_resample_slices(m._h, img.ctypes.data, 2, 40, 40, img.ctypes.data, M, out.ctypes.data) == _lib.E_INVALID
            assert "too many points" in _lib.last_error()
            d_i = m.device_array(img.shape).copy_from(img)
            assert m._lib.msiren_resample_slices_dev(m._h, d_i.ptr, 2, 40, 40, d_i.ptr, M, d_i.ptr) == _lib.E_INVALID
        with pytest.raises(ValueError):
            m.resample(img, np.zeros((5, 3), np.float32))
        with pytest.raises(ValueError, match="too small"):
            m.resample(np.ones((1, 8, 8), np.float32), np.zeros((5, 2), np.float32))
        m.sync()
        assert m.profile_kernels() == []
    finally:
        _lib.check(m._lib.msiren_profile_enable(m._h, 0))


def test_profile_names_the_steps():
    m = model()
    _lib.check(m._lib.msiren_profile_enable(m._h, 1))
    try:
        m.resample_with_gradient(images(), data()["points"])
        names = [e["kernel"] for e in m.profile_kernels()]
        assert "resample_bin_kernels" in names and "siren_trunk_f32_jet_ragged_kernel<256,0>" in names and "resample_blend_kernel" in names, names
    finally:
        _lib.check(m._lib.msiren_profile_enable(m._h, 0))
