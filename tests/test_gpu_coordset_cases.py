"""Every instance of the trunk families that evaluate the model at one coordinate set per patch (f32_ragged, f32_jet_ragged,
f16x3n_ragged, f32_ragged_cond) against the fp64 references, each case on the instance it names
(tests/coordset_cases.py; tests/test_coordset_cases.py shows on the CPU that the manifest is complete and its gates meaningful).

Per case: the handle is built as the case says, the call runs once with the profile on, the profile's kernel names must be exactly the
case's (native calls: the native instance and siren_trunk_f32_ragged_cond_kernel<ACT> behind it), the outputs are finite and meet the
gates.  What must not depend on the batch is compared bit for bit: every patch's slice is the same handle's call of that patch alone
(value: sample_mods; grad: sample_mods_grad; native: the native call), a split-fp16 handle's exact call gives the fp32 handle's bits.

Guard cases: modulation elements of 1e5 that reach nothing downstream put the native launch outside the fp16 domain while the fp64
reference still judges the output: siren_trunk_f32_ragged_cond_kernel<ACT> has to run to the end, on the host and the _dev form.

Every case prints `COORDCASE <case> <max> <rms> gate ..` before it asserts (LAB_NOTES.md holds a run's figures).
"""
import ctypes as C
import functools
from dataclasses import replace

import numpy as np
import pytest

import coordset_cases as cc
import grad_reference as gr
import test_gpu_resample as tr
from mri_inr_amd import ModulatedSiren, _lib, synthetic as syn

pytestmark = pytest.mark.gpu

ids = lambda c: c.id
COND = "siren_trunk_f32_ragged_cond_kernel<%d>"  # <ACT>


@functools.lru_cache(maxsize=None)
def _handle(m: cc.Case):
    h = ModulatedSiren(dim_in=2, dim_hidden=m.H, dim_out=1, num_layers=m.L, latent_dim=m.Z, w0=m.w0, w0_initial=m.w0_initial,
                       use_bias=m.use_bias, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None, outer_patch_size=32,
                       inner_patch_size=16, siren_patch_size=24, device="cuda", activation=m.act, residual=m.residual, precision=m.precision)
    h.load_state_dict(cc.state_dict(m), strict=False)
    h.to("cuda")
    h.eval()
    return h


def model_of(c: cc.Case, precision=None):
    """the case's model (cases with equal `model` share a handle), or the same weights on another precision"""
    return _handle(replace(c.model, precision=precision or c.precision))


def range_events(m) -> int:
    n = C.c_int64()
    _lib.check(m._lib.msiren_range_events(m._h, C.byref(n)))
    return n.value


def bits(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32).view(np.uint32)


def profiled(m, fn):
    _lib.check(m._lib.msiren_profile_enable(m._h, 1))
    try:
        out = fn()
        m.sync()
        return out, m.profile_kernels()
    finally:
        _lib.check(m._lib.msiren_profile_enable(m._h, 0))


def call(m, form, mods, xy, off):
    """one call of a case's form -> (value (T,), grad (2, T) or None)"""
    if form == "grad":
        v, g = m.sample_mods_ragged_grad(mods, xy, off)
        return np.array(v), np.array(g)
    return np.array(m.sample_mods_ragged(mods, xy, off, exact=form != "native")), None


def alone(m, form, mods, xy, b):
    """patch b alone, its coordinates as one shared set (value, grad) or as a one-patch native call"""
    if form == "native":
        return call(m, form, mods[:, b:b + 1], xy, np.array([0, len(xy)], np.int32))
    if form == "grad":
        v, g = m.sample_mods_grad(mods[:, b:b + 1], xy)
        return np.asarray(v)[0], np.asarray(g)[:, 0]
    return np.asarray(m.sample_mods(mods[:, b:b + 1], xy))[0], None


def inputs(c: cc.Case):
    return np.array(cc.mods(c)), np.array(cc.coords_of(c)), cc.offsets(c)


def check_gate(c: cc.Case, val, grad=None, what="gpu"):
    (e, r), (te, tr_) = cc.distance(c, val), cc.tolerance(c, exact=what == "exact")
    extra = f" l0_floor {cc.l0_floor(c):.2e}" if c.form == "native" else ""
    print(f"COORDCASE {c.id} {what} {e:.2e} {r:.2e} gate {te:.2e} {tr_:.2e} ratio {e / te:.2f} e32 {cc.e32(c):.2e}{extra}")
    if grad is not None:
        (ge, gr_), (gte, gtr) = cc.grad_distance(c, grad), cc.grad_tolerance(c)
        print(f"COORDCASE {c.id} {what} gradient {ge:.2e} {gr_:.2e} gate {gte:.2e} {gtr:.2e} ratio {ge / gte:.2f} draw {cc.draw_of(c)}")
    assert val.dtype == np.float32 and val.shape == (c.T,) and np.isfinite(val).all()
    assert e <= te and r <= tr_, (c.id, e, r, te, tr_)
    if grad is not None:
        assert grad.dtype == np.float32 and grad.shape == (2, c.T) and np.isfinite(grad).all()
        assert ge <= gte and gr_ <= gtr, (c.id, ge, gr_, gte, gtr)


_outputs = {}   # case -> (value, grad) of its call (filled by test_case_on_its_instance)


def run(c: cc.Case):
    m = model_of(c)
    mods, xy, off = inputs(c)
    (val, grad), entries = profiled(m, lambda: call(m, c.form, mods, xy, off))
    assert [e["kernel"] for e in entries] == list(c.launches), (entries, c.launches)
    assert entries[0]["launches"] == 1 and entries[0]["coords"] == c.T, entries
    return m, val, grad


PLAIN = [c for c in cc.CASES if not c.guard]


# ---- 1. every case on its instance, against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", PLAIN, ids=ids)
def test_case_on_its_instance(c):
    e0 = range_events(model_of(c))
    m, val, grad = run(c)
    check_gate(c, val, grad)
    assert range_events(m) == e0  # (a native case that left the fp16 domain would test the conditional kernel instead)
    _outputs[c] = (val, grad)


# ---- 2. bit invariants -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", PLAIN, ids=ids)
def test_every_patch_is_the_patch_alone(c):
    """EDGES: every patch that holds coordinates; MANY: the patches around the 256-patch block of ragged_items_kernel and the last one."""
    if c not in _outputs:   # (run alone, or the case's own test failed: run it here)
        _outputs[c] = run(c)[1:]
    val, grad = _outputs[c]
    m = model_of(c)
    mods, xy, off = inputs(c)
    todo = [p for p in cc.patches(c) if not c.many or p[0] in cc.MANY_ALONE]
    assert len(todo) == 5
    for b, lo, hi in todo:
        v, g = alone(m, c.form, mods, xy[lo:hi], b)
        assert np.array_equal(bits(val[lo:hi]), bits(v)), (c.id, b, lo, hi)
        if grad is not None:
            assert np.array_equal(bits(grad[:, lo:hi]), bits(g)), (c.id, b, lo, hi)


@pytest.mark.parametrize("c", cc.NATIVE, ids=ids)
def test_exact_call_on_a_split_fp16_handle_gives_the_fp32_handles_bits(c):
    m16, m32 = model_of(c), model_of(c, "fp32")
    mods, xy, off = inputs(c)
    a = 1 if c.act == "morlet" else 0
    exact, entries = profiled(m16, lambda: np.array(m16.sample_mods_ragged(mods, xy, off)))
    assert [e["kernel"] for e in entries] == [f"siren_trunk_f32_ragged_kernel<256,{a},0>"], entries
    want, entries = profiled(m32, lambda: np.array(m32.sample_mods_ragged(mods, xy, off, exact=False)))  # (not native: the exact kernel)
    assert [e["kernel"] for e in entries] == [f"siren_trunk_f32_ragged_kernel<256,{a},0>"], entries
    assert np.array_equal(bits(exact), bits(want)) and np.array_equal(bits(exact), bits(m32.sample_mods_ragged(mods, xy, off)))
    check_gate(c, exact, what="exact")
    if c in _outputs:  # the native trunk's own bits are not the fp32 trunk's
        assert not np.array_equal(bits(_outputs[c][0]), bits(exact))


# ---- 3. guard cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.GUARDS, ids=ids)
def test_guard_case_is_redone_by_the_conditional_fp32_kernel(c):
    m = model_of(c)
    mods, xy, off = inputs(c)
    plain = np.array(mods)
    for l, b, j in c.guard:
        plain[l, b, j] = 1.0
    e0 = range_events(m)
    before = call(m, "native", plain, xy, off)[0]  # in-domain on the same handle: nothing is redone
    assert range_events(m) == e0
    m_, val, _ = run(c)
    assert m_ is m and range_events(m) > e0, "the case no longer leaves the fp16 domain"
    check_gate(c, val)
    exact = call(m, "value", mods, xy, off)[0]
    check_gate(c, exact, what="exact")
    assert np.array_equal(bits(val), bits(exact))
    # the _dev form alike
    e1 = range_events(m)
    d_m, d_c = m.device_array(mods.shape).copy_from(mods), m.device_array(xy.shape).copy_from(xy)
    assert np.array_equal(bits(m.sample_mods_ragged(d_m, d_c, off, exact=False).numpy()), bits(exact))
    assert range_events(m) > e1
    # the next in-domain call is untouched, and its bits are the native trunk's, not the exact kernel's
    e2 = range_events(m)
    after = call(m, "native", plain, xy, off)[0]
    assert range_events(m) == e2
    assert np.array_equal(bits(after), bits(before)) and not np.array_equal(bits(after), bits(call(m, "value", plain, xy, off)[0]))
    if c.many:  # the patches around the 256-patch block and the last one, alone, on the exact path (the flagged call holds its bits)
        for b, lo, hi in [p for p in cc.patches(c) if p[0] in cc.MANY_ALONE]:
            one = call(m, "value", mods[:, b:b + 1], xy[lo:hi], np.array([0, hi - lo], np.int32))[0]  # (sample_mods is this handle's split-fp16 trunk)
            assert np.array_equal(bits(val[lo:hi]), bits(one)), (b, lo, hi)
    print(f"COORDGUARD {c.id} range_events {range_events(m)}")


# ---- 4. an inactive unit's stand-in row raises nothing ---------------------------------------------------------------------------------------
def test_inactive_units_raise_nothing():
    """Surplus units and dropped or empty patches run on modulation row 0 (siren_trunk_f16x3n_ragged.hip.h); patch 0 is empty here and its
    row holds 1e30 and a NaN, and so does an empty patch in the middle: 7 items = one full pass and one with a surplus unit.  The flag must
    stay down (msiren_range_events does not move, the conditional kernel leaves) and the other patches' bits must be the native trunk's."""
    c = cc.NATIVE[0]
    assert c.kernel == "siren_trunk_f16x3n_ragged_kernel<0,3,5>" and c.L == 5 and c.act == "sine"
    m = model_of(c)
    counts = [0, 1, 31, 0, 33, 70, 0]
    assert sum((n + 31) // 32 for n in counts) % 4 == 3
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    xy = np.random.default_rng(31).uniform(-1.2, 1.2, size=(int(off[-1]), 2)).astype(np.float32)
    ordinary = syn.make_mods(32, c.L, len(counts), c.H)
    mods = ordinary.copy()
    for b in (0, 3):
        mods[:, b, 5], mods[:, b, 9] = 1e30, np.nan
    want = call(m, "native", ordinary, xy, off)[0]
    e0 = range_events(m)
    (got, _), entries = profiled(m, lambda: call(m, "native", mods, xy, off))
    assert [e["kernel"] for e in entries] == list(c.launches), entries
    assert range_events(m) == e0
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(got), bits(call(m, "value", ordinary, xy, off)[0]))  # (the exact kernel's bits would differ)
    d_m, d_c = m.device_array(mods.shape).copy_from(mods), m.device_array(xy.shape).copy_from(xy)
    assert np.array_equal(bits(m.sample_mods_ragged(d_m, d_c, off, exact=False).numpy()), bits(want)) and range_events(m) == e0


# ---- 5. replicas and the plan's pos on a second model: resample on Morlet, L = 3 -------------------------------------------------------------
RS = ("morlet", 3)


def test_resample_on_a_second_model():
    """tests/test_gpu_resample.py's two 40 x 40 slices (the second with a black row of tiles: reps = 2, negative rows in pos) with its
    references and gates, on a Morlet model of depth 3: the jet <256,1> and the native loop form <1,4,0> behind the plan."""
    d, img = tr.data(*RS), tr.images()
    pts, ok = d["points"], d["finite"]
    m = tr.model("fp32", *RS)
    (val, grad), entries = profiled(m, lambda: tuple(np.array(a) for a in m.resample_with_gradient(img, pts)))
    names = [e["kernel"] for e in entries]
    assert [n for n in names if n.startswith("siren_trunk")] == ["siren_trunk_f32_jet_ragged_kernel<256,1>"], names
    assert "resample_bin_kernels" in names and "resample_blend_kernel" in names, names
    em, er = gr.distances(val[:, ok], d["value"][:, ok])
    gm, g_r = gr.distances(grad[:, :, ok], d["grad"][:, :, ok])
    print(f"COORDRESAMPLE morlet L3 draw {d['draw']}: values {em:.2e} {er:.2e} (norm {tr.NORM_MAX:.0e} / {tr.NORM_RMS:.0e}); "
          f"gradients {gm:.2e} {g_r:.2e} (gate {d['gate'][0]:.2e} / {d['gate'][1]:.2e})")
    assert val.shape == (2, len(pts)) and grad.shape == (2, 2, len(pts))
    assert em <= tr.NORM_MAX and er <= tr.NORM_RMS
    assert gm <= d["gate"][0] and g_r <= d["gate"][1]
    assert np.isnan(val[:, ~ok]).all() and np.isnan(grad[:, :, ~ok]).all() and d["black"] == [[], [0, 1, 2]]
    m16 = tr.model("f16x3", *RS)
    nat, entries = profiled(m16, lambda: np.array(m16.resample(img, pts, exact=False)))
    names = [e["kernel"] for e in entries]
    assert names == ["resample_bin_kernels", "siren_trunk_f16x3n_ragged_kernel<1,4,0>", COND % 1, "resample_blend_kernel"], names
    nm, nr = gr.distances(nat[:, ok], d["value"][:, ok])
    print(f"COORDRESAMPLE morlet L3 native: values {nm:.2e} {nr:.2e} (norm {tr.NORM_MAX:.0e} / {tr.NORM_RMS:.0e})")
    assert nat.shape == (2, len(pts)) and nat.dtype == np.float32
    assert nm <= tr.NORM_MAX and nr <= tr.NORM_RMS and np.isnan(nat[:, ~ok]).all()
    # points under black tiles only: rows of tiles 0 alone
    only_top = np.isfinite(pts).all(1) & (pts[:, 0] >= tr.LO) & (pts[:, 0] < 2 * tr.I - tr.PAD - tr.I) & (pts[:, 1] >= tr.LO) & (pts[:, 1] <= tr.HI)
    assert only_top.sum() >= 5
    for v in (val, nat):
        assert np.all(v[1, only_top] == 0) and np.all(v[0, only_top] != 0)
    assert np.all(grad[:, 1, only_top] == 0)
