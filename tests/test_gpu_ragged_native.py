"""Per-patch coordinate sets and the reconstruction at points in the handle's OWN trunk arithmetic:
model.sample_mods_ragged(..., exact=False) / model.resample(..., exact=False), i.e. msiren_sample_ragged_mods_native(_dev) /
msiren_resample_slices_native(_dev) on siren_trunk_f16x3n_ragged_kernel -- the split-fp16 trunk with layer 0 computed in the kernel -- and
siren_trunk_f32_ragged_cond_kernel behind it.

Values against the fp64 reference (grad_reference.value_and_grad / resample_reference) within the project's norm (DESIGN.md section 2:
max <= 1e-4 and rms <= 1e-5 of max|ref|); what must not depend on position, batch, stream or run is compared bit for bit.  Handles are
f16x3, H = 256, unless said.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import grad_reference as gr
import test_gpu_resample as tr
from mri_inr_amd import _lib, synthetic as syn
from test_gpu_ragged import build, profile_off, profile_on

pytestmark = pytest.mark.gpu

NORM_MAX, NORM_RMS = 1e-4, 1e-5
COUNTS = [0, 1, 31, 32, 33, 130, 0]  # patches without coordinates at both ends; around the chunk of 32; four chunks and a ragged fifth

CASES = {
    "H256-sine-L5": (gr.Case("H256-sine-L5", 256, 5, "sine"), "siren_trunk_f16x3n_ragged_kernel<0,3,5>"),
    "H256-morlet-L3": (gr.Case("H256-morlet-L3", 256, 3, "morlet"), "siren_trunk_f16x3n_ragged_kernel<1,4,0>"),
    "H256-sine-L7": (gr.Case("H256-sine-L7", 256, 7, "sine"), "siren_trunk_f16x3n_ragged_kernel<0,3,0>"),
    "H256-sine-L5-zeros": (gr.Case("H256-sine-L5-zeros", 256, 5, "sine", zero_fraction=0.3), "siren_trunk_f16x3n_ragged_kernel<0,3,5>"),
}
COND = "siren_trunk_f32_ragged_cond_kernel<%d>"  # <ACT>


@functools.lru_cache(maxsize=None)
def case_model(name, prec="f16x3"):
    c = CASES[name][0]
    return build(gr.case_state_dict(c), H=c.H, L=c.L, act=c.act, prec=prec)


def inputs(case, counts, seed=11):
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    coords = np.random.default_rng(seed).uniform(-1.2, 1.2, size=(int(offsets[-1]), 2)).astype(np.float32)
    return syn.make_mods(2, case.L, len(counts), case.H, zero_fraction=case.zero_fraction), coords, offsets


def reference(case, mods, coords, offsets):
    """fp64, patch by patch -> (T,)"""
    sd = gr.case_state_dict(case)
    out = np.empty(len(coords), np.float64)
    for b in range(mods.shape[1]):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi > lo:
            out[lo:hi] = gr.value_and_grad(sd, mods[:, b:b + 1], coords[lo:hi], num_layers=case.L, activation=case.act)[0][0]
    return out


def bits(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32).view(np.uint32)


def native(m, mods, coords, offsets):
    return np.array(m.sample_mods_ragged(mods, coords, offsets, exact=False))


def range_events(m):
    n = C.c_int64()
    _lib.check(m._lib.msiren_range_events(m._h, C.byref(n)))
    return n.value


def kernels_of(m, fn):
    profile_on(m)
    try:
        out = fn()
        m.sync()
        return out, m.profile_kernels()
    finally:
        profile_off(m)


# ---- 1. values on each form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_values_vs_reference(name):
    case, kernel = CASES[name]
    m = case_model(name)
    mods, coords, offsets = inputs(case, COUNTS)
    out, entries = kernels_of(m, lambda: native(m, mods, coords, offsets))
    assert out.shape == (len(coords),) and out.dtype == np.float32
    assert [e["kernel"] for e in entries] == [kernel, COND % (case.act == "morlet")], entries
    assert entries[0]["launches"] == 1 and entries[0]["coords"] == len(coords), entries
    em, er = gr.distances(out, reference(case, mods, coords, offsets))
    print(f"{name}: max {em:.2e} rms {er:.2e} (norm {NORM_MAX:.0e} / {NORM_RMS:.0e})")
    assert em <= NORM_MAX and er <= NORM_RMS
    assert "ragged" not in m.last_trunk_kernel()  # (the ragged calls do not rename the last trunk)


# ---- 2. a coordinate's bits do not depend on where it stands -----------------------------------------------------------------------
def test_position_invariance():
    case, _ = CASES["H256-sine-L5"]
    m = case_model("H256-sine-L5")
    mods, coords, offsets = inputs(case, COUNTS)
    base = native(m, mods, coords, offsets)
    b = 5  # the patch of 130
    lo = int(offsets[b])
    probe, want = coords[lo + 7], bits(base[lo + 7])
    fill = np.random.default_rng(3).uniform(-1.2, 1.2, size=(100, 2)).astype(np.float32)  # three chunks and a ragged fourth
    for at in (0, 15, 16, 31, 32 + 5, 64 + 31):  # element 0 / 15 / 16 / 31 of a chunk (both column groups' ends), in a second and a third chunk
        for alone in (True, False):  # the patch alone, and inside the batch
            set_b = fill.copy()
            set_b[at] = probe
            if alone:
                out = native(m, mods[:, b:b + 1], set_b, np.array([0, len(set_b)], np.int32))
                got = out[at]
            else:
                counts = list(COUNTS)
                counts[b] = len(set_b)
                off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
                c2 = np.concatenate([coords[:lo], set_b, coords[int(offsets[b + 1]):]])
                out = native(m, mods, c2, off)
                got = out[lo + at]
                assert np.array_equal(bits(out[:lo]), bits(base[:lo]))  # the other patches' bits are untouched
            assert bits(got) == want, (at, alone)
    # a permutation of a patch's set permutes its outputs
    perm = np.random.default_rng(9).permutation(130)
    c2 = coords.copy()
    c2[lo:lo + 130] = coords[lo:lo + 130][perm]
    out = native(m, mods, c2, offsets)
    assert np.array_equal(bits(out[lo:lo + 130]), bits(base[lo:lo + 130][perm]))
    assert np.array_equal(bits(np.delete(out, np.arange(lo, lo + 130))), bits(np.delete(base, np.arange(lo, lo + 130))))
    # one stream and two streams, the device form, reruns: the same bits
    d_m, d_c = m.device_array(mods.shape).copy_from(mods), m.device_array(coords.shape).copy_from(coords)
    try:
        for n in (1, 2):
            _lib.check(m._lib.msiren_set_streams(m._h, n))
            for _ in range(n + 1):
                assert np.array_equal(bits(m.sample_mods_ragged(d_m, d_c, offsets, exact=False).numpy()), bits(base)), n
    finally:
        _lib.check(m._lib.msiren_set_streams(m._h, 1))
    assert np.array_equal(bits(native(m, mods, coords, offsets)), bits(base))


# ---- 3. more than one pass per workgroup -----------------------------------------------------------------------------------------------
def test_more_units_than_one_round():
    case, kernel = CASES["H256-sine-L5"]
    m = case_model("H256-sine-L5")
    counts = [13_000, 17_001, 9_999]  # T = 40 000 = 1 252 units of 32: more than 4 waves x 256 CUs
    mods, coords, offsets = inputs(case, counts, seed=21)
    out, entries = kernels_of(m, lambda: native(m, mods, coords, offsets))
    assert entries[0]["kernel"] == kernel and entries[0]["coords"] == 40_000, entries
    exact = np.asarray(m.sample_mods_ragged(mods, coords, offsets))
    em, er = gr.distances(out, exact)
    print(f"T = 40 000 against exact=True: max {em:.2e} rms {er:.2e}")
    assert em <= NORM_MAX and er <= NORM_RMS
    for b in range(3):  # the first and the last 64 outputs of each patch, recomputed as a small call
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        for a, z in ((lo, lo + 64), (hi - 64, hi)):
            small = native(m, mods[:, b:b + 1], coords[a:z], np.array([0, 64], np.int32))
            assert np.array_equal(bits(small), bits(out[a:z])), (b, a)
    assert np.array_equal(bits(native(m, mods, coords, offsets)), bits(out))  # (the pass counter is where the next call expects it)


# ---- 4. the domain guard ---------------------------------------------------------------------------------------------------------------
def test_domain_guard_returns_the_exact_bits():
    case, _ = CASES["H256-sine-L5"]
    m = case_model("H256-sine-L5")
    mods, coords, offsets = inputs(case, COUNTS)
    before = native(m, mods, coords, offsets)
    big = mods.copy()
    big[2, 3] *= 1e6  # one modulation row beyond fp16: patch 3 (32 coordinates), layer 2
    exact = np.asarray(m.sample_mods_ragged(big, coords, offsets))
    e0 = range_events(m)
    assert np.array_equal(bits(native(m, big, coords, offsets)), bits(exact))
    assert range_events(m) > e0, "the recipe no longer leaves the fp16 domain"
    d_m, d_c = m.device_array(big.shape).copy_from(big), m.device_array(coords.shape).copy_from(coords)
    assert np.array_equal(bits(m.sample_mods_ragged(d_m, d_c, offsets, exact=False).numpy()), bits(exact))  # the _dev form alike
    after = native(m, mods, coords, offsets)  # the next in-domain call is untouched
    assert np.array_equal(bits(after), bits(before)) and not np.array_equal(bits(after), bits(m.sample_mods_ragged(mods, coords, offsets)))


# ---- 5. fallback: an fp32 handle -------------------------------------------------------------------------------------------------------
def test_fp32_handle_runs_the_exact_kernel():
    case, _ = CASES["H256-sine-L5"]
    m = case_model("H256-sine-L5", "fp32")
    mods, coords, offsets = inputs(case, COUNTS)
    out, entries = kernels_of(m, lambda: native(m, mods, coords, offsets))
    assert [e["kernel"] for e in entries] == ["siren_trunk_f32_ragged_kernel<256,0,0>"], entries
    assert np.array_equal(bits(out), bits(m.sample_mods_ragged(mods, coords, offsets)))


# ---- 6. the device form with malformed offsets ---------------------------------------------------------------------------------------
def test_malformed_device_offsets_stay_inside_the_output():
    case, _ = CASES["H256-sine-L5"]
    m = case_model("H256-sine-L5")
    mods, coords, _ = inputs(case, [40, 50, 60])
    T, B, G = len(coords), 3, 64
    guard = np.float32(-12345.0)
    d_m, d_c = m.device_array(mods.shape).copy_from(mods), m.device_array(coords.shape).copy_from(coords)
    for bad in ([0, -7, 90, 150], [0, 100, 40, 150], [0, 40, 90, 10_000], [5, 3, 1 << 30, -(1 << 31)], [-1, -1, -1, -1], [T + 1] * 4):
        o = np.asarray(bad, np.int64).astype(np.int32)
        # what the exact _dev form documents: o0 = clamp(offsets[t], 0, T), o1 = clamp(offsets[t + 1], o0, T); patch t stores [o0, o1)
        o0 = np.clip(o[:-1].astype(np.int64), 0, T)
        o1 = np.clip(np.maximum(o[1:].astype(np.int64), o0), None, T)
        d_o = m.device_array((B + 1,))
        _lib.check(m._lib.msiren_memcpy_h2d(m._h, d_o.ptr, o.ctypes.data, o.nbytes))
        d_out = m.device_array((G + T + G,)).copy_from(np.full(G + T + G, guard, np.float32))
        _lib.check(m._lib.msiren_sample_ragged_mods_native_dev(m._h, d_c.ptr, d_o.ptr, d_m.ptr, B, T, d_out.ptr + 4 * G))
        m.sync()
        got = d_out.numpy()
        assert np.all(got[:G] == guard) and np.all(got[G + T:] == guard), bad  # the guard words around the buffer
        body = got[G:G + T]
        written = np.zeros(T, bool)
        for t in range(B):
            written[o0[t]:o1[t]] = True
        assert np.all(body[~written] == guard), bad
        for t in range(B):  # a patch whose clamped range overlaps no other's holds its own values
            others = np.zeros(T, bool)
            for u in range(B):
                if u != t:
                    others[o0[u]:o1[u]] = True
            if o1[t] > o0[t] and not others[o0[t]:o1[t]].any():
                want = native(m, mods[:, t:t + 1], coords[o0[t]:o1[t]], np.array([0, o1[t] - o0[t]], np.int32))
                assert np.array_equal(bits(body[o0[t]:o1[t]]), bits(want)), (bad, t)
        # the host forms refuse them
        out = np.empty(T, np.float32)
        assert m._lib.msiren_sample_ragged_mods_native(m._h, coords.ctypes.data, o.ctypes.data, mods.ctypes.data, B, T, out.ctypes.data) == _lib.E_INVALID, bad
        with pytest.raises(ValueError, match="offsets"):
            m.sample_mods_ragged(mods, coords, o, exact=False)


# ---- 7. resample ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resample_native():
    m = tr.model("f16x3")
    out, entries = kernels_of(m, lambda: np.array(m.resample(tr.images(), tr.data()["points"], exact=False)))
    return out, [e["kernel"] for e in entries]


def test_resample_vs_reference():
    d = tr.data()
    val, names = resample_native()
    ok = d["finite"]
    assert val.shape == (2, len(d["points"])) and val.dtype == np.float32
    assert names == ["resample_bin_kernels", "siren_trunk_f16x3n_ragged_kernel<0,3,5>", COND % 0, "resample_blend_kernel"], names
    em, er = gr.distances(val[:, ok], d["value"][:, ok])
    print(f"resample, native: max {em:.2e} rms {er:.2e} (norm {NORM_MAX:.0e} / {NORM_RMS:.0e})")
    assert em <= NORM_MAX and er <= NORM_RMS
    assert np.isnan(val[:, ~ok]).all()  # uncovered and non-finite points
    pts = d["points"]
    only_top = np.isfinite(pts).all(1) & (pts[:, 0] >= tr.LO) & (pts[:, 0] < 2 * tr.I - tr.PAD - tr.I) & (pts[:, 1] >= tr.LO) & (pts[:, 1] <= tr.HI)
    assert only_top.sum() >= 5 and np.all(val[1, only_top] == 0) and np.all(val[0, only_top] != 0)  # points under black tiles only


def test_resample_permutation_batch_and_rerun_bit_for_bit():
    d = tr.data()
    val, _ = resample_native()
    m = tr.model("f16x3")
    perm = np.random.default_rng(9).permutation(len(d["points"]))
    assert np.array_equal(bits(m.resample(tr.images(), d["points"][perm], exact=False)), bits(val[:, perm]))
    for s in range(2):  # a slice alone is the slice in the batch
        assert np.array_equal(bits(m.resample(tr.images()[s], d["points"], exact=False)), bits(val[s])), s
    assert np.array_equal(bits(m.resample(tr.images(), d["points"], exact=False)), bits(val))
    img, pts = tr.images(), d["points"]
    d_i, d_p, d_v = m.device_array(img.shape).copy_from(img), m.device_array(pts.shape).copy_from(pts), m.device_array(val.shape)
    _lib.check(m._lib.msiren_resample_slices_native_dev(m._h, d_i.ptr, 2, 40, 40, d_p.ptr, len(pts), d_v.ptr))
    m.sync()
    assert np.array_equal(bits(d_v.numpy()), bits(val))
    assert np.array_equal(bits(m.reconstruct(img)), bits(m.reconstruct(img)))  # (the slice pipeline's pass counter is intact)


# ---- 8. against the handle's sample_mods (shared set, layer-0 table built in fp64) ---------------------------------------------------
def test_against_the_shared_set_path():
    case, _ = CASES["H256-sine-L5"]
    m = case_model("H256-sine-L5")
    B, Q = 5, 70
    mods = syn.make_mods(2, case.L, B, case.H)
    shared = np.random.default_rng(4).uniform(-1.2, 1.2, size=(Q, 2)).astype(np.float32)
    coords, offsets = np.tile(shared, (B, 1)), np.arange(B + 1, dtype=np.int32) * Q
    rag = native(m, mods, coords, offsets).reshape(B, Q)
    tab = np.asarray(m.sample_mods(mods, shared))
    ref = gr.value_and_grad(gr.case_state_dict(case), mods, shared, num_layers=case.L, activation=case.act)[0]
    em, er = gr.distances(rag, tab)
    print(f"native ragged against sample_mods (layer 0 computed in fp32 / read from the fp64-built table): max {em:.2e} rms {er:.2e}; "
          f"against fp64: ragged {gr.distances(rag, ref)}, sample_mods {gr.distances(tab, ref)}")
    assert em <= NORM_MAX and er <= NORM_RMS
