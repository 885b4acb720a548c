"""oracle/x1_oracle.py (the single-product 16-bit trunk with its documented roundings) on the CPU:

* with every rounding off it IS the fp64 oracle the rest of the suite trusts (pins the restatement's structure);
* its rounding helpers round as the formats do;
* the gate built on it (tests/x1_cases.py, used by tests/test_gpu_x1.py on the kernels) can fail: errors of the kind that
  hand-placed fragment orders, weights addressed by register name and epilogues interleaved into MFMA gaps produce, seeded
  into the restatement through its test-only hook, land outside it -- and a second, independently seeded legitimate variation
  lands inside;
* the reference-only noise floor of every gated case stays within the caps, so the gate cannot quietly become meaningless.
"""
import numpy as np
import pytest

import x1_cases as xc
from conftest import nerr
from mri_inr_amd import synthetic as syn
from oracle import siren_oracle as orc
from oracle import x1_oracle as x1


# ---- structure ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [7, 24])
@pytest.mark.parametrize("w0,w0_initial", [(1.0, 30.0), (2.0, 10.0)])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("act", ["sine", "morlet"])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_roundings_disabled_equals_fp64_oracle(fmt, act, res, bias, w0, w0_initial, S):
    """The scaling by w0/2pi and 2^e, the activation in revolutions, the bias as the accumulator's initial value and 2^-e behind the
    accumulation are a restatement of siren_forward, not another model: without the roundings the two agree to fp64 rounding."""
    L, B = 4, 3
    sd = syn.make_state_dict(seed=33, dim_hidden=512, num_layers=L, latent_dim=128, siren_patch_size=S, w0=w0, use_bias=bias,
                             with_encoder=False)
    mods = syn.make_mods(12, L, B, 512, lo=0.1, hi=0.6)
    got = x1.x1_forward(sd, mods, num_layers=L, fmt=fmt, residual=res, activation=act, w0=w0, w0_initial=w0_initial,
                        siren_patch_size=S, use_bias=bias, roundings=False)
    ref = orc.siren_forward(sd, mods, num_layers=L, w0=w0, w0_initial=w0_initial, activation=act, siren_patch_size=S,
                            residual=res, dtype=np.float64)
    assert got.shape == ref.shape == (B, S * S) and got.dtype == np.float64
    assert np.abs(ref).max() > 1e-2  # not a degenerate output
    assert np.abs(got - ref).max() <= 1e-12, np.abs(got - ref).max()
    # and with them the distance is the format's, not zero: the switch switches something
    q = x1.x1_forward(sd, mods, num_layers=L, fmt=fmt, residual=res, activation=act, w0=w0, w0_initial=w0_initial,
                      siren_patch_size=S, use_bias=bias)
    assert 1e-5 < nerr(q, ref) < (2e-2 if fmt == "bf16" else 3e-3), nerr(q, ref)


# ---- roundings ---------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_bf16_round_to_nearest_even_on_bit_patterns():
    f = lambda u: np.array(u, dtype=np.uint32).view(np.float32)
    # below, at (ties to even, both parities) and above the midpoint; carry into the exponent; overflow to inf; signs; inf
    src = f([0x3F800000, 0x3F807FFF, 0x3F808000, 0x3F808001, 0x3F818000, 0x3F81FFFF, 0x3FFF8000, 0x7F7F8000, 0xBF808001,
             0x7F800000, 0x00000000, 0x80000000, 0x00008000, 0x00018000])
    want = [0x3F800000, 0x3F800000, 0x3F800000, 0x3F810000, 0x3F820000, 0x3F820000, 0x40000000, 0x7F800000, 0xBF810000,
            0x7F800000, 0x00000000, 0x80000000, 0x00000000, 0x00020000]
    assert _bits(x1.rne_bf16(src)).tolist() == want
    assert np.isnan(x1.rne_bf16(f([0x7FC00000, 0x7F800001, 0xFFFFFFFF]))).all()
    # against exact arithmetic: the result is a bf16 value, at most half a bf16 ulp away, and no other bf16 value is nearer
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(200000) * np.exp(rng.uniform(-30, 30, 200000))).astype(np.float32)
    r = x1.rne_bf16(x)
    assert (_bits(r) & 0xFFFF == 0).all()
    ulp = np.ldexp(1.0, np.frexp(x.astype(np.float64))[1] - 1 - 7)  # bf16: 8 significant bits
    assert (np.abs(r.astype(np.float64) - x) <= ulp / 2).all()
    t = x1.trunc_bf16(x)
    assert (np.abs(t) <= np.abs(x)).all() and (np.abs(t.astype(np.float64) - x) < ulp).all()
    assert (r != t).mean() > 0.4  # truncation is another rounding on about half of the values


def test_f16_rounding_and_truncation():
    x = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.0, 65520.0, 1e6, -1e6, 6e-8], dtype=np.float32)
    r = x1.rne_f16(x)
    assert r.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -9, 65504.0, 65504.0, np.inf, np.inf, -np.inf, 2.0 ** -24]
    rng = np.random.default_rng(4)
    y = (rng.standard_normal(100000) * np.exp(rng.uniform(-8, 8, 100000))).astype(np.float32)
    t = x1.trunc_f16(y)
    assert (t.astype(np.float16).astype(np.float32) == t).all()
    assert (np.abs(t) <= np.abs(y)).all()
    assert (np.abs(np.nextafter(t.astype(np.float16), np.float16(np.inf) * np.sign(y).astype(np.float16)).astype(np.float32)) > np.abs(y)).all()


@pytest.mark.parametrize("scale", [1.0, 37.0, 1e-3])
def test_fp16_weight_scale_brings_the_largest_weight_under_16384(scale):
    W = (np.random.default_rng(5).uniform(-0.108, 0.108, (512, 512)) * scale).astype(np.float32)
    c = 1.0 / x1.TWO_PI
    e = x1.weight_scale_exponent(W, c, "f16")
    assert 8192.0 <= np.abs(W.astype(np.float64) * c).max() * 2.0 ** e < 16384.0
    assert x1.weight_scale_exponent(W, c, "bf16") == 0


# ---- the gate ----------------------------------------------------------------------------------------------------------------------
def _gate_applies_on_cpu(c):
    """Modulation magnitudes: the gate applies where an fp32 evaluation of the same model still meets the fp64 oracle's 1e-4 (on
    the GPU file: the fp32-trunk handle).  Beyond it the sine arguments are so large that no 16-bit reference means anything."""
    if c.mod_scale == 1.0:
        return True
    kw = dict(num_layers=c.L, w0=c.w0, w0_initial=c.w0_initial, activation=c.act, siren_patch_size=c.S, residual=c.res)
    ref = orc.siren_forward(xc.state_dict(c), xc.mods(c), dtype=np.float64, **kw)
    return nerr(orc.siren_forward(xc.state_dict(c), xc.mods(c), dtype=np.float32, **kw), ref) <= 1e-4


@pytest.mark.parametrize("c", xc.GATED, ids=lambda c: c.id)
def test_floor_of_every_gated_case_stays_within_its_caps(c):
    if not _gate_applies_on_cpu(c):
        assert c in xc.MAGNITUDES and c.mod_scale > 1.0  # only the large-magnitude cases may leave the gate
        return
    g = xc.gate(c)
    assert np.isfinite(g.q).all() and np.abs(g.q).max() > 1e-2
    assert 0.0 < xc.FACTOR * g.floor_max <= c.caps[0] and 0.0 < xc.FACTOR * g.floor_rms <= c.caps[1], (g.floor_max, g.floor_rms)
    assert g.passes(g.q)


def test_every_instance_and_every_deep_layer_has_a_case():
    names = {c.kernel for c in xc.END_TO_END}
    assert len(names) == 16 and all(c.B == 9 and c.S == 24 for c in xc.END_TO_END)
    for f in xc.FMTS:
        assert {c.isolate for c in xc.ISOLATED if c.fmt == f and c.act == "sine"} == set(range(1, 10))
        assert {c.isolate for c in xc.ISOLATED if c.fmt == f and c.act == "morlet"} == {1, 9}
    assert {c.S * c.S for c in xc.SHAPES} == {49, 100, 576, 1089} and {c.B for c in xc.SHAPES} == {1, 2, 7, 57}
    assert all(c.res and c.L == 10 and c.kernel.startswith("siren_trunk_x1w") for c in xc.ISOLATED)
    # the middle hidden layer of the four instances without the residual: three layers, errors seeded into layer 1
    assert {c.kernel for c in xc.MIDDLE} == {f"siren_trunk_x1w_kernel<{b},{a},0>" for b in (0, 1) for a in (0, 1)}
    assert all(c.L == 3 and not c.res and c.B == 9 and c.S == 24 and xc.seeded_layer(c) == 1 and c.caps == xc.CAP_SHALLOW for c in xc.MIDDLE)
    for c in xc.ISOLATED:  # the isolation is exact: every other hidden layer's modulation row is zero
        m = xc.mods(c)
        assert all((m[l] == 0).all() == (l not in (0, c.isolate)) for l in range(c.L))


@pytest.mark.parametrize("c", xc.END_TO_END + xc.ISOLATED + xc.MIDDLE, ids=lambda c: c.id)
def test_seeded_errors_land_outside_the_gate(c):
    """Each error goes into ONE hidden layer of the restatement (x1_cases.seeded_errors) on the inputs the GPU file uses.

    Not seeded: a wrong rounding mode end to end at num_layers = 10.  Measured there (distance / gate, max and rms): truncation
    of one layer's output 0.2 ... 0.6 (one instance: 1.5 in rms), of every layer's 0.4 ... 1.3 (LAB_NOTES.md) -- the deep gate,
    whose floor is the model's own amplification of fp32 summation order, does not see a rounding mode reliably.  The isolated-layer cases (l = 1 .. 8, both formats) and the two-layer instances do, and assert it here."""
    g = xc.gate(c)
    errs = xc.seeded_errors(c)
    want = {"weight_fragment_zeroed", "weight_rows_swapped", "ksteps_swapped", "bias_dropped", "modulation_row_of_next_patch"}
    if (c.isolate and c.isolate < c.L - 1) or (not c.isolate and c.L <= 4):
        want.add("activations_truncated")
    assert set(errs) == want
    te, tr = g.tol
    for name, kw in errs.items():
        bad = xc.forward(c, **kw)
        e, r = g.distance(bad)
        print(f"X1SEED {c.id} {name} max {e:.2e} ({e / te:.1f} x gate) rms {r:.2e} ({r / tr:.1f} x gate)")
        assert not g.passes(bad) and (e > te or r > tr), (name, e, r, te, tr)
    # the other direction: a legitimate variation with seeds of its own (another k order, other sine signs) is inside
    other = xc.forward(c, accumulate=np.float32, perturb=x1.Perturb(seed=77))
    assert g.passes(other), (g.distance(other), g.tol)
