"""The single-product 16-bit trunks (H = 512: siren_trunk_x1w_kernel, siren_trunk_x1n_kernel; BASELINE config 5) against their
operand-rounding oracle.

The fp64 oracle is a thousand times the distance the kernels should keep (the gates of test_config5_16bit_trunk_vs_own_oracle
measure the number format: 6e-2 / 8e-3).  oracle/x1_oracle.py restates the kernels' DOCUMENTED arithmetic with every operand
rounded where the headers say it is rounded; what is left between it and a correct kernel is the accumulation order and the
hardware sine.  The gate of a case (tests/x1_cases.py) is 4 x that noise floor, computed on the CPU inside the test from the
restatement alone; tests/test_x1_oracle.py shows on the CPU that a zeroed weight fragment, swapped weight rows or k-steps, a
dropped bias, another patch's modulation row and (where the floor allows) a wrong rounding mode land outside it.

Every case prints `X1GATE <case> floor <max> <rms> gpu <max> <rms>` before it asserts (LAB_NOTES.md holds a run's figures).
"""
import numpy as np
import pytest

import x1_cases as xc
from conftest import nerr
from mri_inr_amd import ModulatedSiren, _lib
from oracle import siren_oracle as orc

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)  # no sine is -7.25
PAD = 1024                    # floats in front of and behind the output window


def make(c: xc.Case, precision=None):
    """The case's model on the 16-bit trunk of its format (precision=None) or on another trunk of the same weights."""
    m = ModulatedSiren(dim_in=2, dim_hidden=xc.H, dim_out=1, num_layers=c.L, latent_dim=xc.Z, w0=c.w0, w0_initial=c.w0_initial,
                       use_bias=c.use_bias, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                       outer_patch_size=32, inner_patch_size=16, siren_patch_size=c.S, device="cuda", activation=c.act,
                       residual=c.res, **({"precision": precision or c.fmt} if (precision or c.fmt) != "fp32" else {}))
    m.load_state_dict(xc.state_dict(c), strict=False)
    m.to("cuda")
    return m


def check_gate(c: xc.Case, out, g=None):
    g = g or xc.gate(c)
    e, r = g.distance(out)
    te, tr = g.tol
    print(f"X1GATE {c.id} floor {g.floor_max:.2e} {g.floor_rms:.2e} gpu {e:.2e} {r:.2e} gate {te:.2e} {tr:.2e}")
    assert np.isfinite(out).all()
    assert e <= te and r <= tr, (c.id, e, r, te, tr)


def run(c: xc.Case, m=None):
    m = m or make(c)
    mods = xc.mods(c)
    out = m.forward_mods(mods)
    assert m.last_trunk_kernel() == c.kernel, (m.last_trunk_kernel(), c.kernel)
    assert out.shape == (c.B, c.S, c.S) and out.dtype == np.float32
    return m, mods, out.reshape(c.B, -1)


@pytest.mark.parametrize("c", xc.END_TO_END, ids=lambda c: c.id)
def test_all_sixteen_instances_end_to_end(c):
    """{bf16, f16} x {sine, morlet} x {residual, none}: ten layers reach the weight-stationary kernel, two the register-resident
    one.  9 tiles of 24 x 24."""
    m, mods, out = run(c)
    check_gate(c, out)
    assert np.array_equal(out, m.forward_mods(mods).reshape(c.B, -1))


@pytest.mark.parametrize("c", xc.MIDDLE, ids=lambda c: c.id)
def test_middle_layer_of_the_instances_without_the_residual(c):
    """Three layers without the residual on the four RES = 0 weight-stationary instances: layer 1, a middle layer of the pipeline,
    is one attenuating layer away from the output, at a floor of ~2e-4 (tests/test_x1_oracle.py seeds its errors there: a zeroed
    fragment is 35 x the bf16 gate, truncation in place of rounding 3 ... 5 x)."""
    m, mods, out = run(c)
    check_gate(c, out)
    assert np.array_equal(out, m.forward_mods(mods).reshape(c.B, -1))


@pytest.mark.parametrize("c", xc.ISOLATED, ids=lambda c: c.id)
def test_one_hidden_layer_at_a_time_in_the_deep_model(c):
    """Residual model of ten layers, modulations zero everywhere but in layers 0 and l: every other layer is x + 0 * act(..) = x
    exactly (repacking a 16-bit value is the identity), so layer l's weights, bias, modulation slot and pipeline slot are alone
    between the input and the output, at a floor of ~2e-4: a wrong fragment in that one layer is 2.4e-2."""
    _, _, out = run(c)
    check_gate(c, out)


@pytest.mark.parametrize("c", xc.SHAPES, ids=lambda c: c.id)
def test_ragged_units_and_pass_shapes(c):
    """P = 49, 100, 576, 1089 coordinates (a last unit of 17, 4, 32, 1 of 32) x batches of 1, 2, 7 tiles and, at P = 576, 57 tiles
    = 1026 units (one full round of 4-unit passes plus a 2-unit pass); three layers (the shortest weight-stationary pipeline)
    and two (register-resident).  Beyond the gate: the last patch's ragged unit is finite, and the launch writes nothing outside
    its B * P outputs (sentinels in front of and behind the window)."""
    m, mods, out = run(c)
    check_gate(c, out)
    P = c.S * c.S
    assert np.isfinite(out[-1, 32 * ((P - 1) // 32):]).all()
    d_mods = m.device_array(mods.shape).copy_from(mods)
    d_out = m.device_array((PAD + c.B * P + PAD,)).copy_from(np.full(PAD + c.B * P + PAD, SENTINEL, dtype=np.float32))
    _lib.check(m._lib.msiren_forward_mods_dev(m._h, d_mods.ptr, c.B, d_out.ptr + 4 * PAD))
    m.sync()
    buf = d_out.numpy()
    assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + c.B * P:] == SENTINEL).all()
    assert np.array_equal(buf[PAD:PAD + c.B * P].reshape(c.B, P), out)


@pytest.mark.parametrize("c", xc.OPTIONS, ids=lambda c: c.id)
def test_model_options(c):
    """use_bias = False (the accumulators start from a zero table) and w0 = 2 with w0_initial = 10 (the weights' w0/2pi scale and,
    for fp16, the power-of-two scale that follows it), four layers."""
    _, _, out = run(c)
    check_gate(c, out)


@pytest.mark.parametrize("c", xc.MAGNITUDES, ids=lambda c: c.id)
def test_modulation_magnitudes_inside_the_fp16_tables_range(c):
    """U(0.1, 0.6) x 1e-3, 1e2, 3e4: every modulation is an fp16 normal below 65 504 (the kernels read an fp16 table, the bf16
    instances too), so hardware denormal modes do not enter.  The gate applies wherever the exact-fp32 trunk of the same model
    still meets the fp64 oracle's 1e-4.  With modulations of 10 and more the sine arguments reach thousands of revolutions
    per layer: the fp32 trunk itself is then far from the fp64 oracle, no 16-bit reference means anything, and what is asserted
    is that the output is finite (for fp16 with the residual at x 3e4 the sums pass 65 504 and the launch is redone by the
    exact-fp32 trunk: finite as well)."""
    mods = xc.mods(c)
    assert (np.abs(mods) >= 2.0 ** -14).all() and (np.abs(mods) < 65504).all()
    m, _, out = run(c)
    assert np.isfinite(out).all()
    ref = orc.siren_forward(xc.state_dict(c), mods, num_layers=c.L, activation=c.act, residual=c.res, dtype=np.float64)
    e32 = nerr(make(c, "fp32").forward_mods(mods).reshape(c.B, -1), ref)
    print(f"X1MAG {c.id} fp32 trunk vs fp64 oracle {e32:.2e}")
    if e32 <= 1e-4:
        check_gate(c, out)
    else:
        assert c.mod_scale > 1.0  # small modulations never leave the gate


@pytest.mark.parametrize("L", [2, 10])
def test_bf16_modulations_beyond_the_fp16_table_are_redone_in_fp32(L):
    """The bf16 instances read their modulations from an fp16 table like the fp16 ones: U(0.1, 0.6) x 1e6 is inf there and NaN one
    sine later, where the exact-fp32 trunk of the same model is finite.  The promise of the f16 handles
    (test_f16_single_product_domain_identical_to_fp32_outside_it) holds for bf16 as well: a launch that stores a non-finite
    output raises its stream's flag and the exact-fp32 trunk behind it redoes the batch -- after a synchronous call and after
    msiren_forward_mods_dev + sync on one and two streams the buffer is finite and holds the exact-fp32 trunk's bits; inside the
    table's range nothing is redone."""
    c = xc.Case(fmt="bf16", L=L, B=9, sd_seed=27)
    m, f = make(c), make(c, "fp32")
    small = xc.mods(c)
    big = (small * np.float32(1e6)).astype(np.float32)
    want = f.forward_mods(big)
    assert np.isfinite(want).all()
    inside = m.forward_mods(small)
    assert m.last_trunk_kernel() == c.kernel
    assert np.isfinite(inside).all() and not np.array_equal(inside, f.forward_mods(small))
    got = m.forward_mods(big)
    assert np.isfinite(got).all()
    assert np.array_equal(got, want)
    d_big, d_small = m.device_array(big.shape).copy_from(big), m.device_array(small.shape).copy_from(small)
    for streams in (1, 2):
        _lib.check(m._lib.msiren_set_streams(m._h, streams))
        outs = [m.device_array((c.B, c.S, c.S)) for _ in range(6)]
        for k in range(6):  # flagged and clean launches interleaved
            _lib.check(m._lib.msiren_forward_mods_dev(m._h, (d_big if k % 2 == 0 else d_small).ptr, c.B, outs[k].ptr))
        m.sync()
        for k in range(6):
            assert np.array_equal(outs[k].numpy(), want if k % 2 == 0 else inside), (streams, k)
