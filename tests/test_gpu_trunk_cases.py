"""Every launched instance of the exact-fp32 and split-fp16 trunk families against the fp64 oracle, each case on the instance it
names (tests/trunk_cases.py; tests/test_trunk_cases.py shows on the CPU that the manifest is complete and its gate meaningful).

Per case: the handle is built as the case says, msiren_last_trunk_kernel must report the case's instance, msiren_range_events
must not move (a case that left the fp16 domain would test the fp32 rerun instead), the output meets the suite's gate against
oracle.siren_forward in fp64 (1e-4 max, 1e-5 rms, and max(10 e32, 2e-5): the fp32 noise floor of the same model), and a second
run gives the same bits.  Cases that share model and inputs over instances DESIGN.md 5.1 calls bit-identical agree bit for bit.

Guard cases: modulation elements of 1e5 that reach nothing downstream (their readers' weight columns are zero) put the 16-bit
launch outside its domain while the fp64 oracle still judges the output: the conditional exact-fp32 kernels behind the launch
(siren_trunk_f32_cond_kernel<ACT>; siren_trunk_f32_kernel<512,ACT,RES> behind the H = 512 trunks) have to run to the end.

Every case prints `TRUNKGATE <case> e32 .. gpu <max> <rms> gate ..` before it asserts (LAB_NOTES.md holds a run's figures).
"""
import ctypes as C
import os

import numpy as np
import pytest

import trunk_cases as tc
from mri_inr_amd import ModulatedSiren, _lib

pytestmark = pytest.mark.gpu

ids = lambda c: c.id


def make(c: tc.Case, precision=None):
    """The case's model under the case's environment knobs (read once, at msiren_create), or on another trunk of the same weights."""
    env = {k: str(v) for k, v in c.env.items()}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        m = ModulatedSiren(dim_in=2, dim_hidden=c.H, dim_out=1, num_layers=c.L, latent_dim=c.Z, w0=c.w0, w0_initial=c.w0_initial,
                           use_bias=c.use_bias, dropout=0.1, modulate=True, encoder_type="custom", encoder_path=None,
                           outer_patch_size=32, inner_patch_size=16, siren_patch_size=c.S, device="cuda", activation=c.act,
                           residual=c.residual, precision=precision or c.precision)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    m.load_state_dict(tc.state_dict(c), strict=False)
    m.to("cuda")
    _lib.check(m._lib.msiren_set_streams(m._h, c.streams))
    return m


def range_events(m) -> int:
    n = C.c_int64()
    _lib.check(m._lib.msiren_range_events(m._h, C.byref(n)))
    return n.value


def call(m, c: tc.Case, mods, dev=None):
    """One trunk call as the case says: the synchronous msiren_forward_mods, or msiren_forward_mods_dev + sync."""
    if not (c.dev if dev is None else dev):
        return m.forward_mods(mods).reshape(c.B, -1)
    d_mods, d_out = m.device_array(mods.shape).copy_from(mods), m.device_array((c.B, c.P))
    _lib.check(m._lib.msiren_forward_mods_dev(m._h, d_mods.ptr, c.B, d_out.ptr))
    m.sync()
    return d_out.numpy()


def check_gate(c: tc.Case, out, what="gpu"):
    (e, r), (te, tr) = tc.distance(c, out), tc.tolerance(c)
    print(f"TRUNKGATE {c.id} e32 {tc.e32(c):.2e} {what} {e:.2e} {r:.2e} gate {te:.2e} {tr:.2e} ratio {e / te:.2f}")
    assert out.dtype == np.float32 and np.isfinite(out).all()
    assert e <= te and r <= tr, (c.id, e, r, te, tr)


_outputs = {}   # case -> its output, for the bit-identity test below (filled by test_case_on_its_instance)


def run(c: tc.Case):
    m = make(c)
    mods = np.array(tc.mods(c))
    e0 = range_events(m)
    out = call(m, c, mods)
    assert m.last_trunk_kernel() == c.kernel, (m.last_trunk_kernel(), c.kernel)
    assert out.shape == (c.B, c.P)
    return m, mods, e0, out


@pytest.mark.parametrize("c", tc.F32 + tc.F16X3, ids=ids)
def test_case_on_its_instance(c):
    m, mods, e0, out = run(c)
    assert range_events(m) == e0
    check_gate(c, out)
    assert np.array_equal(out, call(m, c, mods))
    assert m.last_trunk_kernel() == c.kernel and range_events(m) == e0
    _outputs[c] = out


@pytest.mark.parametrize("group", tc.SAME_BITS, ids=lambda g: g[0].numerics.id)
def test_instances_that_share_a_case_give_the_same_bits(group):
    """the weight-stationary, the register-resident (ring of 3 or 4, unrolled or loop form) and the half-unit
    instance do the same arithmetic in the same order.  Depth 5: f16x3w = f16x3n<ACT,4,5> = f16x3h<ACT,4,5> = f16x3h<ACT,3,5>
    (7 tiles) and f16x3w = f16x3n<ACT,3,5> = f16x3n<ACT,4,5> (29 tiles); depths 3 and 4: f16x3w = f16x3n<ACT,4,0>; both
    activations, and Morlet with w0 = 1.5, w0_initial = 20, no bias."""
    outs = []
    for c in group:
        if c not in _outputs:   # (run alone, or the case's own test failed: run it here)
            _outputs[c] = run(c)[3]
        outs.append(_outputs[c])
    for c, o in zip(group[1:], outs[1:]):
        assert np.array_equal(o, outs[0]), (group[0].id, c.id, float(np.abs(o - outs[0]).max()))


@pytest.mark.parametrize("c", tc.GUARDS, ids=ids)
def test_guard_case_is_redone_by_the_conditional_fp32_kernel(c):
    """The profile lists the 16-bit trunk of a call, not the conditional launch behind it (launch_dispatch.hip), so the evidence
    that the conditional kernel ran is msiren_range_events plus the output: the 16-bit launch's own output for these inputs is
    NaN (H = 512: 0 * inf) or computed from an fp16 inf (H = 256), while the buffer must hold the exact-fp32 trunk's bits and
    meet the fp64 oracle -- on the synchronous call and on msiren_forward_mods_dev with one and two streams."""
    m, mods, e0, out = run(c)
    assert range_events(m) > e0, "the case no longer leaves the fp16 domain"
    check_gate(c, out)
    f = make(c, "fp32")
    want = call(f, c, mods)
    assert f.last_trunk_kernel() == f"siren_trunk_f32_kernel<{c.H},{tc.ACTS.index(c.act)},{int(c.residual)}>" and range_events(f) == 0
    check_gate(c, want, what="fp32")
    assert np.array_equal(out, want)
    # in-domain inputs on the same handle: nothing is redone, and the 16-bit kernel's own bits are not the fp32 trunk's
    plain = np.array(mods)
    for l, b, j in c.guard:
        plain[l, b, j] = 1.0
    for streams in (1, 2):
        _lib.check(m._lib.msiren_set_streams(m._h, streams))
        e1 = range_events(m)
        inside = call(m, c, plain, dev=True)
        assert range_events(m) == e1 and np.isfinite(inside).all() and not np.array_equal(inside, call(f, c, plain))
        for _ in range(2):   # (two calls: both streams of a two-stream handle)
            e1 = range_events(m)
            assert np.array_equal(call(m, c, mods, dev=True), want), streams
            assert range_events(m) > e1
    print(f"TRUNKGUARD {c.id} range_events {range_events(m)}")
