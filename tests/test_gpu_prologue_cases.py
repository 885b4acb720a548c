"""The split-fp16 prologue's kernels (encoder_conv_f16x3_kernel<1> + the nine latent_mods_f16x3_kernel instances) against their
operand-rounding oracle, one pinned case per instance and call shape (tests/prologue_cases.py).

The suite's older gate, 1e-5 against the fp64 oracle over the whole array, sits 25-100 times above the kernels: a single wrong
``lo`` fragment in conv3 (4e-6) passes it.  oracle/em_oracle.py restates the kernels' DOCUMENTED arithmetic; what is left
between it and a correct kernel is fp32 accumulation in the MFMA's own order.  The gate of a case is 4 x that floor, per row,
computed on the CPU from the restatement alone; tests/test_em_oracle.py shows on the CPU that it is at most half the smallest
seeded error and that every seeded error lands at least 2 x outside.

Per case: msiren_last_prologue_kernel reports the case's instance; latent and modulations within the gate; within the older
1e-5 of the fp64 oracle; modulations >= 0; the same bits on a rerun; the bits of the one launch (MODE 3) equal those of
model.encoder followed by model.modulator (MODE 1, MODE 2).  Every case prints
`EMGATE <case> <kernel> floor <latent> <mods> gate <latent> <mods> gpu <latent> <mods> = <fractions of the gate>` before it
asserts (LAB_NOTES.md section 16 holds a run's figures).
"""
import numpy as np
import pytest

import prologue_cases as pc
from conftest import nerr
from mri_inr_amd import _lib
from oracle import em_oracle as em
from test_gpu_parity import make_with_env

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)  # no modulation is negative
PAD = 1024                    # floats in front of and behind a device output window
_MODELS, _OUT = {}, {}


def model(c: pc.Case, precision=None):
    """The case's handle (cached: cases that differ in the call only share it)."""
    key = (c.numerics, precision or c.precision, c.em_depth)
    if key not in _MODELS:
        if len(_MODELS) >= 6:
            _MODELS.pop(next(iter(_MODELS)))
        _MODELS[key] = make_with_env(pc.state_dict(c), c.env, H=c.H, L=c.L, Z=c.Z, precision=precision or c.precision)
    return _MODELS[key]


def dev_call(m, t, streams, calls=1):
    """msiren_encode_modulate_tiles_dev on `streams` streams, `calls` times back to back into buffers of their own (two streams:
    consecutive calls alternate, one's prologue runs beside the other's) -> [(latent, mods)]; nothing is written outside them."""
    B, L, H, Z = t.shape[0], m.num_layers, m.dim_hidden, m.latent_dim
    _lib.check(m._lib.msiren_set_streams(m._h, streams))
    d_t = m.device_array(t.shape).copy_from(t)
    nz, nm = B * Z, L * B * H
    bufs = [(m.device_array((PAD + nz + PAD,)).copy_from(np.full(PAD + nz + PAD, SENTINEL, np.float32)),
             m.device_array((PAD + nm + PAD,)).copy_from(np.full(PAD + nm + PAD, SENTINEL, np.float32))) for _ in range(calls)]
    for d_z, d_m in bufs:
        _lib.check(m._lib.msiren_encode_modulate_tiles_dev(m._h, d_t.ptr, B, d_z.ptr + 4 * PAD, d_m.ptr + 4 * PAD))
    m.sync()
    name = m.last_prologue_kernel()
    _lib.check(m._lib.msiren_set_streams(m._h, 1))
    outs = []
    for d_z, d_m in bufs:
        z, mm = d_z.numpy(), d_m.numpy()
        for a, n in ((z, nz), (mm, nm)):
            assert (a[:PAD] == SENTINEL).all() and (a[PAD + n:] == SENTINEL).all()
        outs.append((z[PAD:PAD + nz].reshape(B, Z), mm[PAD:PAD + nm].reshape(L, B, H)))
    return outs, name


def run(c: pc.Case):
    """-> (latent (B, Z), mods (L, B, H)) of the case's call, with the kernel name(s) asserted; cached per case."""
    if c.id in _OUT:
        return _OUT[c.id]
    m, t = model(c), pc.tiles(c)
    if c.call == "host":
        mods, z = m.encode_modulate(t, return_latent=True)
        assert m.last_prologue_kernel() == c.kernel, (m.last_prologue_kernel(), c.kernel)
        mods2, z2 = m.encode_modulate(t, return_latent=True)
    elif c.call in ("dev1", "dev2"):
        outs, name = dev_call(m, t, int(c.call[-1]), calls=2)
        assert name == c.kernel, (name, c.kernel)
        (z, mods), (z2, mods2) = outs
    else:
        z = m.encoder(t)
        assert m.last_prologue_kernel() == c.kernel, (m.last_prologue_kernel(), c.kernel)
        mods = np.stack(m.modulator(z), 0)
        assert m.last_prologue_kernel() == c.kernel2, (m.last_prologue_kernel(), c.kernel2)
        z2, mods2 = m.encoder(t), np.stack(m.modulator(z), 0)
    assert z.shape == (c.B, c.Z) and mods.shape == (c.L, c.B, c.H) and z.dtype == mods.dtype == np.float32
    assert np.array_equal(z, z2) and np.array_equal(mods, mods2)  # the same bits on a rerun (two streams: side by side)
    if len(_OUT) >= 8:
        _OUT.pop(next(iter(_OUT)))
    _OUT[c.id] = (z, mods)
    return z, mods


@pytest.mark.parametrize("c", pc.CASES, ids=lambda c: c.id)
def test_every_instance_against_the_operand_rounding_oracle(c):
    z, mods = run(c)
    rows = list(c.eval_rows)
    g = pc.gate(c)
    (tz, tm), m = g.tol, model(c)
    zr, mr = z[rows], mods[:, rows]
    ez = pc.distance(zr, g.z)
    if c.call == "halves":
        # MODE 2 starts from the latent it is given: the restatement of the Modulator alone on the kernel's own latent, its own floor
        sd = pc.state_dict(c)
        q = em.prologue_forward(sd, z_in=zr, num_layers=c.L)[1]
        fm = pc.distance(em.prologue_forward(sd, z_in=zr, num_layers=c.L, accumulate="fp32_ksteps")[1], q)
        tm, em_ = pc.FACTOR * fm, pc.distance(mr, q)
    else:
        fm, em_ = g.floor_m, pc.distance(mr, g.mods)
    print(f"EMGATE {c.id} {m.last_prologue_kernel()} floor {g.floor_z:.2e} {fm:.2e} gate {tz:.2e} {tm:.2e} gpu {ez:.2e} {em_:.2e} "
          f"= {ez / tz:.2f} {em_ / tm:.2f} of gate")
    assert np.isfinite(z).all() and np.isfinite(mods).all() and (mods >= 0).all()
    assert ez <= tz and em_ <= tm, (c.id, ez, tz, em_, tm)
    z64, m64 = pc.ref64(c)  # the older gate stays: the whole array against the fp64 oracle
    assert nerr(zr, z64) < pc.FP64_TOL and nerr(mr, m64) < pc.FP64_TOL
    for l in range(c.L):    # (and per layer, so that a small layer does not hide behind a large one)
        assert nerr(mr[l], m64[l]) < pc.FP64_TOL, l
    # one launch (the latent stays in the workgroup) against the two halves through HBM: the same bits
    if c.call == "halves":
        m3, z3 = m.encode_modulate(pc.tiles(c), return_latent=True)
        assert m.last_prologue_kernel().endswith(",3>")
    else:
        z3 = m.encoder(pc.tiles(c))
        m3 = np.stack(m.modulator(z3), 0)
        assert m.last_prologue_kernel().endswith(",2>")
    assert np.array_equal(z3, z) and np.array_equal(m3, mods)


@pytest.mark.parametrize("grp", pc.SAME_BITS, ids=lambda g: g[0].numerics.id)
def test_instances_of_one_shape_give_the_same_bits(grp):
    """One model, one batch: ring depths 2, 4 and 8, one stream alone (H = 256: with the 64 prefetch workgroups) against two
    streams (without), the synchronous host call against the asynchronous one, bf16 against f16 handles."""
    z0, m0 = run(grp[0])
    for c in grp[1:]:
        z, m = run(c)
        assert np.array_equal(z, z0) and np.array_equal(m, m0), (grp[0].id, c.id)


@pytest.mark.parametrize("H,L,precision", [(256, 5, "f16x3"), (512, 10, "bf16"), (256, 5, "fp32")])
def test_scaling_a_row_by_a_power_of_two_scales_its_outputs_exactly(H, L, precision):
    """With every bias of the encoder and the Modulator zero the chain is positively homogeneous (LeakyReLU, ReLU) and every scale
    of the split-fp16 arithmetic is an exact power of two: row r of the tiles times 2^k scales that row's latent and modulations
    by exactly 2^k -- bit for bit, no tolerance -- and leaves every other row's bits alone.  k per row from [-30, 30] inside one
    row block (17 rows: the block and a ragged one), some rows unscaled, one row zero; every intermediate is a normal fp32
    number (checked on the restatement).  A kernel that took its block's maximum, or a neighbour's, for a row's scale fails this
    on the rows whose neighbours moved.  The fp32 handle runs its per-layer launches: the same property, no scales involved."""
    n = pc.Case("", H=H, L=L, B=17, weights="nobias", sd_seed=12 if H == 256 else 9, in_seed=50, precision=precision)
    sd = pc.state_dict(n)
    rng = np.random.default_rng(51)
    t = pc.tiles(n).copy()
    t[7] = 0.0
    k = rng.permutation(np.round(np.linspace(-30, 30, n.B)).astype(np.int64))  # every row its own power of two, -30 .. 30, shuffled
    k[[2, 9, 16]] = 0
    k[[0, 12]] = -30, 30
    assert k.min() == -30 and k.max() == 30 and (k == 0).sum() >= 3
    ts = np.ldexp(t, k[:, None, None]).astype(np.float32)
    feats = em.prologue_forward(sd, ts, num_layers=L, return_features=True)
    for a in feats:  # every intermediate of the scaled run: zero or a normal number with room to spare
        nz = np.abs(a[a != 0])
        assert nz.min() > 2.0 ** -100 and nz.max() < 2.0 ** 100
    m = model(n)
    assert m.last_prologue_kernel() == ""
    mods, z = m.encode_modulate(t, return_latent=True)
    name = m.last_prologue_kernel()
    assert name == ("" if precision == "fp32" else f"latent_mods_f16x3_kernel<{H // 128},{n.Z // 128},8,3>"), name
    mods_s, z_s = m.encode_modulate(ts, return_latent=True)
    assert np.abs(z[0]).max() > 0 and np.abs(mods[-1, 0]).max() > 0 and not z[7].any() and not mods[:, 7].any()
    assert np.array_equal(z_s, np.ldexp(z, k[:, None]))
    assert np.array_equal(mods_s, np.ldexp(mods, k[None, :, None]))
    # one row alone moves: the others keep their bits (row 4 up by 2^25 beside its unscaled neighbours)
    t1 = t.copy()
    t1[4] = np.ldexp(t[4], 25)
    mods_1, z_1 = m.encode_modulate(t1, return_latent=True)
    keep = [r for r in range(n.B) if r != 4]
    assert np.array_equal(z_1[keep], z[keep]) and np.array_equal(mods_1[:, keep], mods[:, keep])
    assert np.array_equal(z_1[4], np.ldexp(z[4], 25)) and np.array_equal(mods_1[:, 4], np.ldexp(mods[:, 4], 25))
    if precision != "fp32":  # the asynchronous call on two streams (ring of 2 at H = 256): the same
        (za, ma), = dev_call(m, ts, 2)[0]
        assert np.array_equal(za, z_s) and np.array_equal(ma, mods_s)


def test_fp32_handle_reports_no_prologue_instance_and_meets_the_fp64_oracle():
    """An fp32 handle runs the exact-fp32 launches per layer behind the same entry point: msiren_last_prologue_kernel is empty."""
    n = next(x for x in pc.CASES if x.L == 5 and x.inputs == "uniform" and x.call == "host" and x.em_depth is None and x.H == 256)
    m = model(n, precision="fp32")
    mods, z = m.encode_modulate(pc.tiles(n), return_latent=True)
    assert m.last_prologue_kernel() == ""
    z64, m64 = pc.ref64(n)
    assert nerr(z, z64) < pc.FP64_TOL and nerr(mods, m64) < pc.FP64_TOL and (mods >= 0).all()
    assert np.array_equal(z, m.encoder(pc.tiles(n))) and np.array_equal(mods, np.stack(m.modulator(z), 0))
    assert np.array_equal(mods, m.encode_modulate(pc.tiles(n)))  # the latent may be left out


def test_a_host_call_that_cuts_itself_runs_its_chunks_prologues_and_gives_the_same_bits():
    """msiren_encode_modulate_tiles follows msiren_forward_tiles' plan (host_plan.h): with MSIREN_HOST_PIPE_MIN=128 a call of 300
    tiles is two chunks on two streams, the second one's prologue beside the first one's trunk -- the ring of 2 -- and its rows
    land behind the first chunk's in every layer.  Same bits as the one-chunk call; and the trunk on these modulations is
    msiren_forward_tiles, bit for bit."""
    n = pc.Case("", L=5, B=300, sd_seed=7, in_seed=60)
    t = pc.tiles(n)
    whole = model(n)
    mods, z = whole.encode_modulate(t, return_latent=True)
    assert whole.last_prologue_kernel() == "latent_mods_f16x3_kernel<2,2,8,3>"
    cut = make_with_env(pc.state_dict(n), {"MSIREN_HOST_PIPE_MIN": 128}, precision="f16x3")
    mods_c, z_c = cut.encode_modulate(t, return_latent=True)
    assert cut.last_prologue_kernel() == "latent_mods_f16x3_kernel<2,2,2,3>"
    assert np.array_equal(z_c, z) and np.array_equal(mods_c, mods)
    assert np.array_equal(cut.encode_modulate(t), mods)
    out = whole(t)
    assert np.array_equal(whole.forward_mods(mods), out) and np.array_equal(cut(t), out)
