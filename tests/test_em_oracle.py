"""oracle/em_oracle.py (the split-fp16 prologue with its documented roundings) and tests/prologue_cases.py on the CPU:

* with every rounding off the restatement IS the fp64 oracle the rest of the suite trusts (pins its structure: the powers of
  two, conv3's k order and halves, the padded k-steps, the hoisted latent part);
* its split and scale helpers round and scale as ``em_split8``, ``em_row_scale`` and ``scale_of`` do; conv3's k order as the
  packer states it is the order in which the conv kernel's threads store their features;
* the manifest names every latent_mods instance of trunk_instances.h, and pick_prologue (dispatch.h, compiled with g++)
  returns each case's name for the handle and call the case describes;
* the gate built on it (used by tests/test_gpu_prologue_cases.py on the kernels) can fail: 4 x floor of every case is at most
  half the distance of the smallest seeded error -- one ``lo`` fragment of conv3 zeroed for one k-step -- and every error of the
  kind a ring slot refilled late, a packer index off by one or a wrong scale produces, seeded into the restatement through its
  test-only hook in every stage it applies to, lands at least 2 x outside; a second legitimate variant (another grouping of
  each MFMA's sum, seeded) lands inside.

Every figure is printed (`EMFLOOR`, `EMSEED` lines; LAB_NOTES.md section 16 holds a run's).
"""
import os
import re
import shutil
import subprocess
import textwrap
from dataclasses import replace

import numpy as np
import pytest

import prologue_cases as pc
from mri_inr_amd import synthetic as syn
from oracle import em_oracle as em
from oracle import siren_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mri_inr_amd", "csrc")
ids = lambda c: c.id


# ---- structure ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Z,L", [(256, 256, 1), (256, 256, 2), (256, 256, 5), (256, 256, 7), (512, 128, 2), (512, 128, 10)])
def test_roundings_disabled_equals_fp64_oracle(H, Z, L):
    sd = syn.make_state_dict(seed=7 if H == 256 else 9, dim_hidden=H, num_layers=L, latent_dim=Z, trained_like=True)
    t = np.random.default_rng(3).random((5, 32, 32), dtype=np.float32)
    t[3] *= np.float32(1e-5)
    z64 = orc.encoder_forward(sd, t, dtype=np.float64)
    m64 = orc.modulator_forward(sd, z64, num_layers=L, dtype=np.float64)
    z, m, feat = em.prologue_forward(sd, t, num_layers=L, roundings=False, return_features=True)
    assert z.shape == (5, Z) and m.shape == (L, 5, H) and feat.shape == (5, 2048) and z.dtype == m.dtype == np.float64
    assert np.abs(z64).max() > 1.0 and np.abs(m64).max() > 0.5  # not a degenerate model
    assert np.abs(z - z64).max() <= 1e-12 and np.abs(m - m64).max() <= 1e-12, (np.abs(z - z64).max(), np.abs(m - m64).max())
    # the accumulation switch changes nothing that is not a rounding; neither does the entry at the latent (MODE 2) or the encoder alone
    zk, mk = em.prologue_forward(sd, t, num_layers=L, roundings=False, accumulate="fp64", group_seed=3)
    assert np.array_equal(zk, z) and np.array_equal(mk, m)
    assert np.abs(em.prologue_forward(sd, z_in=z64.astype(np.float32), num_layers=L, roundings=False)[1]
                  - orc.modulator_forward(sd, z64.astype(np.float32), num_layers=L, dtype=np.float64)).max() <= 1e-12
    assert np.array_equal(em.prologue_forward(sd, t, num_layers=L, roundings=False, modulate=False)[0], z)
    # with the roundings the distance is the arithmetic's, per row: not zero, and far below the suite's 1e-5
    zq, mq = em.prologue_forward(sd, t, num_layers=L)
    for e in (pc.row_distance(zq, z64), pc.row_distance(mq, m64)):
        assert (e > 0).all() and (e < 1e-6).all(), e
    for kw in (dict(accumulate="fp32_ksteps"), dict(accumulate="fp32_ksteps", group_seed=1)):
        zk, mk = em.prologue_forward(sd, t, num_layers=L, **kw)
        assert 0 < pc.distance(zk, zq) < 1e-6 and 0 < pc.distance(mk, mq) < 1e-6


def test_conv3_k_order_of_the_packer_is_the_conv_kernels_store_order():
    """em_oracle.conv3_ksteps restates weights_pack.hip:477-483 (which feature the packer puts at element j of lane q of k-step s).
    The conv kernel's side, stated independently from encoder_modulator_f16x3.hip.h:474-476 and :586-589: thread (wave w, lane) holds
    channel 16 (w & 1) + 4 (lane >> 4) + r at position 16 (2 (w >> 1) + t) + (lane & 15) as element j = 4 t + r, and stores its
    eight values as the piece (k-step 16 w + (lane >> 2), q = lane & 3)."""
    ks = em.conv3_ksteps()
    assert sorted(ks.ravel().tolist()) == list(range(2048))
    for w in range(4):
        for lane in range(64):
            for j in range(8):
                t, r = j >> 2, j & 3
                feature = (16 * (w & 1) + 4 * (lane >> 4) + r) * 64 + 16 * (2 * (w >> 1) + t) + (lane & 15)
                assert ks[16 * w + (lane >> 2), 8 * (lane & 3) + j] == feature
    assert np.array_equal(em.natural_ksteps(128), np.arange(128).reshape(4, 32))


# ---- roundings and scales ------------------------------------------------------------------------------------------------------------
def _f16_bits(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def test_split_rounds_as_fp16_does():
    f = lambda *v: np.array(v, dtype=np.float32)
    # ties to even on hi (1 + 2^-11 -> 1, 1 + 3 2^-11 -> 1 + 2^-9), the residual exact in lo; hi's bit patterns
    hi, lo = em.split_f16(f(1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -22, -(1.0 + 2.0 ** -11)))
    assert _f16_bits(hi).tolist() == [0x3C00, 0x3C02, 0x3C01, 0xBC00]
    assert lo.tolist() == [2.0 ** -11, -(2.0 ** -11), -(2.0 ** -11) + 2.0 ** -22, -(2.0 ** -11)]
    # the 2^14 edge of the scaled range: the largest fp32 below 2^14 rounds up to 2^14 in hi, lo takes the (negative) rest
    hi, lo = em.split_f16(np.nextafter(f(16384.0), f(0.0)))
    assert hi.tolist() == [16384.0] and lo.tolist() == [-(2.0 ** -10)]
    # ties in lo: hi = 1024 (ulp 1), the residual 0.25 + 2^-13 | 0.25 + 3 2^-13 lies halfway between two fp16 values (ulp 2^-12): to even
    hi, lo = em.split_f16(f(1024.25 + 2.0 ** -13, 1024.25 + 3 * 2.0 ** -13))
    assert hi.tolist() == [1024.0, 1024.0] and lo.tolist() == [0.25, 0.25 + 2.0 ** -11]
    # subnormal lo: below 2^-14 the residual keeps multiples of 2^-24 only (round to nearest even), and flushes nothing
    hi, lo = em.split_f16(f(0.25 + 2.0 ** -15 + 2.0 ** -25, 0.25 + 3 * 2.0 ** -25, 2.0 ** -25, 3 * 2.0 ** -25))
    assert hi.tolist() == [0.25, 0.25, 0.0, 2.0 ** -23] and lo.tolist() == [2.0 ** -15, 2.0 ** -23, 0.0, 0.0]
    # beyond the fp16 range hi is inf (65 520 rounds up) and the row is lost, as the header says of non-finite inputs
    hi, lo = em.split_f16(f(65519.0, 65520.0))
    assert hi.tolist() == [65504.0, np.inf] and lo[0] == 15.0 and not np.isfinite(lo[1])
    # against exact arithmetic: hi and lo are fp16 values, hi is the nearest one, hi + lo is within 2^-22 of v (22 significant
    # bits) wherever lo is a normal number, and within 2^-25 absolute below
    rng = np.random.default_rng(3)
    v = (rng.uniform(-1, 1, 200000) * np.exp2(rng.uniform(-12, 14, 200000))).astype(np.float32)
    hi, lo = em.split_f16(v)
    assert (hi.astype(np.float16).astype(np.float32) == hi).all() and (lo.astype(np.float16).astype(np.float32) == lo).all()
    v64, hi64, lo64 = v.astype(np.float64), hi.astype(np.float64), lo.astype(np.float64)
    ulp_hi = np.maximum(np.exp2(np.frexp(v64)[1] - 1 - 10), 2.0 ** -24)
    assert (np.abs(v64 - hi64) <= ulp_hi / 2).all()
    err = np.abs(v64 - (hi64 + lo64))
    assert (err <= np.maximum(np.abs(v64) * 2.0 ** -22, 2.0 ** -25)).all()
    th, tl = em.split_f16(v, em.trunc_f16)
    assert (np.abs(th) <= np.abs(v)).all() and (th != hi).mean() > 0.4  # truncation is another rounding on about half of the values


def test_scale_helpers_reproduce_em_row_scale_and_scale_of():
    f = lambda *v: np.array(v, dtype=np.float32)
    one = np.float32(1.0)
    # exact powers of two and one ulp either side: m 2^s in [2^13, 2^14)
    m = f(1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), 8192.0, 16384.0, np.nextafter(np.float32(16384.0), np.float32(0)),
          2.0 ** -20, 1e-5, 3.0e38)
    s = em.row_scale_exponent(m)
    scaled = m.astype(np.float64) * np.exp2(s.astype(np.float64))
    assert ((scaled >= 8192.0) & (scaled < 16384.0))[:-1].all()
    assert s.tolist() == [13, 14, 13, 0, -1, 0, 33, 30, -100]
    # zero (and NaN): 0; the clamp: +-100, so that 2^s and 2^-s are normal numbers; subnormal maxima and inf end at the clamp
    assert em.row_scale_exponent(f(0.0, np.nan, 2.0 ** -100, 2.0 ** -120, 1e-45, 2.0 ** 120, np.inf)).tolist() == [0, 0, 100, 100, 100, -100, -100]
    assert em.row_scale_exponent(f(2.0 ** -86, 2.0 ** -87, 2.0 ** 113, 2.0 ** 114)).tolist() == [99, 100, -100, -100]
    # scale_of: the same interval, from frexp of the fp64 maximum; a zero or non-finite layer: 0
    for w, a in ((1.0, 13), (float(np.nextafter(one, np.float32(0))), 14), (float(np.nextafter(one, np.float32(2))), 13), (16384.0, -1), (0.0416, 18)):
        assert em.weight_scale_exponent(np.array([[w, -w / 3], [0.0, w / 7]])) == a
        assert 8192.0 <= w * 2.0 ** a < 16384.0
    assert em.weight_scale_exponent(np.zeros((3, 3))) == 0 and em.weight_scale_exponent(np.array([1.0, np.inf])) == 0
    assert em.weight_scale_exponent(np.array([2.0 ** -120])) == 100 and em.weight_scale_exponent(np.array([-2.0 ** 120])) == -100


# ---- the manifest --------------------------------------------------------------------------------------------------------------------
def prologue_instances():
    text = open(os.path.join(CSRC, "trunk_instances.h")).read()
    block = text[text.index("#define MSIREN_PROLOGUE_INSTANCES"):text.index("// HIP units only")]
    return {f"latent_mods_f16x3_kernel<{a}>" for a in re.findall(r"X\(latent_mods, ([\d,]+)\)", block)}


def test_every_prologue_instance_has_a_case():
    inst = prologue_instances()
    assert len(inst) == 9
    named = {c.kernel for c in pc.CASES} | {c.kernel2 for c in pc.CASES if c.call == "halves"}
    assert named == inst, sorted(named ^ inst)
    by = lambda k: [c for c in pc.CASES if c.kernel == k]
    # every mode-3 instance by the call production reaches it with; where MSIREN_EM_DEPTH is used, it is a second reach
    assert {c.call for c in by("latent_mods_f16x3_kernel<2,2,8,3>")} >= {"host", "dev1"}
    assert any(c.call == "dev2" and c.em_depth is None for c in by("latent_mods_f16x3_kernel<2,2,2,3>"))
    assert any(c.call == "dev1" and c.em_depth is None and c.B > 16 * 256 for c in by("latent_mods_f16x3_kernel<2,2,4,3>"))
    assert any(c.em_depth == 4 for c in by("latent_mods_f16x3_kernel<2,2,4,3>")) and any(c.em_depth == 2 for c in by("latent_mods_f16x3_kernel<2,2,2,3>"))
    assert {c.precision for c in by("latent_mods_f16x3_kernel<4,1,8,3>")} == {"bf16", "f16"} == {c.precision for c in by("latent_mods_f16x3_kernel<4,1,4,3>")}
    assert any(c.call == "dev2" and c.em_depth is None for c in by("latent_mods_f16x3_kernel<4,1,4,3>"))
    # shapes: batches on the row-block thresholds, every depth at every ring depth of its shape, the inputs a wrong kernel gets wrong
    for depth in (2, 4, 8):
        assert {c.L for c in by(f"latent_mods_f16x3_kernel<2,2,{depth},3>")} >= {1, 2, 5, 7}
    for depth in (4, 8):
        assert {c.L for c in by(f"latent_mods_f16x3_kernel<4,1,{depth},3>")} == {2, 10}
    assert {c.B for c in pc.CASES} >= {1, 16, 17, 37} and all(c.B <= 64 or (c is pc.BIG and len(c.rows) == 5) for c in pc.CASES)
    assert {c.inputs for c in pc.CASES} == {"uniform", "fastmri", "spread20", "zero_rows", "loguniform"}
    assert {c.weights for c in pc.CASES} == {"plain", "outliers", "nobias"}
    for g in pc.SAME_BITS:
        assert len({c.numerics for c in g}) == 1 and len({(c.kernel, c.call, c.em_depth) for c in g}) == len(g) >= 2
    # with and without the 64 prefetch workgroups, same rows: one stream alone against two streams
    assert any({"host", "dev2"} <= {c.call for c in g} and g[0].H == 256 for g in pc.SAME_BITS)
    # spread20: the rows of the first block really span 2^-20 .. 2^20, neighbours in shuffled order
    for c in pc.CASES:
        if c.inputs == "spread20":
            k = pc.row_exponents(c)[:16]
            assert k.min() == -20 and k.max() == 20 and (np.diff(k) > 0).sum() not in (0, 15)
            assert np.array_equal(pc.tiles(c)[1], np.ldexp(np.random.default_rng(c.in_seed).random((c.B, 32, 32), dtype=np.float32)[1], int(k[1])))
        if c.inputs == "zero_rows":
            assert all(not pc.tiles(c)[r].any() for r in pc.ZERO_ROWS(c.B)) and pc.tiles(c)[0].any()


PROG = textwrap.dedent(r"""
    #include <cstdio>
    #include "dispatch.h"
    using namespace msiren;
    struct Row { int prec, H, L, nstreams, sync, em_depth, mode; long long B; };
    static const Row rows[] = {
    %s
    };
    int main() {
        for (const Row& r : rows) {
            DispatchHandle d;
            d.precision = r.prec; d.H = r.H; d.HP = r.H; d.L = r.L; d.Z = r.H == 512 ? 128 : 256; d.P = 576; d.num_cus = 256;
            d.em_enc = d.em_mod = r.prec != MSIREN_PREC_F32;  // (weights_pack.hip: pack_prologue_f16x3)
            d.em_depth = r.em_depth;
            CallMode m;
            m.nstreams = r.nstreams; m.sync = r.sync != 0;
            const ProloguePick p = pick_prologue(d, m, r.mode, (r.B + 15) / 16);
            std::printf("%%s %%d\n", p.inst < 0 ? "none" : kInstances[p.inst].name, p.pf_blocks);
        }
        return 0;
    }
""")
PREC = {"f16x3": "MSIREN_PREC_F16X3", "f16": "MSIREN_PREC_F16", "bf16": "MSIREN_PREC_BF16"}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_dispatch_picks_every_cases_instance(tmp_path):
    rows, want = [], []
    for c in pc.CASES:
        streams, sync = {"host": (1, 1), "halves": (1, 0), "dev1": (1, 0), "dev2": (2, 0)}[c.call]
        for mode, name in ((1, c.kernel), (2, c.kernel2)) if c.call == "halves" else ((3, c.kernel),):
            rows.append(f"    {{{PREC[c.precision]}, {c.H}, {c.L}, {streams}, {sync}, {c.em_depth or 0}, {mode}, {c.B}}},")
            # the 64 prefetch workgroups: the H = 256 model alone (one stream, or a synchronous call) up to 64 row blocks, mode 3
            want.append((c.id, name, 64 if (c.H == 256 and mode == 3 and c.call != "dev2" and c.B <= 1024) else 0))
    src = tmp_path / "pick.cpp"
    src.write_text(PROG % "\n".join(rows))
    exe = tmp_path / "pick"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True)
    picked = [line.split() for line in res.stdout.splitlines()]
    assert len(picked) == len(want)
    for (cid, name, pf), (got, got_pf) in zip(want, picked):
        assert got == name and int(got_pf) == pf, (cid, got, got_pf)
    # one of every SAME_BITS group of the H = 256 shape runs with the prefetch workgroups and one without
    assert {pf for _, _, pf in want} == {0, 64}


# ---- the gate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.NUMERICS, ids=ids)
def test_gate_is_at_most_half_the_smallest_seeded_error_and_a_second_variant_is_inside(n):
    g = pc.gate(n)
    tz, tm = g.tol
    assert np.isfinite(g.z).all() and np.isfinite(g.mods).all() and (g.mods >= 0).all()
    assert 0 < g.floor_z and 0 < g.floor_m
    assert g.passes(g.z, g.mods)
    # the restatement itself is where the suite's fp64 gate wants the kernels, per row
    z64, m64 = pc.ref64(n)
    assert pc.distance(g.z, z64) < pc.FP64_TOL and pc.distance(g.mods, m64) < pc.FP64_TOL
    zs, ms = pc.forward(n, _hook=pc.zero_fragment(pc.SMALLEST["stage"], 0, pc.SMALLEST["tile"], pc.SMALLEST["kstep"]))
    ez, em_ = g.distance(zs, ms)
    zv, mv = pc.forward(n, accumulate="fp32_ksteps", group_seed=11)
    vz, vm = g.distance(zv, mv)
    print(f"EMFLOOR {n.id} floor {g.floor_z:.2e} {g.floor_m:.2e} gate {tz:.2e} {tm:.2e} smallest seeded {ez:.2e} {em_:.2e} "
          f"= {ez / tz:.1f} {em_ / tm:.1f} x gate; second variant {vz / tz:.2f} {vm / tm:.2f} of gate")
    assert tz <= 0.5 * ez and tm <= 0.5 * em_, (tz, ez, tm, em_)
    assert g.passes(zv, mv), (vz, tz, vm, tm)
    # rows whose reference is identically zero compare exactly (zero tiles through a chain without biases)
    if n.weights == "nobias" and n.inputs == "zero_rows":
        zr = list(pc.ZERO_ROWS(n.B))
        assert not g.z[zr].any() and not g.mods[:, zr].any() and g.z[0].any()
        bad = g.z.copy()
        bad[zr[0], 5] = 1e-30
        assert not g.passes(bad, g.mods)


# ---- seeded errors -------------------------------------------------------------------------------------------------------------------
def _stages(n):
    """(stage, layer) of every GEMM stage an error is seeded into: conv2, conv3, Linear(64, Z), the latent part and the hidden part
    of the first, a middle and the last Modulator layer."""
    mid = n.L // 2
    zs = sorted({0, mid, n.L - 1})
    hs = sorted({1, mid, n.L - 1} - {0}) if n.L > 1 else []
    return [("conv2", 0), ("conv3", 0), ("fc", 0)] + [("mod_z", l) for l in zs] + [("mod_h", l) for l in hs]


def _features(n, stage):
    return {"conv2": 32, "conv3": 64, "fc": n.Z, "mod_z": n.H, "mod_h": n.H}[stage]


def _real_ksteps(n, stage):
    """k-steps that carry data (conv2's fifth holds one tap and a zero one; Linear(64, Z)'s last two are padding)"""
    return {"conv2": 4, "conv3": 64, "fc": 2, "mod_z": n.Z // 32, "mod_h": n.H // 32}[stage]


def at(stage, layer, phase, fn):
    def hook(st, l, ph, ops):
        if (st, l, ph) == (stage, layer, phase):
            fn(ops)
    return hook


def seeded_errors(n, stage, layer):
    """name -> hook: ONE error each in (stage, layer) of the restatement."""
    F, nk = _features(n, stage), _real_ksteps(n, stage)
    tile = (F // 16) - 2                      # a 16-feature tile of the stage's LAST pass (not its first or last tile)
    rows = slice(16 * tile, 16 * tile + 16)
    g0, g1 = (0, 1) if nk == 2 else (1, nk - 1)  # two k-steps that carry data
    sd = pc.state_dict(n)
    errs = {}

    def operands(fn):
        return at(stage, layer, "operands", fn)

    def zero_lo(o):
        o["A"][0][rows, o["ksteps"][g0]] = 0.0
    errs["lo_fragment_zeroed"] = operands(zero_lo)

    def drop(i):
        def fn(o):
            o["A"][i][rows, :] = 0.0
        return fn
    errs["W_lo_x_hi_dropped_for_a_tile"] = operands(drop(0))
    errs["W_hi_x_lo_dropped_for_a_tile"] = operands(drop(1))

    def swap_ksteps(o):
        a, b = o["ksteps"][g0], o["ksteps"][g1]
        for A in o["A"]:
            A[rows, a], A[rows, b] = A[rows, b].copy(), A[rows, a].copy()
    errs["two_ksteps_swapped"] = operands(swap_ksteps)

    def swap_halves(o):  # the fragment's hi where lo belongs and the other way round, one tile, one k-step
        c = o["ksteps"][g0]
        lo, hi = o["A"][0][rows, c].copy(), o["A"][1][rows, c].copy()
        o["A"][0][rows, c], o["A"][1][rows, c], o["A"][2][rows, c] = hi, lo, lo
    errs["hi_and_lo_swapped"] = operands(swap_halves)

    # a missed ring refill: the fragments (both tiles of a wave: 32 features) of the k-step DEPTH positions earlier in the wave's
    # stream, which runs on across the passes of a stage (encoder_modulator_f16x3.hip.h:165-197)
    if stage in ("conv3", "mod_z", "mod_h"):
        per_pass = 32 if stage == "conv3" else nk  # (conv3: one pass, a wave consumes its K half: 32 k-steps)
        last_pass = 0 if stage == "conv3" else F // 128 - 1
        for depth in (2, 4, 8):
            pos = last_pass * per_pass + (1 if stage != "conv3" else depth + 1)
            src = pos - depth
            if src < 0:
                continue  # (the stream's earlier k-steps belong to another stage: H = 256's first layer at depth 8)
            (ps, gs), (pd, gd) = divmod(src, per_pass), divmod(pos, per_pass)

            def stale(o, ps=ps, gs=gs, pd=pd, gd=gd):
                wave = slice(128 * pd + 32, 128 * pd + 64) if stage != "conv3" else slice(0, 32)
                from_ = slice(128 * ps + 32, 128 * ps + 64) if stage != "conv3" else slice(0, 32)
                for A in o["A"]:
                    A[wave, o["ksteps"][gd]] = A[from_, o["ksteps"][gs]].copy()
            errs[f"ring_refill_missed_depth{depth}"] = operands(stale)

    if stage == "fc":
        def stale_padding(o):  # k-steps 2, 3: the image not zeroed and the stream not zero there (what sat in the slots before)
            k = o["ksteps"]
            for A in o["A"]:
                A[:, k[2]], A[:, k[3]] = A[:, k[0]].copy(), A[:, k[1]].copy()
            for X in o["X"]:
                X[:, k[2]], X[:, k[3]] = X[:, k[1]].copy(), X[:, k[0]].copy()
        errs["padded_ksteps_carry_stale_data"] = operands(stale_padding)
    if stage == "conv3":
        def one_half(o):
            o["halves"] = o["halves"][:1]
        errs["second_K_half_not_added"] = operands(one_half)

    def epilogue(fn):
        return at(stage, layer, "epilogue", fn)

    if stage == "mod_z":
        other = layer + 1 if layer + 1 < n.L else layer - 1
        if other >= 0 and other != layer:
            c_other = sd[f"modulator.layers.{other}.0.bias"].astype(np.float64)[None, :]
            errs["c_of_the_neighbouring_layer"] = epilogue(lambda o: o.update(bias=c_other))
    block = {"conv2": 16, "conv3": 32, "fc": 128 if n.Z > 128 else 32, "mod_z": 128, "mod_h": 128}[stage]
    errs["bias_of_the_neighbouring_pass"] = epilogue(lambda o: o.update(bias=np.roll(np.broadcast_to(o["bias"], (o["bias"].shape[0], F)), block, axis=1)))
    if stage in ("mod_z", "mod_h") and layer >= 1:
        W = sd[f"modulator.layers.{layer}.0.weight"].astype(np.float64)
        wrong = W[:, :n.Z] if stage == "mod_z" else W[:, n.Z:n.Z + n.H]  # [z ; h]: the latent first

        def z_first(o):
            o["W"] = wrong
            o["a"] = em.weight_scale_exponent(wrong)
        errs["latent_first_instead_of_hidden_first"] = at(stage, layer, "weights", z_first)
    if stage in ("conv2", "conv3"):
        errs["slope_0.02"] = epilogue(lambda o: o.update(act=lambda v: np.where(v >= 0, v, np.float32(0.02) * v)))
        errs["relu_for_leaky"] = epilogue(lambda o: o.update(act=lambda v: np.where(v <= 0, 0.0, v)))
    return errs


SEEDED = [replace(pc._N256[5], rows=tuple(range(6))), replace(pc._N512[10], rows=tuple(range(6)))]


@pytest.mark.parametrize("n", SEEDED, ids=ids)
def test_seeded_errors_land_outside_the_gate(n):
    """On the rows 0..5 of the two cases whose models are the benchmark's shapes (H = Z = 256, L = 5; H = 512, Z = 128, L = 10),
    against the gate of the WHOLE case (its floor is a maximum over 37 rows: no smaller than these six rows' own)."""
    full = replace(n, rows=()).numerics
    g = pc.gate(full)
    tz, tm = g.tol
    qz, qm = g.z[:6], g.mods[:, :6]
    worst = {}
    for stage, layer in _stages(n):
        for name, hook in seeded_errors(n, stage, layer).items():
            z, m = pc.forward(n, _hook=hook)
            ez, em_ = pc.distance(z, qz), pc.distance(m, qm)
            ratio = max(ez / tz, em_ / tm)
            print(f"EMSEED {n.id} {stage}[{layer}] {name}: latent {ez:.2e} mods {em_:.2e} = {ratio:.1f} x gate")
            worst[name] = min(worst.get(name, np.inf), ratio)
            assert ratio >= 2.0, (stage, layer, name, ez, em_, tz, tm)
            if stage in ("mod_z", "mod_h"):
                assert ez == 0.0  # (nothing upstream moved)
    assert set(worst) >= {"lo_fragment_zeroed", "W_lo_x_hi_dropped_for_a_tile", "W_hi_x_lo_dropped_for_a_tile", "two_ksteps_swapped",
                          "hi_and_lo_swapped", "ring_refill_missed_depth2", "ring_refill_missed_depth4", "ring_refill_missed_depth8",
                          "padded_ksteps_carry_stale_data", "second_K_half_not_added", "c_of_the_neighbouring_layer",
                          "bias_of_the_neighbouring_pass", "latent_first_instead_of_hidden_first", "slope_0.02", "relu_for_leaky"}
    print("EMSEED", n.id, "smallest per kind:", {k: round(v, 1) for k, v in sorted(worst.items(), key=lambda kv: kv[1])})


@pytest.mark.parametrize("n", [pc._N256[7].numerics, pc._N512[2].numerics], ids=ids)
def test_a_wrong_rows_scale_lands_outside_the_gate(n):
    """Rows of one block spanning 2^-20 .. 2^20 in shuffled order.  A neighbour row's scale (used to scale AND to undo, as a kernel
    that indexed the row maxima wrongly would): a brighter row under a dimmer row's scale leaves the fp16 range, its outputs are
    not finite.  The block's maximum in place of the row's: nothing overflows, the dim rows lose their low bits -- 2^-24 of the
    block's scaled maximum against a row 2^-20 below it."""
    g = pc.gate(n)
    tz, tm = g.tol
    per_tile = {"conv2": 64}

    def neighbour(stage):
        return lambda o: o.update(s=np.roll(o["s"], per_tile.get(stage, 1)))

    def block_max(stage):
        def fn(o):
            s = o["s"].reshape(-1, per_tile.get(stage, 1))
            for b in range(0, s.shape[0], 16):
                s[b:b + 16] = s[b:b + 16].min()  # (the largest maximum has the smallest exponent)
            o["s"] = s.reshape(-1)
        return fn

    for stage, layer in _stages(n):
        for name, fn in (("neighbour_rows_scale", neighbour(stage)), ("block_maximum_for_the_rows", block_max(stage))):
            z, m = pc.forward(n, _hook=at(stage, layer, "input", fn))
            ez, em_ = g.distance(z, m)
            ratio = max(ez / tz, em_ / tm)
            print(f"EMSEED {n.id} {stage}[{layer}] {name}: latent {ez:.2e} mods {em_:.2e} = {ratio:.1f} x gate")
            assert ratio >= 2.0, (stage, layer, name, ez, em_, tz, tm)


def test_truncation_is_visible_on_the_split_alone_and_nowhere_behind_a_sum():
    """fp16 truncation in place of round-to-nearest.

    Where it is visible, and asserted: on the split itself, against exact arithmetic.  Round to nearest leaves
    |v - (hi + lo)| <= 2^-23 |v| with either sign (lo a normal number); truncation of both halves leaves up to 1.5 x 2^-22 |v|,
    always towards zero, 3.5 times as much on average.

    Where it is not, and why nothing is asserted there (figures of this test's printout: LAB_NOTES.md section 16):
    * of ``hi`` alone it cannot be seen at all: ``lo = f16(v - hi)`` takes up what ``hi`` left, the pair keeps 21 bits for 22;
    * of both halves, on an ISOLATED stage -- the Modulator's first layer alone, the latent given, num_layers = 1: one GEMM of
      K = 256 and its epilogue -- the outputs move by 1.8e-7 per row with the inputs truncated and 1.5e-7 with the weights: the
      size of that stage's own fp32 accumulation floor (1.8e-7), a quarter of its gate.  The errors of 256 operands average out
      in the sum.  Behind the encoder's four stages the floor is larger still.
    A rounding mode is therefore pinned by this test for the restatement and by nothing for the kernels; the gate does not claim it."""
    rng = np.random.default_rng(7)
    v = (rng.choice([-1.0, 1.0], 200000) * rng.uniform(1, 2, 200000) * np.exp2(rng.integers(0, 13, 200000))).astype(np.float32)  # (lo: a normal number or zero)
    v64 = v.astype(np.float64)
    rec = lambda pair: pair[0].astype(np.float64) + pair[1].astype(np.float64)
    e_rne, e_trunc = (rec(em.split_f16(v)) - v64) / v64, (rec(em.split_f16(v, em.trunc_f16)) - v64) / v64
    assert np.abs(e_rne).max() <= 2.0 ** -23 and (e_rne > 0).mean() > 0.1 and (e_rne < 0).mean() > 0.1
    assert (e_trunc <= 0).all() and 2.0 ** -22 < np.abs(e_trunc).max() <= 2.0 ** -21 and np.abs(e_trunc).mean() > 3 * np.abs(e_rne).mean()
    # the isolated stage: measured, printed, and inside the gate
    n = pc._N256[1].numerics
    sd = pc.state_dict(n)
    z_in = np.random.default_rng(5).standard_normal((16, 256)).astype(np.float32)
    fwd = lambda **kw: em.prologue_forward(sd, z_in=z_in, num_layers=1, **kw)[1]
    q = fwd()
    floor = pc.distance(fwd(accumulate="fp32_ksteps"), q)
    trunc_both = lambda v: em.split_f16(v, em.trunc_f16)

    def trunc_hi(v):
        hi = em.trunc_f16(v)
        return hi, em.rne_f16(np.asarray(v, dtype=np.float32) - hi)

    e_both = pc.distance(fwd(_hook=at("mod_z", 0, "input", lambda o: o.update(split=trunc_both))), q)
    e_hi = pc.distance(fwd(_hook=at("mod_z", 0, "input", lambda o: o.update(split=trunc_hi))), q)
    e_w = pc.distance(fwd(_hook=at("mod_z", 0, "weights", lambda o: o.update(split=trunc_both))), q)
    print(f"EMSEED isolated mod_z[0]: floor {floor:.2e} gate {4 * floor:.2e}; truncation of hi and lo: inputs {e_both:.2e} weights {e_w:.2e}; of hi alone {e_hi:.2e}")
    assert 0 < e_hi < e_both and 0 < e_w  # the hook reaches the split; the sizes are the docstring's
