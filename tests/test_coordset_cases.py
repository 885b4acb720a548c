"""tests/coordset_cases.py on the CPU: the manifest the GPU file (tests/test_gpu_coordset_cases.py) runs

* names every instance of the f32_ragged, f32_jet_ragged, f16x3n_ragged and f32_ragged_cond lists (trunk_instances.h) at least once -- an
  instance that loses its last case fails here -- and finds the four f32_jet instances covered by grad_reference.CASES;
* reaches each native case's instance: ragged_native_pick (dispatch.h, compiled with g++) returns the ring and lfix of the case's name,
  and native == false for every other case;
* rests on two references that agree (grad_reference.value_and_grad, oracle.siren_forward with a `grid` entry);
* has gates that mean something: 10 e32 stays within the 1e-4 contract, the float32 rounding of the reference passes, and the reference of
  another model, of a neighbouring patch's modulation rows or of a set with its chunks rotated lands more than 100 x the gate away; the
  seeded gradient errors of grad_reference lie at least twice beyond the gradient gate;
* keeps every non-guard native case well inside the fp16 domain and every guard case outside it through elements that reach nothing;
* draws every gradient case's coordinates inside the caps within its 16 draws.
"""
import os
import re
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

import coordset_cases as cc
import grad_reference as gr
from conftest import nerr
from oracle import siren_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mri_inr_amd", "csrc")
FAMILIES = {"f32_ragged": 16, "f32_jet_ragged": 4, "f16x3n_ragged": 6, "f32_ragged_cond": 2, "f32_jet": 4}

ids = lambda c: c.id


def launched_instances():
    """name -> family of every instance of the five lists, parsed from trunk_instances.h (as test_trunk_cases.launched_instances)."""
    text = open(os.path.join(CSRC, "trunk_instances.h")).read()
    out = {}
    for fam, args, stamped in re.findall(r"X\((\w+), ([\d,]+)\)(\s*/\* stamped build)?", text):
        if fam in FAMILIES and not stamped:
            out[f"siren_trunk_{fam}_kernel<{args}>"] = fam
    return out


def test_every_launched_instance_has_a_case():
    inst = launched_instances()
    assert {f: sum(1 for v in inst.values() if v == f) for f in FAMILIES} == FAMILIES  # 28 ragged ones and the jet's 4
    ragged = {k for k, f in inst.items() if f != "f32_jet"}
    covered = {c.kernel for c in cc.CASES}
    assert not ragged - covered, sorted(ragged - covered)
    assert covered <= ragged, sorted(covered - ragged)  # every name a case states is a compiled one
    # the conditional instances: guard cases, and only those, each behind a compiled native instance of its own activation
    cond = {k for k, f in inst.items() if f == "f32_ragged_cond"}
    assert {c.kernel for c in cc.GUARDS} == cond and all(c.guard and c.form == "native" for c in cc.GUARDS)
    assert not any(c.kernel in cond for c in cc.CASES if c not in cc.GUARDS)
    for c in cc.GUARDS:
        assert inst.get(c.trunk) == "f16x3n_ragged" and c.trunk.startswith(f"siren_trunk_f16x3n_ragged_kernel<{cc.ACTS.index(c.act)},"), c.id
        assert c.launches == (c.trunk, c.kernel)
    # the shared-set jet: tests/test_gpu_grad.py runs grad_reference.CASES, which reach all four <HP,ACT>
    jet = {f"siren_trunk_f32_jet_kernel<{(g.H + 127) // 128 * 128},{cc.ACTS.index(g.act)}>" for g in gr.CASES}
    assert jet == {k for k, f in inst.items() if f == "f32_jet"}


def test_the_manifest_holds_the_shapes_it_is_meant_to():
    of = lambda k: [c for c in cc.CASES if c.kernel == k or c.trunk == k]
    edges = [c for c in cc.CASES if not c.many]
    assert all(c.counts == cc.EDGES(c.chunk) and 7 <= c.NP <= 11 and c.T <= 400 for c in edges)
    assert {c.kernel for c in edges} == {c.kernel for c in cc.CASES}  # EDGES for every instance
    many = [c for c in cc.CASES if c.many]
    assert all(c.counts == cc.MANY(c.chunk) and c.NP == 300 and c.T < 700 and c.H == 256 and c.act == "sine" for c in many)
    assert sorted(c.family for c in many) == sorted(cc.CHUNK) and sum(1 for c in many if c.guard) == 1
    for c in many:  # work on both sides of ragged_items_kernel's 256-patch block, and a set of more than one chunk at its edge
        assert sum(c.counts[:256]) > 0 and sum(c.counts[256:]) > 0 and c.counts[255] == c.chunk + 1 and c.counts[256] == 1 and c.counts[299] == c.chunk
    # f32_ragged: trunk_cases.F32's widths and depths
    f32 = [c for c in cc.F32_RAGGED if not c.many]
    assert len({c.kernel for c in f32}) == 16 and all(c.precision == "fp32" and c.form == "value" and c.L in (3, 4) for c in cc.F32_RAGGED)
    for hp in (128, 256, 384, 512):
        assert {c.H for c in f32 if (c.H + 127) // 128 * 128 == hp} == {hp, {128: 100, 256: 200, 384: 300, 512: 400}[hp]}
    assert sum(not c.use_bias for c in f32) >= 2 and sum(c.w0 == 1.5 and c.w0_initial == 20.0 for c in f32) >= 2
    for c in cc.F32_RAGGED:
        hp, a, r = (int(v) for v in re.search(r"<(\d+),(\d),(\d)>", c.kernel).groups())
        assert ((c.H + 127) // 128 * 128, cc.ACTS.index(c.act), int(c.residual)) == (hp, a, r), c.id
    # the jet
    jet = [c for c in cc.JET_RAGGED if not c.many]
    assert sorted(c.H for c in jet) == [100, 128, 200, 256] and all(c.form == "grad" and c.precision == "fp32" and not c.residual for c in cc.JET_RAGGED)
    assert sum(not c.use_bias for c in jet) >= 1 and sum(c.options for c in jet) >= 1
    for c in cc.JET_RAGGED:
        hp, a = (int(v) for v in re.search(r"<(\d+),(\d)>", c.kernel).groups())
        assert ((c.H + 127) // 128 * 128, cc.ACTS.index(c.act)) == (hp, a), c.id
    # the native trunk at the depth edges of each instance
    for a in (0, 1):
        assert {c.L for c in of(f"siren_trunk_f16x3n_ragged_kernel<{a},3,5>")} == {5}
        assert {c.L for c in of(f"siren_trunk_f16x3n_ragged_kernel<{a},4,0>")} >= {2, 4}
        assert {c.L for c in of(f"siren_trunk_f16x3n_ragged_kernel<{a},3,0>")} >= {6, 11}
    for k in ("siren_trunk_f16x3n_ragged_kernel<1,4,0>", "siren_trunk_f16x3n_ragged_kernel<1,3,5>"):
        assert any(c.w0 == 1.5 and c.w0_initial == 20.0 and not c.use_bias and c.act == "morlet" for c in of(k)), k
    assert any(c.zero_fraction == 0.3 and (cc.mods(c) == 0).mean() > 0.25 for c in cc.NATIVE)
    assert all(c.precision == "f16x3" and c.form == "native" and c.H == 256 and not c.residual for c in cc.NATIVE + cc.GUARDS)
    assert [(c.act, c.L) for c in cc.GUARDS if not c.many] == [("sine", 5), ("morlet", 7)]
    # inputs
    for c in cc.CASES:
        xy, m = cc.coords_of(c), cc.mods(c)
        assert xy.dtype == np.float32 and xy.shape == (c.T, 2) and np.abs(xy).max() <= 1.2 and np.abs(xy).max() > 1.0
        assert m.dtype == np.float32 and m.shape == (c.L, c.NP, c.H)
        lo, hi = (0.1, 0.6) if c.residual else (0.5, 1.5)
        body = m[(m != 0) & (m != cc.BIG)]
        assert lo <= body.min() and body.max() <= hi and ((m == 0).any() == bool(c.zero_fraction))


# ---- dispatch -------------------------------------------------------------------------------------------------------------------------------
PROG = textwrap.dedent(r"""
    #include <cstdio>
    #include "dispatch.h"
    using namespace msiren;
    struct Row { int prec, H, L, act, res; };
    static const Row rows[] = {
    %s
    };
    int main() {
        for (const Row& r : rows) {
            DispatchHandle d;
            d.precision = r.prec; d.H = r.H; d.HP = (r.H + 127) / 128 * 128; d.L = r.L; d.Z = r.H == 512 ? 128 : 256; d.P = 24 * 24;
            d.act = r.act; d.res = r.res;
            // as msiren_commit_weights describes the handle (weights_pack.hip, launch_dispatch.hip: describe_for_dispatch)
            d.f16_ring4_fits = r.L <= 5; d.f16_ring3_fits = r.L <= 11; d.ws_depth_ok = r.L >= 3 && r.L <= 5;
            d.f16x3_ready = r.prec == MSIREN_PREC_F16X3 && r.H == 256 && r.L >= 2 && d.f16_ring3_fits;
            d.x1_ready = (r.prec == MSIREN_PREC_BF16 || r.prec == MSIREN_PREC_F16) && r.H == 512;
            const RaggedNativePick p = ragged_native_pick(d);
            std::printf("%%d %%d %%d\n", (int)p.native, p.ring, p.lfix);
        }
        return 0;
    }
""")
PREC = {"fp32": "MSIREN_PREC_F32", "f16x3": "MSIREN_PREC_F16X3"}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_dispatch_picks_every_native_cases_instance(tmp_path):
    rows = "\n".join(f"    {{{PREC[c.precision]}, {c.H}, {c.L}, {'MSIREN_ACT_MORLET' if c.act == 'morlet' else 'MSIREN_ACT_SINE'}, {int(c.residual)}}},"
                     for c in cc.CASES)
    src = tmp_path / "pick.cpp"
    src.write_text(PROG % rows)
    exe = tmp_path / "pick"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True)
    picked = [tuple(int(v) for v in line.split()) for line in res.stdout.splitlines()]
    assert len(picked) == len(cc.CASES)
    for c, (native, ring, lfix) in zip(cc.CASES, picked):
        if c.form != "native":
            assert not native, c.id
            continue
        a, r, lf = (int(v) for v in re.fullmatch(r"siren_trunk_f16x3n_ragged_kernel<(\d),(\d),(\d)>", c.trunk or c.kernel).groups())
        assert native and (ring, lfix) == (r, lf) and a == cc.ACTS.index(c.act), (c.id, native, ring, lfix)


# ---- the references ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in cc.CASES if not c.residual], ids=ids)
def test_the_two_references_agree(c):
    ref = cc.ref64(c)
    sd, m, xy = cc.state_dict(c), cc.mods(c), cc.coords_of(c)
    for b, lo, hi in cc.patches(c):
        sdg = dict(sd)
        sdg["grid"] = xy[lo:hi]
        o = orc.siren_forward(sdg, m[:, b:b + 1], num_layers=c.L, w0=c.w0, w0_initial=c.w0_initial, activation=c.act, dtype=np.float64)[0]
        assert np.abs(o - ref[lo:hi]).max() <= 1e-12 * np.abs(ref).max(), (c.id, b)


# ---- the gates --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.CASES, ids=ids)
def test_gate_is_within_the_contract_and_sees_the_mutants(c):
    """e32 from the references alone; 10 e32 <= 1e-4, so the floor term of the gate never exceeds the contract.  Every mutant is the fp64
    reference of the same weights and inputs with ONE thing changed, and lies more than 100 x the gate away."""
    ref = cc.ref64(c)
    assert ref.shape == (c.T,) and np.isfinite(ref).all() and np.abs(ref).max() > 1e-2  # not a degenerate output
    e32 = cc.e32(c)
    gate = cc.tolerance(c)[0]
    extra = f" l0_floor {cc.l0_floor(c):.2e}" if c.form == "native" else ""
    print(f"COORDCASE {c.id} T {c.T} e32 {e32:.2e}{extra} max|ref| {np.abs(ref).max():.3f} gate {gate:.2e}")
    assert 0.0 < cc.FLOOR_FACTOR * e32 <= cc.TOL, e32
    if c.form == "native":
        assert 0.0 < cc.FLOOR_FACTOR * cc.l0_floor(c) <= cc.TOL
    assert cc.passes(c, ref.astype(np.float32))
    mutants = {"activation": lambda: cc.evaluate(c, act="sine" if c.act == "morlet" else "morlet")[0],
               "residual": lambda: cc.evaluate(c, residual=not c.residual)[0],
               "neighbour's rows": lambda: cc.evaluate(c, rows=cc.next_patch_rows(c))[0],
               "chunks rotated": lambda: cc.chunks_rotated(c, ref)}
    if c.options:
        mutants["w0 = 1"] = lambda: cc.evaluate(c, w0=1.0)[0]
        mutants["w0_initial = 30"] = lambda: cc.evaluate(c, w0_initial=30.0)[0]
        mutants["w0 = 1, w0_initial = 30"] = lambda: cc.evaluate(c, w0=1.0, w0_initial=30.0)[0]
    if not c.use_bias:
        mutants["biases"] = lambda: cc.evaluate(c, sd=cc.with_biases(c))[0]
    assert any(n > c.chunk for n in c.counts)  # (the rotation moves something)
    for name, make in mutants.items():
        bad = make()
        e, _ = cc.distance(c, bad)
        print(f"COORDCASE {c.id} mutant {name}: {e:.2e} = {e / gate:.0f} x gate")
        assert not cc.passes(c, bad) and e > 100 * gate, (name, e)


GRAD = [c for c in cc.CASES if c.form == "grad"]


@pytest.mark.parametrize("c", GRAD, ids=ids)
def test_gradient_gate_is_inside_the_caps_and_half_the_smallest_seeded_error(c):
    """The draw rule of grad_reference.case_data ends inside the caps (no case is skipped to get there), and every seeded error of
    grad_reference.SEEDS lies at least twice beyond the gate, as tests/test_grad_reference.py requires of the shared-set cases."""
    (fm, fr), (gmax, grms) = cc.grad_floor(c), cc.grad_tolerance(c)
    assert cc.draw_of(c) < cc.DRAWS and 0 < gr.FACTOR * fm == gmax <= gr.CAP_MAX and 0 < gr.FACTOR * fr == grms <= gr.CAP_RMS, (cc.draw_of(c), fm, fr)
    ref = cc.grad64(c)
    assert ref.shape == (2, c.T) and np.isfinite(ref).all()
    assert cc.grad_distance(c, ref.astype(np.float32))[0] <= gmax
    errs = {}
    for seed in gr.SEEDS:
        if (seed == "envelope_dropped" and c.act != "morlet") or (seed == "bias_in_tangent" and not c.use_bias):
            continue
        errs[seed] = cc.grad_distance(c, cc.evaluate(c, grad=True, seed=seed, seed_layer=min(1, c.L - 1))[1])
    errs["chunks rotated"] = cc.grad_distance(c, cc.chunks_rotated(c, ref))
    smallest = min(errs, key=lambda k: errs[k][0])
    print(f"COORDCASE {c.id} draw {cc.draw_of(c)} gradient gate {gmax:.2e} / {grms:.2e}; smallest seeded error {smallest} {errs[smallest][0]:.2e} / {errs[smallest][1]:.2e}")
    assert all(gmax <= e[0] / 2 and grms <= e[1] / 2 for e in errs.values()), (gmax, grms, errs)


# ---- domain -----------------------------------------------------------------------------------------------------------------------------------
def test_only_guard_cases_leave_the_fp16_domain():
    for c in cc.NATIVE + cc.GUARDS:
        m = cc.mods(c)
        if not c.guard:
            assert cc.scaled_modulation_max(c) <= 2.0, c.id   # 65 504 is four orders of magnitude away
            continue
        assert cc.scaled_modulation_max(c) > 65504.0, c.id
        assert (np.abs(m) > 2.0).sum() == len(c.guard) and all(m[l, b, j] == cc.BIG and c.counts[b] > 0 for l, b, j in c.guard)
        assert any(l == c.L - 1 for l, _, _ in c.guard) and any(0 < l < c.L - 1 for l, _, _ in c.guard)
        # the elements reach nothing downstream: the reference of the same case WITHOUT them is the same function up to fp64 rounding
        plain = np.array(m)
        for l, b, j in c.guard:
            plain[l, b, j] = 1.0
        assert nerr(cc.evaluate(c, mods_=plain)[0], cc.ref64(c)) <= 1e-12, c.id
    assert not any(c.guard for c in cc.F32_RAGGED + cc.JET_RAGGED + cc.NATIVE)
