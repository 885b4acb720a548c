"""tests/trunk_cases.py on the CPU: the manifest the GPU file (tests/test_gpu_trunk_cases.py) runs

* names every launched instance of the f32, f32_cond, f16x3n, f16x3h and f16x3w families (trunk_instances.h; not the stamped
  diagnostic builds) at least once -- an instance that loses its last case fails here;
* reaches each case's instance: pick_trunk (dispatch.h, compiled with g++) returns the case's name for the handle and call the
  case describes, with the LDS facts launch_dispatch.hip pins by static_assert (ring of 4: L <= 5, ring of 3: L <= 11);
* has a gate that means something: 10 x the fp32 oracle's own distance from fp64 stays within the 1e-4 contract, and the fp64
  oracle of the same weights with the other activation, the other residual switch or w0 = 1 lands outside it;
* keeps every non-guard case well inside the fp16 domain (a case at its edge would quietly test the fp32 rerun), and every guard
  case outside it through elements that reach nothing downstream.
"""
import os
import re
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

import trunk_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mri_inr_amd", "csrc")
FAMILIES = {"f32": 16, "f32_cond": 2, "f16x3n": 8, "f16x3h": 4, "f16x3w": 2}

ids = lambda c: c.id


def launched_instances():
    """name -> family of every non-stamped instance of the five families, parsed from trunk_instances.h."""
    text = open(os.path.join(CSRC, "trunk_instances.h")).read()
    out = {}
    for fam, args, stamped in re.findall(r"X\((\w+), ([\d,]+)\)(\s*/\* stamped build)?", text):
        if fam in FAMILIES and not stamped:
            out[f"siren_trunk_{fam}_kernel<{args}>"] = fam
    return out


def test_every_launched_instance_has_a_case():
    inst = launched_instances()
    assert {f: sum(1 for v in inst.values() if v == f) for f in FAMILIES} == FAMILIES  # 32 in all
    covered = {c.kernel for c in tc.CASES} | {tc.conditional_kernel(c) for c in tc.GUARDS}
    assert not set(inst) - covered, sorted(set(inst) - covered)
    # the conditional instances are named by guard cases only through conditional_kernel: each of those by its own handle kind
    assert {tc.conditional_kernel(c) for c in tc.GUARD_256} == {k for k, f in inst.items() if f == "f32_cond"}
    assert {tc.conditional_kernel(c) for c in tc.GUARD_512} == {k for k in inst if k.startswith("siren_trunk_f32_kernel<512,")}
    assert {c.precision for c in tc.GUARD_512} == {"f16", "bf16"}
    # every name a case states is a compiled one (the x1w names of the H = 512 guard cases included)
    text = open(os.path.join(CSRC, "trunk_instances.h")).read()
    compiled = {f"siren_trunk_{f}_kernel<{a}>" for f, a in re.findall(r"X\((\w+), ([\d,]+)\)", text)}
    assert {c.kernel for c in tc.CASES} <= compiled


def test_the_manifest_holds_the_shapes_it_is_meant_to():
    f32 = {c.kernel: c for c in tc.F32}
    assert len(f32) == 16 and all(c.precision == "fp32" and c.L in (3, 4) and c.B <= 5 for c in tc.F32)
    for hp in (128, 256, 384, 512):  # a padded width and the full one per HP
        assert {c.H for c in tc.F32 if (c.H + 127) // 128 * 128 == hp} == {hp, {128: 100, 256: 200, 384: 300, 512: 400}[hp]}
    assert {c.S for c in tc.CASES} == {7, 10, 24, 33} and max(c.B for c in tc.CASES) <= 60

    def of(kernel):
        return [c for c in tc.F16X3 if c.kernel == kernel]

    for a in (0, 1):
        assert {c.L for c in of(f"siren_trunk_f16x3n_kernel<{a},4,0>")} >= {2, 3, 4}
        assert {c.L for c in of(f"siren_trunk_f16x3n_kernel<{a},3,0>")} == {6, 11}
        assert {c.L for c in of(f"siren_trunk_f16x3w_kernel<{a},4>")} >= {3, 4, 5}
        assert any(c.ws == 0 and c.streams == 1 for c in of(f"siren_trunk_f16x3n_kernel<{a},4,5>"))
        assert any(c.streams == 2 and c.dev and c.B > 28 for c in of(f"siren_trunk_f16x3n_kernel<{a},3,5>"))
        assert any(c.streams == 1 and c.B <= 28 for c in of(f"siren_trunk_f16x3h_kernel<{a},4,5>"))
        assert any(c.streams == 2 and c.dev and c.B <= 28 for c in of(f"siren_trunk_f16x3h_kernel<{a},3,5>"))
    ragged = lambda cs: any(c.S != 24 for c in cs)
    assert ragged(of("siren_trunk_f16x3n_kernel<1,4,0>")) and ragged(of("siren_trunk_f16x3n_kernel<1,3,0>"))
    w1 = of("siren_trunk_f16x3w_kernel<1,4>")
    assert {c.S for c in w1} >= {7, 33} and {c.B for c in w1} >= {1, 3, 29, 57}
    for k in ("siren_trunk_f16x3w_kernel<1,4>", "siren_trunk_f16x3n_kernel<1,4,0>"):
        assert any(c.w0 == 1.5 and c.w0_initial == 20.0 and not c.use_bias for c in of(k))
    for g in tc.SAME_BITS:  # one model, one batch, several instances
        assert len({c.numerics for c in g}) == 1 and len({c.kernel for c in g}) == len(g) >= 2


# ---- dispatch -----------------------------------------------------------------------------------------------------------------------
PROG = textwrap.dedent(r"""
    #include <cstdio>
    #include "dispatch.h"
    using namespace msiren;
    struct Row { int prec, H, L, P, act, res, ws, half, nstreams, dev; long long B; };
    static const Row rows[] = {
    %s
    };
    int main() {
        for (const Row& r : rows) {
            DispatchHandle d;
            d.precision = r.prec; d.H = r.H; d.HP = (r.H + 127) / 128 * 128; d.L = r.L; d.Z = r.H == 512 ? 128 : 256; d.P = r.P;
            d.act = r.act; d.res = r.res; d.num_cus = 256;
            // as msiren_commit_weights describes the handle (weights_pack.hip, launch_dispatch.hip: describe_for_dispatch)
            d.f16_ring4_fits = r.L <= 5; d.f16_ring3_fits = r.L <= 11; d.ws_depth_ok = r.L >= 3 && r.L <= 5;
            d.f16x3_ready = r.prec == MSIREN_PREC_F16X3 && r.H == 256 && r.L >= 2 && d.f16_ring3_fits;
            d.x1_ready = (r.prec == MSIREN_PREC_BF16 || r.prec == MSIREN_PREC_F16) && r.H == 512;
            d.f16_ws = r.ws; d.half_allowed = r.half;
            CallMode m;
            m.nstreams = r.nstreams; m.sync = !r.dev;
            const TrunkPick t = pick_trunk(d, m, r.B);
            std::printf("%%s %%d\n", t.inst < 0 ? "none" : kInstances[t.inst].name, (int)t.guard);
        }
        return 0;
    }
""")
PREC = {"fp32": "MSIREN_PREC_F32", "f16x3": "MSIREN_PREC_F16X3", "f16": "MSIREN_PREC_F16", "bf16": "MSIREN_PREC_BF16"}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_dispatch_picks_every_cases_instance(tmp_path):
    rows = "\n".join(
        f"    {{{PREC[c.precision]}, {c.H}, {c.L}, {c.P}, {'MSIREN_ACT_MORLET' if c.act == 'morlet' else 'MSIREN_ACT_SINE'}, "
        f"{int(c.residual)}, {1 if c.ws is None else c.ws}, {1 if c.half is None else c.half}, {c.streams}, {int(c.dev)}, {c.B}}},"
        for c in tc.CASES)
    src = tmp_path / "pick.cpp"
    src.write_text(PROG % rows)
    exe = tmp_path / "pick"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True)
    picked = [line.split() for line in res.stdout.splitlines()]
    assert len(picked) == len(tc.CASES)
    for c, (name, guard) in zip(tc.CASES, picked):
        assert name == c.kernel, (c.id, name)
        # Guard: 0 none, 1 f32_cond, 2 f32_512 (dispatch.h)
        assert int(guard) == (0 if c.precision == "fp32" else 1 if c.H == 256 else 2), (c.id, guard)


# ---- the gate -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", sorted({c.numerics for c in tc.CASES}, key=ids), ids=ids)
def test_gate_is_within_the_contract_and_sees_another_model(c):
    """e32 from the oracle alone; 10 e32 <= 1e-4, so the floor term of the gate never exceeds the contract.  The fp64 oracle of
    the same weights and inputs with ONE model switch changed is outside the gate: a Morlet case with tiny pre-activations would
    be a sine case, a residual case with tiny modulations a plain one."""
    ref = tc.ref64(c)
    assert ref.shape == (c.B, c.P) and np.isfinite(ref).all() and np.abs(ref).max() > 1e-2  # not a degenerate output
    e32 = tc.e32(c)
    print(f"TRUNKCASE {c.id} e32 {e32:.2e} max|ref| {np.abs(ref).max():.3f}")
    assert 0.0 < tc.FLOOR_FACTOR * e32 <= tc.TOL, e32
    assert tc.passes(c, ref.astype(np.float32))
    others = {"activation": dict(activation="sine" if c.act == "morlet" else "morlet"), "residual": dict(residual=not c.residual)}
    if c.w0 != 1.0:
        others["w0"] = dict(w0=1.0)
    for name, kw in others.items():
        bad = tc.oracle_of_another_model(c, **kw)
        e, _ = tc.distance(c, bad)
        print(f"TRUNKCASE {c.id} other {name}: {e:.2e} = {e / tc.tolerance(c)[0]:.0f} x gate")
        assert not tc.passes(c, bad) and e > 100 * tc.tolerance(c)[0], (name, e)


# ---- domain -------------------------------------------------------------------------------------------------------------------------
def test_only_guard_cases_leave_the_fp16_domain():
    for c in tc.CASES:
        m = tc.mods(c)
        if not c.guard:
            assert tc.scaled_modulation_max(c) <= 2.0, c.id   # 65 504 is four orders of magnitude away
            continue
        assert c.precision != "fp32" and tc.scaled_modulation_max(c) > 65504.0, c.id
        assert (np.abs(m) > 2.0).sum() == len(c.guard) and all(m[l, b, j] == tc.BIG for l, b, j in c.guard)
        assert any(l == c.L - 1 for l, _, _ in c.guard) and any(l < c.L - 1 for l, _, _ in c.guard)
        # the elements reach nothing downstream: the oracle of the same case WITHOUT them (the ordinary model) is the same
        # function up to fp64 rounding
        plain = np.array(m)
        for l, b, j in c.guard:
            plain[l, b, j] = 1.0
        from oracle import siren_oracle as orc
        other = orc.siren_forward(tc.state_dict(c), plain, num_layers=c.L, w0=c.w0, w0_initial=c.w0_initial, activation=c.act,
                                  siren_patch_size=c.S, residual=c.residual, dtype=np.float64)
        assert np.abs(other - tc.ref64(c)).max() <= 1e-12, c.id
