"""tests/grad_reference.py on the CPU: its value is the oracle's, its gradient agrees with central differences of the oracle, and the
gate it gives every case of tests/test_gpu_grad.py lies at most half way to the smallest error a forward-mode kernel would make."""
import numpy as np
import pytest

import grad_reference as gr
from conftest import nerr
from mri_inr_amd import synthetic as syn
from oracle import siren_oracle as orc

L = 5


def scattered(Q, seed=3):
    return np.random.default_rng(seed).uniform(-1.2, 1.2, size=(Q, 2)).astype(np.float32)


def oracle_at(sd, mods, coords, act):
    sdg = dict(sd)
    sdg["grid"] = np.asarray(coords, dtype=np.float64)
    return orc.siren_forward(sdg, mods, num_layers=L, activation=act, dtype=np.float64)


@pytest.mark.parametrize("act", ["sine", "morlet"])
def test_value_is_the_oracles_and_gradient_matches_central_differences(act):
    sd = syn.make_state_dict(seed=7)
    mods = syn.make_mods(2, L, 5, 256)
    coords = scattered(77).astype(np.float64)
    val, grad = gr.value_and_grad(sd, mods, coords, num_layers=L, activation=act)
    assert val.dtype == np.float64 and grad.shape == (2, 5, 77)
    assert np.array_equal(val, oracle_at(sd, mods, coords, act))
    h = 1e-6
    for i in range(2):
        step = np.zeros(2)
        step[i] = h
        fd = (oracle_at(sd, mods, coords + step, act) - oracle_at(sd, mods, coords - step, act)) / (2 * h)
        e = nerr(grad[i], fd)
        print(f"{act} d/dcoords[:, {i}]: max|grad| {np.abs(grad[i]).max():.1f}, nerr against central differences {e:.2e}")
        assert e <= 1e-7, e


def test_plain_fp32_variant_sits_far_inside_the_cap():
    sd = syn.make_state_dict(seed=7)
    mods, coords = syn.make_mods(2, L, 5, 256), scattered(77)
    for act in ("sine", "morlet"):
        _, ref = gr.value_and_grad(sd, mods, coords, num_layers=L, activation=act)
        _, g32 = gr.value_and_grad(sd, mods, coords, num_layers=L, activation=act, dtype=np.float32)
        fm, fr = gr.distances(g32, ref)
        print(f"{act}: plain fp32 against fp64: nerr {fm:.2e} rms {fr:.2e}")
        assert g32.dtype == np.float32 and fm <= gr.CAP_MAX / 10 and fr <= gr.CAP_RMS / 3, (fm, fr)


@pytest.mark.parametrize("case", gr.CASES, ids=str)
def test_gate_is_at_most_half_the_smallest_seeded_error(case):
    sd = gr.case_state_dict(case)
    kw = dict(num_layers=case.L, activation=case.act)
    for Q, B in gr.SIZES:
        d = gr.case_data(case, Q, B)
        mods, coords, ref, (gmax, grms) = d["mods"], d["coords"], d["grad"], d["gate"]
        # the reference alone sits inside the caps: the gate is 4 x the floor, not the cap
        assert 0 < gr.FACTOR * d["floor"][0] == gmax <= gr.CAP_MAX and 0 < gr.FACTOR * d["floor"][1] == grms <= gr.CAP_RMS, (Q, B, d["floor"], d["draw"])
        errs = {}
        for seed in gr.SEEDS:
            if seed == "envelope_dropped" and case.act != "morlet":
                continue
            if seed == "bias_in_tangent" and not case.use_bias:
                continue
            if seed == "neighbour_cosine" and Q == 1:
                continue  # (no neighbour to take a cosine from)
            _, g = gr.value_and_grad(sd, mods, coords, seed=seed, seed_layer=min(1, case.L - 1), **kw)
            errs[seed] = gr.distances(g, ref)
        smallest = min(errs, key=lambda k: errs[k][0])
        print(f"{case} Q={Q} B={B} (draw {d['draw']}): gate {gmax:.2e} / {grms:.2e}; smallest seeded error {smallest} {errs[smallest][0]:.2e} / {errs[smallest][1]:.2e}")
        assert all(gmax <= e[0] / 2 and grms <= e[1] / 2 for e in errs.values()), (Q, B, gmax, grms, errs)
