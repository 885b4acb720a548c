"""``ModulatedSiren.align_stack_cost`` and ``align_stack_solve`` on a host without a device, with tests/test_binding_calls.py's recording stand-in for
the library (imported, not edited): the two methods commit no weights, pass null for what was not given, pre-fill their outputs per DESIGN.md section
5.21 (NaN for sampled images, 0 for sums and reports, (1, 0) rows for an absent intensity), build the scales, the rigid states and the singleton
groups themselves, and raise ValueError for wrong shapes before the library is entered."""
import numpy as np
import pytest

import test_binding_calls as tb

N, HH, WW, M, TH, TW, G = tb.N, tb.HH, tb.WW, tb.M, tb.TH, tb.TW, tb.G
_GROUP = {10: (np.int32, lambda a: a[11] + 1), 13: (np.float64, lambda a: 12 * a[11])}
# the host arrays the binding builds itself for the new calls, read through their pointers like the others (the recorder looks them up by name)
tb.BUILT.setdefault("msiren_align_stack_r", {12: (np.float64, lambda a: a[6])})
tb.BUILT.setdefault("msiren_align_stack_solve_group_r", {**_GROUP, 16: (np.float64, lambda a: a[6])})
INF = "inf"  # (how the recorder writes a float JSON has no literal for)


def rec(fn):
    return tb.record("align_stack", fn)


def held(arg):
    assert arg["pointer"] == "fresh"
    return arg["holds"]


def test_cost_with_nothing_optional():
    r = rec(lambda m, x: m.align_stack_cost(x["volume"], x["targets"], x["maps"]))
    assert r["commits"] is False and [c["function"] for c in r["calls"]] == ["msiren_align_stack_r"]
    a = r["calls"][0]["arguments"]
    assert a[:10] == ["handle", "in:volume", N, HH, WW, "in:targets", M, TH, TW, "in:maps"]
    assert a[10:12] == ["null", "null"] and held(a[12]) == {"type": "ndarray", "dtype": "float64", "shape": [M], "fill": INF}  # the default scale: +inf per target
    assert a[13:] == ["fresh", "null", "null", "null"]  # sums (unpacked into the result), then no warped, no wgrad, no rweight
    f = r["result"]["fields"]
    assert r["result"]["type"] == "AlignResultR" and f["warped"] is None and f["wgrad"] is None and f["rweight"] is None
    assert f["count"]["fill"] == 0 and f["cost"]["fill"] == 0.0 and f["grad"]["shape"] == [M, 11] and f["grad"]["fill"] == 0.0 and f["jtj"]["shape"] == [M, 11, 11]


def test_cost_with_everything():
    r = rec(lambda m, x: m.align_stack_cost(x["volume"], x["targets"], x["maps"], scale=x["scales"], weights=x["weights"], intensity=x["intensity"], warped=True,
                                            gradient=True, rweight=True))
    assert r["commits"] is False
    a = r["calls"][0]["arguments"]
    assert a[:12] == ["handle", "in:volume", N, HH, WW, "in:targets", M, TH, TW, "in:maps", "in:weights", "in:intensity"]
    assert a[12] == "in:scales" and a[14:] == ["out:warped", "out:wgrad", "out:rweight"]
    f = r["result"]["fields"]
    for name, shape in (("warped", [M, TH, TW]), ("wgrad", [3, M, TH, TW]), ("rweight", [M, TH, TW])):
        assert f[name]["shape"] == shape and f[name]["dtype"] == "float32" and f[name]["fill"] == "nan", name


def test_cost_with_one_scale_and_torch_inputs():
    r = rec(lambda m, x: m.align_stack_cost(tb._t(x["volume"]), tb._t(x["targets"]), tb._t(x["maps"]), scale=4.0, gradient=True))
    a = r["calls"][0]["arguments"]
    assert a[1] == "in:volume" and a[5] == "in:targets" and held(a[12])["fill"] == 4.0 and a[14:] == ["null", "out:wgrad", "null"]
    assert r["result"]["fields"]["wgrad"]["type"] == "ndarray"  # numpy out


def test_solve_with_nothing_optional_means_singletons():
    r = rec(lambda m, x: m.align_stack_solve(x["volume"], x["targets"], x["planes"], 2.5))
    assert r["commits"] is False and [c["function"] for c in r["calls"]] == ["msiren_align_stack_solve_group_r"]
    a = r["calls"][0]["arguments"]
    assert a[:9] == ["handle", "in:volume", N, HH, WW, "in:targets", M, TH, TW] and a[9]["opts"] == "AlignVolumeSolveGroupOpts"
    o = np.frombuffer(bytes.fromhex(a[9]["bytes"]), np.uint8)
    assert o[:16].view(np.int32).tolist() == [64, 12, 1, 0] and o[16:].view(np.float64).tolist() == [1e-3, 0.1, 10.0, 1e-9, 1e9, 2.5]
    assert held(a[10])["values"] == list(range(M + 1)) and a[11] == M and a[12] == "in:planes"
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    assert held(a[13])["values"] == ident * M and a[14:16] == ["null", "null"] and held(a[16])["fill"] == INF
    assert a[17:] == ["out:maps", "out:intensity", "fresh", "fresh", "fresh", "null"]  # rigid_out, report and target_report are unpacked into the result
    f = r["result"]["fields"]
    assert r["result"]["type"] == "SolveResultG" and f["trace"] is None and f["maps"]["fill"] == 0.0 and f["intensity"]["values"] == [1.0, 0.0] * M
    assert f["rotation"]["shape"] == [M, 3, 3] and f["flags"]["fill"] == 0 and f["cost"]["fill"] == 0.0 and f["accepted"]["shape"] == [M]


def test_solve_with_everything():
    r = rec(lambda m, x: m.align_stack_solve(x["volume"], x["targets"], x["planes"], 2.5, groups=[3, 1], scale=x["scales"], rotation=x["rotation_g"], shift=x["shift_g"],
                                             weights=x["weights"], intensity=x["intensity"], estimate_intensity=False, iterations=3, damping=0.5, down=0.25, up=4.0,
                                             lam_min=1e-3, lam_max=1e3, trace=True))
    assert r["commits"] is False
    a = r["calls"][0]["arguments"]
    o = np.frombuffer(bytes.fromhex(a[9]["bytes"]), np.uint8)
    assert o[:16].view(np.int32).tolist() == [64, 3, 0, 0] and o[16:].view(np.float64).tolist() == [0.5, 0.25, 4.0, 1e-3, 1e3, 2.5]
    assert held(a[10])["values"] == [0, 3, M] and a[11] == G
    x = tb.inputs()
    want = np.concatenate([x["rotation_g"].reshape(G, 9), x["shift_g"]], axis=1).ravel().tolist()
    assert held(a[13])["values"] == want and a[14:17] == ["in:weights", "in:intensity", "in:scales"] and a[22] == "out:trace"
    f = r["result"]["fields"]
    assert f["trace"]["shape"] == [3, G, 15] and f["trace"]["fill"] == 0.0 and f["intensity"]["values"] == x["intensity"].ravel().tolist()
    assert f["rotation"]["values"] == x["rotation_g"].ravel().tolist() and f["shift"]["values"] == x["shift_g"].ravel().tolist()  # the start, where nothing is written


def test_solve_without_iterations_has_an_empty_trace():
    r = rec(lambda m, x: m.align_stack_solve(x["volume"], x["targets"], x["planes"], 2.5, iterations=-2, trace=True))
    assert r["result"]["fields"]["trace"]["shape"] == [0, M, 15]


REFUSED = [
    ("stack-2d", lambda m, x: m.align_stack_cost(x["volume"][0], x["targets"], x["maps"])),
    ("stack-4d", lambda m, x: m.align_stack_cost(x["volume"][None], x["targets"], x["maps"])),
    ("targets", lambda m, x: m.align_stack_cost(x["volume"], x["targets"][0], x["maps"])),
    ("maps-width", lambda m, x: m.align_stack_cost(x["volume"], x["targets"], x["maps"][:, :6])),
    ("maps-rows", lambda m, x: m.align_stack_cost(x["volume"], x["targets"], x["maps"][:N])),
    ("weights", lambda m, x: m.align_stack_cost(x["volume"], x["targets"], x["maps"], weights=x["weights2"])),
    ("intensity", lambda m, x: m.align_stack_cost(x["volume"], x["targets"], x["maps"], intensity=x["intensity2"])),
    ("scale", lambda m, x: m.align_stack_cost(x["volume"], x["targets"], x["maps"], scale=x["scales"][:N])),
    ("solve-stack", lambda m, x: m.align_stack_solve(x["volume"][0], x["targets"], x["planes"], 2.5)),
    ("solve-targets", lambda m, x: m.align_stack_solve(x["volume"], x["targets"][0], x["planes"], 2.5)),
    ("solve-planes", lambda m, x: m.align_stack_solve(x["volume"], x["targets"], x["planes"][:N], 2.5)),
    ("solve-groups", lambda m, x: m.align_stack_solve(x["volume"], x["targets"], x["planes"], 2.5, groups=[0, 1, M + 1])),
    ("solve-rotation", lambda m, x: m.align_stack_solve(x["volume"], x["targets"], x["planes"], 2.5, groups=[3, 1], rotation=x["rotation"])),
    ("solve-shift", lambda m, x: m.align_stack_solve(x["volume"], x["targets"], x["planes"], 2.5, shift=x["shift_g"])),
    ("solve-weights", lambda m, x: m.align_stack_solve(x["volume"], x["targets"], x["planes"], 2.5, weights=x["weights2"])),
    ("solve-intensity", lambda m, x: m.align_stack_solve(x["volume"], x["targets"], x["planes"], 2.5, intensity=x["intensity2"])),
    ("solve-scale", lambda m, x: m.align_stack_solve(x["volume"], x["targets"], x["planes"], 2.5, scale=x["scales"][:N])),
]


@pytest.mark.parametrize("name,fn", REFUSED, ids=[n for n, _ in REFUSED])
def test_wrong_shapes_raise_before_the_library_is_entered(name, fn):
    assert rec(fn) == {"raises": "ValueError", "calls": []}
