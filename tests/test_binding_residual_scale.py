"""``ModulatedSiren.residual_scale`` on a host without a device, with tests/test_binding_calls.py's recording stand-in for the library (imported, not
edited): the method commits no weights, passes the scalars and the 32 bytes of msiren_scale_opts as documented, null for what was not given and for
every per-target pointer where there is no target, builds the group offsets itself, pre-fills its outputs per DESIGN.md section 5.21 (+inf for the
scale, 0 for stats), and raises ValueError for wrong shapes before the library is entered."""
import numpy as np
import pytest

import test_binding_calls as tb

M, TH, TW = tb.M, tb.TH, tb.TW
# the group offsets the binding builds itself, read through their pointer (the recorder looks them up by name)
tb.BUILT.setdefault("msiren_residual_scale", {9: (np.int32, lambda a: a[10] + 1)})
INF = "inf"  # (how the recorder writes a float JSON has no literal for)


def rec(fn):
    return tb.record("residual_scale", fn)


def opts_of(arg):
    assert arg["opts"] == "ScaleOpts"
    o = np.frombuffer(bytes.fromhex(arg["bytes"]), np.uint8)
    assert len(o) == 32
    return o[:8].view(np.int32).tolist(), o[8:].view(np.float64).tolist()


def test_with_nothing_optional():
    r = rec(lambda m, x: m.residual_scale(x["targets"], tune=2.5))
    assert r["commits"] is False and [c["function"] for c in r["calls"]] == ["msiren_residual_scale"]
    a = r["calls"][0]["arguments"]
    assert a[:8] == ["handle", "in:targets", "null", "null", "null", M, TH, TW]
    assert opts_of(a[8]) == ([32, 0], [0.5, 2.5, 0.0])                      # struct_size, centre; quantile, tune, floor
    assert a[9:] == ["null", 0, "out:scale", "null"]                        # no groups, the scale, no stats
    f = r["result"]["fields"]
    assert r["result"]["type"] == "ResidualScaleResult" and f["stats"] is None
    assert f["scale"] == {"type": "ndarray", "dtype": "float64", "shape": [M], "fill": INF}


def test_with_everything():
    r = rec(lambda m, x: m.residual_scale(x["targets"], x["volume"][:1].reshape(-1)[:M * TH * TW].reshape(M, TH, TW), tune=8.9, weights=x["weights"],
                                          intensity=x["intensity"], groups=[3, 1], quantile=0.29, centre=True, floor=1e-6, stats=True))
    assert r["commits"] is False
    a = r["calls"][0]["arguments"]
    assert a[1] == "in:targets" and a[2] == "in:volume" and a[3:8] == ["in:weights", "in:intensity", M, TH, TW]
    assert opts_of(a[8]) == ([32, 1], [0.29, 8.9, 1e-6])
    assert a[9]["pointer"] == "fresh" and a[9]["holds"] == {"type": "ndarray", "dtype": "int32", "shape": [3], "values": [0, 3, M]} and a[10] == 2
    assert a[11:] == ["out:scale", "out:stats"]
    f = r["result"]["fields"]
    assert f["scale"]["fill"] == INF and f["stats"] == {"type": "ndarray", "dtype": "float64", "shape": [2, 4], "fill": 0.0}


def test_groups_as_offsets_pooled_and_torch_inputs():
    r = rec(lambda m, x: m.residual_scale(tb._t(x["targets"]), tb._t(x["weights"]), tune=1.0, groups=[0, M], stats=True))
    a = r["calls"][0]["arguments"]
    assert a[1:3] == ["in:targets", "in:weights"] and a[9]["holds"]["values"] == [0, M] and a[10] == 1
    f = r["result"]["fields"]
    assert f["stats"]["shape"] == [1, 4] and f["scale"]["type"] == "ndarray"  # numpy out
    r = rec(lambda m, x: m.residual_scale(x["targets"], tune=1.0, stats=True))
    assert r["result"]["fields"]["stats"]["shape"] == [M, 4] and r["calls"][0]["arguments"][12] == "out:stats"  # without groups: one row per target


def test_no_targets_pass_null_for_every_per_target_pointer():
    r = rec(lambda m, x: m.residual_scale(x["targets0"], x["weights0"], tune=1.0, weights=x["weights0"], intensity=x["intensity0"], stats=True))
    a = r["calls"][0]["arguments"]
    assert a[:8] == ["handle", "null", "null", "null", "null", 0, TH, TW] and a[9:] == ["null", 0, "null", "null"]
    f = r["result"]["fields"]
    assert f["scale"]["shape"] == [0] and f["stats"]["shape"] == [0, 4]


REFUSED = [
    ("targets-2d", lambda m, x: m.residual_scale(x["targets"][0], tune=1.0)),
    ("simulated", lambda m, x: m.residual_scale(x["targets"], x["targets2"], tune=1.0)),
    ("weights", lambda m, x: m.residual_scale(x["targets"], tune=1.0, weights=x["weights2"])),
    ("intensity", lambda m, x: m.residual_scale(x["targets"], x["weights"], tune=1.0, intensity=x["intensity2"])),
    ("intensity-alone", lambda m, x: m.residual_scale(x["targets"], tune=1.0, intensity=x["intensity"])),
    ("groups-sizes", lambda m, x: m.residual_scale(x["targets"], tune=1.0, groups=[3, 2])),
    ("groups-offsets", lambda m, x: m.residual_scale(x["targets"], tune=1.0, groups=[0, 2, 2, M])),
]


@pytest.mark.parametrize("name,fn", REFUSED, ids=[n for n, _ in REFUSED])
def test_wrong_shapes_raise_before_the_library_is_entered(name, fn):
    assert rec(fn) == {"raises": "ValueError", "calls": []}
