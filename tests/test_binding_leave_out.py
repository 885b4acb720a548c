"""``ModulatedSiren.leave_out_targets`` on a host without a device, with tests/test_binding_calls.py's recording stand-in for the library (imported, not
edited): the method commits no weights, passes the scalars and the 32 bytes of msiren_fuse_opts as documented, null for what was not given and for
every per-target pointer where there is no target, builds the group offsets itself, pre-fills its outputs per DESIGN.md section 5.21 (NaN for simulated,
residual and the volume, 0 for the coverages, stats and flags), and raises ValueError for wrong shapes before the library is entered."""
import numpy as np
import pytest

import test_binding_calls as tb

M, TH, TW, GRID = tb.M, tb.TH, tb.TW, tb.GRID
# the group offsets the binding builds itself, read through their pointer (the recorder looks them up by name)
tb.BUILT.setdefault("msiren_leave_out_targets", {9: (np.int32, lambda a: a[10] + 1)})
NAN = "nan"  # (how the recorder writes a float JSON has no literal for)


def rec(fn):
    return tb.record("leave_out_targets", fn)


def opts_of(arg):
    assert arg["opts"] == "FuseOpts"
    o = np.frombuffer(bytes.fromhex(arg["bytes"]), np.uint8)
    assert len(o) == 32
    return o[:8].view(np.int32).tolist(), o[8:].view(np.float64).tolist()


def array(shape, fill, dtype="float32"):
    return {"type": "ndarray", "dtype": dtype, "shape": list(shape), "fill": fill}


def test_with_nothing_optional():
    r = rec(lambda m, x: m.leave_out_targets(x["targets"], x["maps"], GRID, 4.0))
    assert r["commits"] is False and [c["function"] for c in r["calls"]] == ["msiren_leave_out_targets"]
    a = r["calls"][0]["arguments"]
    assert a[:8] == ["handle", "in:targets", M, TH, TW, "in:maps", "null", "null"]
    assert opts_of(a[8]) == ([32, 0], [4.0, 4.0, 0.0])                      # struct_size, reserved; spacing, thickness = spacing, min_coverage
    assert a[9:14] == ["null", 0, GRID[0], GRID[1], GRID[2]]                # no groups; n, H, W
    assert a[14:] == ["out:simulated", "null", "null", "null", "out:flags", "null", "null"]
    f = r["result"]["fields"]
    assert r["result"]["type"] == "LeaveOutResult" and all(f[k] is None for k in ("coverage", "residual", "stats", "volume", "volume_coverage"))
    assert f["simulated"] == array((M, TH, TW), NAN) and f["flags"] == array((M,), 0, "int32")


def test_with_everything():
    r = rec(lambda m, x: m.leave_out_targets(x["targets"], x["maps"], GRID, 4.0, groups=[3, 1], thickness=1.5, weights=x["weights"], intensity=x["intensity"],
                                             min_coverage=0.25, coverage=True, residual=True, stats=True, volume=True))
    assert r["commits"] is False
    a = r["calls"][0]["arguments"]
    assert a[:8] == ["handle", "in:targets", M, TH, TW, "in:maps", "in:weights", "in:intensity"]
    assert opts_of(a[8]) == ([32, 0], [4.0, 1.5, 0.25])
    assert a[9]["pointer"] == "fresh" and a[9]["holds"] == {"type": "ndarray", "dtype": "int32", "shape": [3], "values": [0, 3, M]} and a[10] == 2
    assert a[11:] == [GRID[0], GRID[1], GRID[2], "out:simulated", "out:coverage", "out:residual", "out:stats", "out:flags", "out:volume", "out:volume_coverage"]
    f = r["result"]["fields"]
    assert f["simulated"] == array((M, TH, TW), NAN) and f["residual"] == array((M, TH, TW), NAN) and f["coverage"] == array((M, TH, TW), 0.0)
    assert f["stats"] == array((M, 4), 0.0, "float64") and f["volume"] == array(GRID, NAN) and f["volume_coverage"] == array(GRID, 0.0)


def test_groups_as_offsets_and_torch_inputs():
    r = rec(lambda m, x: m.leave_out_targets(tb._t(x["targets"]), tb._t(x["maps"]), GRID, 2.0, groups=[0, 1, M], weights=tb._t(x["weights"]), volume=True))
    a = r["calls"][0]["arguments"]
    assert a[1] == "in:targets" and a[5:7] == ["in:maps", "in:weights"] and a[9]["holds"]["values"] == [0, 1, M] and a[10] == 2
    assert a[15:18] == ["null", "null", "null"] and a[19:] == ["out:volume", "out:volume_coverage"]
    assert r["result"]["fields"]["volume"]["type"] == "ndarray"             # numpy out


def test_no_targets_pass_null_for_every_per_target_pointer():
    r = rec(lambda m, x: m.leave_out_targets(x["targets0"], x["maps0"], GRID, 4.0, weights=x["weights0"], intensity=x["intensity0"], coverage=True, residual=True,
                                             stats=True, volume=True))
    a = r["calls"][0]["arguments"]
    assert a[:8] == ["handle", "null", 0, TH, TW, "null", "null", "null"] and a[9:11] == ["null", 0]
    assert a[14:] == ["null", "null", "null", "null", "null", "out:volume", "out:volume_coverage"]
    f = r["result"]["fields"]
    assert f["simulated"]["shape"] == [0, TH, TW] and f["stats"]["shape"] == [0, 4] and f["volume"] == array(GRID, NAN)


REFUSED = [
    ("targets-2d", lambda m, x: m.leave_out_targets(x["targets"][0], x["maps"], GRID, 4.0)),
    ("maps-rows", lambda m, x: m.leave_out_targets(x["targets"], x["maps"][:2], GRID, 4.0)),
    ("maps-width", lambda m, x: m.leave_out_targets(x["targets"], x["maps"][:, :6], GRID, 4.0)),
    ("weights", lambda m, x: m.leave_out_targets(x["targets"], x["maps"], GRID, 4.0, weights=x["weights2"])),
    ("intensity", lambda m, x: m.leave_out_targets(x["targets"], x["maps"], GRID, 4.0, intensity=x["intensity2"])),
    ("shape", lambda m, x: m.leave_out_targets(x["targets"], x["maps"], GRID[:2], 4.0)),
    ("groups-sizes", lambda m, x: m.leave_out_targets(x["targets"], x["maps"], GRID, 4.0, groups=[3, 2])),
    ("groups-offsets", lambda m, x: m.leave_out_targets(x["targets"], x["maps"], GRID, 4.0, groups=[0, 2, 2, M])),
]


@pytest.mark.parametrize("name,fn", REFUSED, ids=[n for n, _ in REFUSED])
def test_wrong_shapes_raise_before_the_library_is_entered(name, fn):
    assert rec(fn) == {"raises": "ValueError", "calls": []}
