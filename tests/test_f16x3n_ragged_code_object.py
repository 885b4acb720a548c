"""siren_trunk_f16x3n_ragged_kernel and siren_trunk_f32_ragged_cond_kernel in the built library, from the code objects' metadata (no GPU):
the six split-fp16 ragged instances are there; the straight-line (L = 5) and ring-of-4 loop forms use no scratch; the ring-of-3 loop form
uses no more than its siren_trunk_f16x3n_kernel sibling (which spills ~200 bytes a lane, LAB_NOTES.md section 15); registers fit the one
workgroup per CU the kernel is laid out for and its dynamic LDS (F16Lds<R>::total) the CU."""
import os

import pytest

from test_jet_code_object import LDS_PER_CU, LIB, READELF, kernel_metadata
from test_ragged_code_object import f32_lds_bytes

CHUNK = 32768


def f16_lds_total(R, L):  # siren_trunk_f16_common.hip.h: F16Lds<R>::total(L)
    bias = R * CHUNK + 4096 + 1024 + 1024
    mods = bias + (L - 1) * 1024
    queue = mods + 4 * L * 1024
    return queue + 16 + 64


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


def name_of(kernel, act, ring, lfix, params):
    return f"_ZN6msiren{len(kernel)}{kernel}ILi{act}ELi{ring}ELi{lfix}EEEvNS_{len(params)}{params}E"


def test_the_six_instances(meta):
    got = {k: v for k, v in meta.items() if "siren_trunk_f16x3n_ragged_kernel" in k}
    want = {name_of("siren_trunk_f16x3n_ragged_kernel", act, ring, lfix, "TrunkF16RaggedParams"): (act, ring, lfix)
            for act in (0, 1) for ring, lfix in ((3, 5), (4, 0), (3, 0))}
    assert set(got) == set(want), sorted(got)
    for name, m in got.items():
        act, ring, lfix = want[name]
        print(name, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64, (name, m)
        assert m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 512 and m["group_segment_fixed_size"] == 0, (name, m)  # one workgroup per CU; all LDS is dynamic
        if (ring, lfix) == (3, 0):
            sibling = meta[name_of("siren_trunk_f16x3n_kernel", act, 3, 0, "TrunkF16Params").replace("ELi0EEEv", "ELi0ELi0EEEv")]
            assert m["private_segment_fixed_size"] <= sibling["private_segment_fixed_size"], (name, m, sibling)
            assert m["vgpr_spill_count"] <= sibling["vgpr_spill_count"], (name, m, sibling)
        else:
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
    # the depths each instance serves fit the CU: the ring of 4 up to L = 5, the ring of 3 up to L = 11
    assert f16_lds_total(3, 5) <= LDS_PER_CU and f16_lds_total(4, 4) <= LDS_PER_CU and f16_lds_total(3, 11) <= LDS_PER_CU
    assert f16_lds_total(4, 6) > LDS_PER_CU and f16_lds_total(3, 12) > LDS_PER_CU


def test_the_conditional_exact_trunk(meta):
    got = {k: v for k, v in meta.items() if "siren_trunk_f32_ragged_cond_kernel" in k}
    assert set(got) == {f"_ZN6msiren34siren_trunk_f32_ragged_cond_kernelILi{act}EEEvNS_17TrunkRaggedParamsE" for act in (0, 1)}, sorted(got)
    for name, m in got.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] * 2 <= 512 and (m["group_segment_fixed_size"] + f32_lds_bytes(256)) * 2 <= LDS_PER_CU, (name, m)
