"""siren_trunk_f32_ragged_kernel / siren_trunk_f32_jet_ragged_kernel in the built library, from the code objects' metadata (no GPU): every
instance of the two lists is there, none uses scratch (private segment 0, no spills), and registers and LDS fit the occupancy each kernel
is laid out for -- the fp32 trunk's (two workgroups per CU up to a hidden width of 256, one above) and the jet's (one)."""
import os

import pytest

from test_jet_code_object import LDS_PER_CU, LIB, READELF, jet_lds_bytes, kernel_metadata


def f32_lds_bytes(HP):  # siren_trunk_f32.hip.h: X image [HP/4][64] float4 + layer-0 rows [HP] float4, dynamic
    return HP * 256 + HP * 16


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


def check_common(name, m):
    print(name, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64, (name, m)


def test_value_instances(meta):
    got = {k: v for k, v in meta.items() if "siren_trunk_f32_ragged_kernel" in k}
    want = {f"_ZN6msiren29siren_trunk_f32_ragged_kernelILi{hp}ELi{act}ELi{res}EEEvNS_17TrunkRaggedParamsE": hp
            for hp in (128, 256, 384, 512) for act in (0, 1) for res in (0, 1)}
    assert set(got) == set(want), sorted(got)
    for name, m in got.items():
        hp = want[name]
        check_common(name, m)
        wgs = 2 if hp <= 256 else 1  # workgroups of 4 waves per CU = waves per SIMD: they share the 512 registers per lane and the 160 KB
        assert m["vgpr_count"] * wgs <= 512, (name, m)
        assert (m["group_segment_fixed_size"] + f32_lds_bytes(hp)) * wgs <= LDS_PER_CU, (name, m)


def test_jet_instances(meta):
    got = {k: v for k, v in meta.items() if "siren_trunk_f32_jet_ragged_kernel" in k}
    want = {f"_ZN6msiren33siren_trunk_f32_jet_ragged_kernelILi{hp}ELi{act}EEEvNS_17TrunkRaggedParamsE": hp for hp in (128, 256) for act in (0, 1)}
    assert set(got) == set(want), sorted(got)
    for name, m in got.items():
        hp = want[name]
        check_common(name, m)
        assert m["vgpr_count"] <= 512, (name, m)
        assert m["group_segment_fixed_size"] + jet_lds_bytes(hp) <= LDS_PER_CU, (name, m)
    assert jet_lds_bytes(256) > 64 * 1024  # (the opt-in dynamic-LDS limit, raised by the launcher)


def test_item_table_kernel_is_there(meta):
    got = [k for k in meta if "ragged_items_kernel" in k]
    assert len(got) == 2, got  # chunks of 64 and of 32
    for name in got:
        check_common(name, meta[name])
