"""The kernels of msiren_project_volume* (project.hip.h) in the built library, from the code objects' metadata only (no GPU): each is there once, uses
no scratch (private segment 0, no spills: num, den and the target's record stay in registers), workgroups of 256, the gather no LDS, and the registers
are those recorded in LAB_NOTES.md section 32."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

GATHER = "_ZN6msiren21project_gather_kernelEPKfPKdiiiiiiidddPfS4_"
STATS = "_ZN6msiren20project_stats_kernelEPKfS1_S1_iiPdPfS2_"
REGISTERS = {GATHER: (62, 84), STATS: (28, 38)}  # (VGPRs, SGPRs) as built; the gather holds the record of 20 doubles and the box in SGPRs


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("name", [GATHER, STATS])
def test_kernel_is_there_once_without_scratch(meta, name):
    assert sorted(k for k in meta if "msiren" in k and ("project_gather" in k or "project_stats" in k)) == sorted([GATHER, STATS])
    m = meta[name]
    print(name, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64 and m["group_segment_fixed_size"] == 0, m
    vgprs, sgprs = REGISTERS[name]
    assert m["vgpr_count"] <= vgprs and m["agpr_count"] == 0 and m["sgpr_count"] <= sgprs, m


def test_no_old_name_hides_in_the_new_ones(meta):
    """the code-object tests of the other families count instantiations by substring: none of their names is inside the new ones"""
    old = ["fuse_", "align_volume_partial", "align_volume_combine", "align_volume_step", "align_partial", "align_group_", "resample_"]
    assert not any(o in name for o in old for name in (GATHER, STATS))
