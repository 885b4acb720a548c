"""The kernels of msiren_fuse_targets* (fuse.hip.h) in the built library, from the code objects' metadata only (no GPU): each is there once, uses no
scratch (private segment 0, no spills: num, den and a target's record stay in registers), no LDS, workgroups of 256, and the registers are those
recorded in LAB_NOTES.md section 31."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

SETUP = "_ZN6msiren17fuse_setup_kernelEPKfS1_ddiPdPi"
GATHER = "_ZN6msiren18fuse_gather_kernelEPKfS1_PKdiiiiiiiddPfS4_"
REGISTERS = {SETUP: (42, 26), GATHER: (76, 68)}  # (VGPRs, SGPRs) as built; the gather holds a record of 20 doubles in SGPRs


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("name", [SETUP, GATHER])
def test_kernel_is_there_once_without_scratch_or_lds(meta, name):
    assert sorted(k for k in meta if "fuse_" in k) == sorted([SETUP, GATHER])
    m = meta[name]
    print(name, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64 and m["group_segment_fixed_size"] == 0, m
    vgprs, sgprs = REGISTERS[name]
    assert m["vgpr_count"] <= vgprs and m["agpr_count"] == 0 and m["sgpr_count"] <= sgprs, m


def test_no_old_name_hides_in_the_new_ones(meta):
    """the code-object tests of the align families count instantiations by substring: none of their names is inside the new ones"""
    old = ["align_volume_partial", "align_volume_combine", "align_volume_step", "align_partial", "align_group_", "resample_"]
    assert not any(o in name for o in old for name in (SETUP, GATHER))
