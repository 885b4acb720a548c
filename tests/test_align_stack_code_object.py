"""The kernel of msiren_align_stack_r* (align_stack.hip.h) in the built library, from the code objects' metadata only (no GPU): it is there once, uses
no scratch (private segment 0, no spills: the 80 accumulators, the eight corners and the robust factors stay in registers), the LDS of the weighted
reduce (80 x 4 doubles), workgroups of 256, and its registers are those recorded in LAB_NOTES.md section 37.  The combine kernel and the four group
step kernels are the older families', so nothing else appears, and the two reduces whose body it shares keep their names."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

KERNEL = "align_stack_partial_r_kernel"
NAME = "_ZN6msiren28align_stack_partial_r_kernelEPKfS1_S1_S1_S1_PKdPfS4_S4_Pdiiiiiii"
REGISTERS = 208  # of the unified file, as built; a wave has 512
SGPRS = 72


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


def test_kernel_is_there_once_without_scratch(meta):
    got = [k for k in meta if "align_stack" in k]
    assert got == [NAME], got
    m = meta[NAME]
    print(NAME, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64, m
    assert m["group_segment_fixed_size"] == 80 * 4 * 8, m
    assert m["vgpr_count"] <= REGISTERS and m["agpr_count"] == 0 and m["sgpr_count"] <= SGPRS, m


def test_no_old_name_hides_in_the_new_one_and_the_shared_kernels_stay_single(meta):
    """the code-object tests of the other align families count instantiations by substring: none of their names is inside the new one"""
    old = ["align_volume_partial_kernel", "align_volume_partial_w_kernel", "align_volume_partial_r_kernel", "align_volume_combine", "align_volume_step", "align_partial_w_kernel",
           "align_partial_kernel", "align_group_"]
    assert not any(o in NAME for o in old)
    assert len([k for k in meta if "align_volume_combine_w_kernel" in k]) == 1 and not [k for k in meta if "combine_s" in k or "align_stack_combine" in k]
    for shared in ("align_volume_partial_w_kernel", "align_volume_partial_r_kernel"):  # the pixel source became a callable: the names did not move
        assert len([k for k in meta if shared in k]) == 1, shared
