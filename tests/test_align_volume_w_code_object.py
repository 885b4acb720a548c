"""The four kernels of msiren_align_volume_w* (align_volume_w.hip.h) in the built library, from the code objects' metadata only (no GPU): all are
there, the init kernel once per geometry mode and the step kernel once per (geometry mode, intensity mode), none uses scratch (private segment 0,
no spills: the 80 accumulators of the reduce and the 9 x 9, 11 x 11, 6 x 6 and 8 x 8 systems of the step stay in registers -- the step keeps
only the triangle its solve reads, no LDS), workgroups of 256; only the reduce uses LDS (80 x 4 doubles)."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

# kernel -> (instantiations, bytes of LDS, workgroup size)
KERNELS = {"align_volume_partial_w_kernel": (1, 80 * 4 * 8, 256), "align_volume_combine_w_kernel": (1, 0, 256),
           "align_volume_solve_init_w_kernel": (2, 0, 256), "align_volume_step_w_kernel": (4, 0, 256)}
# the step kernel's registers of the unified file (AGPRs included) per (geometry mode, intensity mode), as built and recorded in LAB_NOTES.md
# section 27: affine 158 (9 x 9) / 208 (11 x 11), rigid 256 (9 x 6 -> 6 x 6) / 266 (11 x 8 -> 8 x 8, 10 of them AGPRs).  A wave has 512.
STEP_REGISTERS = {(0, 0): 158, (0, 1): 208, (1, 0): 256, (1, 1): 266}
STEP_INSTANCES = {f"_ZN6msiren26align_volume_step_w_kernelILi{mode}ELi{est}EEEvNS_23AlignVolumeSolveWParamsE" for mode in (0, 1) for est in (0, 1)}
INIT_INSTANCES = {f"_ZN6msiren32align_volume_solve_init_w_kernelILi{mode}EEEvNS_23AlignVolumeSolveWParamsEPKfPKdS3_d" for mode in (0, 1)}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_is_there_without_scratch(meta, kernel):
    count, lds, wg = KERNELS[kernel]
    got = [k for k in meta if kernel in k]
    assert len(got) == count, (kernel, got)
    for name in got:
        m = meta[name]
        print(name, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["max_flat_workgroup_size"] == wg and m["wavefront_size"] == 64, m
        assert m["group_segment_fixed_size"] == lds, m


def test_step_and_init_are_instantiated_per_mode(meta):
    assert {k for k in meta if "align_volume_step_w_kernel" in k} == STEP_INSTANCES
    assert {k for k in meta if "align_volume_solve_init_w_kernel" in k} == INIT_INSTANCES
    for (mode, est), regs in STEP_REGISTERS.items():
        m = meta[f"_ZN6msiren26align_volume_step_w_kernelILi{mode}ELi{est}EEEvNS_23AlignVolumeSolveWParamsE"]
        assert m["vgpr_count"] <= regs and m["agpr_count"] <= m["vgpr_count"] <= 512, ((mode, est), m)


def test_new_names_do_not_hide_in_the_existing_kernels_counts(meta):
    """the code-object tests of the other align families count instantiations by substring: none of their names is inside a new one"""
    old = ["align_volume_partial_kernel", "align_volume_combine_kernel", "align_volume_solve_init_kernel", "align_volume_step_kernel", "align_partial_w_kernel",
           "align_combine_w_kernel", "align_solve_init_w_kernel", "align_step_w_kernel", "align_partial_kernel", "align_combine_kernel", "align_step_kernel"]
    for new in (k for k in meta if any(x in k for x in KERNELS)):
        assert not any(o in new for o in old), new
