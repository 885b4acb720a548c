"""The kernels of msiren_align_volume_solve_group* (align_group.hip.h) in the built library, from the code objects' metadata only (no GPU): all are
there, the project, step and apply kernels once per intensity mode, none uses scratch (private segment 0, no spills: the 11 x 8 Jacobian and the
column of H B in the project kernel, the 6 x 6 system in the step kernel stay in registers; the upload kernel reads its 512 offsets from its
arguments, not from a private copy), no LDS, workgroups of 256."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

# kernel -> instantiations
KERNELS = {"align_group_upload_kernel": 1, "align_group_init_kernel": 1, "align_group_decide_kernel": 1, "align_group_project_kernel": 2, "align_group_step_kernel": 2,
           "align_group_apply_kernel": 2}
# registers of the unified file per kernel as built and recorded in LAB_NOTES.md section 28 (a wave has 512): (fixed, estimated)
REGISTERS = {"align_group_project_kernel": (90, 130), "align_group_step_kernel": (82, 124), "align_group_apply_kernel": (76, 100)}
LENGTHS = {"align_group_project_kernel": 26, "align_group_step_kernel": 23, "align_group_apply_kernel": 24}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_is_there_without_scratch(meta, kernel):
    got = [k for k in meta if kernel in k]
    assert len(got) == KERNELS[kernel], (kernel, got)
    for name in got:
        m = meta[name]
        print(name, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64, m
        assert m["group_segment_fixed_size"] == 0, m


def test_the_templated_kernels_are_instantiated_per_intensity_mode(meta):
    for kernel, regs in REGISTERS.items():
        names = {est: f"_ZN6msiren{LENGTHS[kernel]}{kernel}ILi{est}EEEvNS_16AlignGroupParamsE" for est in (0, 1)}
        assert {k for k in meta if kernel in k} == set(names.values())
        for est in (0, 1):
            m = meta[names[est]]
            assert m["vgpr_count"] <= regs[est] and m["agpr_count"] == 0, (kernel, est, m)


def test_new_names_do_not_hide_in_the_existing_kernels_counts(meta):
    """the code-object tests of the other align families count instantiations by substring: none of their names is inside a new one"""
    old = ["align_volume_partial", "align_volume_combine", "align_volume_solve_init", "align_volume_step", "align_partial", "align_combine", "align_solve_init",
           "align_step", "align_volume_count", "align_volume_fill", "align_count", "align_fill"]
    for new in (k for k in meta if any(x in k for x in KERNELS)):
        assert not any(o in new for o in old), new
