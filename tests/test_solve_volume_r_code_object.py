"""The kernels of msiren_solve_volume_r* (solve_volume_r.hip.h) in the built library, from the code objects' metadata only (no GPU): each irls_* kernel is
there once, uses no scratch (private segment 0, no spills), workgroups of 256, no LDS, and the registers are those recorded in LAB_NOTES.md section
35; the kernels the call launches as they are (solve_volume.hip.h, fuse.hip.h, project.hip.h) are still there once."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

# short name -> (VGPRs, SGPRs) as built; the reweighting gather holds the record of 20 doubles and the box in SGPRs, as solve_forward_kernel does
REGISTERS = {
    "irls_reweight_kernel": (58, 96),
    "irls_stats_kernel": (30, 36),
    "irls_stop_kernel": (2, 14),
}
PARENTS = ("17fuse_setup_kernelE", "18fuse_gather_kernelE", "21project_gather_kernelE", "20project_stats_kernelE", "18solve_start_kernelE", "21solve_coverage_kernelE",
           "20solve_forward_kernelE", "22solve_transpose_kernelE", "21solve_residual_kernelE", "16solve_dot_kernelE", "19solve_reduce_kernelE", "22solve_update_xr_kernelE",
           "21solve_update_p_kernelE", "18solve_store_kernelE")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


def irls_kernels(meta):
    return sorted(k for k in meta if "msiren" in k and "irls_" in k)


def test_every_kernel_is_there_once(meta):
    names = irls_kernels(meta)
    print(names)
    assert len(names) == len(REGISTERS)
    for short in REGISTERS:
        assert sum(f"{len(short)}{short}E" in k for k in names) == 1, short  # (the mangled name: length, name, end of the nested name)


@pytest.mark.parametrize("short", sorted(REGISTERS))
def test_kernel_has_no_scratch_and_the_recorded_registers(meta, short):
    (name,) = [k for k in irls_kernels(meta) if f"{len(short)}{short}E" in k]
    m = meta[name]
    print(name, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64, m
    assert m["group_segment_fixed_size"] == 0, m  # no LDS: the stats park their column sums in the stream's scratch
    vgprs, sgprs = REGISTERS[short]
    assert m["vgpr_count"] <= vgprs and m["agpr_count"] == 0 and m["sgpr_count"] <= sgprs, m


def test_the_parents_kernels_are_still_there_once(meta):
    """everything but the reweighting is launched as it is: not copied, not instantiated a second time"""
    for parent in PARENTS:
        assert sum(parent in k for k in meta) == 1, parent


def test_no_old_name_hides_in_the_new_ones(meta):
    """the code-object tests of the other families count instantiations by substring: none of their names is inside the new ones"""
    old = ["solve_", "fuse_", "project_", "align_volume_partial", "align_volume_combine", "align_volume_step", "align_partial", "align_group_", "align_", "resample_"]
    assert not any(o in name for o in old for name in REGISTERS)
