"""The kernels of msiren_solve_volume* (solve_volume.hip.h) in the built library, from the code objects' metadata only (no GPU): each is there once, uses
no scratch (private segment 0, no spills), workgroups of 256, the two gathers and every pointwise kernel no LDS, and the registers are those recorded
in LAB_NOTES.md section 33."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

# short name -> (VGPRs, SGPRs) as built; the gathers hold the record of 20 doubles (and the forward ones the box) in SGPRs
REGISTERS = {
    "solve_start_kernel": (5, 12),
    "solve_coverage_kernel": (58, 90),
    "solve_forward_kernel": (58, 80),
    "solve_transpose_kernel": (70, 71),
    "solve_residual_kernel": (10, 14),
    "solve_dot_kernel": (48, 30),
    "solve_reduce_kernel": (14, 26),
    "solve_update_xr_kernel": (12, 18),
    "solve_update_p_kernel": (8, 14),
    "solve_store_kernel": (4, 14),
}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


def solve_kernels(meta):
    return sorted(k for k in meta if "msiren" in k and "solve_" in k and "align" not in k)


def test_every_kernel_is_there_once(meta):
    names = solve_kernels(meta)
    print(names)
    assert len(names) == len(REGISTERS)
    for short in REGISTERS:
        assert sum(f"{len(short)}{short}E" in k for k in names) == 1, short  # (the mangled name: length, name, end of the nested name)


@pytest.mark.parametrize("short", sorted(REGISTERS))
def test_kernel_has_no_scratch_and_the_recorded_registers(meta, short):
    (name,) = [k for k in solve_kernels(meta) if f"{len(short)}{short}E" in k]
    m = meta[name]
    print(name, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64, m
    assert m["group_segment_fixed_size"] == 0, m  # no kernel of the solve uses LDS: the reduction parks its sums in the stream's scratch
    vgprs, sgprs = REGISTERS[short]
    assert m["vgpr_count"] <= vgprs and m["agpr_count"] == 0 and m["sgpr_count"] <= sgprs, m


def test_the_parents_kernels_are_still_there_once(meta):
    """fuse_setup_kernel and fuse_gather_kernel are reused, not copied"""
    for parent in ("17fuse_setup_kernelE", "18fuse_gather_kernelE", "21project_gather_kernelE", "20project_stats_kernelE"):
        assert sum(parent in k for k in meta) == 1, parent


def test_no_old_name_hides_in_the_new_ones(meta):
    """the code-object tests of the other families count instantiations by substring: none of their names is inside the new ones"""
    old = ["fuse_", "project_", "align_volume_partial", "align_volume_combine", "align_volume_step", "align_partial", "align_group_", "resample_"]
    assert not any(o in name for o in old for name in REGISTERS)
