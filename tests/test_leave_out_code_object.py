"""The kernels of msiren_leave_out_targets* (leave_out.hip.h) in the built library, from the code objects' metadata only (no GPU): every loo_* kernel is
there exactly once, uses no scratch (private segment 0, no spills), workgroups of 256 in wave64, no LDS -- the gathers keep their sums in registers --
and no more registers than LAB_NOTES.md section 42 records from the build.  None of the substrings by which the older families' code-object tests count
their kernels hides in a new mangled name, and those families' kernels are still there once each: the fuse unit gained kernels, none a second time."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

# name -> (LDS bytes, VGPRs, SGPRs as built: upper bounds)
KERNELS = {
    "loo_upload_kernel": (0, 4, 12),
    "loo_sums_kernel": (0, 76, 70),
    "loo_gather_kernel": (0, 118, 104),
}
OLD = ("fuse_", "project_", "solve_", "align_", "rscale", "irls_", "resample_", "combine_r", "combine_s", "ragged")
SINGLE = ("align_group_upload_kernel", "align_group_init_kernel", "fuse_setup_kernel", "fuse_gather_kernel", "project_gather_kernel", "project_stats_kernel",
          "solve_forward_kernel", "solve_transpose_kernel", "solve_coverage_kernel", "solve_reduce_kernel", "irls_reweight_kernel", "irls_stats_kernel", "irls_stop_kernel",
          "rscale_upload_kernel", "rscale_keys_kernel", "rscale_hist_kernel", "rscale_rekey_kernel", "rscale_choose_kernel", "rscale_finish_kernel")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


def test_every_kernel_is_there_once_without_scratch(meta):
    got = sorted(k for k in meta if "loo_" in k)
    assert len(got) == len(KERNELS), got
    for name, (lds, vgprs, sgprs) in KERNELS.items():
        mine = [k for k in got if name in k]
        assert len(mine) == 1, (name, mine)
        m = meta[mine[0]]
        print(mine[0], {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64, (name, m)
        assert m["group_segment_fixed_size"] == lds, (name, m)
        assert m["vgpr_count"] <= vgprs and m["agpr_count"] == 0 and m["sgpr_count"] <= sgprs, (name, m)


def test_no_old_name_hides_in_the_new_ones_and_the_older_kernels_stay_single(meta):
    for k in meta:
        if "loo_" in k:
            assert not any(o in k for o in OLD), k
    for name in SINGLE:
        assert len([k for k in meta if name in k]) == 1, name
