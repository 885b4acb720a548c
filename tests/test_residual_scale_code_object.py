"""The kernels of msiren_residual_scale* (residual_scale.hip.h) in the built library, from the code objects' metadata only (no GPU): every rscale_* kernel
is there exactly once, uses no scratch (private segment 0, no spills), workgroups of 256 in wave64, the LDS of its histograms (four wave-private
histograms of 256 bins; in the choice the four waves' sums and one row of 256 for the scan) and no more registers than LAB_NOTES.md section 39 records.  None of the substrings by which the
older families' code-object tests count their kernels hides in a new mangled name, and those families' kernels are still there once each."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

# name -> (LDS bytes, VGPRs, SGPRs as built: upper bounds)
KERNELS = {
    "rscale_upload_kernel": (0, 4, 12),
    "rscale_keys_kernel": (4096, 26, 34),
    "rscale_hist_kernel": (4096, 12, 28),
    "rscale_rekey_kernel": (4096, 13, 23),
    "rscale_choose_kernel": (5120, 68, 28),
    "rscale_finish_kernel": (0, 16, 22),
}
OLD = ("fuse_", "solve_", "project_", "align_", "resample_", "irls_", "combine_r", "combine_s", "ragged")
SINGLE = ("align_group_upload_kernel", "align_group_init_kernel", "fuse_setup_kernel", "fuse_gather_kernel", "project_gather_kernel", "project_stats_kernel",
          "solve_forward_kernel", "solve_transpose_kernel", "solve_reduce_kernel", "irls_reweight_kernel", "irls_stats_kernel", "irls_stop_kernel")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


def test_every_kernel_is_there_once_without_scratch(meta):
    got = sorted(k for k in meta if "rscale" in k)
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
        if "rscale" in k:
            assert not any(o in k for o in OLD), k
    for name in SINGLE:
        assert len([k for k in meta if name in k]) == 1, name
