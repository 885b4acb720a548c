"""The kernels of msiren_align_slices_w / msiren_align_solve_w (align_w.hip.h) in the built library, from the code objects' metadata (no GPU):
the four are there, none uses scratch (private segment 0, no spills: the 47 accumulators and the 8 x 8 / 5 x 5 systems stay in registers),
workgroups of 256; only the partial kernel has LDS (its 47 x 4 wave totals).  The section 5.10 / 5.11 kernels are still there beside them."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

KERNELS = {"align_partial_w_kernel": 47 * 4 * 8, "align_combine_w_kernel": 0, "align_solve_init_w_kernel": 0, "align_step_w_kernel": 0}
PLAIN = ("align_partial_kernel", "align_combine_kernel", "align_solve_init_kernel", "align_step_kernel")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_kernel_is_there_without_scratch(meta, kernel):
    got = [k for k in meta if kernel in k]
    assert len(got) == 1, (kernel, got)
    m = meta[got[0]]
    print(got[0], {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64, m
    assert m["group_segment_fixed_size"] == KERNELS[kernel], m
    assert m["vgpr_count"] <= 512, m  # (one workgroup of four waves: a wave per SIMD has the whole unified file)


def test_the_plain_kernels_are_still_there(meta):
    for kernel in PLAIN:
        assert len([k for k in meta if kernel in k]) == 1, kernel
