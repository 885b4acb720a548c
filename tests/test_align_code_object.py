"""The bin and reduce kernels of the align call (align.hip.h) in the built library, from the code objects' metadata (no GPU): the four are
there, none uses scratch (private segment 0, no spills), workgroups of 256; only the partial kernel has LDS (its 29 x 4 wave totals)."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

KERNELS = {"align_count_kernel": 0, "align_fill_kernel": 0, "align_partial_kernel": 29 * 4 * 8, "align_combine_kernel": 0}


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
    assert m["group_segment_fixed_size"] == KERNELS[kernel] and m["vgpr_count"] <= 128, m  # (four waves per SIMD and more)
