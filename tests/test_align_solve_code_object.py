"""The two kernels of msiren_align_solve (align.hip.h) in the built library, from the code objects' metadata (no GPU): both are there, neither
uses scratch (private segment 0, no spills: the 6 x 6 and 3 x 3 systems stay in registers), workgroups of 256, no LDS."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

KERNELS = ("align_solve_init_kernel", "align_step_kernel")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_is_there_without_scratch(meta, kernel):
    got = [k for k in meta if kernel in k]
    assert len(got) == 1, (kernel, got)
    m = meta[got[0]]
    print(got[0], {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64, m
    assert m["group_segment_fixed_size"] == 0, m
