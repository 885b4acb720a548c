"""The bin and blend kernels of the volume calls (resample_volume.hip.h) in the built library, from the code objects' metadata (no GPU):
the three are there, none uses scratch (private segment 0, no spills), workgroups of 256."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

KERNELS = ("resample_volume_count_kernel", "resample_volume_fill_kernel", "resample_volume_blend_kernel")


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
    assert m["group_segment_fixed_size"] == 0 and m["vgpr_count"] <= 128, m  # (no LDS; four waves per SIMD and more)
