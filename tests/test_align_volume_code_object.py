"""The six kernels of msiren_align_volume* (align_volume.hip.h) in the built library, from the code objects' metadata only (no GPU): all are
there, the init and step kernels once per mode, none uses scratch (private segment 0, no spills: the 56 accumulators of the reduce and the 9 x 9 and
6 x 6 systems of the step stay in registers), workgroups of 256; only the reduce uses LDS (56 x 4 doubles)."""
import os

import pytest

from test_jet_code_object import LIB, READELF, kernel_metadata

# kernel -> (instantiations, bytes of LDS)
KERNELS = {"align_volume_count_kernel": (1, 0), "align_volume_fill_kernel": (1, 0), "align_volume_partial_kernel": (1, 56 * 4 * 8),
           "align_volume_combine_kernel": (1, 0), "align_volume_solve_init_kernel": (2, 0), "align_volume_step_kernel": (2, 0)}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    return kernel_metadata(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_is_there_without_scratch(meta, kernel):
    count, lds = KERNELS[kernel]
    got = [k for k in meta if kernel in k]
    assert len(got) == count, (kernel, got)
    for name in got:
        m = meta[name]
        print(name, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64, m
        assert m["group_segment_fixed_size"] == lds, m
