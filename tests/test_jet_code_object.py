"""siren_trunk_f32_jet_kernel in the built library, from its code object's metadata (no GPU): the four instances are there, none uses
scratch (private segment 0, no spills), and registers and LDS leave room for the one workgroup per CU the kernel is laid out for."""
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
LIB = os.path.join(ROOT, "mri_inr_amd", "libmsiren.so")
LDS_PER_CU = 160 * 1024


def jet_lds_bytes(HP):  # siren_trunk_f32_jet.hip.h: X image [HP/4][96] float4 + layer-0 rows [HP] float4, dynamic
    return HP * 384 + HP * 16


def kernel_metadata(tmp_path):
    """{kernel name: {field: int}} of every gfx950 code object bundled into the library"""
    blob = open(LIB, "rb").read()
    out, at, nobj = {}, blob.find(b"__CLANG_OFFLOAD_BUNDLE__"), 0
    while at >= 0:
        (n,), pos = struct.unpack_from("<Q", blob, at + 24), at + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + tl].decode()
            pos += 24 + tl
            if "gfx950" in triple and size:
                co = tmp_path / f"co{nobj}.elf"
                co.write_bytes(blob[at + off:at + off + size])
                nobj += 1
                res = subprocess.run([READELF, "--notes", str(co)], capture_output=True, text=True, timeout=300)
                assert res.returncode == 0, res.stderr[-2000:]
                for entry in re.split(r"\n\s+- \.agpr_count:", res.stdout)[1:]:
                    entry = ".agpr_count:" + entry
                    name = re.search(r"\.name:\s+(\S+)", entry).group(1)
                    out[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, flags=re.M)}
        at = blob.find(b"__CLANG_OFFLOAD_BUNDLE__", at + 24)
    return out


def test_jet_instances_have_no_scratch_and_fit_one_workgroup_per_cu(tmp_path):
    if not (os.path.exists(READELF) and os.path.exists(LIB)):
        pytest.skip("needs the built library and llvm-readelf")
    meta = kernel_metadata(tmp_path)
    jets = {k: v for k, v in meta.items() if "siren_trunk_f32_jet_kernel" in k}
    want = {f"_ZN6msiren26siren_trunk_f32_jet_kernelILi{hp}ELi{act}EEEvNS_14TrunkJetParamsE": hp for hp in (128, 256) for act in (0, 1)}
    assert set(jets) == set(want), sorted(jets)
    for name, m in jets.items():
        hp = want[name]
        print(name, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64, (name, m)
        # one workgroup of 4 waves per CU = one wave per SIMD: the whole unified file of 512 registers per lane, the CU's 160 KB of LDS
        assert m["vgpr_count"] <= 512, (name, m)
        assert m["group_segment_fixed_size"] + jet_lds_bytes(hp) <= LDS_PER_CU, (name, m)
    assert jet_lds_bytes(256) > 64 * 1024  # (H = 256 needs the opt-in dynamic-LDS limit: launch_dispatch.hip raises it)
