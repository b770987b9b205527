"""Build-time guard for the image transfers (csrc/transfer.hip), in the style of test_kernel_resources_shadow.py: every kernel
builds for gfx950 without scratch and without spills, the fused mip kernel keeps its tile in the LDS DESIGN.md section 7.3
records, and registers and LDS leave 8 waves per SIMD.  The build reports 10-19 VGPRs for k_mips_level<*>, 15-24 for
k_mips_fused<*>, 16 / 38 for the NEAREST / LINEAR blit and 12 for the clear; LDS per block of the fused kernel: 5456 B for
the 4-byte-and-smaller texels (1364 stored texels of 4 bytes), 7504 B with the two sRGB tables, 10912 B for RGBA16_SFLOAT.  The
caps are those values rounded up (registers to the allocation step of 8, LDS to 512 B).  The template argument is the
vkr_format value: 3 RG16_SFLOAT, 4 RGBA8_SRGB, 5 RGBA8_UNORM, 7 RGBA16_SFLOAT, 8 R16_SFLOAT, 9 R32_SFLOAT, 10 R8_UNORM."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

LDS_PER_CU = 160 * 1024
MIP_FORMATS = (3, 4, 5, 7, 8, 9, 10)

# kernel: (threads per block, max VGPRs, max LDS bytes per block, min resident waves per SIMD)
TRANSFER = {
    "k_transfer_clear": (256, 16, 1536, 8),
    "k_transfer_blit<false>": (256, 16, 2048, 8),
    "k_transfer_blit<true>": (256, 40, 2048, 8),
}
for _f in MIP_FORMATS:
    TRANSFER[f"k_mips_level<{_f}>"] = (256, 24, 2048 if _f == 4 else 0, 8)
    TRANSFER[f"k_mips_fused<{_f}>"] = (256, 24, 7680 if _f == 4 else 11264 if _f == 7 else 5632, 8)


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["transfer.hip"])


def test_every_transfer_kernel_is_listed(res):
    assert sorted(k for k in res if k.startswith(("k_transfer_", "k_mips_"))) == sorted(TRANSFER)


@pytest.mark.parametrize("kernel", sorted(TRANSFER))
def test_transfer_kernel_resources(res, kernel):
    threads, max_vgprs, max_lds, min_waves = TRANSFER[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    # whole blocks only: by registers (512 VGPRs per SIMD lane, steps of 8), by LDS (160 KiB per CU), by wave slots
    waves_per_block = threads // 64
    alloc = max(8, (r["vgprs"] + 7) // 8 * 8)
    by_regs = min(8, 512 // alloc) * 4 // waves_per_block
    by_lds = LDS_PER_CU // r["lds_bytes"] if r["lds_bytes"] else 10 ** 9
    waves = min(by_regs, by_lds, 8 * 4 // waves_per_block) * waves_per_block / 4
    assert waves >= min_waves, f"{kernel}: {waves} waves per SIMD < {min_waves}"
