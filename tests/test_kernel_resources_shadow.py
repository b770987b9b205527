"""Build-time guard for the shadow-map pass (csrc/shadow.hip), in the style of test_kernel_resources_cubemap.py: every kernel
builds for gfx950 without scratch and without spills (the near-plane clip keeps its polygon in registers), and the register
counts keep the occupancy DESIGN.md section 7.2 records.  The build reports 44 VGPRs for k_shadow_setup and 56 / 58 for the two
coverage kernels (k_raster_small / k_raster_large need 96 / 96 around the same walk_blocks() of raster_common.hpp: no record
beyond positions and depth, no alpha test), 6 for the clear and 10 for the draw table (the shared upload kernel
k_store_table of raster_common.hpp, 32 draws per launch); the caps are the values of the first build of each kernel rounded
up to the allocation step of 8, so all five run at 8 waves per SIMD."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (threads per block, max VGPRs, max LDS bytes per block, min resident waves per SIMD)
SHADOW = {
    "k_store_table<ShadowDraw, 32>": (64, 16, 0, 8),
    "k_shadow_clear": (256, 8, 0, 8),
    "k_shadow_setup": (256, 48, 0, 8),
    "k_shadow_small": (256, 64, 0, 8),
    "k_shadow_large": (256, 64, 0, 8),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["shadow.hip"])


def test_every_shadow_kernel_is_listed(res):
    assert sorted(k for k in res if k.startswith(("k_shadow_", "k_store_table"))) == sorted(SHADOW)


@pytest.mark.parametrize("kernel", sorted(SHADOW))
def test_shadow_kernel_resources(res, kernel):
    threads, max_vgprs, max_lds, min_waves = SHADOW[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    alloc = max(8, (r["vgprs"] + 7) // 8 * 8)
    waves = min(8, 512 // alloc)  # per SIMD, by registers
    assert waves >= min_waves, f"{kernel}: {waves} waves per SIMD < {min_waves}"
