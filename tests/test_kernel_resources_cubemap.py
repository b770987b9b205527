"""Build-time guard for the cube-face bake (csrc/cubemap.hip), in the style of test_kernel_resources_probe.py: every kernel
builds for gfx950 without scratch and without spills (the near-plane clip picks its polygon slots with selects, not with an
indexed store), and the register counts keep the occupancy DESIGN.md records.  The build reports 84 VGPRs for k_cubemap_setup,
95 / 96 for the two coverage kernels (k_raster_small / k_raster_large: 96 / 96, 5 waves per SIMD; the caps still stand at the
4 waves of the first build) and 57 for the resolve; the two tables go through the shared upload kernel k_store_table of
raster_common.hpp (8 draws, 4 textures per launch); the caps leave the headroom of one allocation step."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (threads per block, max VGPRs, max LDS bytes per block, min resident waves per SIMD)
CUBEMAP = {
    "k_cubemap_clear": (256, 16, 0, 8),
    "k_store_table<CubeDraw, 8>": (64, 72, 0, 7),
    "k_store_table<Pyramid, 4>": (64, 72, 0, 7),
    "k_cubemap_setup": (256, 96, 0, 5),
    "k_cubemap_small": (256, 112, 0, 4),
    "k_cubemap_large": (256, 112, 0, 4),
    "k_cubemap_resolve": (256, 72, 2048, 7),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["cubemap.hip"])


def test_every_cubemap_kernel_is_listed(res):
    assert sorted(k for k in res if k.startswith(("k_cubemap_", "k_store_table"))) == sorted(CUBEMAP)


@pytest.mark.parametrize("kernel", sorted(CUBEMAP))
def test_cubemap_kernel_resources(res, kernel):
    threads, max_vgprs, max_lds, min_waves = CUBEMAP[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    alloc = max(8, (r["vgprs"] + 7) // 8 * 8)
    waves = min(8, 512 // alloc)  # per SIMD, by registers; the LDS of the resolve (2 KiB of 160 KiB) does not bind
    assert waves >= min_waves, f"{kernel}: {waves} waves per SIMD < {min_waves}"
