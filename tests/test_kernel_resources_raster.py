"""Build-time guard for the G-buffer rasteriser (csrc/raster.hip), in the style of test_kernel_resources_shadow.py: the scratch
and the LDS of every kernel are exactly those of the build before the coverage stage moved into raster_common.hpp
(k_raster_setup keeps its own clip walk with its indexed polygon: 384 B of scratch per lane and 13312 B of LDS; nothing else
has any scratch), nothing spills, and the register counts do not rise above that build's: 4 (clear), 10 / 68 (the draw and the
texture table through k_store_table, 8 draws and 4 textures per launch), 132 (setup), 106 / 107 (small / large) and 76
(resolve), each rounded up to the allocation step of 8.  The build after the move reports 96 / 96 for small / large."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (threads per block, max VGPRs, scratch bytes per lane, LDS bytes per block, min resident waves per SIMD)
RASTER = {
    "k_store_table<DrawDev, 8>": (64, 16, 0, 0, 8),
    "k_store_table<Pyramid, 4>": (64, 72, 0, 0, 7),
    "k_raster_clear": (256, 8, 0, 0, 8),
    "k_raster_setup": (256, 136, 384, 13312, 3),
    "k_raster_small": (256, 112, 0, 0, 4),
    "k_raster_large": (256, 112, 0, 0, 4),
    "k_raster_resolve": (256, 80, 0, 2048, 6),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["raster.hip"])


def test_every_raster_kernel_is_listed(res):
    assert sorted(k for k in res if k.startswith(("k_raster_", "k_store_table"))) == sorted(RASTER)


@pytest.mark.parametrize("kernel", sorted(RASTER))
def test_raster_kernel_resources(res, kernel):
    threads, max_vgprs, scratch, lds, min_waves = RASTER[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == scratch, f"{kernel}: {r['scratch_bytes']} B of scratch per lane, {scratch} before"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] == lds, f"{kernel}: {r['lds_bytes']} B LDS, {lds} before"
    alloc = max(8, (r["vgprs"] + 7) // 8 * 8)
    waves = min(8, 512 // alloc)  # per SIMD, by registers
    assert waves >= min_waves, f"{kernel}: {waves} waves per SIMD < {min_waves}"
    assert r["occupancy"] >= min_waves, f"{kernel}: the compiler reports {r['occupancy']} waves per SIMD < {min_waves}"
