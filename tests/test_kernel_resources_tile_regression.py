"""Build-time guard for the tile plane regression (csrc/tile_regression.hip), in the style of test_kernel_resources_ssao.py: the
kernel builds for gfx950 without scratch, without spills and without LDS (the reductions are cross-lane: a shared-memory
staging area would mean the design has changed), and the register count keeps the occupancy DESIGN.md section 7.5 records.
The first build (sums through __shfl_xor) reported 32 VGPRs for k_tile_regression; the cap is that value rounded up to the
allocation step of 8, 32, so the kernel runs at 8 waves per SIMD.  The build with DPP / permlane sums reports 26."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (threads per block, max VGPRs, max LDS bytes per block, min resident waves per SIMD)
TILE_REGRESSION = {
    "k_tile_regression": (256, 32, 0, 8),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["tile_regression.hip"])


def test_every_tile_regression_kernel_is_listed(res):
    assert sorted(k for k in res if k.startswith("k_tile_regression")) == sorted(TILE_REGRESSION)


@pytest.mark.parametrize("kernel", sorted(TILE_REGRESSION))
def test_tile_regression_kernel_resources(res, kernel):
    threads, max_vgprs, max_lds, min_waves = TILE_REGRESSION[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    alloc = max(8, (r["vgprs"] + 7) // 8 * 8)
    waves = min(8, 512 // alloc)  # per SIMD, by registers
    assert waves >= min_waves, f"{kernel}: {waves} waves per SIMD < {min_waves}"
