"""Build-time guard for the backbuffer texdraw pass (csrc/texdraw.hip), in the style of test_kernel_resources_ssao.py: the kernel
builds for gfx950 without scratch and without spills (the four raw taps of a footprint are indexed statically: a scratch array
would mean that has changed), its only LDS is the two sRGB tables (2 x 1 KiB), and the register count keeps the occupancy
DESIGN.md section 7.6 records.  The first build reported 40 VGPRs for k_texdraw; the cap is that value rounded up to the
allocation step of 8, 40, which leaves 8 waves per SIMD.  The encode's self-test kernel is held to no scratch and no spills."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (threads per block, max VGPRs, max LDS bytes per block, min resident waves per SIMD)
TEXDRAW = {
    "k_texdraw": (256, 40, 2048, 8),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["texdraw.hip"])


def test_every_texdraw_kernel_is_listed(res):
    assert sorted(k for k in res if k.startswith("k_texdraw")) == sorted(TEXDRAW)
    assert sorted(res) == sorted(list(TEXDRAW) + ["k_selftest_srgb_encode"])


@pytest.mark.parametrize("kernel", sorted(TEXDRAW))
def test_texdraw_kernel_resources(res, kernel):
    threads, max_vgprs, max_lds, min_waves = TEXDRAW[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    alloc = max(8, (r["vgprs"] + 7) // 8 * 8)
    waves = min(8, 512 // alloc)  # per SIMD, by registers
    assert waves >= min_waves, f"{kernel}: {waves} waves per SIMD < {min_waves}"
    assert 65536 // max(1, r["lds_bytes"]) * (threads // 64) >= 4 * min_waves  # ... and by LDS: 32 blocks of 4 waves per CU


def test_selftest_kernel_has_no_scratch(res):
    r = res["k_selftest_srgb_encode"]
    assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
