"""Build-time guard for the SSAO pass (csrc/ssao.hip), in the style of test_kernel_resources_shadow.py: both instances of the
kernel build for gfx950 without scratch, without spills and without LDS, and the register counts keep the occupancy DESIGN.md
section 7.4 records.  The first build reports 51 VGPRs for k_ssao<true> (each footprint row one 8-byte load) and 48 for
k_ssao<false> (depth images one texel wide); the caps are those values rounded up to the allocation step of 8, 56 and 48, so
both run at 8 waves per SIMD."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (threads per block, max VGPRs, max LDS bytes per block, min resident waves per SIMD)
SSAO = {
    "k_ssao<true>": (256, 56, 0, 8),
    "k_ssao<false>": (256, 48, 0, 8),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["ssao.hip"])


def test_every_ssao_kernel_is_listed(res):
    assert sorted(k for k in res if k.startswith("k_ssao")) == sorted(SSAO)


@pytest.mark.parametrize("kernel", sorted(SSAO))
def test_ssao_kernel_resources(res, kernel):
    threads, max_vgprs, max_lds, min_waves = SSAO[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    alloc = max(8, (r["vgprs"] + 7) // 8 * 8)
    waves = min(8, 512 // alloc)  # per SIMD, by registers
    assert waves >= min_waves, f"{kernel}: {waves} waves per SIMD < {min_waves}"
