"""Build-time guard for the kernels of the shadow-mask accumulation (csrc/shadow_mask_accumulate.hip), in the style of
test_kernel_resources_shadow_mask_filter.py.

k_shadow_mask_accumulate must build for gfx950 without scratch, without spills and without LDS (hard conditions: the gather is one
texel per image, nothing is shared between lanes).  The first build reports 38 VGPRs for it (a lane walks its four pixels one after
the other; only the four count bytes live across them) and 12 for k_selftest_accum_division; the caps are those values rounded up
to the allocation step of 8: 40 and 16.  512 / 40 = 12 waves fit a SIMD's registers, so both leave 8 waves per SIMD, the most the
hardware keeps resident: the pass is bound by memory, and occupancy is what hides its gather."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (max VGPRs, max LDS bytes per block, min resident waves per SIMD by registers)
NEW = {
    "k_shadow_mask_accumulate": (40, 0, 8),
    "k_selftest_accum_division": (16, 0, 8),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["shadow_mask_accumulate.hip"])


def _waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))  # per SIMD, by registers


def test_every_kernel_is_listed(res):
    assert sorted(res) == sorted(NEW)
    assert all(res[k]["file"] == "shadow_mask_accumulate.hip" for k in NEW)


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_new_kernel_resources(res, kernel):
    max_vgprs, max_lds, min_waves = NEW[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    assert _waves(r["vgprs"]) >= min_waves, f"{kernel}: {_waves(r['vgprs'])} waves per SIMD < {min_waves}"
