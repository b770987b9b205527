"""Build-time guard for the kernels of the traced shadow mask with area lights (csrc/shadow_mask_rt_soft.hip), in the style of
test_kernel_resources_shadow_mask_rt.py.

k_shadow_mask_rt_soft and k_shadow_mask_rt_soft_cutout must build for gfx950 without scratch and without spills (hard conditions)
and with at most the 1024 B of LDS of the four stacks (the sample table is not staged).  The first build reports 80 VGPRs for both
(the hard pass's 58 plus dvec, the frame across the light and the table pointer, which stay live across a walk; the build with the
light-volume cull reports 80 too); the cap is that value, a multiple of the allocation step of 8 already.  80 registers leave 6 waves per SIMD, not the 8 of the hard pass (DESIGN.md
section 7.12 says so; what the two waves cost has not been measured on their own).  k_shadow_mask_rt and k_shadow_mask_rt_cutout
are pinned to what they were by test_kernel_resources_shadow_mask_rt.py and test_kernel_resources_ray_cutout.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (max VGPRs, max LDS bytes per block, min resident waves per SIMD by registers)
NEW = {
    "k_shadow_mask_rt_soft": (80, 1024, 6),
    "k_shadow_mask_rt_soft_cutout": (80, 1024, 6),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["shadow_mask_rt_soft.hip"])


def _waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))  # per SIMD, by registers


def test_every_kernel_is_listed(res):
    # the texture table's upload kernel comes with ray_cutout.hpp, as in accel_cutout.hip
    assert sorted(k for k in res if not k.startswith("k_store_table")) == sorted(NEW)
    assert all(res[k]["file"] == "shadow_mask_rt_soft.hip" for k in NEW)


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
