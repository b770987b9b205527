"""Build-time guard for the shadow mask (csrc/shadow_mask.hip) and the shading kernel it made a template over a second bool
(csrc/shading.hip), in the style of test_kernel_resources_ssao.py: every instance of k_shadow_mask builds for gfx950 without
scratch, without spills and without LDS, and the register counts keep the occupancy DESIGN.md section 7.7 records.  The first
build reports 20 / 32 / 56 VGPRs for k_shadow_mask<0> / <1> / <2> (1, 9, 25 taps: the loads of a row are in flight together);
the caps are those values rounded up to the allocation step of 8: 24, 32 and 56, all at 8 waves per SIMD.

The <*, false> instances of k_defered_shading are the kernels of program "defered_shading".  Before the second template
parameter they built to 62 VGPRs / 82 SGPRs (<true>) and 69 / 74 (<false>), 2048 B of LDS, no scratch; they must build to exactly
that still.  The shadowed instances (62 / 82 and 68 / 76 in the first build) get the same caps."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (max VGPRs, max LDS bytes per block, min resident waves per SIMD by registers)
MASK = {
    "k_shadow_mask<0>": (24, 0, 8),
    "k_shadow_mask<1>": (32, 0, 8),
    "k_shadow_mask<2>": (56, 0, 8),
}
# kernel: (VGPRs, SGPRs, LDS bytes) of the tree before the template parameter
PLAIN_SHADING = {
    "k_defered_shading<true, false>": (62, 82, 2048),
    "k_defered_shading<false, false>": (69, 74, 2048),
}
SHADOWED_SHADING = {
    "k_defered_shading<true, true>": (64, 2048, 8),
    "k_defered_shading<false, true>": (72, 2048, 7),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["shadow_mask.hip", "shading.hip"])


def _waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))  # per SIMD, by registers


def test_every_kernel_is_listed(res):
    assert sorted(k for k in res if k.startswith("k_shadow_mask")) == sorted(MASK)
    assert sorted(k for k in res if k.startswith("k_defered_shading")) == sorted(list(PLAIN_SHADING) + list(SHADOWED_SHADING))


@pytest.mark.parametrize("kernel", sorted(list(MASK) + list(SHADOWED_SHADING)))
def test_new_kernel_resources(res, kernel):
    max_vgprs, max_lds, min_waves = {**MASK, **SHADOWED_SHADING}[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    assert _waves(r["vgprs"]) >= min_waves, f"{kernel}: {_waves(r['vgprs'])} waves per SIMD < {min_waves}"


@pytest.mark.parametrize("kernel", sorted(PLAIN_SHADING))
def test_plain_shading_builds_to_what_it_built_to(res, kernel):
    vgprs, sgprs, lds = PLAIN_SHADING[kernel]
    r = res[kernel]
    assert (r["vgprs"], r["sgprs"], r["lds_bytes"], r["scratch_bytes"], r["vgpr_spill"], r["sgpr_spill"]) == (vgprs, sgprs, lds, 0, 0, 0), r
