"""Build-time guard for the ray-query kernels after the traversal moved into csrc/accel_traverse.hpp, in the style of
test_kernel_resources_shadow_mask.py.

k_accel_query and k_gtao_rt only had their helpers moved to a header: they must build for gfx950 to exactly the figures of the
tree before the move, 44 VGPRs / 62 SGPRs and 62 VGPRs / 53 SGPRs, 1024 B of LDS (four 64-word stacks), no scratch, no spills.

The new kernels, k_accel_occluded (accel.hip) and k_shadow_mask_rt (shadow_mask_rt.hip), walk with the per-ray cull: no scratch,
no spills, at most the 1024 B of LDS of the four stacks, and register counts that keep 8 waves per SIMD (DESIGN.md section 7.8:
latency is hidden by resident waves).  The first build reports 52 and 58 VGPRs; the caps are those values rounded up to the
allocation step of 8: 56 and 64."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (VGPRs, SGPRs, LDS bytes) of the tree before the traversal became a header
MOVED = {
    "k_accel_query": (44, 62, 1024),
    "k_gtao_rt": (62, 53, 1024),
}
# kernel: (max VGPRs, max LDS bytes per block, min resident waves per SIMD by registers)
NEW = {
    "k_accel_occluded": (56, 1024, 8),
    "k_shadow_mask_rt": (64, 1024, 8),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["accel.hip", "shadow_mask_rt.hip"])


def _waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))  # per SIMD, by registers


def test_every_kernel_is_listed(res):
    assert sorted(res) == sorted(list(MOVED) + list(NEW))
    assert res["k_shadow_mask_rt"]["file"] == "shadow_mask_rt.hip" and res["k_accel_occluded"]["file"] == "accel.hip"


@pytest.mark.parametrize("kernel", sorted(MOVED))
def test_moved_kernels_build_to_what_they_built_to(res, kernel):
    vgprs, sgprs, lds = MOVED[kernel]
    r = res[kernel]
    assert (r["vgprs"], r["sgprs"], r["lds_bytes"], r["scratch_bytes"], r["vgpr_spill"], r["sgpr_spill"]) == (vgprs, sgprs, lds, 0, 0, 0), r


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_new_kernel_resources(res, kernel):
    max_vgprs, max_lds, min_waves = NEW[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert max_vgprs <= 64
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    assert _waves(r["vgprs"]) >= min_waves, f"{kernel}: {_waves(r['vgprs'])} waves per SIMD < {min_waves}"
