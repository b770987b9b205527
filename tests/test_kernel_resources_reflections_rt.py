"""Build-time guard for the closest-hit kernels, in the style of test_kernel_resources_shadow_mask_rt.py.

k_accel_closest (accel_closest.hip) and k_reflections_rt (reflections_rt.hip) walk with wave_closest_hit: no scratch and no spills
(hard conditions: the stack is in LDS, nothing may go to private memory), at most the 1024 B of LDS of the four stacks, plus the
1 KiB sRGB table for the pass, and register counts that keep 8 waves per SIMD (latency is hidden by resident
waves).  The first build reports 60 and 62 VGPRs; the caps are those values rounded up to the allocation step of 8: 64 and 64.
The only other kernel of the two files is the shared host preamble's k_store_table (raster_common.hpp), which copies the texture
table into scratch: one block of 64 lanes, not a hot path."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (file, max VGPRs, max LDS bytes per block, min resident waves per SIMD by registers)
NEW = {
    "k_accel_closest": ("accel_closest.hip", 64, 1024, 8),     # first build: 60 VGPRs
    "k_reflections_rt": ("reflections_rt.hip", 64, 2048, 8),   # first build: 62 VGPRs
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["accel_closest.hip", "reflections_rt.hip"])


def _waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))  # per SIMD, by registers


def test_every_kernel_is_listed(res):
    others = sorted(k for k in res if k not in NEW)
    assert sorted(k for k in res if k in NEW) == sorted(NEW), sorted(res)
    assert all("k_store_table" in k and res[k]["file"] == "reflections_rt.hip" for k in others), others
    for kernel, (file, _, _, _) in NEW.items():
        assert res[kernel]["file"] == file


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_new_kernel_resources(res, kernel):
    _, max_vgprs, max_lds, min_waves = NEW[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert max_vgprs <= 64
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    assert _waves(r["vgprs"]) >= min_waves, f"{kernel}: {_waves(r['vgprs'])} waves per SIMD < {min_waves}"
