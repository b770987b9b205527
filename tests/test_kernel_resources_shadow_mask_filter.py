"""Build-time guard for the kernels of the shadow-mask filter (csrc/shadow_mask_filter.hip), in the style of
test_kernel_resources_shadow_mask_rt_soft.py.

The four instances of k_shadow_mask_filter (reach 1..4) must build for gfx950 without scratch and without spills (hard conditions)
and with at most 16 KiB of LDS per block: the window of reach 4 is 22 x 22 texels of a mask word and a 28-byte guide record,
15488 B (the build reports 15744 with the word of the block-wide vote), and ten such blocks still fit the 160 KiB of a CU, so LDS
never limits occupancy.  The first build reports 3 / 28 / 28 / 31 VGPRs for reach 1 / 2 / 3 / 4 (the rows of taps are a loop, each row
unrolled; with the whole window unrolled reach 4 held 110); the caps are those values rounded up to the allocation step of 8: 8 and
32, which leave 8 waves per SIMD, the most the hardware keeps resident."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

LDS_CAP = 16 * 1024
# kernel: (max VGPRs, max LDS bytes per block, min resident waves per SIMD by registers)
NEW = {
    "k_shadow_mask_filter<1>": (8, 0, 8),
    "k_shadow_mask_filter<2>": (32, LDS_CAP, 8),
    "k_shadow_mask_filter<3>": (32, LDS_CAP, 8),
    "k_shadow_mask_filter<4>": (32, LDS_CAP, 8),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["shadow_mask_filter.hip"])


def _waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))  # per SIMD, by registers


def test_every_kernel_is_listed(res):
    assert sorted(res) == sorted(NEW)
    assert all(res[k]["file"] == "shadow_mask_filter.hip" for k in NEW)


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
    assert 10 * max(r["lds_bytes"], 1) <= 160 * 1024, "ten blocks no longer fit a CU's LDS"
