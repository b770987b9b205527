"""Build-time guard for the refit of the ray-query structure (csrc/accel_refit.hip), in the style of
test_kernel_resources_ray_cutout.py: every kernel of the file is listed, none uses scratch or spills (hard conditions: the record
and the box under construction live in registers), none uses LDS (no byte is shared between lanes: visibility between levels comes
from kernel boundaries and, in the tail, from __syncthreads() over global memory), and the register counts keep 8 waves per SIMD.
The first build reports 28, 20, 26 and 30 VGPRs; the caps are those values rounded up to the allocation step of 8.

The kernels the refit must not touch — the walks of accel.hip and accel_closest.hip, which include the same headers — are held to
their registers and instruction counts by test_kernel_resources_ray_cutout.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (max VGPRs, min resident waves per SIMD by registers)
NEW = {
    "k_accel_refit_records": (32, 8),  # first build: 28 VGPRs
    "k_accel_refit_level": (24, 8),    # first build: 20 VGPRs
    "k_accel_refit_tail": (32, 8),     # first build: 26 VGPRs
    "k_scene_triangles": (32, 8),      # first build: 30 VGPRs
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["accel_refit.hip"])


def _waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))  # per SIMD, by registers


def test_every_kernel_of_the_file_is_listed(res):
    mine = sorted(k for k, v in res.items() if v["file"] == "accel_refit.hip")
    assert sorted(k for k in mine if "k_store_table" not in k) == sorted(NEW), mine


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_kernel_resources(res, kernel):
    max_vgprs, min_waves = NEW[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    print(f"[accel refit] {kernel}: {r['vgprs']} VGPRs, {r['sgprs']} SGPRs, {r['lds_bytes']} B LDS, scratch {r['scratch_bytes']}")
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert r["lds_bytes"] == 0, f"{kernel}: {r['lds_bytes']} B of LDS"
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert _waves(r["vgprs"]) >= min_waves
