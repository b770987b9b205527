"""Build-time guard for the lit ray-traced reflections, in the style of test_kernel_resources_reflections_rt.py.

k_reflections_rt_lit and k_reflections_rt_lit_cutout (reflections_rt_lit.hip) walk twice per wave, the closest hit and then one
any-hit walk per light: no scratch and no spills (hard conditions: the stack is in LDS, nothing may go to private memory), the LDS
of k_reflections_rt (the four stacks and the 1 KiB sRGB table: 2048 B), and register counts that keep 8 waves per SIMD (DESIGN.md
section 7.15).  The first build reports 64 and 60 VGPRs; the caps are those values rounded up to the next occupancy step: 64 and 64.
k_scene_triangle_normals (scene_normals.hip) is a streaming kernel without LDS.

The kernels that existed before share headers with the new ones (reflections_rt.hpp, ray_cutout.hpp, accel_traverse.hpp,
scene_triangles.hpp) and must be the code they were: k_reflections_rt, k_reflections_rt_cutout, k_shadow_mask_rt and
k_scene_triangles report the VGPR / SGPR / LDS figures of a build of the commit before this pass existed (tools/kernel_resources.py
there: 62 / 68 / 2048, 58 / 76 / 2048, 58 / 82 / 1024 and 30 / 19 / 0)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (file, max VGPRs, LDS bytes per block, min resident waves per SIMD by registers)
NEW = {
    "k_reflections_rt_lit": ("reflections_rt_lit.hip", 64, 2048, 8),          # first build: 64 VGPRs
    "k_reflections_rt_lit_cutout": ("reflections_rt_lit.hip", 64, 2048, 8),   # first build: 60 VGPRs
    "k_scene_triangle_normals": ("scene_normals.hip", 32, 0, 8),              # first build: 25 VGPRs
}
# kernel: (file, VGPRs, SGPRs, LDS bytes) on the parent commit
BEFORE = {
    "k_reflections_rt": ("reflections_rt.hip", 62, 68, 2048),
    "k_reflections_rt_cutout": ("accel_cutout.hip", 58, 76, 2048),
    "k_shadow_mask_rt": ("shadow_mask_rt.hip", 58, 82, 1024),
    "k_scene_triangles": ("accel_refit.hip", 30, 19, 0),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(sorted({v[0] for v in NEW.values()} | {v[0] for v in BEFORE.values()}))


def _waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))  # per SIMD, by registers


def test_every_kernel_of_the_new_files_is_listed(res):
    mine = sorted(k for k, v in res.items() if v["file"] in ("reflections_rt_lit.hip", "scene_normals.hip"))
    assert sorted(k for k in mine if "k_store_table" not in k) == sorted(NEW), mine
    for kernel, (file, _, _, _) in NEW.items():
        assert res[kernel]["file"] == file


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_new_kernel_resources(res, kernel):
    _, max_vgprs, lds, min_waves = NEW[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    print(f"[reflections rt lit] {kernel}: {r['vgprs']} VGPRs, {r['sgprs']} SGPRs, {r['lds_bytes']} B LDS, scratch {r['scratch_bytes']}")
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert max_vgprs <= 64
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] == lds, f"{kernel}: {r['lds_bytes']} B LDS, {lds} expected"
    assert _waves(r["vgprs"]) >= min_waves, f"{kernel}: {_waves(r['vgprs'])} waves per SIMD < {min_waves}"


def test_the_lit_kernels_have_the_lds_of_the_unlit_pass(res):
    for kernel in ("k_reflections_rt_lit", "k_reflections_rt_lit_cutout"):
        assert res[kernel]["lds_bytes"] == res["k_reflections_rt"]["lds_bytes"]


@pytest.mark.parametrize("kernel", sorted(BEFORE))
def test_the_kernels_that_existed_are_what_they_were(res, kernel):
    file, vgprs, sgprs, lds = BEFORE[kernel]
    r = res[kernel]
    assert r["file"] == file
    assert (r["vgprs"], r["sgprs"], r["lds_bytes"]) == (vgprs, sgprs, lds), (kernel, r)
    assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
