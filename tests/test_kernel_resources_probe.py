"""Build-time guard for the octahedral probe kernels (csrc/probe.hip), in the style of test_kernel_resources_rt.py: nothing may
go to scratch (the trace's segment bounds are picked with constant indices), and the register count of the divergent,
latency-bound trace keeps at least 4 waves per SIMD (it builds to 71 VGPRs: 7 waves)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (threads per block, max VGPRs, max LDS bytes per block, min resident waves per SIMD)
PROBE = {
    "k_cube2oct": (64, 64, 0, 8),
    "k_probe_downsample": (64, 32, 0, 8),
    "k_trace_probe": (64, 80, 512, 4),
}


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(["probe.hip"])


@pytest.mark.parametrize("kernel", sorted(PROBE))
def test_probe_kernel_resources(res, kernel):
    threads, max_vgprs, max_lds, min_waves = PROBE[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    waves_per_block = threads // 64
    alloc = max(8, (r["vgprs"] + 7) // 8 * 8)
    by_regs = min(8, 512 // alloc) * 4 // waves_per_block
    by_lds = 160 * 1024 // r["lds_bytes"] if r["lds_bytes"] else 10 ** 9
    waves = min(by_regs, by_lds, 8 * 4 // waves_per_block) * waves_per_block / 4
    assert waves >= min_waves
