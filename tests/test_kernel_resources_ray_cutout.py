"""Build-time guard for the kernels of alpha cutouts in the ray query, in the style of test_kernel_resources_reflections_rt.py.

The four kernels of accel_cutout.hip walk with the cutout filter of ray_cutout.hpp: no scratch and no spills (hard conditions: the
stack is in LDS, nothing may go to private memory), the 1024 B of LDS of the four stacks (plus the 1 KiB sRGB table for the
reflections pass, which shades what lies behind a hole), and register counts that keep 8 waves per SIMD.  The first build reports
48, 56, 56 and 58 VGPRs; the caps are those values rounded up to the allocation step of 8.

The default filter must cost nothing: the six kernels that existed before keep the registers, LDS and instruction counts of the
table in DESIGN.md 7.9, "The fold" (348 / 1366 / 455 / 808 / 415 / 1137 instructions, counted as the lines of the kernel's body in
the compiler's assembly that are neither labels, directives nor comments)."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402

# kernel: (max VGPRs, max LDS bytes per block, min resident waves per SIMD by registers)
NEW = {
    "k_accel_occluded_cutout": (48, 1024, 8),   # first build: 48 VGPRs
    "k_accel_closest_cutout": (56, 1024, 8),    # first build: 56 VGPRs
    "k_shadow_mask_rt_cutout": (56, 1024, 8),   # first build: 56 VGPRs
    "k_reflections_rt_cutout": (64, 2048, 8),   # first build: 58 VGPRs
}
# kernel: (file, VGPRs, SGPRs, LDS bytes, instructions) of DESIGN.md 7.9, "The fold"
FOLD = {
    "k_accel_query": ("accel.hip", 44, 62, 1024, 348),
    "k_gtao_rt": ("accel.hip", 62, 53, 1024, 1366),
    "k_accel_occluded": ("accel.hip", 52, 74, 1024, 455),
    "k_shadow_mask_rt": ("shadow_mask_rt.hip", 58, 82, 1024, 808),
    "k_accel_closest": ("accel_closest.hip", 60, 58, 1024, 415),
    "k_reflections_rt": ("reflections_rt.hip", 62, 68, 2048, 1137),
}
FILES = ["accel.hip", "accel_closest.hip", "shadow_mask_rt.hip", "reflections_rt.hip", "accel_cutout.hip"]


@pytest.fixture(scope="module")
def res():
    return kernel_resources.resources(FILES)


def instruction_counts(files):
    """{kernel (short name): instructions of its body} from the compiler's assembly, with the flags of tools/kernel_resources.py"""
    flags = [f for f in kernel_resources.FLAGS if not f.startswith("-Rpass")]
    counts = {}
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for f in files:
            out = os.path.join(tmp, f + ".s")
            procs.append((out, subprocess.Popen([kernel_resources.HIPCC] + flags + ["-o", out, os.path.join(kernel_resources.CSRC, f)],
                                                stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        for out, p in procs:
            log, _ = p.communicate()
            assert p.returncode == 0, log[-3000:]
            name, n = None, 0
            for line in open(out):
                m = re.match(r"^(_Z\w+):", line)
                if m:
                    name, n = m.group(1), 0
                    continue
                s = line.strip()
                if name is None:
                    continue
                if s.startswith(".Lfunc_end"):
                    counts[name] = n
                    name = None
                elif s and not s.startswith((".", ";", "//")) and not s.endswith(":"):
                    n += 1
    names = list(counts)
    return {kernel_resources.short(d): counts[m] for m, d in zip(names, kernel_resources.demangle(names))}


def _waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))  # per SIMD, by registers


def test_every_kernel_of_the_new_file_is_listed(res):
    mine = sorted(k for k, v in res.items() if v["file"] == "accel_cutout.hip")
    assert sorted(k for k in mine if "k_store_table" not in k) == sorted(NEW), mine


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_new_kernel_resources(res, kernel):
    max_vgprs, max_lds, min_waves = NEW[kernel]
    assert kernel in res, f"{kernel} not reported (renamed?)"
    r = res[kernel]
    print(f"[ray cutout] {kernel}: {r['vgprs']} VGPRs, {r['sgprs']} SGPRs, {r['lds_bytes']} B LDS, scratch {r['scratch_bytes']}")
    assert r["file"] == "accel_cutout.hip"
    assert r["scratch_bytes"] == 0, f"{kernel}: {r['scratch_bytes']} B of scratch per lane"
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert max_vgprs <= 64
    assert r["vgprs"] <= max_vgprs, f"{kernel}: {r['vgprs']} VGPRs > {max_vgprs}"
    assert r["lds_bytes"] <= max_lds, f"{kernel}: {r['lds_bytes']} B LDS > {max_lds}"
    assert _waves(r["vgprs"]) >= min_waves, f"{kernel}: {_waves(r['vgprs'])} waves per SIMD < {min_waves}"


@pytest.fixture(scope="module")
def instructions():
    return instruction_counts(sorted({v[0] for v in FOLD.values()}))


@pytest.mark.parametrize("kernel", sorted(FOLD))
def test_the_default_filter_costs_nothing(res, instructions, kernel):
    file, vgprs, sgprs, lds, count = FOLD[kernel]
    r = res[kernel]
    assert r["file"] == file
    assert (r["vgprs"], r["sgprs"], r["lds_bytes"]) == (vgprs, sgprs, lds), (kernel, r)
    assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert instructions[kernel] == count, f"{kernel}: {instructions[kernel]} instructions, {count} before the filter"
