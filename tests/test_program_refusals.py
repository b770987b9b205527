"""The first refusal of every program of the host layer's program table (host/gpu/gpu.cpp), on the CPU: each program is launched
on an empty descriptor set, with no attachments and no push constants (vkrh_selftest_programs), and must refuse before it
reaches a kernel.  The messages are written out here: they pin the order of each program's checks and, through them, the texts
of the accessors the programs share (tex, ubo, the attachment and buffer accessors)."""
import ctypes as C
import os
import re

from vk_renderer_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
brdf_preintegrate: brdf_preintegrate: Halton buffer (binding 0) is not bound
cube2oct: cube2oct: binding 0 is not bound as expected
cubemap_probe: cubemap_probe: expects colour, distance and depth attachments
default_shadow: default_shadow: expects one depth attachment
defered_shading: defered_shading: expects one colour attachment
defered_shading_shadowed: defered_shading_shadowed: expects one colour attachment
deinterleave_depth: deinterleave_depth: binding 0 is not bound as expected
depth_mips: depth_mips: expects at least one depth attachment
downsample_gbuffer: downsample_gbuffer: expects 2 colour attachments + depth
gbuf_opaque_taa: gbuf_opaque_taa: expects 4 colour attachments + depth
gtao_accumulate: gtao_accumulate: binding 0 is not bound as expected
gtao_compute_main: gtao_compute_main: binding 0 is not bound as expected
gtao_filter: gtao_filter: binding 0 is not bound as expected
gtao_main: gtao_main: expects one colour attachment
gtao_reproject: gtao_reproject: binding 1 is not bound as expected
gtao_rt_main: gtao_rt_main: expects one colour attachment
main_deinterleaved: main_deinterleaved: binding 0 is not bound as expected
pdf_preintegrate: pdf_preintegrate: binding 0 is not bound as expected
probe_downsample: probe_downsample: expects one colour attachment
reflections_rt: reflections_rt: binding 0 is not bound as expected
reflections_rt_cutout: reflections_rt_cutout: binding 0 is not bound as expected
screen_trace_accumulate: screen_trace_accumulate: binding 0 is not bound as expected
screen_trace_filter: screen_trace_filter: binding 0 is not bound as expected
screen_trace_main: screen_trace_main: binding 0 is not bound as expected
shadow_mask: shadow_mask: binding 0 is not bound as expected
shadow_mask_rt: shadow_mask_rt: binding 0 is not bound as expected
shadow_mask_rt_cutout: shadow_mask_rt_cutout: binding 0 is not bound as expected
shadow_mask_rt_soft: shadow_mask_rt_soft: binding 0 is not bound as expected
shadow_mask_rt_soft_cutout: shadow_mask_rt_soft_cutout: binding 0 is not bound as expected
ssao: ssao: expects one colour attachment
ssr: ssr: expects one colour attachment
sssr_blur: sssr_blur: binding 0 is not bound as expected
sssr_classification: sssr_classification: binding 0 is not bound as expected
sssr_filter: sssr_filter: binding 0 is not bound as expected
sssr_trace: sssr_trace: binding 0 is not bound as expected
sssr_trace_indirect: sssr_trace_indirect: must be launched with dispatch_indirect
sssr_trace_windowed: sssr_trace_windowed: binding 0 is not bound as expected
sssr_trace_windowed_head: sssr_trace_windowed_head: binding 0 is not bound as expected
sssr_trace_windowed_resume: sssr_trace_windowed_resume: binding 0 is not bound as expected
synthetic_gbuffer: synthetic_gbuffer: uniform block 0 is not bound
taa_resolve: taa_resolve: binding 0 is not bound as expected
texdraw: texdraw: expects one colour attachment
tile_regression: tile_regression: binding 0 is not bound as expected
trace_probe: trace_probe: binding 0 is not bound as expected
"""


def _selftest():
    l = host.lib()
    buf = C.create_string_buffer(16384)
    assert l.vkrh_selftest_programs(buf, 16384) == 0, l.vkrh_last_error().decode()
    return buf.value.decode()


def test_every_program_refuses_an_empty_set_with_its_own_message():
    got = _selftest()
    assert "no error" not in got, [line for line in got.splitlines() if "no error" in line]
    assert len(EXPECTED.splitlines()) == 44
    assert got.splitlines() == EXPECTED.splitlines()


def test_the_table_holds_exactly_the_programs_the_passes_name():
    """tests/test_program_table.py in the other direction: nothing is registered that no pass of host/passes.cpp names"""
    src = open(os.path.join(ROOT, "vk-renderer_amd", "host", "passes.cpp")).read()
    lib = host.lib()
    named = {n for n in re.findall(r'"([a-z_0-9]+)"', src) if lib.vkrh_has_program(n.encode())}
    registered = [line.split(":")[0] for line in _selftest().splitlines()]
    assert len(registered) == len(set(registered)) == 44
    assert set(registered) == named, (sorted(set(registered) - named), sorted(named - set(registered)))
