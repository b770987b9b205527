"""Drop-in boundary check: the reference's own pass sources compile UNCHANGED against the host mirror.

`host/` keeps the reference's operator interface — rendergraph::RenderGraph / RenderGraphBuilder / RenderResources,
gpu::CmdContext, the binding structs, pipelines looked up by program name, and the pass structs with their public
signatures — so that each pass "drops into" the frame loop.  This test feeds every hot-path pass source of the
reference (`src/{taa,downsample_pass,ssr,screen_trace,gtao,advanced_ssr,defered_shading}.cpp`, read where they lie and
piped to the compiler: nothing is copied) through `g++ -c` with `host/` as the only project include directory: build()
does that by oracle/ref.mk wherever the reference's sources are present, into oracle/_ref/ref_<pass>.o plus the list of
every header the compile read.  Every name those files spell — includes, types, members, overloads, initialiser shapes —
must resolve against the mirror.  Skipped where build() ran without the reference (no oracle/_ref/)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vk-renderer_amd", "host")
REF_OUT = os.path.join(ROOT, "oracle", "_ref")  # oracle/ref.mk
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
PASS_SOURCES = ["taa.cpp", "downsample_pass.cpp", "ssr.cpp", "screen_trace.cpp", "gtao.cpp", "advanced_ssr.cpp", "defered_shading.cpp"]


@pytest.mark.parametrize("source", PASS_SOURCES)
def test_reference_pass_source_compiles_against_host_mirror(source):
    if not os.path.isdir(REF_OUT):
        pytest.skip("oracle/_ref/ not built: build() ran where the reference's sources are not present")
    stem = os.path.join(REF_OUT, "ref_" + source[:-len(".cpp")])
    assert os.path.exists(stem + ".o"), f"{source} does not compile against host/ (make -C oracle -f ref.mk)"
    defined = subprocess.run(["nm", "--defined-only", stem + ".o"], capture_output=True, text=True, check=True).stdout
    assert " T " in defined, f"{source}: the object defines no function"
    # the compile ran with host/ as its directory: every header it read by a relative name lies in the repository (the
    # mirror, include/), every other one is a system or ROCm header; no header of the reference tree was pulled in
    with open(stem + ".d") as f:
        deps = f.read().split(":", 1)[1].replace("\\\n", " ").split()
    assert deps
    for d in deps:
        if os.path.isabs(d):
            assert d.startswith(("/usr/", ROCM.rstrip("/") + "/")), f"{source} read {d}"
        else:
            assert os.path.realpath(os.path.join(HOST, d)).startswith(os.path.realpath(ROOT) + os.sep), f"{source} read {d}"


def test_mirror_headers_resolve_inside_the_mirror():
    """every header name the reference's pass sources include exists under host/ (so the test above cannot silently
    fall back to a system or reference header)"""
    for name in ("rendergraph/rendergraph.hpp", "gpu/gpu.hpp", "gtao.hpp", "advanced_ssr.hpp", "taa.hpp", "ssr.hpp", "screen_trace.hpp",
                 "downsample_pass.hpp", "defered_shading.hpp", "scene_renderer.hpp", "imgui_pass.hpp", "gpu_transfer.hpp", "trace_samples.hpp"):
        assert os.path.exists(os.path.join(HOST, name)), name
