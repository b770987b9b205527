"""Every pass that takes a camera as data, on the GPU under the cameras of tests/camera_cases.py: pitched, rolled, yawed, narrow,
wide and anamorphic lenses, other depth ranges, a previous frame that pitched and rolled.  The frozen camera of every other parity
test has a view matrix of zeros and +-1, tan(fovy / 2) < 1, aspect = W / H and znear equal to a literal of the reference
shaders; tests/test_camera_cases.py shows on the oracle that under these cases every camera input of every pass is observable.

The chain, the rows either side of it and the shading run step by step on the oracle's pre-step bytes (tests/camera_cases.py
Record), as tests/test_content_gpu.py test_stagewise does: integer outputs bit for bit, the others under tests/parity.py with
the cap of tests/test_fuzz_gpu.py and the non-finite strictness of tests/test_content_gpu.py.  70x38 for everything, 206x226 in
addition for the chain.

gtao_accumulate on the texels of camera_cases.sky_half is compared with two reference values, the oracle's output and the
oracle's output with clear_history = 1: there the shader linearises a reprojected ndc.z ~ 1 and compares it with 0.2
(DESIGN_NUMERICS.md "Cameras").  The class comes from the input depth, never from the differences.

The generator and the passes with exact restatements (ssao, tile_regression, gtao_rt_main, trace_probe, shadow_mask, shadow_mask_rt
and its cutout form, shadow_mask_rt_soft, shadow_mask_filter, reflections_rt and its cutout form) are compared byte for byte under
every case, as their own tests do under the frozen camera, the ray-traced ones on the procedural scene those tests use.

vkr_selftest_division runs at every case's depth range; the C++ host frame runs chain and shading under three of the cases."""
import ctypes as C

import numpy as np
import pytest

from vk_renderer_amd import abi

import camera_cases as cc
from parity import record
from test_content_gpu import _report

pytestmark = pytest.mark.gpu

NAMES = tuple(cc.CASES)


def _size_id(s):
    return f"{s[0]}x{s[1]}"


def _tag(rec):
    return f"{rec.name} {rec.size[0]}x{rec.size[1]}"


def _where(bad):
    return [(int(x), int(y)) for y, x in zip(*np.nonzero(bad))][:4]


def _check(rec, step, results):
    """the outputs of `step` on the product against the oracle's bytes -> texels outside tolerance"""
    total = 0
    for out, (img, want) in results.items():
        host = img.to_host()
        what = f"{_tag(rec)} {step.name}:{out}"
        if step.is_exact(out):
            nbad = 0
            for mip in range(img.mips):
                a, b = cc.bits(img, mip, host), cc.bits(img, mip, want)
                n = int((a != b).any(axis=-1).sum())
                record(f"{what}.{mip}", a.shape[0] * a.shape[1], a.shape[0] * a.shape[1] - n, n, 0.0, "bit-exact")
                nbad += n
            print(f"[camera] {what}: differing texels {nbad} (bit for bit)")
            assert nbad == 0, f"{what}: {nbad} texels differ (integer path must be bit-exact)"
            continue
        assert img.mips == 1
        got, ref = img.decode(0, host), img.decode(0, want)
        nbad, bad = _report(what, img.format, got, ref)
        texels = img.width * img.height
        if step.name == "gtao_accumulate":
            # sky_half: either reference value; everything else under the cap
            _, bad_cleared = _report(what + "[cleared]", img.format, got, img.decode(0, rec.acc_ao_cleared))
            sky = rec.sky
            kept, cleared = int((sky & ~bad).sum()), int((sky & bad & ~bad_cleared).sum())
            neither = sky & bad & bad_cleared
            bad = bad & ~sky
            nbad = int(bad.sum())
            print(f"[camera] {what}: outside tolerance {nbad} of {texels - int(sky.sum())} texels off the sky (cap {cc.cap(texels)}); sky_half "
                  f"{int(sky.sum())} texels: {kept} as the oracle, {cleared} as the oracle with its history cleared, {int(neither.sum())} neither")
            assert not neither.any(), f"{what}: {int(neither.sum())} sky texels hold neither reference value, first at (x, y) {_where(neither)}"
        else:
            print(f"[camera] {what}: outside tolerance {nbad} of {texels} texels (cap {cc.cap(texels)})")
        assert nbad <= cc.cap(texels), f"{what}: {nbad} texels outside tolerance, first at (x, y) {_where(bad)}"
        total += nbad
    return total


def _product(rec):
    import torch

    assert torch.cuda.is_available()
    return rec.chain("product", device="cuda")


@pytest.mark.parametrize("size", cc.SIZES, ids=_size_id)
@pytest.mark.parametrize("name", NAMES)
def test_chain_stagewise(name, size, oracle_lib):
    """the frame loop, every stage on the oracle's pre-stage bytes"""
    rec = cc.record(name, size)
    gpu = _product(rec)
    total = sum(_check(rec, step, rec.run(gpu, step)) for step in cc.CHAIN_STEPS)
    print(f"[camera] {_tag(rec)} stagewise: texels outside tolerance over all stages: {total}")


@pytest.mark.parametrize("name", NAMES)
def test_side_rows_and_shading(name, oracle_lib):
    """graphics / deinterleaved / non-MIS GTAO, the static AO reprojection, ScreenSpaceTrace, simple SSR, the classified indirect
    trace and the deferred shading, each on the oracle's bytes"""
    rec = cc.record(name, cc.SMALL)
    gpu = _product(rec)
    total = sum(_check(rec, step, rec.run(gpu, step)) for step in cc.SIDE_STEPS)
    print(f"[camera] {_tag(rec)} side rows: texels outside tolerance over all steps: {total}")


@pytest.mark.parametrize("name", NAMES)
def test_synth(name, oracle_lib):
    """the generator under the case's camera: the six G-buffer images byte for byte"""
    rec = cc.record(name, cc.SMALL)
    _check(rec, cc.SYNTH, rec.run(_product(rec), cc.SYNTH))


def test_division_selftest_at_every_depth_range():
    """vkr_selftest_division (div_normal against IEEE '/' for linearize_depth2 over all 2^24 stored depths, and the hashed
    operand pairs) at every case's (znear, zfar): all five counters zero"""
    import torch

    lib = abi.product()
    lib.vkr_selftest_division.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    ranges = sorted({(float(s.fazz[2]), float(s.fazz[3])) for s in (cc.setup(n, cc.SMALL) for n in NAMES)})
    assert len(ranges) >= 5
    for znear, zfar in ranges:
        counters = torch.zeros(5, dtype=torch.int32, device="cuda")
        abi.check(lib.vkr_selftest_division(counters.data_ptr(), znear, zfar, torch.cuda.current_stream().cuda_stream), lib)
        torch.cuda.synchronize()
        print(f"[camera] selftest_division znear {znear} zfar {zfar}: {counters.tolist()}")
        assert counters.tolist() == [0, 0, 0, 0, 0], (znear, zfar, counters.tolist())


@pytest.mark.parametrize("name", ["pitch_down_roll", "deep_range", "all_moved"])
def test_host_frame(name, oracle_lib):
    """the C++ host frame, chain and shading, two frames without resynchronisation: the rule of
    tests/test_parity_gpu.py test_host_mirror_frame_with_shading"""
    from test_parity_gpu import host_frame_with_shading

    counts = host_frame_with_shading(cc.setup(name, cc.SMALL), tag=f"host {name}")
    for image, bad in counts.items():
        print(f"[camera] {name} 70x38 host frame {image}: outside tolerance {bad}")


# ---- the passes with exact restatements -------------------------------------------------------------------------------------------------
# Each is the parity test of the pass's own module on the rasterised procedural scene, called with an extent that names the case
# (camera_cases.Extent): the same launch, the same restatement, the same assertions, another camera.  The callee prints the count
# it measured ("differing texels N"; gtao_rt_main, held to tests/parity.py with no exception, "outside-tol N") and asserts it zero; the [camera] line repeats the counts read from what it printed.
HALF = (cc.SMALL[0] // 2, cc.SMALL[1] // 2)  # the passes that read depth mip 1 take the extent of that view


def _exact(capsys, name, what, size=cc.SMALL):
    import re

    printed = capsys.readouterr().out
    counts = [int(n) for n in re.findall(r"(?:differing texels|outside-tol)\s+(\d+)", printed)]
    assert counts, f"{what}: the parity test printed no count"
    with capsys.disabled():  # (printed under the capture, the lines would be read again as the next callee's)
        print(printed, end="")
        print(f"[camera] {name} {size[0]}x{size[1]} {what}: differing texels {sum(counts)} over {len(counts)} comparison(s) (byte for byte)")
    assert sum(counts) == 0


@pytest.mark.parametrize("name", NAMES)
def test_ssao(name, capsys):
    import test_side_pass_content_gpu as side

    side.test_ssao("raster", (cc.Extent(cc.SMALL, name), cc.SMALL), "fixed")
    _exact(capsys, name, "ssao")


@pytest.mark.parametrize("name", NAMES)
def test_tile_regression(name, capsys):
    import test_side_pass_content_gpu as side

    side.test_tile_regression("raster", cc.Extent(HALF, name), "frame")
    _exact(capsys, name, "tile_regression", HALF)


@pytest.mark.parametrize("name", NAMES)
def test_gtao_rt_main(name, capsys):
    import test_side_pass_content_gpu as side

    side.test_traced_ao("raster", cc.Extent(HALF, name), 0.3, "scene")
    _exact(capsys, name, "gtao_rt_main", HALF)


@pytest.mark.parametrize("name", NAMES)
def test_trace_probe(name, capsys):
    import test_side_pass_content_gpu as side

    side.test_probe_trace("raster", "room", cc.Extent(cc.SMALL, name), 4, 16)
    _exact(capsys, name, "trace_probe")


@pytest.mark.parametrize("name", NAMES)
def test_shadow_mask(name, capsys):
    """the shadow-map lookup: depth by vkr_raster_gbuffer through the case's camera, maps by vkr_default_shadow, radii 0, 1, 2"""
    from test_shadow_mask_gpu import rasterised_content

    rasterised_content(cc.setup(name, cc.SMALL), both_in_light_a=False)
    _exact(capsys, name, "shadow_mask")


@pytest.mark.parametrize("name", NAMES)
def test_shadow_mask_rt(name, capsys):
    import test_ray_cutout_passes_gpu as cutout
    import test_shadow_mask_rt_gpu as hard

    size = cc.Extent(cc.SMALL, name)
    hard.test_parity("raster", size, 4)
    _exact(capsys, name, "shadow_mask_rt")
    cutout.test_mask_parity("raster", size, "lod0_masked")
    _exact(capsys, name, "shadow_mask_rt_cutout")


@pytest.mark.parametrize("name", NAMES)
def test_shadow_mask_rt_soft(name, capsys):
    import test_shadow_mask_rt_soft_gpu as soft

    soft.test_parity("raster", cc.Extent(cc.SMALL, name), (4, 2))
    _exact(capsys, name, "shadow_mask_rt_soft")


@pytest.mark.parametrize("name", NAMES)
def test_shadow_mask_filter(name, capsys):
    import test_shadow_mask_filter_gpu as filt

    filt.test_parity("raster", cc.Extent(cc.SMALL, name))
    _exact(capsys, name, "shadow_mask_filter")


@pytest.mark.parametrize("name", NAMES)
def test_reflections_rt(name, capsys):
    import test_ray_cutout_passes_gpu as cutout
    import test_reflections_rt_gpu as opaque

    size = cc.Extent(cc.SMALL, name)
    opaque.test_parity("raster", size, "lod0")
    _exact(capsys, name, "reflections_rt")
    cutout.test_reflections_parity("raster", size, "lod0", False)
    _exact(capsys, name, "reflections_rt_cutout")
