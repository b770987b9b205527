"""CPU tests (no GPU) of what the three compute rasterisers share on the host side (csrc/raster_common.hpp): check_scene(), which
every entry point runs before it launches anything, and the scratch layouts behind the three *_scratch_bytes functions.

The images of every call live in host memory and the scratch pointer is never dereferenced: a refusal comes first.  The row
index_offset = 0xFFFFFFF0 is the one that a 32-bit index_offset + index_count lets through (it wraps to a small number)."""
import ctypes as C

import numpy as np
import pytest

from vk_renderer_amd import abi
from vk_renderer_amd import scene as scn
from vk_renderer_amd.images import ArrayImageBuf, ImageBuf

import shadow_light as sl

ERR_NULL, ERR_EXTENT = 1001, 1003
N = 64
HUGE = 1 << 40  # scratch_bytes: never the reason of a refusal here


@pytest.fixture(scope="module")
def lib():
    return abi.product()


def _shadow(lib, scene):
    layers = ArrayImageBuf(abi.FMT_D24_UNORM_S8, N, N, 1)
    mats = (abi.Mat4 * 1)(abi.Mat4.from_np(sl.mvp("A")))
    fake = np.zeros(64, np.uint8)
    return lib.vkr_default_shadow(C.byref(scene), mats, layers.descs(), 1, fake.ctypes.data, HUGE, None)


def _cubemap(lib, scene):
    color = ArrayImageBuf(abi.FMT_RGBA8_SRGB, N, N, 6)
    distance = ArrayImageBuf(abi.FMT_R16_SFLOAT, N, N, 6)
    pos = (C.c_float * 3)(0.0, 1.0, 4.0)
    fake = np.zeros(64, np.uint8)
    return lib.vkr_cubemap_probe(C.byref(scene), C.byref(pos), color.descs(), distance.descs(), fake.ctypes.data, HUGE, None)


def _gbuffer(lib, scene):
    att = [ImageBuf(f, N, N) for f in (abi.FMT_RGBA8_SRGB, abi.FMT_RG16_UNORM, abi.FMT_RGBA8_SRGB, abi.FMT_RG16_SFLOAT, abi.FMT_D24_UNORM_S8)]
    ad = [a.desc() for a in att]
    consts = abi.GbufConst()
    consts.view_projection = consts.prev_view_projection = abi.Mat4.from_np(sl.mvp("A"))
    fake = np.zeros(64, np.uint8)
    return lib.vkr_raster_gbuffer(C.byref(scene), C.byref(consts), C.byref(ad[0]), C.byref(ad[1]), C.byref(ad[2]), C.byref(ad[3]), C.byref(ad[4]),
                                  fake.ctypes.data, HUGE, None)


ENTRIES = {"default_shadow": _shadow, "cubemap_probe": _cubemap, "gbuf_opaque_taa": _gbuffer}
# (field of the bad draw, its value as a function of the scene, a word of the message)
BAD_DRAWS = {
    "transform_index": ("transform_index", lambda sc: len(sc.transforms), "transform_index"),
    "index_count": ("index_count", lambda sc: len(sc.indices) + 3, "indices"),
    "index_offset_wraps": ("index_offset", lambda sc: 0xFFFFFFF0, "indices"),
}


@pytest.mark.parametrize("row", sorted(BAD_DRAWS) + ["null_index_array"])
@pytest.mark.parametrize("program", sorted(ENTRIES))
def test_scene_refusals_without_a_device(lib, program, row):
    """a draw that points outside the scene, or a scene with draws and no index array, is refused with VKR_ERR_EXTENT /
    VKR_ERR_NULL and a message "<program>: scene: ..." (with "draw N:" where a draw is at fault) before anything is launched"""
    sc = scn.procedural_scene(detail=6)
    bad, keep = sc.upload(None)
    # the bad draw: the first after draw 0 with 16 indices or more, so that 0xFFFFFFF0 + index_count wraps in 32 bits
    k = next(i for i, d in enumerate(sc.draws) if i >= 1 and d["index_count"] >= 16)
    if row == "null_index_array":
        bad.indices = None
        want, words = ERR_NULL, ("draws", "NULL", "index")  # no draw was looked at: the message names none
    else:
        field, value, word = BAD_DRAWS[row]
        draws = C.cast(bad.draws, C.POINTER(abi.RasterDraw))
        if row == "index_offset_wraps":
            assert (0xFFFFFFF0 + draws[k].index_count) & 0xFFFFFFFF <= bad.index_count, "the 32-bit sum must pass for the row to mean anything"
        setattr(draws[k], field, value(sc))
        want, words = ERR_EXTENT, (f"draw {k}:", word)
    rc = ENTRIES[program](lib, bad)
    msg = (lib.vkr_last_error() or b"").decode()
    assert rc == want, (rc, msg)
    assert msg.startswith(program + ": scene: ") and all(w in msg for w in words), msg


@pytest.mark.parametrize("program", ["cubemap_probe", "gbuf_opaque_taa"])
def test_texture_indices_are_checked_where_textures_are_read(lib, program):
    """(default.frag reads no texture: default_shadow ignores the indices, which tests/test_shadow.py pins)"""
    sc = scn.procedural_scene(detail=6)
    bad, keep = sc.upload(None)
    C.cast(bad.draws, C.POINTER(abi.RasterDraw))[1].albedo_index = len(sc.textures)
    rc = ENTRIES[program](lib, bad)
    msg = (lib.vkr_last_error() or b"").decode()
    assert rc == ERR_EXTENT and "draw 1" in msg and "texture" in msg, (rc, msg)


# the values of the build before the layouts were written down once (ScratchCarver): (arguments) -> bytes
RASTER_BYTES = {(0, 0, 0): 250368, (1, 1, 0): 250624, (640, 360, 1000): 2669824, (201, 119, 12345): 7552768, (200, 120, 7): 446720,
                (3840, 2160, 1000000): 642605568}
CUBE_BYTES = {(0, 0): 446976, (72, 0): 695808, (73, 12): 723456, (128, 12): 1253888, (128, 1200): 3249408, (256, 100001): 171594752}
SHADOW_BYTES = {(1024, 1, 0): 82176, (200, 1, 1000): 202496, (1024, 4, 1000): 807936, (1023, 8, 12345): 12507136, (360, 8, 0): 655616,
                (64, 1, 1): 82944}


def test_scratch_sizes_are_unchanged(lib):
    """zero triangles, odd extents, one layer and eight layers"""
    for args, want in RASTER_BYTES.items():
        assert lib.vkr_raster_scratch_bytes(*args) == want, args
    for args, want in CUBE_BYTES.items():
        assert lib.vkr_cubemap_probe_scratch_bytes(*args) == want, args
    for args, want in SHADOW_BYTES.items():
        assert lib.vkr_default_shadow_scratch_bytes(*args) == want, args
