"""The edge-aware filter of the shadow mask without a GPU: the C-ABI block (header, library and abi.py agree), every refusal of
vkr_shadow_mask_filter and of vkrh_set_shadow_mask_filter with its own message (validation never reaches a launch), and the numpy
restatement (tests/shadow_mask_filter_reference.py) alone on the rasterised procedural scene at 64 x 36: reach 1 is the identity, a
uniform mask stays itself, every output byte lies between the smallest and the largest accepted tap of its channel, sky pixels
pass through, and the partition of unity: on the all-accepted plane a mask whose texel depends only on (x mod R, y mod R) filters
to the half-up rounded mean of its R * R class values at every pixel at least R - 1 from the border.

Measured here (oracle rasteriser, procedural scene at detail 8, thresholds 0.9 and 0.01, 64 x 36, a mask of random bytes): of 2024
geometry pixels 1443 / 981 / 677 accept every tap at reach 2 / 3 / 4, the mean accepted weight is 14.9 of 16 / 68.6 of 81 / 201.1 of
256, and 2021 texels change (test_reference_on_the_scene prints them)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PostFxChain

import shadow_mask_filter_cases as cases
import shadow_mask_filter_reference as ref
from test_abi_errors import ERR_EXTENT, ERR_FORMAT, ERR_LAYOUT, ERR_NULL, FAKE, img
from test_shadow_mask_rt import _HostMemoryFrame

F32 = np.float32
D24 = abi.FMT_D24_UNORM_S8
RG16 = abi.FMT_RG16_UNORM
RGBA8 = abi.FMT_RGBA8_UNORM
SKY = 0xFFFFFF
NAN = float("nan")


# ---- declarations -------------------------------------------------------------------------------------------------------------------
def test_block_layout_and_symbols():
    txt = open(abi.ROOT + "/include/vkr_postfx.h").read()
    body = re.search(r"typedef struct vkr_shadow_filter_params \{(.*?)\} vkr_shadow_filter_params;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert fields == ["vkr_mat4 inverse_camera", "float fovy, aspect, znear, zfar", "uint32_t reach", "float normal_min_dot", "float plane_tolerance",
                      "uint32_t reserved"]
    assert C.sizeof(abi.ShadowFilterParams) == 64 + 16 + 16 == 96
    offsets = {"inverse_camera": 0, "fovy": 64, "aspect": 68, "znear": 72, "zfar": 76, "reach": 80, "normal_min_dot": 84, "plane_tolerance": 88, "reserved": 92}
    for name, off in offsets.items():
        assert getattr(abi.ShadowFilterParams, name).offset == off, name
    assert re.search(r"\bint\s+vkr_shadow_mask_filter\(const vkr_img\* depth, const vkr_img\* normal, const vkr_img\* mask, "
                     r"const vkr_shadow_filter_params\* params,\s+const vkr_img\* out_mask, void\* stream\);", txt)
    assert hasattr(abi.product(), "vkr_shadow_mask_filter")
    # the library's own size of the block: a 96-byte block whose last word is not 0 is refused as `reserved`
    assert "int vkrh_set_shadow_mask_filter(void* frame, uint32_t reach, float normal_min_dot, float plane_tolerance);" in \
        open(abi.ROOT + "/vk-renderer_amd/host/frame.hpp").read()
    assert (abi.SHADOW_FILTER_NORMAL_MIN_DOT, abi.SHADOW_FILTER_PLANE_TOLERANCE) == (0.9, 0.01)
    p = abi.shadow_filter_params(np.eye(4), 1.0, 2.0, 0.05, 80.0, 4)
    assert (p.reach, p.reserved) == (4, 0) and p.normal_min_dot == F32(0.9) and p.plane_tolerance == F32(0.01)


def test_setter_is_exported_and_no_program_is_registered():
    assert hasattr(host.lib(), "vkrh_set_shadow_mask_filter") and hasattr(host.HostFrame, "set_shadow_mask_filter")
    assert host.lib().vkrh_has_program(b"shadow_mask_filter") == 0  # the task calls the entry: the table stays as it is
    assert hasattr(PostFxChain, "shadow_mask_filter")


# ---- the entry's gates ----------------------------------------------------------------------------------------------------------------
W, H = 64, 32


def _params(reach=4, normal_min_dot=0.9, plane_tolerance=0.01, reserved=0):
    p = abi.shadow_filter_params(np.eye(4), 1.0, 2.0, 0.05, 80.0, reach, normal_min_dot, plane_tolerance)
    p.reserved = reserved
    return p


def _call(**over):
    lib = abi.product()
    a = dict(depth=img(D24, W, H), normal=img(RG16, W, H), mask=img(RGBA8, W, H), params=_params(), out=img(RGBA8, W, H, base=FAKE + 0x100000))
    a.update(over)
    byref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    rc = lib.vkr_shadow_mask_filter(byref(a["depth"]), byref(a["normal"]), byref(a["mask"]), byref(a["params"]), byref(a["out"]), None)
    return rc, (lib.vkr_last_error() or b"").decode()


WINDOW = dict(full=(W, 2 * H), origin=(0, H))
REFUSALS = {
    "depth NULL": (dict(depth=None), ERR_NULL, "depth is NULL"),
    "normal NULL": (dict(normal=None), ERR_NULL, "normal is NULL"),
    "mask NULL": (dict(mask=None), ERR_NULL, "mask is NULL"),
    "params NULL": (dict(params=None), ERR_NULL, "params is NULL"),
    "out NULL": (dict(out=None), ERR_NULL, "out_mask is NULL"),
    "depth without memory": (dict(depth=img(D24, W, H, base=None)), ERR_NULL, "shadow_mask_filter.depth: NULL image"),
    "normal without memory": (dict(normal=img(RG16, W, H, base=None)), ERR_NULL, "shadow_mask_filter.normal: NULL image"),
    "mask without memory": (dict(mask=img(RGBA8, W, H, base=None)), ERR_NULL, "shadow_mask_filter.mask: NULL image"),
    "out without memory": (dict(out=img(RGBA8, W, H, base=None)), ERR_NULL, "shadow_mask_filter.out_mask: NULL image"),
    "depth format": (dict(depth=img(abi.FMT_R32_SFLOAT, W, H)), ERR_FORMAT, "shadow_mask_filter.depth: format"),
    "normal format": (dict(normal=img(abi.FMT_RG16_SFLOAT, W, H)), ERR_FORMAT, "shadow_mask_filter.normal: format"),
    "mask format": (dict(mask=img(abi.FMT_RGBA8_SRGB, W, H)), ERR_FORMAT, "shadow_mask_filter.mask: format"),
    "out format": (dict(out=img(abi.FMT_RGBA8_SRGB, W, H, base=FAKE + 0x100000)), ERR_FORMAT, "shadow_mask_filter.out_mask: format"),
    "depth extent": (dict(depth=img(D24, W, H + 1)), ERR_EXTENT, "depth is 64x33, normal 64x32, mask 64x32, out_mask 64x32: one extent expected"),
    "normal extent": (dict(normal=img(RG16, W // 2, H)), ERR_EXTENT, "normal 32x32, mask 64x32, out_mask 64x32: one extent expected"),
    "mask extent": (dict(mask=img(RGBA8, W + 1, H)), ERR_EXTENT, "mask 65x32, out_mask 64x32: one extent expected"),
    "out extent": (dict(out=img(RGBA8, W, H - 1, base=FAKE + 0x100000)), ERR_EXTENT, "out_mask 64x31: one extent expected"),
    "extent above 65535": (dict(depth=img(D24, 65536, 1), normal=img(RG16, 65536, 1), mask=img(RGBA8, 65536, 1), out=img(RGBA8, 65536, 1, base=FAKE + 0x100000)),
                           ERR_EXTENT, "out_mask is 65536x1, at most 65535 texels a side"),
    "depth window": (dict(depth=img(D24, W, H, **WINDOW)), ERR_EXTENT, "shadow_mask_filter: depth: windows are not supported (the taps cross strip borders"),
    "normal window": (dict(normal=img(RG16, W, H, **WINDOW)), ERR_EXTENT, "shadow_mask_filter: normal: windows are not supported"),
    "mask window": (dict(mask=img(RGBA8, W, H, **WINDOW)), ERR_EXTENT, "shadow_mask_filter: mask: windows are not supported"),
    "out window": (dict(out=img(RGBA8, W, H, base=FAKE + 0x100000, **WINDOW)), ERR_EXTENT, "shadow_mask_filter: out_mask: windows are not supported"),
    "reach 0": (dict(params=_params(reach=0)), ERR_EXTENT, "reach 0, expected 1..4"),
    "reach 5": (dict(params=_params(reach=5)), ERR_EXTENT, "reach 5, expected 1..4"),
    "normal_min_dot NaN": (dict(params=_params(normal_min_dot=NAN)), ERR_EXTENT, "normal_min_dot is NaN"),
    "plane_tolerance NaN": (dict(params=_params(plane_tolerance=NAN)), ERR_EXTENT, "plane_tolerance is NaN"),
    "reserved": (dict(params=_params(reserved=7)), ERR_EXTENT, "reserved is 7, must be 0"),
    "in place": (dict(out=img(RGBA8, W, H)), ERR_LAYOUT, "mask and out_mask overlap in memory"),
    "overlap by one row": (dict(out=img(RGBA8, W, H, base=FAKE + (H - 1) * W * 4)), ERR_LAYOUT, "mask and out_mask overlap in memory"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_entry_refusals(name):
    kwargs, code, message = REFUSALS[name]
    rc, msg = _call(**kwargs)
    assert rc == code, (name, rc, msg)
    assert message in msg and msg.startswith("shadow_mask_filter"), (name, msg)


def test_refusal_messages_are_distinct():
    texts = [_call(**kwargs)[1] for kwargs, _, _ in REFUSALS.values()]
    assert len(set(texts)) == len(texts) - 1  # "in place" and "overlap by one row" share the one overlap message


# ---- the frame setter -------------------------------------------------------------------------------------------------------------------
def _set_filter(frame, reach, normal_min_dot=0.9, plane_tolerance=0.01):
    l = host.lib()
    rc = l.vkrh_set_shadow_mask_filter(frame.h, reach, normal_min_dot, plane_tolerance)
    return rc, l.vkrh_last_error().decode()


def test_frame_setter_refusals():
    frame = _HostMemoryFrame(tiled=False)
    try:
        for args, text in (((5,), "reach 5, needs 0 (off) or 1..4"), ((2, NAN), "a threshold is NaN"), ((2, 0.9, NAN), "a threshold is NaN")):
            rc, msg = _set_filter(frame, *args)
            assert rc != 0 and "vkrh_set_shadow_mask_filter: " + text in msg, (args, msg)
        for reach in (0, 1, 2, 3, 4, 0):
            assert _set_filter(frame, reach)[0] == 0
        # the stages' own refusals are untouched by the setter
        assert _set_filter(frame, 4)[0] == 0
        rc, msg = frame.run(host.STAGE_SHADOW_MASK_RT)
        assert rc != 0 and "VKRH_STAGE_SHADOW_MASK_RT without a loaded scene" in msg
        l = host.lib()
        assert l.vkrh_image(frame.h, b"shadow_mask_filtered", 0, 1, C.byref(abi.VkrImg())) != 0
        assert "'shadow_mask_filtered' only exists after a mask stage with vkrh_set_shadow_mask_filter on" in l.vkrh_last_error().decode()
    finally:
        frame.close()


def test_frame_setter_is_refused_on_a_tiled_frame():
    frame = _HostMemoryFrame(tiled=True)
    try:
        rc, msg = _set_filter(frame, 4)
        assert rc != 0 and "vkrh_set_shadow_mask_filter: on a tiled frame" in msg
    finally:
        frame.close()


# ---- the reference alone ----------------------------------------------------------------------------------------------------------------
SIZE = (64, 36)
THRESHOLDS = (cases.NORMAL_MIN_DOT, cases.PLANE_TOLERANCE)


def _arith():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


@functools.lru_cache(maxsize=None)
def _raster():
    w, h = SIZE
    setup = FrameSetup(w, h)
    chain = PostFxChain(w, h, backend="oracle", setup=setup)
    chain.raster(scn.procedural_scene(detail=8))
    return chain.depth.raw(0)[..., 0].astype(np.uint32), chain.normal.raw(0).copy(), setup


def _filter(words, codes, setup, mask, reach, thresholds=THRESHOLDS, with_range=False):
    return ref.shadow_mask_filter(_arith(), words, codes, mask, setup.inv_view, *setup.fazz, reach, *thresholds, with_range=with_range)


def _random_mask(seed=0):
    return np.random.default_rng([0x3A5C, seed]).integers(0, 256, size=(SIZE[1], SIZE[0], 4), dtype=np.uint8)


def test_reach_1_is_the_identity():
    words, codes, setup = _raster()
    mask = _random_mask()
    assert np.array_equal(_filter(words, codes, setup, mask, 1), mask)


@pytest.mark.parametrize("reach", [1, 2, 3, 4])
def test_a_uniform_mask_stays_itself(reach):
    words, codes, setup = _raster()
    for value in ((0, 0, 0, 0), (255, 255, 255, 255), (1, 127, 128, 254)):
        mask = np.empty((SIZE[1], SIZE[0], 4), np.uint8)
        mask[:] = value
        assert np.array_equal(_filter(words, codes, setup, mask, reach), mask), value


@pytest.mark.parametrize("reach", [2, 3, 4])
def test_reference_on_the_scene(reach):
    """every byte between the smallest and the largest accepted tap of its channel; sky passes through; not vacuous: some pixel
    accepts every tap, some pixel rejects one, and the filter changes something"""
    words, codes, setup = _raster()
    mask = _random_mask(reach)
    out, lo, hi, A = _filter(words, codes, setup, mask, reach, with_range=True)
    assert (out >= lo).all() and (out <= hi).all()
    sky = (words & SKY) == SKY
    assert sky.any() and np.array_equal(out[sky], mask[sky])
    geometry = ~sky
    full = (A == reach ** 4) & geometry
    print(f"[shadow mask filter] reference, reach {reach}: {int(geometry.sum())} geometry pixels, {int(full.sum())} accept every tap, "
          f"mean accepted weight {float(A[geometry].mean()):.1f} of {reach ** 4}, {int((out != mask).any(axis=-1).sum())} texels changed")
    assert full.any() and ((A < reach ** 4) & geometry & cases.interior(SIZE, reach)).any()
    assert (out[geometry] != mask[geometry]).any()


@pytest.mark.parametrize("reach", [2, 3, 4])
def test_partition_of_unity(reach):
    setup = FrameSetup(*SIZE)
    words, codes = cases.plane_gbuffer(SIZE, setup)
    taps, sky = ref.accept_sets(_arith(), words, codes, setup.inv_view, *setup.fazz, reach, *THRESHOLDS)
    assert not sky.any()
    w, h = SIZE
    y, x = np.mgrid[0:h, 0:w]
    for (dx, dy), acc in taps.items():  # the reference accepts every tap that lies inside the image
        in_image = (x + dx >= 0) & (x + dx < w) & (y + dy >= 0) & (y + dy < h)
        assert np.array_equal(acc, in_image | ((dx, dy) == (0, 0))), (dx, dy)
    out = _filter(words, codes, setup, cases.residue_mask(SIZE, reach), reach)
    inner = cases.interior(SIZE, reach)
    want = cases.residue_mean(reach)
    assert inner.any() and (out[inner] == want).all(), (np.unique(out[inner].reshape(-1, 4), axis=0), want)
    assert len(np.unique(cases.residue_mask(SIZE, reach).reshape(-1, 4), axis=0)) == reach * reach  # the classes do differ


@pytest.mark.parametrize("reach", [1, 2, 3, 4])
def test_single_texel_reaches_exactly_its_window(reach):
    """the cases of the early-out test on the GPU, on the reference: a texel at distance R - 1 from a tile changes that tile's
    output, one at distance R does not"""
    setup = FrameSetup(*SIZE)
    words, codes = cases.plane_gbuffer(SIZE, setup)
    seen = {True: 0, False: 0}
    for name, at, (tx, ty), changes in cases.single_texel_cases(SIZE, reach):
        out = _filter(words, codes, setup, cases.single_texel_mask(SIZE, at), reach)
        tile = out[ty:ty + 8, tx:tx + 8]
        assert (tile != np.array(cases.BASE, np.uint8)).any() == changes, name
        assert (out[..., :3] == np.array(cases.BASE[:3], np.uint8)).all(), name
        seen[changes] += 1
    assert seen[True] >= 3 and seen[False] >= 3
