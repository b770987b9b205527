"""GPU tests of the image transfers: vkr_gen_mipmaps against scene.build_mips and the numpy restatement under both schedules,
vkr_blit_image and vkr_clear_image against the restatement (tests/transfer_reference.py) bit for bit, and the frame's four
additions (final-frame capture, device-built texture mips, the mirror's helpers, the prev_depth clear).

Every image is filled with a poison byte first, so a texel a kernel did not write — or a byte of padding it did — shows."""
import ctypes as C

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.images import ArrayImageBuf, ImageBuf, mip_extent

import transfer_reference as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xCD
CHAIN_SIZES = [(256, 256), (300, 200), (257, 129), (5, 1), (1, 1), (2048, 2048), (4096, 1024)]  # (w, h)
SCHEDULES = [("per_level", abi.SWITCH_MIPS_PER_LEVEL), ("fused", abi.SWITCH_MIPS_FUSED)]


def _sync():
    import torch

    torch.cuda.synchronize()


def _raw(buf, mip=0, host_bytes=None):
    """texels of one mip of an ImageBuf as [h, w, c] of the storage type, for every format of the table"""
    hb = buf.to_host() if host_bytes is None else host_bytes
    dt, c = tr.RAW_DTYPE[buf.format]
    w, h = mip_extent(buf.width, mip), mip_extent(buf.height, mip)
    rows = hb[buf.offset[mip]: buf.offset[mip] + buf.pitch[mip] * h].reshape(h, buf.pitch[mip])[:, : w * buf.bpp]
    return np.ascontiguousarray(rows).view(dt).reshape(h, w, c)


def _padding_mask(buf):
    """True for every byte of the allocation that is not a texel"""
    mask = np.ones(buf.nbytes, bool)
    for m in range(buf.mips):
        w, h = mip_extent(buf.width, m), mip_extent(buf.height, m)
        mask[buf.offset[m]: buf.offset[m] + buf.pitch[m] * h].reshape(h, buf.pitch[m])[:, : w * buf.bpp] = False
    return mask


def _device_image(fmt, w, h, mips=1, level0=None):
    hostbuf = ImageBuf(fmt, w, h, mips, fill=POISON)
    if level0 is not None:
        hostbuf.set_raw(level0, 0)
    dev = ImageBuf(fmt, w, h, mips, device=DEV)
    dev.upload(hostbuf.to_host())
    return dev


@pytest.fixture
def switches():
    lib = abi.product()
    before = lib.vkr_get_switches()
    yield lambda bits: lib.vkr_set_switches((before & ~(abi.SWITCH_MIPS_PER_LEVEL | abi.SWITCH_MIPS_FUSED)) | bits)
    lib.vkr_set_switches(before)


# ---- 6. the mip chain ------------------------------------------------------------------------------------------------------
def _rgba8(w, h, seed):
    img = np.random.default_rng(seed).integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    img[::7, ::5, 3] = 0
    return img


@pytest.mark.parametrize("w,h", CHAIN_SIZES)
def test_gen_mipmaps_equals_build_mips_under_both_schedules(switches, w, h):
    level0 = _rgba8(w, h, 11 * w + h)
    want = scn.build_mips(level0)
    outs = {}
    for name, bit in SCHEDULES:
        switches(bit)
        img = _device_image(abi.FMT_RGBA8_SRGB, w, h, len(want), level0)
        abi.gen_mipmaps(img.desc())
        _sync()
        got = img.to_host()
        for lv in range(len(want)):
            g = _raw(img, lv, got)
            bad = int((g != want[lv]).sum())
            assert bad == 0, f"{name} {w}x{h} level {lv}: {bad} of {g.size} bytes differ from build_mips"
        assert np.all(got[_padding_mask(img)] == POISON), f"{name} {w}x{h}: padding written"
        outs[name] = got
    assert np.array_equal(outs["per_level"], outs["fused"])


@pytest.mark.parametrize("fmt", [f for f in tr.MIP_FORMATS if f != tr.FMT_RGBA8_SRGB])
@pytest.mark.parametrize("w,h", [(300, 200), (257, 129), (5, 1), (1, 1), (1024, 512)])
def test_gen_mipmaps_other_formats_equal_the_restatement(switches, fmt, w, h):
    level0 = tr.random_texels(fmt, w, h, 100 * fmt + w)
    want = tr.mip_chain(fmt, level0)
    for name, bit in SCHEDULES:
        switches(bit)
        img = _device_image(fmt, w, h, len(want), level0)
        abi.gen_mipmaps(img.desc())
        _sync()
        got = img.to_host()
        for lv in range(len(want)):
            g = _raw(img, lv, got)
            assert np.array_equal(g.view(np.uint8), want[lv].view(np.uint8)), f"{name} format {fmt} {w}x{h} level {lv}"
        assert np.all(got[_padding_mask(img)] == POISON)


def test_gen_mipmaps_of_a_partial_view(switches):
    """a view that starts at level 2 and holds 3 levels: only its levels 1 and 2 (image levels 3, 4) are written"""
    w, h = 200, 120
    level0 = _rgba8(w, h, 9)
    for name, bit in SCHEDULES:
        switches(bit)
        img = _device_image(abi.FMT_RGBA8_SRGB, w, h, 7, level0)
        abi.gen_mipmaps(img.desc(0, 3))
        abi.gen_mipmaps(img.desc(2, 3))
        _sync()
        want = scn.build_mips(level0)
        for lv in range(5):
            assert np.array_equal(_raw(img, lv), want[lv]), (name, lv)
        for lv in (5, 6):
            assert np.all(_raw(img, lv) == POISON), (name, lv)


# ---- 7. blit ---------------------------------------------------------------------------------------------------------------
def _blit_case(sfmt, sw, sh, dfmt, dw, dh, filt, seed=1):
    src_texels = tr.random_texels(sfmt, sw, sh, seed)
    src = _device_image(sfmt, sw, sh, 1, src_texels)
    dst = _device_image(dfmt, dw, dh)
    abi.blit_image(src.desc(), dst.desc(), filt)
    _sync()
    got_bytes = dst.to_host()
    got = _raw(dst, 0, got_bytes)
    want = tr.blit(src_texels, sfmt, dw, dh, dfmt, filt)
    bad = int((got.view(np.uint8) != want.view(np.uint8)).sum())
    assert bad == 0, f"blit {sfmt} {sw}x{sh} -> {dfmt} {dw}x{dh} filter {filt}: {bad} of {want.nbytes} bytes differ"
    assert np.all(got_bytes[_padding_mask(dst)] == POISON)


GEOMETRY = [
    ("final_frame", 640, 360, 640, 360),
    ("down_2_1", 256, 128, 128, 64),
    ("down_3_2", 300, 201, 200, 134),
    ("up_1_2", 64, 48, 128, 96),
    ("odd", 257, 129, 100, 77),
]


@pytest.mark.parametrize("filt", [abi.FILTER_LINEAR, abi.FILTER_NEAREST])
@pytest.mark.parametrize("name,sw,sh,dw,dh", GEOMETRY)
def test_blit_half_float_to_srgb8(name, sw, sh, dw, dh, filt):
    """the final-frame pair (main.cpp:392: RGBA16_SFLOAT -> RGBA8_SRGB) over every geometry"""
    _blit_case(abi.FMT_RGBA16_SFLOAT, sw, sh, abi.FMT_RGBA8_SRGB, dw, dh, filt)


@pytest.mark.parametrize("filt", [abi.FILTER_LINEAR, abi.FILTER_NEAREST])
@pytest.mark.parametrize("i", range(len(tr.COLOR_FORMATS)))
def test_blit_format_pairs(i, filt):
    """every colour format once as the source and once as the destination, at an odd ratio"""
    fmts = tr.COLOR_FORMATS
    _blit_case(fmts[i], 93, 41, fmts[(i + 4) % len(fmts)], 50, 67, filt, seed=i)


@pytest.mark.parametrize("filt", [abi.FILTER_LINEAR, abi.FILTER_NEAREST])
def test_blit_srgb8_to_srgb8(filt):
    _blit_case(abi.FMT_RGBA8_SRGB, 300, 200, abi.FMT_RGBA8_SRGB, 150, 100, filt)
    _blit_case(abi.FMT_RGBA8_SRGB, 64, 64, abi.FMT_RGBA8_SRGB, 64, 64, filt)


def test_blit_depth_copies_the_words():
    _blit_case(abi.FMT_D24_UNORM_S8, 130, 70, abi.FMT_D24_UNORM_S8, 130, 70, abi.FILTER_NEAREST)


# ---- 8. clear --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", sorted(tr.RAW_DTYPE))
def test_clear_every_format_and_mip(fmt):
    w, h = 37, 21
    mips = tr.mip_count(w, h)
    color, depth, stencil = (0.25, 1.5, -1.0, 0.6), 0.4, 0x5A
    img = _device_image(fmt, w, h, mips)
    abi.clear_image(img.desc(), color, depth, stencil)
    _sync()
    got = img.to_host()
    want = tr.clear_texel(fmt, color, depth, stencil)
    for lv in range(mips):
        g = _raw(img, lv, got)
        assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(np.broadcast_to(want, g.shape)).view(np.uint8)), (fmt, lv)
    assert np.all(got[_padding_mask(img)] == POISON)


def test_clear_wide_rows_and_a_mip_range():
    """rows longer than one block's 1024 bytes, and a view of levels 1..2 only"""
    img = _device_image(abi.FMT_RGBA32_SFLOAT, 333, 9, 4)
    abi.clear_image(img.desc(1, 2), (1.0, 2.0, 3.0, 4.0))
    _sync()
    assert np.all(_raw(img, 0).view(np.uint8) == POISON) and np.all(_raw(img, 3).view(np.uint8) == POISON)
    for lv in (1, 2):
        assert np.array_equal(_raw(img, lv), np.broadcast_to(np.array([1, 2, 3, 4], np.float32), _raw(img, lv).shape))
    big = _device_image(abi.FMT_D24_UNORM_S8, 1000, 5)
    abi.clear_image(big.desc())
    _sync()
    assert np.all(_raw(big) == 0x00FFFFFF)


@pytest.mark.parametrize("fmt", [abi.FMT_D24_UNORM_S8, abi.FMT_R16_UNORM, abi.FMT_RGBA8_SRGB])
def test_clear_of_one_layer_leaves_its_neighbours(fmt):
    arr = ArrayImageBuf(fmt, 40, 24, 3, mips=3, device=DEV, fill=POISON)
    abi.clear_image(arr.desc(1), (1.0, 1.0, 1.0, 1.0), 1.0, 0)
    _sync()
    got = arr.to_host()
    want = np.full(arr.nbytes, POISON, np.uint8)
    texel = tr.clear_texel(fmt, (1.0, 1.0, 1.0, 1.0), 1.0, 0).view(np.uint8)
    for m in range(3):
        w, h = mip_extent(40, m), mip_extent(24, m)
        start = arr.layer_offset(1, m)
        want[start: start + arr.pitch[m] * h].reshape(h, arr.pitch[m])[:, : w * arr.bpp] = np.tile(texel, w)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"


# ---- 9. the frame ----------------------------------------------------------------------------------------------------------
def test_capture_final_writes_the_blitted_taa_output(tmp_path):
    from PIL import Image

    W, H = 320, 180
    frame = host.HostFrame(FrameSetup(W, H), device=DEV)
    try:
        frame.run(host.STAGE_LUT | host.STAGE_GBUFFER | host.STAGE_PREV_DEPTH)
        frame.run(host.STAGE_CHAIN)
        with pytest.raises(RuntimeError, match="RGBA PNG capture needs 4-byte texels"):
            frame.capture("taa_target", tmp_path / "raw.png", host.HostFrame.CAPTURE_RGBA_PNG)  # what kind 3 is for
        frame.capture_final(tmp_path / "final.png")
        taa = frame.download("taa_target")
        assert taa.format == abi.FMT_RGBA16_SFLOAT
        want = tr.blit(taa.raw(0), tr.FMT_RGBA16_SFLOAT, W, H, tr.FMT_RGBA8_SRGB, tr.LINEAR)
        assert len(np.unique(want[..., :3])) > 32, "a flat frame would prove nothing"
        rb = frame.download("readback")
        assert rb.format == abi.FMT_RGBA8_SRGB and (rb.width, rb.height) == (W, H)
        assert np.array_equal(rb.raw(0), want)
        png = np.array(Image.open(tmp_path / "final.png"))
        assert png.shape == (H, W, 4)
        assert np.array_equal(png[..., :3], want[..., :3]) and np.all(png[..., 3] == 255)
    finally:
        frame.close()


def _gbuffer(frame):
    return {n: frame.download(n).to_host().copy() for n in ("albedo", "normal", "material", "velocity", "depth")}


def test_device_built_texture_mips_match_the_host_built_ones():
    sc = scn.procedural_scene(detail=12, cutout=True)
    W, H = 320, 180
    images = {}
    for device_mips in (False, True):
        frame = host.HostFrame(FrameSetup(W, H), device=DEV)
        try:
            frame.load_scene(sc, device_mips=device_mips)
            texels = []
            for i, levels in enumerate(sc.textures):
                d = frame.scene_texture(i)
                assert d.format == abi.FMT_RGBA8_SRGB and d.mip_count == len(levels) and (d.width, d.height) == levels[0].shape[1::-1]
                buf = frame.download_desc(d)
                for m, lv in enumerate(levels):
                    assert np.array_equal(buf.raw(m), lv), f"device_mips={device_mips} texture {i} level {m}"
                texels.append(buf.to_host().copy())
            frame.run(host.STAGE_RASTER)
            _sync()
            images[device_mips] = (texels, _gbuffer(frame))
        finally:
            frame.close()
    for a, b in zip(images[False][0], images[True][0]):
        assert np.array_equal(a, b)
    for n in images[False][1]:
        assert np.array_equal(images[False][1][n], images[True][1][n]), f"G-buffer image {n} differs with device-built mips"
    assert len(np.unique(images[True][1]["albedo"])) > 16


def test_scene_upload_with_device_mips():
    sc = scn.procedural_scene(detail=6, cutout=True)
    a, keep_a = sc.upload(DEV)
    b, keep_b = sc.upload(DEV, device_mips=True)
    _sync()
    ta, tb = C.cast(a.textures, C.POINTER(abi.VkrImg)), C.cast(b.textures, C.POINTER(abi.VkrImg))
    bufs_a = [k for k in keep_a if isinstance(k, ImageBuf)]
    bufs_b = [k for k in keep_b if isinstance(k, ImageBuf)]
    assert len(bufs_a) == len(bufs_b) == len(sc.textures)
    for i, (x, y) in enumerate(zip(bufs_a, bufs_b)):
        assert ta[i].mip_count == tb[i].mip_count == len(sc.textures[i])
        assert np.array_equal(x.to_host(), y.to_host()), f"texture {i}"
    da, db = C.cast(a.draws, C.POINTER(abi.RasterDraw)), C.cast(b.draws, C.POINTER(abi.RasterDraw))
    assert [da[i].reserved for i in range(a.draw_count)] == [db[i].reserved for i in range(b.draw_count)]


def test_mirror_helpers_leave_what_the_entries_leave():
    """gen_mipmaps / clear_depth / clear_color / blit_image of util_passes.hpp, recorded and submitted through the frame, against
    vkr_gen_mipmaps / vkr_clear_image / vkr_blit_image called by hand on images of the same content"""
    frame = host.HostFrame(FrameSetup(64, 64), device=DEV)
    try:
        w, h = 300, 200
        mips = tr.mip_count(w, h)
        level0 = _rgba8(w, h, 21)
        frame.create_image("tex", abi.FMT_RGBA8_SRGB, w, h, mips)
        frame.create_image("half", abi.FMT_RGBA16_SFLOAT, w, h)
        frame.create_image("small", abi.FMT_RGBA8_SRGB, 100, 77)
        frame.create_image("zs", abi.FMT_D24_UNORM_S8, 40, 24, 3, 2)
        with pytest.raises(RuntimeError, match="is taken"):
            frame.create_image("depth", abi.FMT_R8_UNORM, 8, 8)
        with pytest.raises(RuntimeError, match="is taken"):
            frame.create_image("tex", abi.FMT_R8_UNORM, 8, 8)
        # gen_mipmaps
        seed = ImageBuf(abi.FMT_RGBA8_SRGB, w, h, mips, fill=POISON)
        seed.set_raw(level0, 0)
        frame.upload("tex", seed.to_host())
        frame.transfer(frame.TRANSFER_GEN_MIPMAPS, "tex")
        assert frame.last_tasks() == ["Genmips"] * (mips - 1)
        hand = _device_image(abi.FMT_RGBA8_SRGB, w, h, mips, level0)
        abi.gen_mipmaps(hand.desc())
        _sync()
        assert np.array_equal(frame.download("tex").to_host(), hand.to_host())
        # blit_image (LINEAR, like the reference)
        half_texels = tr.random_texels(tr.FMT_RGBA16_SFLOAT, w, h, 3)
        hb = ImageBuf(abi.FMT_RGBA16_SFLOAT, w, h, fill=POISON)
        hb.set_raw(half_texels, 0)
        frame.upload("half", hb.to_host())
        frame.transfer(frame.TRANSFER_BLIT, "half", dst="small")
        assert frame.last_tasks() == ["CopyImage"]
        src = _device_image(abi.FMT_RGBA16_SFLOAT, w, h, 1, half_texels)
        dst = _device_image(abi.FMT_RGBA8_SRGB, 100, 77)
        abi.blit_image(src.desc(), dst.desc(), abi.FILTER_LINEAR)
        _sync()
        assert np.array_equal(frame.download("small").raw(0), _raw(dst))
        # clear_color, every level
        frame.transfer(frame.TRANSFER_CLEAR_COLOR, "tex", value=(0.2, 0.4, 0.6, 0.8))
        assert frame.last_tasks() == ["Clear_color"]
        abi.clear_image(hand.desc(), (0.2, 0.4, 0.6, 0.8))
        _sync()
        got = frame.download("tex")
        for lv in range(mips):
            assert np.array_equal(got.raw(lv), _raw(hand, lv))
        # clear_depth, every level of every layer
        frame.transfer(frame.TRANSFER_CLEAR_DEPTH, "zs", value=0.25)
        assert frame.last_tasks() == ["Clear_depth"]
        word = tr.clear_texel(tr.FMT_D24_UNORM_S8, depth=0.25)[0]
        for layer in range(2):
            got = frame.download("zs", layer)
            for lv in range(3):
                assert np.all(got.raw(lv) == word), (layer, lv)
        with pytest.raises(RuntimeError, match="onto the source"):
            frame.transfer(frame.TRANSFER_BLIT, "tex", dst="tex")
        with pytest.raises(RuntimeError, match="D24_UNORM_S8"):
            frame.transfer(frame.TRANSFER_GEN_MIPMAPS, "zs")
    finally:
        frame.close()


def test_stage_clear_prev_depth():
    frame = host.HostFrame(FrameSetup(320, 180), device=DEV)
    try:
        frame.run(host.STAGE_LUT | host.STAGE_GBUFFER | host.STAGE_PREV_DEPTH)
        before = frame.download("prev_depth")
        assert not np.all(before.raw(0) == 0x00FFFFFF), "the synthetic prev_depth is not empty"
        frame.run(host.STAGE_CLEAR_PREV_DEPTH | host.STAGE_DOWNSAMPLE)
        assert frame.last_tasks()[0] == "Clear_depth" and "DownsampleGbuffer" in frame.last_tasks()
        after = frame.download("prev_depth")
        assert after.mips > 1
        for lv in range(after.mips):
            assert np.all(after.raw(lv) == 0x00FFFFFF), f"prev_depth mip {lv}"
    finally:
        frame.close()
