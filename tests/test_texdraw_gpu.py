"""Program texdraw (backbuffer_subpass2.cpp:15-52, texdraw/shader.frag) on the GPU: vkr_texdraw against the numpy restatement
(tests/texdraw_reference.py) as raw bytes, zero differing texels allowed, for every source format, both backbuffer formats, equal
extents, down- and up-scales, sources one texel wide or high, every channel flag and non-finite fp16 input; the sRGB encode's
self-test over all 2^32 bit patterns; and the frame stage STAGE_BACKBUFFER."""
import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.images import ImageBuf

import texdraw_reference as ref
import transfer_reference as tr

F32 = np.float32
FILL = 0xA5


def _contract():
    return int(abi.product().vkr_numeric_contract())


def _device_image(fmt, texels):
    h, w = texels.shape[:2]
    staged = ImageBuf(fmt, w, h)
    staged.set_raw(texels, 0)
    img = ImageBuf(fmt, w, h, device="cuda")
    img.upload(staged.to_host())
    return img


def _draw(src_desc, dst_fmt, dw, dh, flags):
    """-> the stored bytes [dh, dw, 4]; checks that nothing outside the rows was written"""
    import torch

    out = ImageBuf(dst_fmt, dw, dh, device="cuda", fill=FILL)
    abi.texdraw(src_desc, out.desc(), abi.texdraw_push(flags), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host_bytes = out.to_host()
    rows = host_bytes[: out.pitch[0] * dh].reshape(dh, out.pitch[0])
    assert (rows[:, dw * 4:] == FILL).all() and (host_bytes[out.pitch[0] * dh:] == FILL).all(), "bytes outside the image were written"
    return out.raw(0, host_bytes)


def _check(name, src_fmt, texels, dst_fmt, dw, dh, flags=0):
    src = _device_image(src_fmt, texels)  # kept alive: its memory must not be handed to the backbuffer
    got = _draw(src.desc(), dst_fmt, dw, dh, flags)
    del src
    want = ref.texdraw(texels, src_fmt, dw, dh, dst_fmt, flags, _contract())
    bad = (got != want).any(axis=-1)
    print(f"[texdraw] {name}: differing texels {int(bad.sum())} of {bad.size}")
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} texels differ, first at {tuple(np.argwhere(bad)[0])}: {got[bad][:4]} != {want[bad][:4]}"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("src_fmt", tr.COLOR_FORMATS)
def test_every_source_format(src_fmt):
    """the eleven colour formats, 64 x 36 -> 64 x 36 RGBA8_SRGB, all channels"""
    assert len(tr.COLOR_FORMATS) == 11
    texels = tr.random_texels(src_fmt, 64, 36, seed=100 + src_fmt)
    _check(f"format {src_fmt}", src_fmt, texels, tr.FMT_RGBA8_SRGB, 64, 36)


SIZES = {
    "equal_250x142": ((250, 142), (250, 142)),   # ends inside a block; 3910 pixel centres with a non-zero fraction
    "down_2_1": ((256, 144), (128, 72)),
    "up_1_2": ((128, 72), (256, 144)),
    "odd_257x129_to_100x77": ((257, 129), (100, 77)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("dst_fmt", [tr.FMT_RGBA8_SRGB, tr.FMT_RGBA8_UNORM])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_final_frame_pair(size, dst_fmt):
    (sw, sh), (dw, dh) = SIZES[size]
    texels = tr.random_texels(tr.FMT_RGBA16_SFLOAT, sw, sh, seed=7)
    got = _check(f"{size} -> format {dst_fmt}", tr.FMT_RGBA16_SFLOAT, texels, dst_fmt, dw, dh)
    assert len(np.unique(got[..., 0])) > 100  # the case is no constant image


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["1x1_to_5x3", "1x9_to_4x9", "3x3_to_1x1", "2x2_to_7x5", "9x1_to_9x4"])
def test_tiny_sources(case):
    """a source one texel wide takes the unpaired loads; two texels wide is the narrowest pair; one texel high clamps both rows"""
    (sw, sh), (dw, dh) = [tuple(int(v) for v in part.split("x")) for part in case.split("_to_")]
    for fmt in (tr.FMT_RGBA16_SFLOAT, tr.FMT_R8_UNORM, tr.FMT_RGBA32_SFLOAT, tr.FMT_R16_UNORM):
        texels = tr.random_texels(fmt, sw, sh, seed=31)
        _check(f"{case} format {fmt}", fmt, texels, tr.FMT_RGBA8_SRGB, dw, dh)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [1, 2, 4, 8, 15, 3, 16])
@pytest.mark.parametrize("src_fmt", [tr.FMT_R8_UNORM, tr.FMT_RGBA16_SFLOAT])
def test_channel_flags(src_fmt, flags):
    """AO shown with ShowR: R8_UNORM's absent channels are 0, 0, 0, 1, so G and B show black and A white"""
    texels = tr.random_texels(src_fmt, 40, 24, seed=5)
    got = _check(f"format {src_fmt} flags {flags}", src_fmt, texels, tr.FMT_RGBA8_SRGB, 50, 30, flags)
    if src_fmt == tr.FMT_R8_UNORM and flags in (2, 4):
        assert not got.any()
    if src_fmt == tr.FMT_R8_UNORM and flags in (8, 15):
        assert (got == 255).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dst_fmt", [tr.FMT_RGBA8_SRGB, tr.FMT_RGBA8_UNORM])
def test_non_finite_and_out_of_range_fp16(dst_fmt):
    """NaN, +-inf, negative values and values above 1: NaN stores 0, the others clamp; a NaN or inf tap poisons its neighbours'
    mixes exactly as IEEE makes them (0 * inf is NaN)"""
    rng = np.random.default_rng(17)
    vals = rng.uniform(-2.0, 3.0, (24, 40, 4)).astype(np.float16)
    pick = rng.random(vals.shape)
    vals[pick < 0.05] = np.nan
    vals[(pick >= 0.05) & (pick < 0.08)] = np.inf
    vals[(pick >= 0.08) & (pick < 0.11)] = -np.inf
    vals[(pick >= 0.11) & (pick < 0.14)] = 65504.0
    vals[(pick >= 0.14) & (pick < 0.17)] = -0.0
    vals[(pick >= 0.17) & (pick < 0.20)] = 6e-8  # an fp16 denormal
    for (dw, dh) in ((40, 24), (64, 36)):
        for flags in (0, 8):
            _check(f"non-finite -> {dw}x{dh} format {dst_fmt} flags {flags}", tr.FMT_RGBA16_SFLOAT, vals, dst_fmt, dw, dh, flags)


@pytest.mark.gpu
def test_fast_srgb_encode_equals_the_search_on_every_bit_pattern():
    import torch

    lib = abi.product()
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    abi.check(lib.vkr_selftest_srgb_encode(counter.data_ptr(), torch.cuda.current_stream().cuda_stream), lib)
    torch.cuda.synchronize()
    print(f"[texdraw] sRGB encode disagreements over 2^32 bit patterns: {int(counter.item())}")
    assert int(counter.item()) == 0


@pytest.mark.gpu
def test_frame_stage():
    import torch

    W, H = 256, 144
    setup = FrameSetup(W, H)
    stream = torch.cuda.current_stream().cuda_stream
    frame = host.HostFrame(setup, device="cuda")
    try:
        with pytest.raises(RuntimeError, match="'backbuffer' only exists after"):
            frame.image("backbuffer")
        frame.run(host.STAGE_GBUFFER)
        frame.run(host.STAGE_LUT | host.STAGE_PREV_DEPTH)
        frame.run(host.STAGE_CHAIN | host.STAGE_BACKBUFFER)
        torch.cuda.synchronize()
        tasks = frame.last_tasks()
        assert tasks[-2:] == ["BackbufSubpass", "presentPrepare"] and tasks[-3] == "TAA", tasks
        d = frame.image("backbuffer")
        assert (d.format, d.width, d.height) == (abi.FMT_RGBA8_SRGB, W, H)
        staged = frame.download("backbuffer").raw(0).copy()
        depth_with = frame.download("depth").raw(0).copy()
        taa_img = frame.download("taa_target")
        taa_with = taa_img.raw(0).copy()
        # the stage equals the entry called by hand on the TAA output
        direct = _draw(frame.image("taa_target", 0, 1), abi.FMT_RGBA8_SRGB, W, H, 0)
        assert np.array_equal(staged, direct)
        want = ref.texdraw(taa_with, taa_img.format, W, H, tr.FMT_RGBA8_SRGB, 0, _contract())
        assert np.array_equal(staged, want)
        assert len(np.unique(staged[..., :3])) > 50  # a picture, not a constant

        # the debug view: the accumulated AO with ShowR at half the extent
        frame.set_backbuffer("acc_ao", abi.TEXDRAW_SHOW_R, W // 2, H // 2)
        frame.run(host.STAGE_BACKBUFFER)
        torch.cuda.synchronize()
        assert frame.last_tasks() == ["BackbufSubpass", "presentPrepare"]
        d = frame.image("backbuffer")
        assert (d.format, d.width, d.height) == (abi.FMT_RGBA8_SRGB, W // 2, H // 2)
        ao = frame.download("acc_ao")
        got = frame.download("backbuffer").raw(0)
        want = ref.texdraw(ao.raw(0), ao.format, W // 2, H // 2, tr.FMT_RGBA8_SRGB, ref.SHOW_R, _contract())
        bad = (got != want).any(axis=-1)
        assert not bad.any(), f"{int(bad.sum())} texels differ"
        assert (got[..., 0] == got[..., 1]).all() and (got[..., 0] == got[..., 2]).all() and len(np.unique(got[..., 3])) > 4

        # refused settings leave the configuration alone
        for args, message in ((("no_such_image", 0, 0, 0), "unknown image 'no_such_image'"), (("depth", 0, 0, 0), "'depth' is a depth image"),
                              (("backbuffer", 0, 0, 0), "cannot be its own source"), ((None, 0, 64, 0), "extent 64x0"),
                              ((None, 0, 70000, 8), "extent 70000x8")):
            with pytest.raises(RuntimeError, match=message):
                frame.set_backbuffer(*args)
        frame.run(host.STAGE_BACKBUFFER)
        torch.cuda.synchronize()
        assert np.array_equal(frame.download("backbuffer").raw(0), got)
    finally:
        frame.close()
    del stream
    plain = host.HostFrame(setup, device="cuda")
    try:
        plain.run(host.STAGE_GBUFFER)
        plain.run(host.STAGE_LUT | host.STAGE_PREV_DEPTH)
        plain.run(host.STAGE_CHAIN)
        torch.cuda.synchronize()
        assert np.array_equal(plain.download("depth").raw(0), depth_with)
        assert np.array_equal(plain.download("taa_target").raw(0), taa_with)
    finally:
        plain.close()


@pytest.mark.gpu
def test_frame_stage_is_refused_on_a_tiled_frame():
    W, H = 256, 144
    tiled = host.HostFrame(FrameSetup(W, H), device="cuda",
                           native_tiled=dict(rank=0, world=1, halo=48, gathered_mips=4, force_tiled=True, comm=None, row_bounds=None))
    try:
        with pytest.raises(RuntimeError, match="VKRH_STAGE_BACKBUFFER on a tiled frame"):
            tiled.run(host.STAGE_GBUFFER | host.STAGE_BACKBUFFER)
        assert "BackbufSubpass" not in tiled.last_tasks()
        with pytest.raises(RuntimeError, match="vkrh_set_backbuffer: on a tiled frame"):
            tiled.set_backbuffer("albedo")
    finally:
        tiled.close()
