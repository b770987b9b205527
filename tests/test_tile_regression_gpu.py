"""Program tile_regression (advanced_ssr.cpp:497-538, advanced_ssr/regression.comp) on the GPU: parity with the numpy restatement
(tests/tile_regression_reference.py) BIT FOR BIT on every texel, the frame stage STAGE_TILE_REGRESSION, its refusal on a tiled
frame and the refusals of the entry.

Parity has no tolerance: the fit is badly conditioned in fp32 (tests/test_tile_regression.py: coefficients off by 0.01 against a
float64 fit), so the only meaningful expectation is the frozen operation order of DESIGN_NUMERICS.md (Tile regression), which
the restatement follows on the depth downloaded from the GPU.  Texels are compared as uint32; where both sides hold a NaN they
count as equal (the kernel and numpy need not agree on a NaN's sign and payload)."""
import ctypes as C

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.images import ImageBuf

import tile_regression_reference as ref

F32 = np.float32
FILL = 0xA5  # 0xA5A5A5A5 is a float (-2.87e-16) no tile produces in all four channels


def _arith():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


def _launch(depth_desc, push, out_w, out_h):
    """-> the texels [out_h, out_w, 4] as float32; checks that nothing outside the rows was written"""
    import torch

    out = ImageBuf(abi.FMT_RGBA32_SFLOAT, out_w, out_h, device="cuda", fill=FILL)
    abi.tile_regression(depth_desc, out.desc(), push, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host_bytes = out.to_host()
    rows = host_bytes[: out.pitch[0] * out_h].reshape(out_h, out.pitch[0])
    assert (rows[:, out_w * 16:] == FILL).all() and (host_bytes[out.pitch[0] * out_h:] == FILL).all(), "bytes outside the image were written"
    return out.raw(0, host_bytes)


def _compare(name, got, want):
    g, w = np.ascontiguousarray(got, F32).view(np.uint32), np.ascontiguousarray(want, F32).view(np.uint32)
    unwritten = (g == 0xA5A5A5A5).all(axis=-1)
    assert not unwritten.any(), f"{name}: {int(unwritten.sum())} texels were not written"
    bad = (g != w) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (f"{name}: {int(bad.any(axis=-1).sum())} of {bad.shape[0] * bad.shape[1]} texels differ, first at "
                           f"{tuple(np.argwhere(bad)[0])}: {got[bad][:8]} != {want[bad][:8]}")


def _upload_depth(bits):
    h, w = bits.shape
    staged = ImageBuf(abi.FMT_D24_UNORM_S8, w, h)
    staged.set_raw(np.ascontiguousarray(bits, np.uint32).reshape(h, w, 1), 0)
    depth = ImageBuf(abi.FMT_D24_UNORM_S8, w, h, device="cuda")
    depth.upload(staged.to_host())
    return depth


# frame cases: (W, H, source, [(out_w, out_h), ...]); the view is mip 1 of the frame's depth, (W / 2, H / 2)
FRAME_CASES = {
    "synth_256x144": (256, 144, "synth", [(16, 9)]),                   # view 128 x 72: whole tiles, 4 blocks across, 9 down
    "synth_250x142": (250, 142, "synth", [(15, 8), (16, 9)]),          # view 125 x 71: the reference's extent; partial right / bottom tiles
    "raster_640x360": (640, 360, "raster", [(40, 22), (40, 23)]),      # view 320 x 180: 10 blocks across; the reference's 22 rows and the partial 23rd
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(FRAME_CASES))
def test_parity_with_numpy_restatement(case):
    import torch

    W, H, source, outs = FRAME_CASES[case]
    setup = FrameSetup(W, H)
    frame = host.HostFrame(setup, device="cuda")
    try:
        if source == "raster":
            frame.load_scene(scn.procedural_scene(detail=16))
            frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE)
        else:
            frame.run(host.STAGE_GBUFFER | host.STAGE_DOWNSAMPLE)
        torch.cuda.synchronize()
        rt = frame.gtao_rt_params()  # camera_to_world = inverse(view), the matrix the frame stage hands over as transpose(normal_mat)
        push = abi.TileRegressionPush(rt.camera_to_world, *[float(v) for v in setup.fazz])
        cam = ref.mat4_to_np(rt.camera_to_world)
        depth_bits = frame.download("depth").raw(1)[..., 0]
        assert depth_bits.shape == (H // 2, W // 2)
        for ow, oh in outs:
            got = _launch(frame.image("depth", 1, 1), push, ow, oh)
            want = ref.tile_regression(_arith(), depth_bits, cam, *setup.fazz, ow, oh)
            differing = int(((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).any(axis=-1).sum())
            res = want[..., 3]
            print(f"[tile_regression] {case} out {ow}x{oh}: differing texels {differing}, finite planes {int(np.isfinite(want[..., :3]).all(axis=-1).sum())}"
                  f" of {ow * oh}, residual min {res.min():.3g} max {res.max():.3g}")
            _compare(f"{case} {ow}x{oh}", got, want)
    finally:
        frame.close()


HAND_CAMERA = np.array([[0.36, 0.48, -0.8, 3.0], [-0.8, 0.6, 0.0, -1.5], [0.48, 0.64, 0.6, 0.25], [0.0, 0.0, 0.0, 1.0]], F32)
HAND_FAZZ = (1.0, 16.0 / 9.0, 0.05, 80.0)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(9, 9), (1, 1)])
def test_parity_on_a_hand_made_depth(size):
    """9 x 9: four tiles, three of them with 56, 56 and 63 outside lanes, depth codes from near to the sky (0xFFFFFF) with
    stencil bits set; 1 x 1: one inside lane, a rank-one system (the plane is whatever IEEE makes of it, on both sides)"""
    w, h = size
    rng = np.random.default_rng(9)
    bits = rng.integers(0x800000, 0x1000000, (h, w)).astype(np.uint32)
    bits[0, 0] = 0xFFFFFF
    bits |= rng.integers(0, 256, (h, w)).astype(np.uint32) << 24
    depth = _upload_depth(bits)
    tw, th = ref.tiles_of(w, h)
    got = _launch(depth.desc(), abi.tile_regression_push(HAND_CAMERA, *HAND_FAZZ), tw, th)
    want = ref.tile_regression(_arith(), bits, HAND_CAMERA, *HAND_FAZZ, tw, th)
    print(f"[tile_regression] hand-made {w}x{h}: got {got.reshape(-1, 4).tolist()} want {want.reshape(-1, 4).tolist()}")
    _compare(f"hand-made {w}x{h}", got, want)


@pytest.mark.gpu
def test_frame_stage():
    import torch

    W, H = 256, 144
    setup = FrameSetup(W, H)
    frame = host.HostFrame(setup, device="cuda")
    try:
        frame.run(host.STAGE_GBUFFER | host.STAGE_DOWNSAMPLE | host.STAGE_TILE_REGRESSION)
        torch.cuda.synchronize()
        tasks = frame.last_tasks()
        assert tasks[-1] == "SSSR_Tile_Regression" and tasks.count("SSSR_Tile_Regression") == 1, tasks
        assert "DownsampleGbuffer" in tasks[:-1], tasks
        d = frame.image("tile_planes")
        assert (d.format, d.width, d.height, d.mip_count) == (abi.FMT_RGBA32_SFLOAT, W // 16, H // 16, 1)
        staged = frame.download("tile_planes").raw(0)
        depth_with = frame.download("depth").raw(0).copy()
        rt = frame.gtao_rt_params()
        push = abi.TileRegressionPush(rt.camera_to_world, *[float(v) for v in setup.fazz])
        direct = _launch(frame.image("depth", 1, 1), push, W // 16, H // 16)
        assert np.array_equal(staged.view(np.uint32), direct.view(np.uint32))
        assert np.isfinite(staged).any()
        # the chain after it is what it is without the stage
        frame.run(host.STAGE_LUT | host.STAGE_PREV_DEPTH)
        frame.run(host.STAGE_CHAIN)
        torch.cuda.synchronize()
        assert "SSSR_Tile_Regression" not in frame.last_tasks()
        taa_with = frame.download("taa_target").raw(0).copy()
    finally:
        frame.close()
    plain = host.HostFrame(setup, device="cuda")
    try:
        plain.run(host.STAGE_GBUFFER | host.STAGE_DOWNSAMPLE)
        plain.run(host.STAGE_LUT | host.STAGE_PREV_DEPTH)
        plain.run(host.STAGE_CHAIN)
        torch.cuda.synchronize()
        assert np.array_equal(plain.download("depth").raw(0), depth_with)
        assert np.array_equal(plain.download("taa_target").raw(0), taa_with)
        with pytest.raises(RuntimeError, match="'tile_planes' only exists after VKRH_STAGE_TILE_REGRESSION"):
            plain.image("tile_planes")
    finally:
        plain.close()


@pytest.mark.gpu
def test_frame_stage_is_refused_on_a_tiled_frame():
    W, H = 256, 144
    tiled = host.HostFrame(FrameSetup(W, H), device="cuda",
                           native_tiled=dict(rank=0, world=1, halo=48, gathered_mips=4, force_tiled=True, comm=None, row_bounds=None))
    try:
        with pytest.raises(RuntimeError, match="VKRH_STAGE_TILE_REGRESSION on a tiled frame"):
            tiled.run(host.STAGE_GBUFFER | host.STAGE_DOWNSAMPLE | host.STAGE_TILE_REGRESSION)
        assert "SSSR_Tile_Regression" not in tiled.last_tasks() and "DownsampleGbuffer" not in tiled.last_tasks()
    finally:
        tiled.close()


@pytest.mark.gpu
def test_refusals():
    """every case returns non-zero with a message before any launch; a valid call right afterwards works"""
    import torch

    lib = abi.product()
    W, H = 64, 36  # 8 x 5 tiles
    push = abi.tile_regression_push(HAND_CAMERA, *HAND_FAZZ)
    depth = ImageBuf(abi.FMT_D24_UNORM_S8, W, H, device="cuda", fill=0x7F)
    out = ImageBuf(abi.FMT_RGBA32_SFLOAT, 8, 5, device="cuda", fill=FILL)
    wrong_depth = ImageBuf(abi.FMT_R32_SFLOAT, W, H, device="cuda")
    wrong_out = ImageBuf(abi.FMT_RGBA16_SFLOAT, 8, 5, device="cuda")
    wide_out = ImageBuf(abi.FMT_RGBA32_SFLOAT, 9, 5, device="cuda")
    high_out = ImageBuf(abi.FMT_RGBA32_SFLOAT, 8, 6, device="cuda")
    window_depth = ImageBuf(abi.FMT_D24_UNORM_S8, W, H // 2, device="cuda", full=(W, H), origin=(0, 2))
    window_out = ImageBuf(abi.FMT_RGBA32_SFLOAT, 8, 2, device="cuda", full=(8, 5), origin=(0, 0))

    def edited(img, **fields):
        d = img.desc()
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    stream = torch.cuda.current_stream().cuda_stream
    good_d, good_o = depth.desc(), out.desc()
    cases = {
        "depth NULL": (None, good_o, push, "depth is NULL"),
        "out NULL": (good_d, None, push, "out_planes is NULL"),
        "push NULL": (good_d, good_o, None, "push is NULL"),
        "depth without memory": (edited(depth, base=None), good_o, push, "tile_regression.depth: NULL image"),
        "out without memory": (good_d, edited(out, base=None), push, "tile_regression.out_planes: NULL image"),
        "depth format": (wrong_depth.desc(), good_o, push, "tile_regression.depth: format"),
        "out format": (good_d, wrong_out.desc(), push, "tile_regression.out_planes: format"),
        "zero extent": (good_d, edited(out, width=0, full_width=0), push, "tile_regression.out_planes: bad layout"),
        "zero depth extent": (edited(depth, height=0, full_height=0), good_o, push, "tile_regression.depth: bad layout"),
        "out too wide": (good_d, wide_out.desc(), push, "a tile further out has no pixel"),
        "out too high": (good_d, high_out.desc(), push, "a tile further out has no pixel"),
        "windowed depth": (window_depth.desc(), good_o, push, "depth: windows are not supported"),
        "windowed out": (good_d, window_out.desc(), push, "out_planes: windows are not supported"),
    }
    for name, (d, o, p, message) in cases.items():
        rc = lib.vkr_tile_regression(C.byref(d) if d is not None else None, C.byref(o) if o is not None else None,
                                     C.byref(p) if p is not None else None, stream)
        assert rc != 0, name
        assert message in lib.vkr_last_error().decode(), (name, lib.vkr_last_error().decode())
        assert lib.vkr_tile_regression(C.byref(good_d), C.byref(good_o), C.byref(push), stream) == 0, name
    torch.cuda.synchronize()
    assert not (out.raw(0).view(np.uint32) == 0xA5A5A5A5).all(axis=-1).any()
