"""The octahedral probe programs cube2oct, probe_downsample and trace_probe (csrc/probe.hip) on the GPU, bit for bit against
the numpy restatement of tests/probe_reference.py.

The probes are baked from analytic cubes: every probe of a 4 x 4 grid sees the same box room around the procedural scene
(distance to the nearest wall per texel-centre direction, a colour per wall), converted by cube2oct and reduced by
probe_downsample on the GPU.  The trace runs on the procedural scene's rasterised G-buffer with the frame's own camera."""
import ctypes as C

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.images import ArrayImageBuf, ImageBuf

import probe_reference as ref

F32 = np.float32
ROOM_LO, ROOM_HI = np.array([-14.0, 0.0, -6.0]), np.array([14.0, 7.0, 14.0])
GRID, PMIN, PMAX = 4, (-6.0, 1.0, 0.0, 1.0), (6.0, 1.0, 12.0, 1.0)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch

    torch.cuda.synchronize()


def _ar():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


def _room_cube(pos, n):
    """6 faces (+X, -X, +Y, -Y, +Z, -Z) of n x n texels: sRGB colour codes of the wall hit first and its distance (fp16)"""
    j, i = np.mgrid[0:n, 0:n]
    sc, tc = (2 * i + 1 - n) / n, (2 * j + 1 - n) / n
    colors = np.zeros((6, n, n, 4), np.uint8)
    dist = np.zeros((6, n, n), np.float16)
    palette = np.array([[200, 60, 50, 255], [60, 200, 80, 255], [230, 220, 200, 255], [90, 90, 100, 255], [70, 90, 220, 255],
                        [220, 180, 40, 255]], np.uint8)
    for f in range(6):
        x, y, z = ref._face_dir(np.full(sc.shape, f), sc, tc, 1.0)
        d = np.stack([x, y, z], -1).astype(np.float64)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        with np.errstate(divide="ignore"):
            t = np.where(d > 0, (ROOM_HI - pos) / d, np.where(d < 0, (ROOM_LO - pos) / d, np.inf))
        axis = np.argmin(t, axis=-1)
        tmin = np.min(t, axis=-1)
        wall = 2 * axis + (np.take_along_axis(d, axis[..., None], -1)[..., 0] < 0)
        hitp = pos + d * tmin[..., None]
        checker = ((np.floor(hitp[..., 0]) + np.floor(hitp[..., 1]) + np.floor(hitp[..., 2])) % 2 == 0)
        c = palette[wall].astype(np.int32)
        c[..., :3] = np.where(checker[..., None], c[..., :3], c[..., :3] // 2)
        colors[f] = c.astype(np.uint8)
        dist[f] = tmin.astype(np.float16)
    return colors, dist


def _cube_bufs(colors, dist):
    n = colors.shape[1]
    cc, cd = [], []
    for f in range(6):
        a = ImageBuf(abi.FMT_RGBA8_SRGB, n, n)
        a.set_raw(colors[f])
        b = ImageBuf(abi.FMT_R16_SFLOAT, n, n)
        b.set_raw(dist[f][..., None])
        da, db = ImageBuf(abi.FMT_RGBA8_SRGB, n, n, device="cuda"), ImageBuf(abi.FMT_R16_SFLOAT, n, n, device="cuda")
        da.copy_from(a)
        db.copy_from(b)
        cc.append(da)
        cd.append(db)
    color_descs = (abi.VkrImg * 6)(*[b.desc() for b in cc])
    dist_descs = (abi.VkrImg * 6)(*[b.desc() for b in cd])
    return cc, cd, color_descs, dist_descs


def _bake(colors_dists, size):
    """cube2oct + probe_downsample of every probe into GPU arrays -> (colour array, depth array)"""
    lib = abi.product()
    layers = len(colors_dists)
    mips = int(np.floor(np.log2(size))) + 1
    color = ArrayImageBuf(abi.FMT_RGBA8_UNORM, size, size, layers, device="cuda")
    depth = ArrayImageBuf(abi.FMT_R16_UNORM, size, size, layers, mips=mips, device="cuda")
    for layer, (cols, dist) in enumerate(colors_dists):
        keep = _cube_bufs(cols, dist)
        one = depth.desc(layer)
        one0 = abi.VkrImg.from_buffer_copy(one)
        one0.mip_count = 1
        abi.check(lib.vkr_cube2oct(keep[2], keep[3], C.byref(color.desc(layer)), C.byref(one0), _stream()), lib)
        abi.check(lib.vkr_probe_downsample(C.byref(one), _stream()), lib)
        _sync()
    return color, depth


def _probe_positions():
    step = (np.array(PMAX[:3], F32) - np.array(PMIN[:3], F32)) / F32(GRID - 1)
    return [np.array(PMIN[:3], np.float64) + step.astype(np.float64) * np.array([x, 0, y]) for y in range(GRID) for x in range(GRID)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,W,H", [(32, 64, 64), (16, 70, 38)])
def test_cube2oct_random_cubes(n, W, H):
    """random seeded cube contents exercise every seam and corner rule; only the dispatch extent is written"""
    lib = abi.product()
    rng = np.random.default_rng(7 + n)
    colors = rng.integers(0, 256, (6, n, n, 4), dtype=np.uint8)
    dist = rng.uniform(0.01, 100.0, (6, n, n)).astype(np.float16)
    keep = _cube_bufs(colors, dist)
    oc, od = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda", fill=0xA5), ImageBuf(abi.FMT_R16_UNORM, W, H, device="cuda", fill=0xA5)
    abi.check(lib.vkr_cube2oct(keep[2], keep[3], C.byref(oc.desc()), C.byref(od.desc()), _stream()), lib)
    _sync()
    got_c, got_d = oc.raw(0), od.raw(0)[..., 0]
    want_c, want_d = ref.cube2oct(_ar(), colors, dist, W, H)
    tw, th = W // 8 * 8, H // 4 * 4
    assert np.array_equal(got_c[:th, :tw], want_c), f"colour: {(got_c[:th, :tw] != want_c).any(-1).sum()} texels differ"
    assert np.array_equal(got_d[:th, :tw], want_d), f"depth: {(got_d[:th, :tw] != want_d).sum()} texels differ"
    assert (got_c[th:] == 0xA5).all() and (got_c[:, tw:] == 0xA5).all(), "texels outside the dispatch extent were written"


@pytest.mark.gpu
def test_cube2oct_room_bake():
    lib = abi.product()
    colors, dist = _room_cube(_probe_positions()[5], 64)
    keep = _cube_bufs(colors, dist)
    oc, od = ImageBuf(abi.FMT_RGBA8_UNORM, 256, 256, device="cuda"), ImageBuf(abi.FMT_R16_UNORM, 256, 256, device="cuda")
    abi.check(lib.vkr_cube2oct(keep[2], keep[3], C.byref(oc.desc()), C.byref(od.desc()), _stream()), lib)
    _sync()
    want_c, want_d = ref.cube2oct(_ar(), colors, dist, 256, 256)
    assert np.array_equal(oc.raw(0), want_c)
    assert np.array_equal(od.raw(0)[..., 0], want_d)
    assert len(np.unique(want_d)) > 500


@pytest.mark.gpu
@pytest.mark.parametrize("size", [256, 45])
def test_probe_downsample(size):
    lib = abi.product()
    mips = int(np.floor(np.log2(size))) + 1
    rng = np.random.default_rng(size)
    mip0 = rng.integers(0, 65536, (size, size), dtype=np.uint16)
    hostbuf = ImageBuf(abi.FMT_R16_UNORM, size, size, mips=mips)
    hostbuf.set_raw(mip0[..., None])
    dev = ImageBuf(abi.FMT_R16_UNORM, size, size, mips=mips, device="cuda")
    dev.copy_from(hostbuf)
    abi.check(lib.vkr_probe_downsample(C.byref(dev.desc()), _stream()), lib)
    _sync()
    want = ref.probe_downsample(mip0, mips)
    host_bytes = dev.to_host()
    for m in range(mips):
        assert np.array_equal(dev.raw(m, host_bytes)[..., 0], want[m]), f"mip {m}"


def _raster_frame(W, H):
    setup = FrameSetup(W, H)
    frame = host.HostFrame(setup, device="cuda")
    frame.load_scene(scn.procedural_scene(detail=16))
    frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE)
    _sync()
    return frame


def _consts(params, grid=GRID):
    c = abi.ProbeTraceConsts()
    c.inverse_view = params.camera_to_world
    for k in range(4):
        c.probe_min[k], c.probe_max[k] = PMIN[k], PMAX[k]
    c.grid_size = grid
    c.fovy, c.aspect, c.znear, c.zfar = params.fovy, params.aspect, params.znear, params.zfar
    return c


def _trace(frame, color, depth, consts, W, H):
    lib = abi.product()
    out = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda", fill=0x5A)
    rc = lib.vkr_trace_probe(C.byref(frame.image("depth")), C.byref(frame.image("normal")), color.descs(), depth.descs(), color.layers,
                             C.byref(consts), C.byref(out.desc()), _stream())
    abi.check(rc, lib)
    _sync()
    return out.raw(0)


def _restate(frame, color, depth, params, W, H):
    depth_bits = frame.download("depth").raw(0)[..., 0]
    normal_codes = frame.download("normal").raw(0)
    hb = depth.to_host()
    pa = ref.ProbeArrays(color.raw(0), [depth.raw(m, hb)[..., 0] for m in range(depth.mips)])
    M = np.array(params.camera_to_world.m, F32).reshape(4, 4).T
    return ref.trace_probe(_ar(), depth_bits, normal_codes, pa, M, PMIN, PMAX, GRID, params.fovy, params.aspect, params.znear,
                           params.zfar, W, H)


@pytest.fixture(scope="module")
def room_probes():
    color, depth = _bake([_room_cube(p, 64) for p in _probe_positions()], 128)
    return color, depth


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(256, 144), (640, 360), (252, 142)])
def test_trace_probe_parity(room_probes, W, H):
    """252 x 142 has a tail past the dispatch extent (248 x 140) that must stay untouched"""
    color, depth = room_probes
    frame = _raster_frame(W, H)
    try:
        params = frame.gtao_rt_params()
        got = _trace(frame, color, depth, _consts(params), W, H)
        want, result, traced = _restate(frame, color, depth, params, W, H)
        tw, th = W // 8 * 8, H // 4 * 4
        diff = (got[:th, :tw] != want).any(-1)
        assert not diff.any(), f"{int(diff.sum())} of {tw * th} pixels differ"
        assert (got[th:] == 0x5A).all() and (got[:, tw:] == 0x5A).all()
        assert (result == ref.HIT).sum() > 0, "some rays hit"
        assert ((result == ref.MISS) | (result == ref.UNKNOWN)).sum() > 0, "some rays do not"
        assert (traced > 1).sum() > 0, "some rays fall back to another probe (UNKNOWN)"
    finally:
        frame.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_trace_probe_constant_probes_known_answer(fill):
    """Known answer: every probe colour texel is one colour C, so a hit stores C (the bilinear filter of a constant rounds
    back to its code) and everything else stores 0: each pixel is 0 or C.  Every probe depth is at the near plane (code 0)
    or at the far plane (code 65535).  Neither is the all-zero image that "nothing in front of the ray" suggests: the trace
    calls a stop a hit when it lies within the hit bias (0.0005) of the sampled depth, and with a constant depth that
    happens for rays that start next to a probe (near plane) or march to depth ~1 (far plane).  So both images must hold
    C somewhere, and agree with the restatement bit for bit."""
    W, H = 256, 144
    C_CODE = np.array([37, 201, 90, 255], np.uint8)
    layers = GRID * GRID
    mips = int(np.floor(np.log2(128))) + 1
    color = ArrayImageBuf(abi.FMT_RGBA8_UNORM, 128, 128, layers, device="cuda")
    import torch

    color.tensor.copy_(torch.from_numpy(np.resize(C_CODE, color.nbytes)))
    depth = ArrayImageBuf(abi.FMT_R16_UNORM, 128, 128, layers, mips=mips, device="cuda", fill=fill)
    frame = _raster_frame(W, H)
    try:
        params = frame.gtao_rt_params()
        got = _trace(frame, color, depth, _consts(params), W, H)
        is_zero = (got == 0).all(-1)
        is_c = (got == C_CODE).all(-1)
        assert (is_zero | is_c).all(), "a pixel that is neither 0 nor the probes' colour"
        assert is_c.sum() > 0 and is_zero.sum() > 0
        want, result, _ = _restate(frame, color, depth, params, W, H)
        assert np.array_equal(got, want)
        assert np.array_equal(is_c, result == ref.HIT)
    finally:
        frame.close()


@pytest.mark.gpu
def test_trace_probe_refusals(room_probes):
    color, depth = room_probes
    W, H = 64, 32
    frame = _raster_frame(W, H)
    lib = abi.product()
    try:
        params = frame.gtao_rt_params()
        out = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda")
        args = lambda c, layers, o: (C.byref(frame.image("depth")), C.byref(frame.image("normal")), color.descs(), depth.descs(), layers,
                                     C.byref(c), C.byref(o.desc()), _stream())
        assert lib.vkr_trace_probe(*args(_consts(params, grid=1), 16, out)) != 0
        assert lib.vkr_trace_probe(*args(_consts(params), 15, out)) != 0
        bad = ImageBuf(abi.FMT_RGBA8_UNORM, W // 2, H, device="cuda")
        assert lib.vkr_trace_probe(*args(_consts(params), 16, bad)) != 0
        wrong = ImageBuf(abi.FMT_RGBA16_SFLOAT, W, H, device="cuda")
        assert lib.vkr_trace_probe(*args(_consts(params), 16, wrong)) != 0
        no_mips = depth.descs()
        for k in range(depth.layers):
            no_mips[k].mip_count = 0
        rc = lib.vkr_trace_probe(C.byref(frame.image("depth")), C.byref(frame.image("normal")), color.descs(), no_mips, 16,
                                 C.byref(_consts(params)), C.byref(out.desc()), _stream())
        assert rc != 0 and b"mips" in lib.vkr_last_error()
        assert lib.vkr_trace_probe(*args(_consts(params), 16, out)) == 0
        _sync()
    finally:
        frame.close()
