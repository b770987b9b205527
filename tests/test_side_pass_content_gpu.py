"""ssao, tile_regression, gtao_rt_main and trace_probe on the GPU under the adversarial content of tests/side_pass_content.py: each
kernel against its numpy restatement, at the smallest extents at which its structure can still go wrong.  What the classes reach
and that they can tell a wrong kernel from a right one is proven on the CPU (tests/test_side_pass_content.py); here the kernels
are held to the restatements on that content: bit for bit (ssao, trace_probe), as uint32 with NaN == NaN (tile_regression),
under the rule of tests/parity.py with no exception (gtao_rt_main, as its own parity test).  stencil_noise must also give the
bytes of raster: the top byte of a D24S8 word is not depth.

Measured on an MI355X: 0 differing texels in all 313 cases, no kernel and no restatement had to change.
ssao: 60 cases (10 classes x depth 70 x 38 -> 70 x 38, 35 x 19 -> 37 x 21, 1 x 19 -> 5 x 3 x fixed / eye_plane samples), 0 of
69 040 texels differ, the 3 452 non-finite sample coordinates of near_all / eye_plane and the 803 of near_codes included.
tile_regression: 54 cases (9 classes x views 35 x 19, 16 x 8, 33 x 9 x the frame's and the hand-made camera), 0 of 486 tiles
differ as uint32 with NaN == NaN; 6 of them hold a NaN plane and the residual 1e10.
gtao_rt_main: 88 cases (11 classes x 35 x 19, 9 x 5 x rotations 0.0, 0.3 x the 3076-triangle scene and the empty structure),
31 240 texels, all bit-equal; sky pixels are (0, 1, 0, 0), the bytes outside the rows keep their fill.
trace_probe: 108 cases (18 (G-buffer, probe) pairs x 70 x 38, 24 x 12 x grids 4 / 16 layers, 3 / 16, 2 / 4), 0 of 139 968 texels
of the dispatch extents differ, the fill outside them is untouched; the room probes the two bake kernels produce are the
restated ones byte for byte (3 cases).
The file takes 7.0 s on the MI355X, restatements included (the slowest case 0.35 s)."""
import ctypes as C
import functools

import numpy as np
import pytest

from vk_renderer_amd import abi
from vk_renderer_amd.images import ArrayImageBuf, ImageBuf

import probe_reference as probe_ref
import side_pass_content as sp
import test_gtao_rt_gpu as ao_gpu
import test_probe_gpu as probe_gpu
import test_ssao_gpu as ssao_gpu
import test_tile_regression_gpu as tile_gpu
from parity import report

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0x5A


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch

    torch.cuda.synchronize()


def _device(fmt, w, h, host_bytes, mips=1):
    img = ImageBuf(fmt, w, h, mips, device="cuda")
    img.upload(np.array(host_bytes))  # a copy: the cached inputs are read-only
    return img


def _size_id(s):
    return f"{s[0]}x{s[1]}"


# ---- ssao -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sp.SSAO_SAMPLE_SETS)
@pytest.mark.parametrize("sizes", sp.SSAO_SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}_out_{s[1][0]}x{s[1][1]}")
@pytest.mark.parametrize("name", list(sp.SSAO_CLASSES))
def test_ssao(name, sizes, which):
    depth_size, (ow, oh) = sizes
    _, _, setup, depth_bytes, _ = sp.inputs("ssao", name, depth_size)
    want, counts, stats = sp.ssao_expected(name, depth_size, (ow, oh), which)
    depth = _device(abi.FMT_D24_UNORM_S8, depth_size[0], depth_size[1], depth_bytes)
    got = ssao_gpu._launch(depth.desc(), ssao_gpu._params(setup, sp.ssao_samples(which)), ow, oh)
    print(f"[side ssao] {name} depth {depth_size} out {(ow, oh)} {which}: non-finite sample_uv {stats['nonfinite_sample_uv']} of {stats['taps']} taps, "
          f"differing texels {int((got != want).sum())}")
    ssao_gpu._compare(f"{name} {depth_size} {which}", got, want)
    if name == "stencil_noise":
        ssao_gpu._compare("stencil_noise against raster", got, sp.ssao_expected("raster", depth_size, (ow, oh), which)[0])


# ---- tile regression --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", sp.TILE_CAMERAS)
@pytest.mark.parametrize("size", sp.TILE_SIZES, ids=_size_id)
@pytest.mark.parametrize("name", list(sp.DEPTH_CLASSES))
def test_tile_regression(name, size, camera):
    words, _, setup, _, _ = sp.inputs("tile_regression", name, size, 1)
    want = sp.tile_expected(name, size, camera)
    cam, fazz = sp.tile_camera(camera, setup)
    depth = tile_gpu._upload_depth(words)
    got = tile_gpu._launch(depth.desc(), abi.tile_regression_push(cam, *fazz), want.shape[1], want.shape[0])
    differing = int(((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).any(axis=-1).sum())
    finite, nan, big = sp.tile_counts(want)
    print(f"[side tile_regression] {name} view {size} {camera}: finite {finite}, NaN {nan}, residual 1e10 {big} of {want.shape[0] * want.shape[1]} "
          f"tiles, differing texels {differing}")
    tile_gpu._compare(f"{name} {size} {camera}", got, want)
    if name == "stencil_noise":
        tile_gpu._compare("stencil_noise against raster", got, sp.tile_expected("raster", size, camera))


# ---- traced AO --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ao_accel(which):
    return abi.Accel(sp.ao_triangles(which))


@functools.lru_cache(maxsize=None)
def _ao_directions():
    dirs, dirs_dev = ao_gpu._directions_device()
    assert np.array_equal(dirs, sp.ao_directions()), "the restatement's directions are not the host library's"
    return dirs_dev


def _ao_launch(name, size, rotation, scene):
    """-> float16 [h, w, 4] of vkr_gtao_rt_main; checks that nothing outside the rows was written"""
    w, h = size
    words, _, setup, _, normal_bytes = sp.inputs("gtao_rt", name, size, 1)
    # the depth the pass is handed: the mip-1 view of a G-buffer depth of twice the extent (mip 0 is not read)
    staged = ImageBuf(abi.FMT_D24_UNORM_S8, 2 * w, 2 * h, 2)
    staged.set_raw(words.reshape(h, w, 1), 1)
    depth = _device(abi.FMT_D24_UNORM_S8, 2 * w, 2 * h, staged.to_host(), mips=2)
    normal = _device(abi.FMT_RG16_UNORM, 2 * w, 2 * h, normal_bytes)
    cam, fovy, aspect, znear, zfar = sp.ao_camera(setup)
    params = abi.GtaoRtParams(abi.Mat4.from_np(cam), fovy, aspect, znear, zfar)
    out = ImageBuf(abi.FMT_RGBA16_SFLOAT, w, h, device="cuda", fill=FILL)
    got = ao_gpu._launch(params, depth.desc(1, 1), normal.desc(), _ao_accel(scene), _ao_directions(), out, rotation)
    host_bytes = out.to_host()
    rows = host_bytes[: out.pitch[0] * h].reshape(h, out.pitch[0])
    assert (rows[:, 8 * w:] == FILL).all() and (host_bytes[out.pitch[0] * h:] == FILL).all(), "bytes outside the image were written"
    return got


@pytest.mark.parametrize("scene", sp.AO_SCENES)
@pytest.mark.parametrize("rotation", sp.AO_ROTATIONS)
@pytest.mark.parametrize("size", sp.AO_SIZES, ids=_size_id)
@pytest.mark.parametrize("name", list(sp.CLASSES))
def test_traced_ao(name, size, rotation, scene):
    w, h = size
    want = sp.ao_expected(name, size, rotation, scene)
    got = _ao_launch(name, size, rotation, scene)
    n, _ = report(f"side gtao_rt {name} {w}x{h} {rotation} {scene}", abi.FMT_RGBA16_SFLOAT, got.astype(F32), want.astype(F32))
    assert n == 0
    sky = sp.ao_sky(name, size)
    assert np.array_equal(got[sky].view(np.uint16), np.tile(np.array([0, 1, 0, 0], np.float16).view(np.uint16), (int(sky.sum()), 1)))
    assert (got[~sky][:, 1] == 1).all()
    if name == "stencil_noise":  # exactly the bytes of raster: the kernel's own image of it
        assert np.array_equal(got.view(np.uint16), _ao_launch("raster", size, rotation, scene).view(np.uint16)), "the stencil byte changes the image"


# ---- probe trace ------------------------------------------------------------------------------------------------------------------
def _upload_array(fmt, per_mip):
    """per_mip: [layers, h_m, w_m(, c)] arrays of the storage dtype, one per mip -> ArrayImageBuf on the device"""
    import torch

    layers, h, w = per_mip[0].shape[:3]
    staged = ArrayImageBuf(fmt, w, h, layers, mips=len(per_mip))
    for m, a in enumerate(per_mip):
        hm, wm = a.shape[1:3]
        rows = staged.host[staged.offset[m]: staged.offset[m] + staged.pitch[m] * hm * layers].reshape(layers, hm, staged.pitch[m])
        rows[:, :, : wm * staged.bpp] = np.ascontiguousarray(a).view(np.uint8).reshape(layers, hm, wm * staged.bpp)
    dev = ArrayImageBuf(fmt, w, h, layers, mips=len(per_mip), device="cuda")
    dev.tensor.copy_(torch.from_numpy(staged.host))
    return dev


@functools.lru_cache(maxsize=None)
def _probes_device(pname, grid, layers):
    colour, depth = sp.probes(pname, grid, layers)
    return _upload_array(abi.FMT_RGBA8_UNORM, [colour]), _upload_array(abi.FMT_R16_UNORM, depth)


@pytest.mark.parametrize("grid,layers", sp.GRIDS)
def test_room_probes_baked_on_the_gpu_are_the_restated_ones(grid, layers):
    """the room probes of the trace tests come from the restatements of cube2oct and probe_downsample (the CPU tests need them
    too); the two kernels bake the same bytes"""
    color, depth = probe_gpu._bake(sp.room_cubes(grid, layers), sp.PROBE_SIZE)
    assert depth.mips == sp.PROBE_MIPS
    want_colour, want_depth = sp.room_probes_host(grid, layers)
    assert np.array_equal(color.raw(0), want_colour)
    hb = depth.to_host()
    for m in range(depth.mips):
        assert np.array_equal(depth.raw(m, hb)[..., 0], want_depth[m]), f"mip {m}"


@pytest.mark.parametrize("grid,layers", sp.GRIDS)
@pytest.mark.parametrize("size", sp.PROBE_SIZES, ids=_size_id)
@pytest.mark.parametrize("gname,pname", sp.PROBE_CASES)
def test_probe_trace(gname, pname, size, grid, layers):
    W, H = size
    _, _, setup, depth_bytes, normal_bytes = sp.inputs("trace_probe", gname, size)
    want, result, traced, past = sp.probe_expected(gname, size, pname, grid, layers)
    colour, pdepth = _probes_device(pname, grid, layers)
    depth = _device(abi.FMT_D24_UNORM_S8, W, H, depth_bytes)
    normal = _device(abi.FMT_RG16_UNORM, W, H, normal_bytes)
    consts = abi.ProbeTraceConsts()
    consts.inverse_view = abi.Mat4.from_np(setup.inv_view)
    for k in range(4):
        consts.probe_min[k], consts.probe_max[k] = sp.PMIN[k], sp.PMAX[k]
    consts.grid_size = grid
    consts.fovy, consts.aspect, consts.znear, consts.zfar = [float(v) for v in setup.fazz]
    out = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda", fill=FILL)
    lib = abi.product()
    abi.check(lib.vkr_trace_probe(C.byref(depth.desc()), C.byref(normal.desc()), colour.descs(), pdepth.descs(), layers, C.byref(consts),
                                  C.byref(out.desc()), _stream()), lib)
    _sync()
    host_bytes = out.to_host()
    rows = host_bytes[: out.pitch[0] * H].reshape(H, out.pitch[0])
    assert (rows[:, 4 * W:] == FILL).all() and (host_bytes[out.pitch[0] * H:] == FILL).all(), "bytes outside the image were written"
    got = out.raw(0, host_bytes)
    th, tw = want.shape[:2]
    differing = int((got[:th, :tw] != want).any(-1).sum())
    print(f"[side trace_probe] {gname} / {pname} {size} grid {grid} ({layers} layers): HIT {int((result == probe_ref.HIT).sum())}, MISS "
          f"{int((result == probe_ref.MISS).sum())}, UNKNOWN {int((result == probe_ref.UNKNOWN).sum())}, traced > 1 {int((traced > 1).sum())}, "
          f"past the last mip {past}, differing texels {differing} of {tw * th}")
    assert differing == 0, f"{differing} of {tw * th} texels differ, first at {tuple(np.argwhere((got[:th, :tw] != want).any(-1))[0])}"
    assert (got[th:] == FILL).all() and (got[:, tw:] == FILL).all(), "texels outside the dispatch extent were written"
    if gname == "stencil_noise":
        assert np.array_equal(got[:th, :tw], sp.probe_expected("raster", size, pname, grid, layers)[0]), "the stencil byte changes the image"
