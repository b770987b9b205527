"""GPU tests of the cube-face bake (csrc/cubemap.hip, program cubemap_probe) and of the frame's probe path (vkrh_bake_probes,
VKRH_STAGE_PROBE_TRACE): the kernel against the numpy restatement tests/cubemap_reference.py, the box-room known answer, skipped
draws, and the frame path against the four programs driven by hand through the C-ABI.

Measured on an MI355X (kernel against the restatement, 2 scenes x 3 positions x 2 sizes, 72 faces): coverage, colour and distance
bit-equal on every face (0 texels outside tolerance); the frame's probe_trace has 39.27 % non-zero pixels on the procedural
scene at 256 x 144, as the restatement of trace_probe has on the same inputs.
"""
import ctypes as C
import os

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.images import ArrayImageBuf

import cubemap_reference as cref
import cubemap_room as room
import parity
import probe_reference as pref

pytestmark = pytest.mark.gpu

SUZANNE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "suzanne", "Suzanne.gltf")
OUTSIDE_SHARE = 1e-4  # of the texels of a face may miss the per-format tolerance (the cap of tests/test_raster.py)
DETAIL = 12


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch

    torch.cuda.synchronize()


def _ar():
    return cref.Arith(int(abi.product().vkr_numeric_contract()))


def _triangles(sc):
    return sum(d["index_count"] // 3 for d in sc.draws)


class Cube:
    """the two cube images of one bake on the device, as regular 6-layer arrays"""

    def __init__(self, size):
        self.size = size
        self.color = ArrayImageBuf(abi.FMT_RGBA8_SRGB, size, size, 6, device="cuda", fill=0x5A)
        self.distance = ArrayImageBuf(abi.FMT_R16_SFLOAT, size, size, 6, device="cuda", fill=0x5A)

    def read(self):
        return self.color.raw(), self.distance.raw()[..., 0]


def bake_gpu(sc, pos, size, uploaded=None):
    import torch

    s, keep = uploaded if uploaded is not None else sc.upload("cuda")
    cube = Cube(size)
    nbytes = abi.cubemap_probe_scratch_bytes(size, _triangles(sc))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    abi.cubemap_probe(s, pos, cube.color.descs(), cube.distance.descs(), scratch.data_ptr(), nbytes, _stream())
    _sync()
    return cube.read()


def _decode_color(codes):
    out = np.empty(codes.shape, np.float32)
    out[..., :3] = pref.SRGB[codes[..., :3]]
    out[..., 3] = codes[..., 3].astype(np.float32) / np.float32(255.0)
    return out


def _scenes():
    suz = scn.load_gltf(SUZANNE)
    return {"procedural": scn.procedural_scene(detail=DETAIL, cutout=True), "suzanne": suz, "room": room.room_scene()}


def _positions(name, sc):
    if name == "room":
        # The ceiling is nearer than any wall is far, so it fills face +Y: the bounding box of both its triangles is the whole face
        # and they go to the large list.  At 72^2 that is 9 x 9 = 81 blocks of 8 x 8: 5 chunks of 16 and a last one of 1.
        p = np.array((0.0, 1.0, 4.0))
        assert room.ROOM_HI[1] - p[1] <= min(np.delete(p - room.ROOM_LO, 1).min(), np.delete(room.ROOM_HI - p, 1).min())
        return [tuple(p)]
    if name == "procedural":  # the floor (y = 0) passes under every position: near-plane clipping on every side face
        return [(0.0, 1.0, 4.0), (-3.5, 0.6, 7.25), (2.5, 2.0, 1.0)]
    idx = np.concatenate([sc.indices[d["index_offset"]:d["index_offset"] + d["index_count"]].astype(np.int64) + d["vertex_offset"] for d in sc.draws])
    p = sc.vertices[idx, :3]
    m = np.asarray(sc.transforms[sc.draws[0]["transform"]][0], np.float64)
    w = p @ m[:3, :3].T + m[:3, 3]
    lo, hi = w.min(0), w.max(0)
    c, e = (lo + hi) / 2, (hi - lo)
    # outside the head in front of it, beside it, and inside its bounding box
    return [tuple(c + e * np.array([0.0, 0.1, 1.5])), tuple(c + e * np.array([-1.2, 0.4, 0.3])), tuple(c + e * np.array([0.1, 0.05, 0.1]))]


@pytest.mark.parametrize("size", [128, 72])
@pytest.mark.parametrize("name", ["procedural", "suzanne", "room"])
def test_cubemap_probe_matches_restatement(name, size, parity_table):
    """Coverage bit-exact on all six faces; colour and distance within one storage step (or REL_TOL) of the restatement, at most
    1e-4 of the texels of a face outside."""
    sc = _scenes()[name]
    uploaded = sc.upload("cuda")
    ar = _ar()
    for pos in _positions(name, sc):
        got_c, got_d = bake_gpu(sc, pos, size, uploaded)
        ref_c, ref_d = cref.cubemap_probe(ar, sc, pos, size)
        cov_g, cov_r = got_d != cref.CLEAR_DISTANCE, ref_d != cref.CLEAR_DISTANCE
        print(f"[cubemap] {name} {size} pos {pos}: covered {int(cov_r.sum())} of {cov_r.size}, coverage differs on {int((cov_g != cov_r).sum())}")
        assert (cov_g == cov_r).all(), f"{name} pos {pos}: coverage differs on {int((cov_g != cov_r).sum())} texels"
        for f in range(6):
            n_c, _ = parity.report(f"{name}{size}.color{f}", abi.FMT_RGBA8_SRGB, _decode_color(got_c[f]), _decode_color(ref_c[f]))
            n_d, _ = parity.report(f"{name}{size}.dist{f}", abi.FMT_R16_SFLOAT, got_d[f].astype(np.float32)[..., None], ref_d[f].astype(np.float32)[..., None])
            assert n_c <= OUTSIDE_SHARE * size * size, f"{name} pos {pos} face {f}: {n_c} colour texels outside tolerance"
            assert n_d <= OUTSIDE_SHARE * size * size, f"{name} pos {pos} face {f}: {n_d} distance texels outside tolerance"


def test_cutout_discards_texels():
    """the restatement reproduces discarded texels: the fence's holes change the faces, and the kernel agrees on where"""
    pos, size = (0.0, 1.0, 4.0), 128
    cut, solid = scn.procedural_scene(detail=DETAIL, cutout=True), scn.procedural_scene(detail=DETAIL, cutout=True)
    tex = solid.draws[-1]["albedo"]
    solid.textures[tex] = [np.concatenate([lv[..., :3], np.full_like(lv[..., 3:], 255)], -1) for lv in solid.textures[tex]]
    ar = _ar()
    ref_cut, _ = cref.cubemap_probe(ar, cut, pos, size)
    ref_solid, _ = cref.cubemap_probe(ar, solid, pos, size)
    differ = (ref_cut != ref_solid).any(-1)
    assert differ.sum() > 100, "the fence's holes are not visible from this position"
    got_cut, _ = bake_gpu(cut, pos, size)
    got_solid, _ = bake_gpu(solid, pos, size)
    assert ((got_cut != got_solid).any(-1) == differ).mean() > 1 - OUTSIDE_SHARE


def test_room_known_answer_gpu():
    sc = room.room_scene()
    uploaded = sc.upload("cuda")
    shares = []
    for pos in room.grid_positions():
        color, distance = bake_gpu(sc, pos, 128, uploaded)
        shares.append(room.assert_room(color, distance, pos, 128))
    assert max(shares) <= room.COLOR_BAND_SHARE


def test_draw_without_albedo_is_skipped():
    sc = room.room_scene()
    for d in sc.draws:
        d["albedo"] = scn.INVALID
    color, distance = bake_gpu(sc, (0.0, 1.0, 4.0), 72)
    assert (color == cref.CLEAR_COLOR).all() and (distance == cref.CLEAR_DISTANCE).all()
    sc = room.room_scene()
    sc.draws[4]["albedo"] = scn.INVALID  # the +Z wall: exactly the texels that see it first keep the clear values
    pos = (0.0, 1.0, 4.0)
    color, distance = bake_gpu(sc, pos, 72)
    _, wall, clear = room.analytic(np.asarray(pos, np.float64), 72)
    assert ((distance == cref.CLEAR_DISTANCE) == (wall == 4))[clear].all()
    assert ((color == cref.CLEAR_COLOR).all(-1) == (wall == 4))[clear].all()
    assert (wall == 4).sum() > 1000


# ---- the frame path ------------------------------------------------------------------------------------------------------------
GRID, PROBE, CUBE = 4, 256, 128
PMIN, PMAX = (-6.0, 1.0, 0.0), (6.0, 1.0, 12.0)


def _grid_positions():
    """as ProbeRenderer::render_probe_grid lays them out, in fp32: min + step * (x, 0, y), layer y * grid + x"""
    lo, hi = np.array(PMIN, np.float32), np.array(PMAX, np.float32)
    step = (hi - lo) / np.float32(GRID - 1)
    return [lo + step * np.array([x, 0, y], np.float32) for y in range(GRID) for x in range(GRID)]


def _bake_by_hand(sc):
    """vkr_cubemap_probe -> vkr_cube2oct -> vkr_probe_downsample per probe through the C-ABI -> (colour array, depth array, last cube)"""
    import torch

    lib = abi.product()
    s, keep = sc.upload("cuda")
    mips = int(np.floor(np.log2(PROBE))) + 1
    color = ArrayImageBuf(abi.FMT_RGBA8_UNORM, PROBE, PROBE, GRID * GRID, device="cuda")
    depth = ArrayImageBuf(abi.FMT_R16_UNORM, PROBE, PROBE, GRID * GRID, mips=mips, device="cuda")
    cube = Cube(CUBE)
    nbytes = abi.cubemap_probe_scratch_bytes(CUBE, _triangles(sc))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for layer, pos in enumerate(_grid_positions()):
        abi.cubemap_probe(s, pos, cube.color.descs(), cube.distance.descs(), scratch.data_ptr(), nbytes, _stream())
        one = depth.desc(layer)
        one0 = abi.VkrImg.from_buffer_copy(one)
        one0.mip_count = 1
        abi.check(lib.vkr_cube2oct(cube.color.descs(), cube.distance.descs(), C.byref(color.desc(layer)), C.byref(one0), _stream()), lib)
        abi.check(lib.vkr_probe_downsample(C.byref(one), _stream()), lib)
    _sync()
    return color, depth, cube


def test_frame_path_matches_the_programs_driven_by_hand():
    """vkrh_bake_probes + VKRH_STAGE_RASTER | VKRH_STAGE_PROBE_TRACE against cubemap_probe -> cube2oct -> probe_downsample ->
    trace_probe through the C-ABI on the same inputs: probe colour, probe depth (all mips, all 16 layers), the last cube and the
    traced image bit for bit.  The trace hits something: the share of non-zero pixels is at least what the numpy restatement of
    trace_probe gives on the same probes and G-buffer."""
    from vk_renderer_amd.images import ImageBuf

    W, H = 256, 144
    sc = scn.procedural_scene(detail=DETAIL, cutout=True)
    frame = host.HostFrame(FrameSetup(W, H), device="cuda")
    try:
        frame.load_scene(sc)
        frame.bake_probes(PMIN, PMAX, GRID, PROBE, CUBE)
        assert frame.last_tasks().count("CubemapSide") == 6 * GRID * GRID and frame.last_tasks().count("Cubemap2Octahedral") == GRID * GRID
        frame.run(host.STAGE_RASTER | host.STAGE_PROBE_TRACE)
        _sync()
        assert frame.last_tasks()[-1] == "TraceProbe"
        color, depth, cube = _bake_by_hand(sc)
        hc, hd = color.raw(0), [depth.raw(m) for m in range(depth.mips)]
        for layer in range(GRID * GRID):
            assert (frame.download("probe_color", layer).raw(0) == hc[layer]).all(), f"probe colour, layer {layer}"
            got = frame.download("probe_depth", layer)
            assert got.mips == depth.mips
            for m in range(depth.mips):
                assert (got.raw(m) == hd[m][layer]).all(), f"probe depth, layer {layer} mip {m}"
        cube_c, cube_d = cube.read()
        for f in range(6):
            assert (frame.download("cubemap_color", f).raw(0) == cube_c[f]).all(), f"cube colour, face {f}"
            assert (frame.download("cubemap_distance", f).raw(0)[..., 0] == cube_d[f]).all(), f"cube distance, face {f}"
        assert (hc[..., 3] != 0).mean() > 0.5, "the baked probes see the scene"
        # the trace by hand, on the frame's own G-buffer
        params = frame.gtao_rt_params()
        consts = abi.ProbeTraceConsts()
        consts.inverse_view = params.camera_to_world
        for k in range(3):
            consts.probe_min[k], consts.probe_max[k] = PMIN[k], PMAX[k]
        consts.probe_min[3] = consts.probe_max[3] = 1.0
        consts.grid_size = GRID
        consts.fovy, consts.aspect, consts.znear, consts.zfar = params.fovy, params.aspect, params.znear, params.zfar
        lib = abi.product()
        out = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda", fill=0)
        abi.check(lib.vkr_trace_probe(C.byref(frame.image("depth")), C.byref(frame.image("normal")), color.descs(), depth.descs(), color.layers,
                                      C.byref(consts), C.byref(out.desc()), _stream()), lib)
        _sync()
        by_hand = out.raw(0)
        got = frame.download("probe_trace").raw(0)
        tw, th = W // 8 * 8, H // 4 * 4
        assert (got[:th, :tw] == by_hand[:th, :tw]).all(), f"{int((got[:th, :tw] != by_hand[:th, :tw]).any(-1).sum())} traced pixels differ"
        # the lower bound of "hits something" comes from the restatement, not from the kernel
        depth_bits = frame.download("depth").raw(0)[..., 0]
        normal_codes = frame.download("normal").raw(0)
        hb = depth.to_host()
        pa = pref.ProbeArrays(hc, [depth.raw(m, hb)[..., 0] for m in range(depth.mips)])
        M = np.array(params.camera_to_world.m, np.float32).reshape(4, 4).T
        want, result, traced = pref.trace_probe(_ar(), depth_bits, normal_codes, pa, M, PMIN + (1.0,), PMAX + (1.0,),
                                                GRID, params.fovy, params.aspect, params.znear, params.zfar, W, H)
        share_ref = float((want != 0).any(-1).mean())
        share_got = float((got[:th, :tw] != 0).any(-1).mean())
        print(f"[probe_trace] non-zero pixels: restatement {share_ref:.4f}, frame {share_got:.4f}, hits {int((result == pref.HIT).sum())}")
        assert share_ref > 0.02, "the restatement itself finds reflections on this scene"
        assert share_got >= share_ref
    finally:
        frame.close()
