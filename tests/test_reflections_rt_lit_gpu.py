"""Program reflections_rt_lit on the GPU: the image byte for byte against the numpy restatement
(tests/reflections_rt_lit_reference.py) at 8 x 8 (one wave), 17 x 9 (partial tiles on both axes), 64 x 36 and the degenerate 1 x 1,
1 x 9, 9 x 1, on the seven G-buffer content classes of tests/test_reflections_rt_gpu.py (whose scene, inputs and helpers this file
imports), with one point light, the four lights of tests/test_reflections_rt_lit.py, no light and ambient 1 (also against what
vkr_reflections_rt writes on the GPU), an empty structure, no textures, a level beyond the chain and both fill patterns; the bytes
outside the rows and the untouched texels of fill mode; under the frozen camera 1 x 1 and 9 x 1 cast no ray at all, so those two
extents run a second time under the pitched-down camera of tests/camera_cases.py, where the restatement lights a hit; the cutout
entry on the scene with the fence, and with a mask of all ones against the opaque entry; vkr_scene_triangle_normals bit for bit
against abi.scene_triangle_normals; and the frame: vkrh_set_reflection_lights in both modes and with cutouts against the entry
called by hand, the task order, the refusals, a frame that never calls it, and moving draws.

Measured on the restatement at 64 x 36 on the scene with the fence: with the lights of tests/test_ray_cutout_passes_gpu.py 7 texels
differ between the lit and the lit-cutout entry where both see the same closest hit, that is because of a shadow ray through a hole;
with its point light behind the fence moved to (2, 1.5, 6.5), FENCE_LIGHTS here, 14 do (the test asserts at least 8), and 29 more
differ because the mirror ray itself passes through a hole."""
import functools

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.images import ImageBuf

import camera_cases as cc
import reflections_rt_lit_reference as ref
import test_ray_cutout_passes_gpu as fence  # the scene with the fence: its kit
import test_reflections_rt_gpu as base      # the scene without: its kit, classes and patterns
from test_reflections_rt_lit import AMBIENT, COLOURS, LIGHTS, SHADOW_OFFSET, SHADOW_TMIN

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL, SKY = base.FILL, base.SKY
OFFSET, TMIN = base.OFFSET, base.TMIN
PITCHED = [cc.Extent((1, 1), "pitch_down"), cc.Extent((9, 1), "pitch_down")]
WHITE = (1.0, 1.0, 1.0)
# variant: (lights, texture_lod, textures bound, empty structure, fill mode: None, "px" or "tile8")
VARIANTS = {"one_point": (1, 0, True, False, None), "four": (4, 0, True, False, None), "zero_ambient1": (0, 0, True, False, None),
            "empty": (4, 0, True, True, None), "no_textures": (4, 0, False, False, None), "lod_beyond": (4, 99, True, False, None),
            "fill_px": (4, 0, True, False, "px"), "fill_tile8": (4, 3, True, False, "tile8")}
# Under the pitched camera at one row the kit's surface points lie below the ground (it rasterises two rows and keeps one: the
# pass is held to the restatement on whatever the G-buffer says), the mirror rays meet the ground from below and its normal turns
# down: of the stock lights none is faced.  These variants put a directional light underneath, in front of the shading pass's.
BELOW = (0.0, -1.0, 0.0, 0.0)
PITCHED_VARIANTS = {"from_below": ("below", 0, True, False, None), "from_below_fill": ("below", 0, True, False, "px")}
ALL_VARIANTS = dict(VARIANTS, **PITCHED_VARIANTS)


def _lighting(count):
    """-> (lights, colours, ambient) of a variant: the first `count` lights; without any, ambient 1 (the unlit pass)"""
    if count == "below":
        return [BELOW, LIGHTS[0]], COLOURS[:2], AMBIENT
    return LIGHTS[:count], COLOURS[:count], AMBIENT if count else WHITE


@functools.lru_cache(maxsize=None)
def _normals():
    return abi.scene_triangle_normals(base._scene()[0])


@functools.lru_cache(maxsize=None)
def _device_normals():
    import torch

    return torch.from_numpy(np.ascontiguousarray(_normals()).view(np.uint8).copy()).to("cuda")


@functools.lru_cache(maxsize=None)
def _expected(name, size, variant):
    count, lod, textured, empty, fill = ALL_VARIANTS[variant]
    words, codes, setup, _, _ = base._inputs(name, size)
    sc, tris, att, _ = base._scene()
    nr = _normals()
    if empty:
        tris, att, nr = np.zeros((0, 3, 3), F32), att[:0], nr[:0]
    before = np.full(words.shape + (4,), FILL, np.uint8)
    return ref.reflections_rt_lit(base._arith(), words, codes, base._rays_w(size, fill) if fill else None, setup.inv_view, *setup.fazz, OFFSET, TMIN,
                                  float(setup.fazz[3]), lod, ref.FILL_MISSES if fill else 0, tris, att, nr, sc.textures if textured else [], before,
                                  *_lighting(count), SHADOW_OFFSET, SHADOW_TMIN)


def _images(name, size, fill):
    """-> (depth, normal, rays or None, out filled with FILL, setup) on the device"""
    w, h = size
    _, _, setup, depth_bytes, normal_bytes = base._inputs(name, size)
    depth = ImageBuf(abi.FMT_D24_UNORM_S8, w, h, device="cuda")
    normal = ImageBuf(abi.FMT_RG16_UNORM, w, h, device="cuda")
    depth.upload(depth_bytes)
    normal.upload(normal_bytes)
    rays = None
    if fill:
        host_rays = ImageBuf(abi.FMT_RGBA16_UNORM, w, h)
        codes = np.full((h, w, 4), 0x1234, np.uint16)
        codes[..., 3] = base._rays_w(size, fill)
        host_rays.set_raw(codes)
        rays = ImageBuf(abi.FMT_RGBA16_UNORM, w, h, device="cuda")
        rays.upload(host_rays.to_host())
    return depth, normal, rays, ImageBuf(abi.FMT_RGBA8_UNORM, w, h, device="cuda", fill=FILL), setup


def _launch(name, size, variant, unlit=False):
    """-> the RGBA8 codes [h, w, 4] of vkr_reflections_rt_lit (unlit: of vkr_reflections_rt) on an image filled with FILL; checks
    that nothing outside the rows was written"""
    import torch

    count, lod, textured, empty, fill = ALL_VARIANTS[variant]
    w, h = size
    depth, normal, rays, out, setup = _images(name, size, fill)
    rs, attribs, _ = base._device_scene()
    textures = rs.texture_count if textured else 0
    nbytes = abi.reflections_rt_scratch_bytes(textures)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    params = abi.reflect_rt_params(setup.inv_view, *setup.fazz, fill_misses=bool(fill), normal_offset=OFFSET, tmin=TMIN, texture_lod=lod)
    n = 0 if empty else len(base._scene()[2])
    head = (depth.desc(), normal.desc(), rays.desc() if fill else None, base._accel(empty), None if empty else attribs.data_ptr(), n)
    tail = (out.desc(), scratch.data_ptr(), nbytes, base._stream())
    if unlit:
        abi.reflections_rt(*head, rs.textures if textured else None, textures, params, *tail)
    else:
        lights = abi.reflect_lights(*_lighting(count), SHADOW_OFFSET, SHADOW_TMIN)
        abi.reflections_rt_lit(*head, None if empty else _device_normals().data_ptr(), n, rs.textures if textured else None, textures, params, lights,
                               *tail)
    base._sync()
    return fence._rows_only(out, w, h)


# ---- byte for byte against the restatement ------------------------------------------------------------------------------------------
def _check(name, size, variant):
    count, lod, textured, empty, fill = ALL_VARIANTS[variant]
    want, traced, index, info = _expected(name, size, variant)
    got = _launch(name, size, variant)
    geometry = (base._inputs(name, size)[0] & SKY) != SKY
    hit = index != ref.MISS
    lit = sum(int(s[2].sum()) for s in info["lights"])
    print(f"[reflections rt lit] {name} {size[0]}x{size[1]} {variant}: {int(geometry.sum())} geometry pixels, {int(traced.sum())} rays, "
          f"{int(hit.sum())} hits, {lit} lit (hit, light) pairs, differing texels {int((got != want).any(axis=-1).sum())}")
    base._differing(f"{name} {size} {variant}", got, want)
    if fill:
        kept = geometry & (base._rays_w(size, fill) != 65535)
        assert (got[kept] == FILL).all(), "a texel with a valid screen-space ray was touched"
        assert (got[~kept][:, 3] == 0).all()
    else:
        assert (got[..., 3] == 0).all(), "alpha is 0"
        assert (got[~geometry] == 0).all() and (got[~hit] == 0).all()
    if empty:
        assert (got[got[..., 3] == 0] == 0).all() and not hit.any()
    if count == 0:
        base._differing(f"{name} {size}: no light and ambient 1 against vkr_reflections_rt on the GPU", got, _launch(name, size, variant, unlit=True))
    if name == "facing_away":
        assert not traced.any(), "a surface seen from behind casts no ray"
    return info


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("size", base.SIZES)
@pytest.mark.parametrize("name", sorted(base.CLASSES))
def test_parity(name, size, variant):
    _check(name, size, variant)


@pytest.mark.parametrize("variant", ["four"] + sorted(PITCHED_VARIANTS))
@pytest.mark.parametrize("size", PITCHED, ids=["1x1", "9x1"])
def test_parity_of_the_one_row_extents_under_a_pitched_camera(size, variant):
    """the frozen camera looks along the ground: at 1 x 1 and 9 x 1 no pixel casts a ray.  Pitched down every pixel does, and with
    the light underneath the restatement lights its hit (measured: 1 of 1 and 9 of 9 hits lit, none by the stock lights)"""
    for frozen in ((1, 1), (9, 1)):
        assert not _expected("raster", frozen, "four")[1].any(), "the frozen camera traces nothing at these extents"
    info = _check("raster", size, variant)
    if variant == "from_below":
        assert int(info["lights"][0][2].sum()) >= 1, "no lit hit under the pitched camera"


def test_the_lit_image_is_not_the_unlit_one():
    lit_image = _launch("raster", (64, 36), "four")
    assert (lit_image != _launch("raster", (64, 36), "four", unlit=True)).any()
    assert (lit_image != _launch("raster", (64, 36), "one_point")).any()


# ---- the cutout entry ---------------------------------------------------------------------------------------------------------------------
CUT_SIZE = (64, 36)
FENCE_LIGHTS = [(2.0, 1.5, 6.5, 1.0)] + fence.LIGHTS[1:]  # the first one moved closer behind the fence: see the module's text


@functools.lru_cache(maxsize=None)
def _fence_normals():
    return abi.scene_triangle_normals(fence._scene()[0])


@functools.lru_cache(maxsize=None)
def _fence_expected(name, cutout, fill=False):
    """cutout: None (the opaque entry) or (alpha_lod, opaque mask)"""
    words, codes, setup, _, _ = fence._inputs(name, CUT_SIZE)
    sc, tris, att, _ = fence._scene()
    before = np.full(words.shape + (4,), FILL, np.uint8)
    return ref.reflections_rt_lit(base._arith(), words, codes, fence._rays_w(CUT_SIZE, fill) if fill else None, setup.inv_view, *setup.fazz, OFFSET, TMIN,
                                  float(setup.fazz[3]), 0, ref.FILL_MISSES if fill else 0, tris, att, _fence_normals(), sc.textures, before,
                                  FENCE_LIGHTS, COLOURS, AMBIENT, SHADOW_OFFSET, SHADOW_TMIN, cutout=cutout)


def _fence_launch(name, cutout, fill=False):
    import torch

    w, h = CUT_SIZE
    depth, normal, setup = fence._upload(name, CUT_SIZE)
    rays = None
    if fill:
        host_rays = ImageBuf(abi.FMT_RGBA16_UNORM, w, h)
        codes = np.full((h, w, 4), 0x1234, np.uint16)
        codes[..., 3] = fence._rays_w(CUT_SIZE, fill)
        host_rays.set_raw(codes)
        rays = ImageBuf(abi.FMT_RGBA16_UNORM, w, h, device="cuda")
        rays.upload(host_rays.to_host())
    out = ImageBuf(abi.FMT_RGBA8_UNORM, w, h, device="cuda", fill=FILL)
    rs, attribs, _, nbytes, scratch = fence._device_scene()
    normals = torch.from_numpy(np.ascontiguousarray(_fence_normals()).view(np.uint8).copy()).to("cuda")
    n = len(fence._scene()[2])
    params = abi.reflect_rt_params(setup.inv_view, *setup.fazz, fill_misses=fill, normal_offset=OFFSET, tmin=TMIN)
    lights = abi.reflect_lights(FENCE_LIGHTS, COLOURS, AMBIENT, SHADOW_OFFSET, SHADOW_TMIN)
    head = (depth.desc(), normal.desc(), rays.desc() if fill else None, fence._accel(), attribs.data_ptr(), n, normals.data_ptr(), n, rs.textures,
            rs.texture_count, params, lights)
    if cutout is None:
        abi.reflections_rt_lit(*head, out.desc(), scratch.data_ptr(), nbytes, base._stream())
    else:
        abi.reflections_rt_lit_cutout(*head, abi.ray_cutout(*cutout), out.desc(), scratch.data_ptr(), nbytes, base._stream())
    base._sync()
    return fence._rows_only(out, w, h)


@pytest.mark.parametrize("fill", [False, True], ids=["all", "fill"])
@pytest.mark.parametrize("cutout", [(0, 0), (0, 0b0111), (3, 0)], ids=["lod0", "lod0_masked", "lod3"])
@pytest.mark.parametrize("name", sorted(fence.CLASSES))
def test_cutout_parity(name, cutout, fill):
    want = _fence_expected(name, cutout, fill)[0]
    got = _fence_launch(name, cutout, fill)
    print(f"[reflections rt lit] cutout {name} {cutout} fill {fill}: differing texels {int((got != want).any(axis=-1).sum())}")
    base._differing(f"cutout {name} {cutout} fill {fill}", got, want)


def test_the_light_passes_through_the_holes():
    """on the restatement: texels whose closest hit is the same triangle with and without cutouts, and whose colour still differs,
    differ because of a shadow ray through a hole; and the opaque lit entry on the scene with the fence is the restatement's too"""
    opaque, _, opaque_index, _ = _fence_expected("raster", None)
    cut, _, cut_index, _ = _fence_expected("raster", (0, 0))
    through = (opaque_index == cut_index) & (opaque_index != ref.MISS) & (opaque != cut).any(axis=-1)
    print(f"[reflections rt lit] 64x36 with the fence: {int(through.sum())} texels differ because of a shadow ray through a hole, "
          f"{int((opaque_index != cut_index).sum())} because of a mirror ray through one")
    assert int(through.sum()) >= 8
    assert (cut[through].astype(int).sum(axis=-1) > opaque[through].astype(int).sum(axis=-1)).all(), "light through a hole only adds"
    base._differing("the opaque lit entry on the scene with the fence", _fence_launch("raster", None), opaque)


def test_a_mask_of_all_ones_is_the_opaque_entry():
    for fill in (False, True):
        base._differing(f"mask of all ones, fill {fill}", _fence_launch("raster", (0, 0xFFFFFFFF), fill), _fence_launch("raster", None, fill))


# ---- vkr_scene_triangle_normals ---------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device_normals_of(sc, guard=64):
    """vkr_scene_triangle_normals into the middle of a buffer of 0xA5: -> (records, guard bytes intact)"""
    import torch

    rs, keep = sc.upload(device="cuda")
    total = sum(d["index_count"] // 3 for d in sc.draws)
    buf = torch.full((guard + 48 * total + guard,), FILL, dtype=torch.uint8, device="cuda")
    nbytes = abi.scene_triangles_scratch_bytes(rs.draw_count)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    lib = abi.product()
    import ctypes as C

    abi.check(lib.vkr_scene_triangle_normals(C.byref(rs), buf.data_ptr() + guard, total, scratch.data_ptr(), nbytes, base._stream()), lib)
    base._sync()
    host_bytes = buf.cpu().numpy()
    intact = (host_bytes[:guard] == FILL).all() and (host_bytes[guard + 48 * total:] == FILL).all()
    del keep
    return host_bytes[guard:guard + 48 * total].view(abi.hit_normal_dtype()), bool(intact)


def _scaled_rotated_scene():
    sc = scn.procedural_scene(detail=5)
    a, b = np.radians(33.0), np.radians(-71.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    rx = np.array([[1, 0, 0, 0], [0, np.cos(b), -np.sin(b), 0], [0, np.sin(b), np.cos(b), 0], [0, 0, 0, 1]])
    model = rz @ rx @ np.diag([0.3, 2.5, 1.7, 1.0])
    model[:3, 3] = (0.5, 1.0, 4.0)
    sc.draws[2]["transform"] = sc.add_transform(model.astype(F32))
    return sc


def test_scene_triangle_normals_against_the_host_rule():
    for what, sc in (("procedural", base._scene()[0]), ("non-uniform scale and rotation", _scaled_rotated_scene())):
        got, intact = _device_normals_of(sc)
        want = abi.scene_triangle_normals(sc)
        assert intact, f"{what}: bytes round the output were written"
        assert len(got) == len(want) > 100 and np.array_equal(_bits(got["n"]), _bits(want["n"])), what
        # abi.scene_world_normals is the same entry
        rs, keep = sc.upload(device="cuda")
        again = abi.scene_world_normals(rs, len(want)).cpu().numpy()
        assert np.array_equal(_bits(again), _bits(want["n"])), what


def test_scene_triangle_normals_with_an_index_outside_the_vertex_buffer():
    sc = scn.procedural_scene(detail=5)
    want = abi.scene_triangle_normals(sc)
    d = sc.draws[2]
    assert d["index_count"] >= 12
    # the fourth triangle of draw 2, a sphere, and of every other draw of the same mesh (the spheres share their index range)
    first = np.cumsum([0] + [x["index_count"] // 3 for x in sc.draws])
    bad = [int(first[i]) + 3 for i, x in enumerate(sc.draws) if x["index_offset"] == d["index_offset"]]
    sc.indices = sc.indices.copy()
    sc.indices[d["index_offset"] + 3 * 3 + 1] = len(sc.vertices) + 1000
    got, intact = _device_normals_of(sc)
    assert intact, "bytes round the output were written"
    assert np.isnan(got["n"][bad][..., :3]).all() and (got["n"][bad][..., 3] == 0).all(), "NaN normals for the triangles with the bad index"
    others = ~np.isin(np.arange(len(want)), bad)
    assert others.sum() == len(want) - len(bad) and np.array_equal(_bits(got["n"][others]), _bits(want["n"][others])), "every other record is intact"


# ---- the frame ----------------------------------------------------------------------------------------------------------------------------
W, H = base.W, base.H
PRE = base.PRE
DEFAULT_LIGHT = dict(lights=[LIGHTS[0]], colours=[(float(F32(10.0) / F32(np.pi)),) * 3], ambient=(0.6, 0.6, 0.6))


def _by_hand(frame, setup, accel, fill, lighting, normals, cutout=None, before=None, **rays):
    """vkr_reflections_rt_lit (cutout: an abi.RayCutout, vkr_reflections_rt_lit_cutout) on the frame's own half-resolution images
    -> the RGBA8 codes; normals: hit_normal records; before: the content the image starts with"""
    import torch

    out = ImageBuf(abi.FMT_RGBA8_UNORM, W // 2, H // 2, device="cuda", fill=FILL)
    if before is not None:
        out.upload(before)
    rs, attribs, _ = base._device_scene_of(frame.scene)
    nbytes = abi.reflections_rt_scratch_bytes(rs.texture_count)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    table = torch.from_numpy(np.ascontiguousarray(normals).view(np.uint8).copy()).to("cuda")
    params = abi.reflect_rt_params(setup.inv_view, *setup.fazz, fill_misses=fill, **rays)
    lights = abi.reflect_lights(lighting["lights"], lighting["colours"], lighting["ambient"], lighting.get("shadow_offset", abi.REFLECT_SHADOW_OFFSET),
                                lighting.get("shadow_tmin", abi.REFLECT_SHADOW_TMIN))
    n = attribs.numel() // 32
    head = (frame.image("depth", 1, 1), frame.image("dn"), frame.image("rays") if fill else None, accel, attribs.data_ptr(), n, table.data_ptr(), len(normals),
            rs.textures, rs.texture_count, params, lights)
    tail = (out.desc(), scratch.data_ptr(), nbytes, base._stream())
    if cutout is None:
        abi.reflections_rt_lit(*head, *tail)
    else:
        abi.reflections_rt_lit_cutout(*head, cutout, *tail)
    base._sync()
    return out.raw(0)


STOCK = dict(lights=LIGHTS, colours=COLOURS, ambient=AMBIENT, shadow_offset=SHADOW_OFFSET, shadow_tmin=SHADOW_TMIN)


def test_frame_stage_lit_all_mode_cutouts_and_refusals():
    sc = scn.procedural_scene(detail=12, cutout=True)
    frame, setup = base._frame(sc)
    accel = abi.Accel.from_scene(sc)
    try:
        frame.load_scene(sc)
        frame.run(PRE)
        # a frame that never called the setter: today's task and today's bytes
        frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE | host.STAGE_REFLECTIONS_RT)
        base._sync()
        assert frame.last_tasks()[-2:] == ["ReflectionsRT", "SSSR_blur"] and "ReflectionsRTLit" not in frame.last_tasks()
        unlit = frame.download("reflections").raw(0)
        base._differing("a frame that never set lights, against vkr_reflections_rt called by hand", unlit, base._by_hand(frame, setup, accel, False))
        # the table the frame made with its structure: the host rule up to the rounding of the normal matrix (the frame inverts in fp32)
        normals = frame.hit_normals()
        want = abi.scene_triangle_normals(sc)
        assert len(normals) == len(want) and np.allclose(normals["n"], want["n"], rtol=0, atol=1e-5) and (normals["n"][..., 3] == 0).all()
        # the stock lights; the stage alone, on the G-buffer of the earlier run
        frame.set_reflection_lights(**STOCK)
        frame.run(host.STAGE_REFLECTIONS_RT)
        base._sync()
        assert frame.last_tasks() == ["ReflectionsRTLit", "SSSR_blur"], frame.last_tasks()
        lit = frame.download("reflections").raw(0)
        base._differing("frame stage, lit, against the entry called by hand", lit, _by_hand(frame, setup, accel, False, STOCK, normals))
        assert (lit != unlit).any() and (lit[..., 3] == 0).all() and (frame.download("blurred").raw(0) != 0).any()
        # the whole frame order keeps its place for the task
        frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE | host.STAGE_REFLECTIONS_RT)
        tasks = frame.last_tasks()
        assert tasks[-2:] == ["ReflectionsRTLit", "SSSR_blur"] and tasks.index("DownsampleGbuffer") < tasks.index("ReflectionsRTLit") and "ReflectionsRT" not in tasks
        # the default light, with other rays
        rays = dict(normal_offset=5e-3, tmin=1e-4, max_distance=6.0, texture_lod=2)
        frame.set_reflection_rays(fill_misses=False, **rays)
        frame.set_reflection_lights()
        frame.run(host.STAGE_REFLECTIONS_RT)
        base._sync()
        default = frame.download("reflections").raw(0)
        base._differing("frame stage, the default light, against the entry called by hand", default, _by_hand(frame, setup, accel, False, DEFAULT_LIGHT, normals, **rays))
        assert (default != lit).any()
        # cutouts compose
        frame.set_reflection_rays(fill_misses=False)
        frame.set_reflection_lights(**STOCK)
        frame.set_ray_cutouts(True, 0)
        frame.run(host.STAGE_REFLECTIONS_RT)
        base._sync()
        assert frame.last_tasks() == ["ReflectionsRTLit", "SSSR_blur"]
        holes = frame.download("reflections").raw(0)
        cutout = abi.ray_cutout(0, abi.scene_opaque_texture_mask(sc))
        base._differing("frame stage, lit with cutouts, against the entry called by hand", holes, _by_hand(frame, setup, accel, False, STOCK, normals, cutout=cutout))
        assert (holes != lit).any(), "the fence's holes change nothing"
        frame.set_ray_cutouts(False)
        # the refusals of the setter
        for kwargs, text in ((dict(lights=LIGHTS + LIGHTS[:1], colours=COLOURS + COLOURS[:1], ambient=AMBIENT), "5 lights, at most 4"),
                             (dict(lights=[(0, 1, 0, 0.5)], colours=COLOURS[:1], ambient=AMBIENT), "light 0 has w = 0.5"),
                             (dict(lights=LIGHTS[:1], colours=[(1, float("nan"), 1)], ambient=AMBIENT), "colour 0 is NaN"),
                             (dict(lights=[], colours=[], ambient=(float("nan"), 0, 0)), "ambient is NaN"),
                             (dict(lights=[], colours=[], ambient=AMBIENT, shadow_offset=float("nan")), "shadow_offset is NaN"),
                             (dict(lights=[], colours=[], ambient=AMBIENT, shadow_tmin=float("nan")), "shadow_tmin is NaN")):
            with pytest.raises(RuntimeError, match="vkrh_set_reflection_lights: " + text):
                frame.set_reflection_lights(**kwargs)
        frame.run(host.STAGE_REFLECTIONS_RT)  # a refused call changed nothing
        base._sync()
        base._differing("after the refused calls", frame.download("reflections").raw(0), lit)
    finally:
        accel.close()
        frame.close()


def test_frame_stage_lit_fill_mode():
    """trace -> filter -> ReflectionsRTLit -> blur: texels with a valid screen-space ray keep the filter's value, the others are the
    lit entry's called by hand on the filter's output"""
    sc = scn.procedural_scene(detail=12, cutout=True)
    frame, setup = base._frame(sc)
    accel = abi.Accel.from_scene(sc)
    try:
        frame.load_scene(sc)
        frame.run(PRE)
        frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE)
        frame.pin_randoms(0.25, 3, 5)
        frame.run(host.STAGE_SSR_TRACE | host.STAGE_SSR_RESOLVE)
        base._sync()
        plain = frame.download("reflections").to_host().copy()
        filtered = frame.download("reflections").raw(0)
        frame.pin_randoms(0.25, 3, 5)
        frame.set_reflection_rays(fill_misses=True)
        frame.set_reflection_lights(**STOCK)
        frame.run(host.STAGE_REFLECTIONS_RT)
        base._sync()
        assert frame.last_tasks() == ["SSSR_trace", "SSSR_filter", "ReflectionsRTLit", "SSSR_blur"], frame.last_tasks()
        filled = frame.download("reflections").raw(0)
        kept = (frame.download("rays").raw(0)[..., 3] != 65535) & ((frame.download("depth").raw(1)[..., 0] & SKY) != SKY)
        assert kept.any() and np.array_equal(filled[kept], filtered[kept]), "a texel with a valid screen-space ray is not the filter's"
        base._differing("frame stage, lit, fill mode, against the entry called by hand on the filter's output", filled,
                        _by_hand(frame, setup, accel, True, STOCK, frame.hit_normals(), before=plain))
        assert (filled[~kept] != filtered[~kept]).any(), "no texel was filled"
    finally:
        accel.close()
        frame.close()


def test_frame_lit_reflections_follow_moving_draws():
    """after set_draw_transforms with a rotated sphere the lit image is the hand call's with the triangles and the normals of the new
    pose, and not the one with the normals of the old pose"""
    import copy

    sc = scn.procedural_scene(detail=12)
    frame, setup = base._frame(sc)
    a, b = np.radians(70.0), np.radians(40.0)
    rot = (np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]]) @
           np.array([[1, 0, 0, 0], [0, np.cos(b), -np.sin(b), 0], [0, np.sin(b), np.cos(b), 0], [0, 0, 0, 1]]))
    moved = copy.deepcopy(sc)
    models = [np.asarray(sc.transforms[d["transform"]][0], F32) for d in sc.draws]
    for i in (2, 3, 4):  # the three spheres turn about their own centres: the triangles land on the same sphere, every normal moves with its vertex
        models[i] = (models[i].astype(np.float64) @ rot).astype(F32)
        moved.draws[i]["transform"] = moved.add_transform(models[i])
    accel = abi.Accel.from_scene(moved)
    try:
        frame.load_scene(sc)
        frame.run(PRE)
        frame.set_reflection_lights(**STOCK)
        stale = frame.hit_normals()
        frame.set_draw_transforms(models)
        frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE | host.STAGE_REFLECTIONS_RT)
        base._sync()
        assert frame.last_tasks()[-2:] == ["ReflectionsRTLit", "SSSR_blur"]
        got = frame.download("reflections").raw(0)
        normals = frame.hit_normals()
        want = abi.scene_triangle_normals(moved)
        assert np.allclose(normals["n"], want["n"], rtol=0, atol=1e-5), "the refit's normals are not those of the new pose"
        assert not np.allclose(normals["n"], stale["n"], rtol=0, atol=1e-3)
        frame.scene = moved  # the textures and attributes are the same; the hand call's structure is the moved one
        base._differing("lit frame after set_draw_transforms, against the entry called by hand in the new pose", got,
                        _by_hand(frame, setup, accel, False, STOCK, normals))
        old = _by_hand(frame, setup, accel, False, STOCK, stale)
        assert (old != got).any(), "stale normals give the same image: the normals do not matter here"
    finally:
        accel.close()
        frame.close()
