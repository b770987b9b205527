"""Program shadow_mask_rt on the GPU: the mask byte for byte against the numpy restatement (tests/shadow_mask_rt_reference.py) at
8 x 8 (one wave), 17 x 9 (partial tiles on both axes) and 64 x 36, with 1 to 4 lights, point and directional mixed, on the
procedural scene and on the G-buffer content at which a wave-wide walk goes wrong (nothing live, live and dead lanes alternating
per pixel and per 8 x 8 tile, every normal facing away, a light inside a sphere, a light exactly at a pixel's ray origin, a NaN
light); the channels beyond light_count, the bytes outside the mask's rows, an empty structure; and the frame stage
STAGE_SHADOW_MASK_RT: against the entry called by hand, applied by the shading, absent, and on the plane-only scene that fixes
the default normal offset."""
import ctypes as C
import functools

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import LIGHT_POS, FrameSetup
from vk_renderer_amd.chain import PostFxChain
from vk_renderer_amd.images import ImageBuf

import camera_cases as cc
import gbuffer_content as content
import shadow_mask_rt_reference as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0xA5
SKY = 0xFFFFFF
SIZES = [(8, 8), (17, 9), (64, 36), (1, 1), (1, 9), (9, 1)]  # a wave is an 8 x 8 tile: the last three are one live lane, one live column, one live row
POINT_A = tuple(LIGHT_POS) + (1.0,)
POINT_B = (3.0, 4.0, 2.0, 1.0)
SUN_A = (1.5, 4.5, -1.5, 0.0)    # long enough to leave the scene from anywhere in it
SUN_B = (-6.0, 9.0, 3.0, 0.0)
LIGHT_SETS = {1: [POINT_A], 2: [SUN_A, POINT_B], 3: [POINT_B, SUN_B, POINT_A], 4: [POINT_A, SUN_A, POINT_B, SUN_B]}
IN_SPHERE = (0.3, 1.4, 6.0, 1.0)  # the centre of the large sphere of scene.procedural_scene
OFFSET, TMIN = abi.SHADOW_RT_NORMAL_OFFSET, abi.SHADOW_RT_TMIN  # the frame's defaults


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch

    torch.cuda.synchronize()


def _arith():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


@functools.lru_cache(maxsize=None)
def _scene():
    sc = scn.procedural_scene(detail=8)
    return sc, abi.scene_triangles(sc)


@functools.lru_cache(maxsize=None)
def _raster(size):
    """-> (depth words [h, w], normal codes [h, w, 2], setup): the procedural scene through the oracle's rasteriser at the next
    even extent (the flat chain driver only takes those), cut to size"""
    w, h = size
    ew, eh = w + (w & 1), h + (h & 1)
    setup = cc.frame_setup(size, ew, eh)  # the frozen camera, or the case an Extent names
    chain = PostFxChain(ew, eh, backend="oracle", setup=setup)
    chain.raster(_scene()[0])
    return chain.depth.raw(0)[:h, :w, 0].astype(np.uint32), chain.normal.raw(0)[:h, :w].copy(), setup


class _Gbuffer:
    """what a content class of tests/gbuffer_content.py touches of a chain: host images of the two inputs of the pass"""

    def __init__(self, size):
        w, h = size
        words, codes, self.setup = _raster(size)
        self.depth = self.prev_depth = ImageBuf(abi.FMT_D24_UNORM_S8, w, h)
        self.normal = ImageBuf(abi.FMT_RG16_UNORM, w, h)
        self.depth.set_raw(words.reshape(h, w, 1))
        self.normal.set_raw(codes)


def _checker_tile8(c, rng):
    x, y = content._grid(c.depth)
    content._set_depth(c.depth, SKY, (((x // 8) + (y // 8)) & 1) == 1)


def _facing_away(c, rng):
    # (0, -1, 0): away from every directional light of LIGHT_SETS and from a point light wherever it stands higher than the surface
    codes = np.zeros((c.normal.height, c.normal.width, 2), np.uint16)
    codes[..., 0] = 32768
    c.normal.set_raw(codes)


CLASSES = {"raster": lambda c, rng: None, "sky_all": content.sky_all, "checker_px": content.checker_px, "checker_tile8": _checker_tile8,
           "facing_away": _facing_away, "normal_noise": content.normal_noise, "normal_poles": content.normal_poles}


@functools.lru_cache(maxsize=None)
def _inputs(name, size):
    g = _Gbuffer(size)
    CLASSES[name](g, np.random.default_rng([0x5AD0, sorted(CLASSES).index(name), size[0], size[1]]))
    return g.depth.raw(0)[..., 0].copy(), g.normal.raw(0).copy(), g.setup, g.depth.to_host().copy(), g.normal.to_host().copy()


@functools.lru_cache(maxsize=None)
def _expected(name, size, lights, empty=False):
    words, codes, setup, _, _ = _inputs(name, size)
    tris = np.zeros((0, 3, 3), F32) if empty else _scene()[1]
    return ref.shadow_mask_rt(_arith(), words, codes, setup.inv_view, *setup.fazz, list(lights), OFFSET, TMIN, tris)


@functools.lru_cache(maxsize=None)
def _accel(empty=False):
    return abi.Accel(np.zeros((0, 3, 3), F32) if empty else _scene()[1])


def _launch(name, size, lights, empty=False):
    """-> the RGBA8 codes [h, w, 4] of vkr_shadow_mask_rt; checks that nothing outside the rows was written"""
    w, h = size
    _, _, setup, depth_bytes, normal_bytes = _inputs(name, size)
    depth = ImageBuf(abi.FMT_D24_UNORM_S8, w, h, device="cuda")
    normal = ImageBuf(abi.FMT_RG16_UNORM, w, h, device="cuda")
    depth.upload(depth_bytes)
    normal.upload(normal_bytes)
    out = ImageBuf(abi.FMT_RGBA8_UNORM, w, h, device="cuda", fill=FILL)
    params = abi.shadow_rt_params(setup.inv_view, list(lights), *setup.fazz, normal_offset=OFFSET, tmin=TMIN)
    abi.shadow_mask_rt(depth.desc(), normal.desc(), _accel(empty), params, out.desc(), _stream())
    _sync()
    host_bytes = out.to_host()
    rows = host_bytes[: out.pitch[0] * h].reshape(h, out.pitch[0])
    assert (rows[:, 4 * w:] == FILL).all() and (host_bytes[out.pitch[0] * h:] == FILL).all(), "bytes outside the image were written"
    return out.raw(0, host_bytes)


def _differing(name, got, want):
    bad = (got != want).any(axis=-1)
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} texels differ, first at {tuple(np.argwhere(bad)[0])}: "
                           f"{got[bad][:4].tolist()} != {want[bad][:4].tolist()}")


# ---- byte for byte against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", sorted(LIGHT_SETS))
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", sorted(CLASSES))
def test_parity(name, size, count):
    lights = tuple(LIGHT_SETS[count])
    want = _expected(name, size, lights)
    got = _launch(name, size, lights)
    geometry = (_inputs(name, size)[0] & SKY) != SKY
    print(f"[shadow mask rt] {name} {size[0]}x{size[1]} {count} lights: {int(geometry.sum())} geometry pixels, per channel 0s "
          f"{[int((want[..., l][geometry] == 0).sum()) for l in range(count)]}, differing texels {int((got != want).any(axis=-1).sum())}")
    _differing(f"{name} {size} {count} lights", got, want)
    assert (got[..., count:] == 255).all(), "a channel at or beyond light_count is not 255"
    assert (got[~geometry] == 255).all()
    assert set(np.unique(got).tolist()) <= {0, 255}
    if name == "sky_all":
        assert not geometry.any()
    if name == "facing_away":  # every directional light shines downwards (the point lights stand below the top of the back wall)
        assert geometry.any() and all((got[..., l][geometry] == 0).all() for l, light in enumerate(lights) if light[3] == 0.0)
    if name == "raster" and size == (64, 36):  # the scene shadows some pixels and not others, under every light
        for l in range(count):
            assert (want[..., l][geometry] == 0).any() and (want[..., l][geometry] == 255).any(), l


@pytest.mark.parametrize("size", SIZES)
def test_light_inside_a_sphere_and_nan_light(size):
    """a point light at the centre of the closed sphere reaches nothing: outside points are shadowed by the sphere, the sphere's
    own surface faces away; a NaN light casts no ray; the third light is an ordinary one"""
    lights = (IN_SPHERE, (float("nan"), 4.0, 2.0, 1.0), POINT_B)
    want = _expected("raster", size, lights)
    got = _launch("raster", size, lights)
    _differing(f"light inside a sphere {size}", got, want)
    geometry = (_inputs("raster", size)[0] & SKY) != SKY
    assert geometry.any() and (got[geometry][:, :2] == 0).all() and (got[..., 3] == 255).all()


@pytest.mark.parametrize("size", SIZES)
def test_light_exactly_at_a_pixels_origin(size):
    words, codes, setup, _, _ = _inputs("raster", size)
    _, origin, _ = ref.pixel_origins(_arith(), words, codes, setup.inv_view, *setup.fazz, OFFSET)
    y, x = np.argwhere((words & SKY) != SKY)[len(words) // 2]
    lights = (tuple(float(v) for v in origin[y, x]) + (1.0,), SUN_A)
    want = _expected("raster", size, lights)
    got = _launch("raster", size, lights)
    _differing(f"light at the origin of pixel ({x}, {y}) {size}", got, want)
    assert got[y, x, 0] == 0, "dvec = 0: facing = 0, the channel is 0 and no ray is cast"


@pytest.mark.parametrize("size", SIZES)
def test_empty_structure(size):
    """node_count == 0 is legal: a pixel reads 255 in the channels of the lights it faces and 0 in the others"""
    lights = tuple(LIGHT_SETS[4])
    for name in ("raster", "normal_noise"):
        want = _expected(name, size, lights, empty=True)
        got = _launch(name, size, lights, empty=True)
        _differing(f"empty structure {name} {size}", got, want)
        words, codes, setup, _, _ = _inputs(name, size)
        _, origin, normal = ref.pixel_origins(_arith(), words, codes, setup.inv_view, *setup.fazz, OFFSET)
        geometry = (words & SKY) != SKY
        for l, light in enumerate(lights):
            _, cast = ref.light_rays(_arith(), origin.reshape(-1, 3), normal.reshape(-1, 3), light)
            assert np.array_equal(got[..., l][geometry] == 255, cast.reshape(geometry.shape)[geometry])


# ---- the frame stage ----------------------------------------------------------------------------------------------------------------
W, H = 256, 144


def _by_hand(frame, setup, accel, lights, normal_offset, tmin):
    out = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda", fill=FILL)
    params = abi.shadow_rt_params(setup.inv_view, lights, *setup.fazz, normal_offset=normal_offset, tmin=tmin)
    abi.shadow_mask_rt(frame.image("depth", 0, 1), frame.image("normal"), accel, params, out.desc(), _stream())
    _sync()
    return out.raw(0)


def test_frame_stage():
    sc = scn.procedural_scene(detail=12, cutout=True)
    setup = FrameSetup(W, H)
    frame = host.HostFrame(setup, device="cuda")
    accel = abi.Accel.from_scene(sc)
    try:
        with pytest.raises(RuntimeError, match="VKRH_STAGE_SHADOW_MASK_RT without a loaded scene"):
            frame.run(host.STAGE_GBUFFER | host.STAGE_SHADOW_MASK_RT)
        frame.load_scene(sc)
        with pytest.raises(RuntimeError, match="VKRH_STAGE_SHADOW_MASK_RT together with VKRH_STAGE_SHADOW_MASK"):
            frame.run(host.STAGE_RASTER | host.STAGE_SHADOW | host.STAGE_SHADOW_MASK | host.STAGE_SHADOW_MASK_RT)
        assert "ShadowMaskRT" not in frame.last_tasks()
        with pytest.raises(RuntimeError, match="'shadow_mask' only exists after"):
            frame.image("shadow_mask")
        # the defaults: one point light at LIGHT_POS, the measured offsets
        frame.run(host.STAGE_RASTER | host.STAGE_SHADOW_MASK_RT)
        _sync()
        assert frame.last_tasks() == ["GbufferPass", "ShadowMaskRT"], frame.last_tasks()
        d = frame.image("shadow_mask")
        assert (d.format, d.width, d.height) == (abi.FMT_RGBA8_UNORM, W, H)
        staged = frame.download("shadow_mask").raw(0)
        _differing("frame stage, defaults, against the entry called by hand", staged, _by_hand(frame, setup, accel, [POINT_A], OFFSET, TMIN))
        a = staged[..., 0]
        assert (staged[..., 1:] == 255).all() and (a == 0).any() and (a == 255).any()
        # lights and offsets of vkrh_set_shadow_rays; the stage alone, on the G-buffer of the earlier run
        lights = [POINT_B, SUN_A, POINT_A]
        frame.set_shadow_rays(lights, normal_offset=5e-3, tmin=1e-4)
        frame.run(host.STAGE_SHADOW_MASK_RT)
        _sync()
        assert frame.last_tasks() == ["ShadowMaskRT"]
        again = frame.download("shadow_mask").raw(0)
        _differing("frame stage, three lights, against the entry called by hand", again, _by_hand(frame, setup, accel, lights, 5e-3, 1e-4))
        assert (again[..., 3] == 255).all() and not np.array_equal(again[..., 0], staged[..., 0])
        with pytest.raises(RuntimeError, match="light 0: w must be 1"):
            frame.set_shadow_rays([(0.0, 1.0, 0.0, 0.25)])
    finally:
        accel.close()
        frame.close()


def test_frame_applies_the_traced_mask_when_asked():
    """vkrh_set_shadow_mask(apply = 1): color_out of a run with STAGE_SHADOW_MASK_RT equals vkr_defered_shading_shadowed called by
    hand on the frame's images; with the default it equals vkr_defered_shading; a run without the stage shades plainly"""
    sc = scn.procedural_scene(detail=12, cutout=True)
    setup = FrameSetup(W, H)
    frame = host.HostFrame(setup, device="cuda")
    try:
        frame.load_scene(sc)
        frame.run(host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH)
        stages = host.STAGE_RASTER | host.STAGE_SHADOW_MASK_RT | host.STAGE_CHAIN | host.STAGE_SHADING
        consts = abi.ShadingParams()
        consts.inverse_camera = abi.Mat4.from_np(setup.inv_view)
        consts.camera = abi.Mat4.from_np(setup.view)
        consts.shadow_mvp = abi.Mat4.from_np(np.eye(4))  # no VKRH_STAGE_SHADOW ran: the frame hands the shading its dummy map
        consts.fovy, consts.aspect, consts.znear, consts.zfar = [float(v) for v in setup.fazz]
        push = abi.ShadingPush((C.c_float * 2)(0.0, 1.0), 0)
        lib = abi.product()

        def by_hand(shadowed):
            images = [frame.image(n) for n in ("albedo", "normal", "material", "depth")]
            tail = [frame.image(n) for n in ("acc_ao", "brdf", "blurred")]
            out = ImageBuf(abi.FMT_RGBA8_SRGB, W, H, device="cuda", fill=FILL)
            if shadowed:
                abi.defered_shading_shadowed(*images, consts, *tail, frame.image("shadow_mask"), out.desc(), push, _stream())
            else:
                abi.check(lib.vkr_defered_shading(*[C.byref(v) for v in images + [consts] + tail], C.byref(out.desc()), C.byref(push), _stream()), lib)
            _sync()
            return out.raw(0)

        for apply in (0, 1):
            frame.set_shadow_mask(apply=apply)
            frame.run(stages)
            _sync()
            tasks = frame.last_tasks()
            assert tasks.index("GbufferPass") < tasks.index("ShadowMaskRT") < tasks.index("DeferedShading"), tasks
            got = frame.download("color_out").raw(0)
            plain, shadowed = by_hand(False), by_hand(True)
            want = shadowed if apply else plain
            assert np.array_equal(got, want), f"apply {apply}: {int((got != want).any(axis=-1).sum())} texels differ from the entry called by hand"
            darker = int((shadowed.astype(int) < plain.astype(int)).any(axis=-1).sum())
            print(f"[shadow mask rt] frame, apply {apply}: {darker} texels of color_out are darker under the traced mask")
            assert darker >= 1 and (shadowed <= plain).all()
        frame.run(host.STAGE_SHADING)
        _sync()
        assert np.array_equal(frame.download("color_out").raw(0), by_hand(False))
    finally:
        frame.close()


def test_a_frame_without_the_stage_is_what_it_was():
    """the stage and its setter leave every other stage alone: a frame that traced a mask first and one that never did produce
    the same bytes from the same stages, and no task of the second run belongs to the stage"""
    sc = scn.procedural_scene(detail=12)
    stages = host.STAGE_RASTER | host.STAGE_CHAIN | host.STAGE_SHADING | host.STAGE_TAA
    outs = []
    for traced in (False, True):
        frame = host.HostFrame(FrameSetup(W, H), device="cuda")
        try:
            frame.pin_randoms(0.25, 3, 5)
            frame.load_scene(sc)
            frame.run(host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH)
            if traced:
                frame.set_shadow_rays([POINT_B, SUN_B], normal_offset=1e-2, tmin=1e-3)
                frame.run(host.STAGE_RASTER | host.STAGE_SHADOW_MASK_RT)
            else:
                frame.run(host.STAGE_RASTER)
            frame.run(stages)
            _sync()
            assert "ShadowMaskRT" not in frame.last_tasks()
            outs.append((frame.last_tasks(), {n: frame.download(n).to_host().copy() for n in ("color_out", "taa_target", "acc_ao", "blurred", "depth")}))
        finally:
            frame.close()
    assert outs[0][0] == outs[1][0]
    for n in outs[0][1]:
        assert np.array_equal(outs[0][1][n], outs[1][1][n]), f"{n} differs after a run of STAGE_SHADOW_MASK_RT"


def plane_scene():
    """a single large floor facing the default light, no occluder: the truth is "every non-sky pixel is lit\""""
    sc = scn.Scene()
    quad = sc.add_mesh(np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], F32), np.array([[0, 1, 0]] * 4, F32),
                       np.array([[0, 0], [8, 0], [8, 8], [0, 8]], F32), np.array([0, 2, 1, 0, 3, 2], np.uint32))
    m = np.array([[40, 0, 0, 0], [0, 1, 0, 0], [0, 0, 40, 30], [0, 0, 0, 1]], dtype=F32)
    sc.add_draw(sc.add_transform(m), quad)
    return sc


def plane_mask(width, height, normal_offset=None, tmin=0.0):
    """-> (light 0's channel [h, w], geometry [h, w]) of the frame stage on plane_scene() at the frame's default camera;
    normal_offset None: the frame's defaults"""
    frame = host.HostFrame(FrameSetup(width, height), device="cuda")
    try:
        frame.load_scene(plane_scene())
        if normal_offset is not None:
            frame.set_shadow_rays([POINT_A], normal_offset=normal_offset, tmin=tmin)
        frame.run(host.STAGE_RASTER | host.STAGE_SHADOW_MASK_RT)
        _sync()
        mask = frame.download("shadow_mask").raw(0)
        geometry = (frame.download("depth").raw(0)[..., 0] & SKY) != SKY
        return mask[..., 0], geometry
    finally:
        frame.close()


def test_plane_only_scene_has_no_acne_under_the_defaults():
    """the floor alone cannot shadow itself: under the frame's default normal_offset and tmin no pixel reads 0.  (The default is
    the smallest power of ten for which that holds at 256 x 144 and at 1920 x 1080; DESIGN.md 7.8 has the count one power below.)"""
    channel, geometry = plane_mask(W, H)
    acne = int((channel[geometry] == 0).sum())
    below, _ = plane_mask(W, H, normal_offset=OFFSET / 10.0)
    print(f"[shadow mask rt] plane only {W}x{H}: {int(geometry.sum())} floor pixels, {acne} read 0 at the default offset, "
          f"{int((below[geometry] == 0).sum())} at a tenth of it")
    assert geometry.sum() >= W * H // 4
    assert acne == 0
    assert (channel[~geometry] == 255).all()
