"""The ray-traced shadow mask without a GPU: the C-ABI block and the program table, every refusal of vkr_shadow_mask_rt and of
the frame stage (validation never reaches a launch), and known answers for the numpy restatement
(tests/shadow_mask_rt_reference.py): a unit quad hangs one unit over a floor; under a point light its shadow on the floor is the
central projection of the quad from the light, under a directional light the parallel projection; pixels well inside the
projected outline read 0, pixels well outside it 255, and a surface that faces away from the light reads 0 whatever the scene
holds.

Measured here (oracle rasteriser, 96 x 64 camera above the floor): point light: 236 floor pixels inside the projected outline (all
0), 5537 outside (all 255), 302 pixels of the quad's own top (all 255); directional light: 131 inside, 5633 outside."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from vk_renderer_amd import abi, camera, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PostFxChain

import shadow_mask_rt_reference as ref
from test_abi_errors import ERR_EXTENT, ERR_FORMAT, ERR_NULL, img

F32 = np.float32
D24 = abi.FMT_D24_UNORM_S8
RG16 = abi.FMT_RG16_UNORM
RGBA8 = abi.FMT_RGBA8_UNORM
SKY = 0xFFFFFF


# ---- struct size and symbols ------------------------------------------------------------------------------------------------------
def test_block_layout_and_symbols():
    txt = open(abi.ROOT + "/include/vkr_postfx.h").read()
    body = re.search(r"typedef struct vkr_shadow_rt_params \{(.*?)\} vkr_shadow_rt_params;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size, offsets = 0, {}
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind, names = decl.split(None, 1)
        unit = {"vkr_mat4": 64, "float": 4, "uint32_t": 4}[kind]
        for name in names.split(","):
            offsets[re.match(r"\s*(\w+)", name).group(1)] = size
            count = 1
            for m in re.finditer(r"\[(\d+)\]", name):
                count *= int(m.group(1))
            size += unit * count
    # a matrix, the camera's four floats, four lights of four floats and four words
    assert size == 64 + 16 + 64 + 16 == 160
    assert C.sizeof(abi.ShadowRtParams) == size
    assert offsets == {"inverse_camera": 0, "fovy": 64, "aspect": 68, "znear": 72, "zfar": 76, "lights": 80, "light_count": 144,
                       "normal_offset": 148, "tmin": 152, "reserved": 156}
    for name, off in offsets.items():
        assert getattr(abi.ShadowRtParams, name).offset == off, name
    assert "int vkr_shadow_mask_rt(" in txt and "int vkr_accel_occluded(" in txt
    lib = abi.product()
    assert hasattr(lib, "vkr_shadow_mask_rt") and hasattr(lib, "vkr_accel_occluded")


def test_program_and_stage_are_registered():
    assert host.lib().vkrh_has_program(b"shadow_mask_rt") == 1
    assert host.STAGE_SHADOW_MASK_RT == 1 << 29
    assert hasattr(host.lib(), "vkrh_set_shadow_rays")
    chain_bits = (1 << 3) | (1 << 5) | (1 << 6) | (1 << 7)
    assert host.STAGE_CHAIN == chain_bits and not (host.STAGE_CHAIN & host.STAGE_SHADOW_MASK_RT)


# ---- error paths ------------------------------------------------------------------------------------------------------------------
W, H = 64, 32


@functools.lru_cache(maxsize=None)
def _empty_accel():
    return abi.Accel(np.zeros((0, 3, 3), F32))  # no triangles: nothing is allocated on a device


def _params(**over):
    lights = over.pop("lights", [(0.0, 4.0, 4.0, 1.0), (1.0, 2.0, 0.0, 0.0)])
    p = abi.shadow_rt_params(np.eye(4), lights, 1.0, 2.0, 0.05, 80.0, normal_offset=1e-3, tmin=over.pop("tmin", 0.0))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _call(depth="ok", normal="ok", accel="ok", params="ok", out="ok"):
    lib = abi.product()
    d = img(D24, W, H) if depth == "ok" else depth
    n = img(RG16, W, H) if normal == "ok" else normal
    o = img(RGBA8, W, H) if out == "ok" else out
    p = _params() if params == "ok" else params
    a = _empty_accel().handle if accel == "ok" else accel
    byref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    rc = lib.vkr_shadow_mask_rt(byref(d), byref(n), a, byref(p), byref(o), None)
    return rc, (lib.vkr_last_error() or b"").decode()


WINDOW = dict(full=(W, 2 * H), origin=(0, 2))
REFUSALS = {
    "depth NULL": (dict(depth=None), ERR_NULL, "depth is NULL"),
    "normal NULL": (dict(normal=None), ERR_NULL, "normal is NULL"),
    "accel NULL": (dict(accel=None), ERR_NULL, "NULL acceleration structure"),
    "params NULL": (dict(params=None), ERR_NULL, "params is NULL"),
    "out NULL": (dict(out=None), ERR_NULL, "out_mask is NULL"),
    "depth without memory": (dict(depth=img(D24, W, H, base=None)), ERR_NULL, "shadow_mask_rt.depth: NULL image"),
    "normal without memory": (dict(normal=img(RG16, W, H, base=None)), ERR_NULL, "shadow_mask_rt.normal: NULL image"),
    "out without memory": (dict(out=img(RGBA8, W, H, base=None)), ERR_NULL, "shadow_mask_rt.out_mask: NULL image"),
    "depth format": (dict(depth=img(abi.FMT_R32_SFLOAT, W, H)), ERR_FORMAT, "shadow_mask_rt.depth: format"),
    "normal format": (dict(normal=img(abi.FMT_RG16_SFLOAT, W, H)), ERR_FORMAT, "shadow_mask_rt.normal: format"),
    "out format": (dict(out=img(abi.FMT_RGBA8_SRGB, W, H)), ERR_FORMAT, "shadow_mask_rt.out_mask: format"),
    "out extent": (dict(out=img(RGBA8, W, H + 1)), ERR_EXTENT, "one extent expected"),
    "normal extent": (dict(normal=img(RG16, W // 2, H // 2)), ERR_EXTENT, "one extent expected"),
    "extent above 65535": (dict(depth=img(D24, 65536, 1), normal=img(RG16, 65536, 1), out=img(RGBA8, 65536, 1)), ERR_EXTENT,
                           "at most 65535 texels a side"),
    "windowed depth": (dict(depth=img(D24, W, H, **WINDOW)), ERR_EXTENT, "depth: windows are not supported"),
    "windowed normal": (dict(normal=img(RG16, W, H, **WINDOW)), ERR_EXTENT, "normal: windows are not supported"),
    "windowed out": (dict(out=img(RGBA8, W, H, full=(W, 2 * H), origin=(0, 0))), ERR_EXTENT, "out_mask: windows are not supported"),
    "light_count 0": (dict(params=_params(light_count=0)), ERR_EXTENT, "light_count 0"),
    "light_count 5": (dict(params=_params(light_count=5)), ERR_EXTENT, "light_count 5"),
    "light w 0.5": (dict(params=_params(lights=[(0, 4, 4, 1), (1, 2, 0, 0.5)])), ERR_EXTENT, "light 1 has w = 0.5"),
    "light w NaN": (dict(params=_params(lights=[(0, 4, 4, float("nan"))])), ERR_EXTENT, "light 0 has w = nan"),
    "reserved": (dict(params=_params(reserved=7)), ERR_EXTENT, "reserved is 7"),
    "tmin NaN": (dict(params=_params(tmin=float("nan"))), ERR_EXTENT, "tmin is NaN"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_shadow_mask_rt_refusals(name):
    kwargs, code, message = REFUSALS[name]
    rc, msg = _call(**kwargs)
    assert rc == code, (name, rc, msg)
    assert message in msg, (name, msg)


def test_a_light_beyond_light_count_is_not_looked_at():
    """only the lights in use are validated: the refusal list ends where the launch would begin, and a launch needs a device, so
    the call is made with a depth descriptor that is refused next"""
    p = _params(lights=[(0, 4, 4, 1)])
    p.lights[1][3] = 0.5
    rc, msg = _call(params=p, depth=img(abi.FMT_R32_SFLOAT, W, H))
    assert rc == ERR_FORMAT and "shadow_mask_rt.depth: format" in msg


# ---- the frame stage's refusals: before anything is recorded, so a frame on host memory will do ---------------------------------------
_LIVE = {}


def _host_alloc(nbytes, _user):
    a = np.zeros(int(nbytes) + 64, np.uint8)
    _LIVE[a.ctypes.data] = a
    return a.ctypes.data


def _host_free(ptr, _user):
    _LIVE.pop(ptr, None)


_ALLOC, _FREE = host._ALLOC(_host_alloc), host._FREE(_host_free)


class _HostMemoryFrame:
    """vkrh_create on host memory: enough for everything vkrh_run refuses before it records"""

    def __init__(self, tiled):
        l = host.lib()
        l.vkrh_set_allocator(_ALLOC, _FREE, None)
        setup = FrameSetup(64, 36)
        cfg = host.HostConfig(64, 36, 0, 0, 64, 36, 1 if tiled else 0, C.c_void_p(None))
        self.h = C.c_void_p(l.vkrh_create(C.byref(cfg)))
        assert self.h, l.vkrh_last_error()
        cam = host.HostCamera()
        cam.view, cam.prev_view, cam.projection = host._mat16(setup.view), host._mat16(setup.prev_view), host._mat16(setup.proj)
        cam.fovy, cam.aspect, cam.znear, cam.zfar = [float(v) for v in setup.fazz]
        assert l.vkrh_set_camera(self.h, C.byref(cam)) == 0

    def run(self, mask):
        l = host.lib()
        rc = l.vkrh_run(self.h, mask)
        return rc, l.vkrh_last_error().decode()

    def set_rays(self, lights, normal_offset=1e-3, tmin=0.0, count=None):
        l = host.lib()
        flat = (C.c_float * (4 * len(lights)))(*[float(x) for v in lights for x in v])
        rc = l.vkrh_set_shadow_rays(self.h, flat, len(lights) if count is None else count, normal_offset, tmin)
        return rc, l.vkrh_last_error().decode()

    def close(self):
        host.lib().vkrh_destroy(self.h)


def test_frame_stage_refusals():
    frame = _HostMemoryFrame(tiled=False)
    try:
        rc, msg = frame.run(host.STAGE_SHADOW_MASK_RT | host.STAGE_SHADOW_MASK)
        assert rc != 0 and "VKRH_STAGE_SHADOW_MASK_RT together with VKRH_STAGE_SHADOW_MASK" in msg
        rc, msg = frame.run(host.STAGE_SHADOW_MASK_RT | host.STAGE_SHADOW_MASK | host.STAGE_SHADOW)
        assert rc != 0 and "VKRH_STAGE_SHADOW_MASK_RT together with VKRH_STAGE_SHADOW_MASK" in msg
        rc, msg = frame.run(host.STAGE_SHADOW_MASK_RT)
        assert rc != 0 and "VKRH_STAGE_SHADOW_MASK_RT without a loaded scene" in msg
        rc, msg = frame.run(host.STAGE_GBUFFER | host.STAGE_SHADOW_MASK_RT | host.STAGE_SHADING)
        assert rc != 0 and "VKRH_STAGE_SHADOW_MASK_RT without a loaded scene" in msg
        for lights, count, text in (([(0, 1, 0, 1)], 0, "count 0"), ([(0, 1, 0, 1)] * 5, 5, "count 5"),
                                    ([(0, 1, 0, 1), (0, 1, 0, 2)], 2, "light 1: w must be 1")):
            rc, msg = frame.set_rays(lights, count=count)
            assert rc != 0 and text in msg, msg
        rc, msg = frame.set_rays([(0, 1, 0, 1)], tmin=float("nan"))
        assert rc != 0 and "tmin is NaN" in msg
        assert host.lib().vkrh_set_shadow_rays(frame.h, None, 1, 1e-3, 0.0) != 0
        assert frame.set_rays([(0, 1, 0, 1), (1, 2, 0, 0)], 1e-2, 1e-3)[0] == 0
    finally:
        frame.close()


def test_frame_stage_is_refused_on_a_tiled_frame():
    frame = _HostMemoryFrame(tiled=True)
    try:
        rc, msg = frame.run(host.STAGE_SHADOW_MASK_RT)
        assert rc != 0 and "VKRH_STAGE_SHADOW_MASK_RT on a tiled frame" in msg
        rc, msg = frame.set_rays([(0, 1, 0, 1)])
        assert rc != 0 and "vkrh_set_shadow_rays: on a tiled frame" in msg
    finally:
        frame.close()


# ---- known answers of the restatement -----------------------------------------------------------------------------------------------
CAM_W, CAM_H = 96, 64
QUAD_Y, QUAD_C, QUAD_R = 1.0, (0.0, 4.0), 0.5  # the unit quad: height, centre (x, z), half edge
POINT = (0.0, 4.0, 4.0, 1.0)                      # a point light three units above the quad's centre
SUN = (2.0, 4.0, 0.0, 0.0)                        # a directional light: the shadow is the quad moved by -QUAD_Y * 2 / 4 in x
GUARD = 0.05                                      # world units either side of the projected outline that are not judged


def _trs(t, s):
    return np.array([[s[0], 0, 0, t[0]], [0, s[1], 0, t[1]], [0, 0, s[2], t[2]], [0, 0, 0, 1]], dtype=F32)


@functools.lru_cache(maxsize=None)
def quad_case():
    """-> dict(depth words [64, 96], normal codes [64, 96, 2], setup, tris, world [64, 96, 3] float64 (analytic), floor, top)"""
    sc = scn.Scene()
    quad = sc.add_mesh(np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], F32), np.array([[0, 1, 0]] * 4, F32),
                       np.zeros((4, 2), F32), np.array([0, 2, 1, 0, 3, 2], np.uint32))
    sc.add_draw(sc.add_transform(_trs((0, 0, 6), (6, 1, 6))), quad)                                      # the floor, y = 0
    sc.add_draw(sc.add_transform(_trs((QUAD_C[0], QUAD_Y, QUAD_C[1]), (QUAD_R, 1, QUAD_R))), quad)    # the unit quad over it
    setup = FrameSetup(CAM_W, CAM_H)
    f32 = lambda a: np.asarray(a, dtype=F32).astype(np.float64)  # noqa: E731
    setup.view = f32(camera.look_at_rh((-0.2, 3.0, 2.0), (-0.2, 0.0, 4.0), (0.0, -1.0, 0.0)))
    setup.prev_view = setup.view
    setup.mvp = setup.prev_mvp = f32(setup.proj @ setup.view)
    setup.inv_view = setup.prev_inv_view = f32(np.linalg.inv(setup.view))
    chain = PostFxChain(CAM_W, CAM_H, backend="oracle", setup=setup)
    chain.raster(sc)
    depth = chain.depth.raw(0)[..., 0].astype(np.uint32)
    normal = chain.normal.raw(0).copy()
    gy, gx = np.mgrid[0:CAM_H, 0:CAM_W]
    d = (depth & SKY).astype(np.float64) / float(SKY)
    ndc = np.stack([(gx + 0.5) / CAM_W * 2 - 1, (gy + 0.5) / CAM_H * 2 - 1, d, np.ones_like(d)], axis=-1).reshape(-1, 4)
    w = ndc @ np.linalg.inv(setup.mvp).T
    world = (w[:, :3] / w[:, 3:4]).reshape(CAM_H, CAM_W, 3)
    geometry = (depth & SKY) != SKY
    floor = geometry & (np.abs(world[..., 1]) < 0.01)
    top = geometry & (np.abs(world[..., 1] - QUAD_Y) < 0.01)
    return dict(depth=depth, normal=normal, setup=setup, tris=abi.scene_triangles(sc), world=world, floor=floor, top=top)


def quad_classes(case, centre, half):
    """(inside, outside): floor pixels at least GUARD inside / outside the square |x - cx| <= half, |z - cz| <= half"""
    dx, dz = np.abs(case["world"][..., 0] - centre[0]), np.abs(case["world"][..., 2] - centre[1])
    inside = case["floor"] & (dx <= half - GUARD) & (dz <= half - GUARD)
    outside = case["floor"] & ((dx >= half + GUARD) | (dz >= half + GUARD))
    return inside, outside


def quad_outline(light):
    """the analytic shadow of the quad on the floor y = 0: (centre (x, z), half edge)"""
    if light[3] == 1.0:  # central projection from the light: a scaling by ly / (ly - QUAD_Y) about the light's foot
        k = light[1] / (light[1] - QUAD_Y)
        return (light[0] + (QUAD_C[0] - light[0]) * k, light[2] + (QUAD_C[1] - light[2]) * k), QUAD_R * k
    return (QUAD_C[0] - QUAD_Y * light[0] / light[1], QUAD_C[1] - QUAD_Y * light[2] / light[1]), QUAD_R


def check_quad_mask(case, light, channel):
    centre, half = quad_outline(light)
    inside, outside = quad_classes(case, centre, half)
    figures = f"light {light}: outline centre {centre} half {half:.4f}, {int(inside.sum())} pixels inside, {int(outside.sum())} outside, {int(case['top'].sum())} on the quad"
    print("[shadow mask rt]", figures)
    assert inside.sum() >= 100 and outside.sum() >= 100 and case["top"].sum() >= 100, figures
    assert (channel[inside] == 0).all(), figures
    assert (channel[outside] == 255).all(), figures
    assert (channel[case["top"]] == 255).all(), figures  # nothing lies between the quad's top and either light


def _arith():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


def _mask(case, lights, tris=None, normal_offset=1e-3, tmin=0.0):
    s = case["setup"]
    return ref.shadow_mask_rt(_arith(), case["depth"], case["normal"], s.inv_view, *s.fazz, lights, normal_offset, tmin,
                              case["tris"] if tris is None else tris)


def test_known_answer_point_and_directional():
    case = quad_case()
    mask = _mask(case, [POINT, SUN])
    assert (mask[..., 2:] == 255).all()
    sky = (case["depth"] & SKY) == SKY
    assert (mask[sky] == 255).all()
    assert set(np.unique(mask).tolist()) <= {0, 255}
    check_quad_mask(case, POINT, mask[..., 0])
    check_quad_mask(case, SUN, mask[..., 1])
    assert quad_outline(POINT) == ((0.0, 4.0), QUAD_R * 4.0 / 3.0) and quad_outline(SUN) == ((-0.5, 4.0), QUAD_R)


def test_a_surface_facing_away_reads_zero_without_any_triangle():
    case = quad_case()
    geometry = (case["depth"] & SKY) != SKY
    below = [(0.0, -3.0, 4.0, 1.0), (0.0, -1.0, 0.0, 0.0)]  # a point light under the floor, a directional light from below
    mask = _mask(case, below, tris=np.zeros((0, 3, 3), F32))
    assert geometry.sum() >= 1000
    assert (mask[geometry][:, :2] == 0).all() and (mask[geometry][:, 2:] == 255).all()
    assert (mask[~geometry] == 255).all()
    # the same empty scene lit from above: every surface that faces the light is lit
    mask = _mask(case, [POINT, SUN], tris=np.zeros((0, 3, 3), F32))
    assert (mask == 255).all()


def test_a_nan_light_and_a_light_at_the_surface_read_zero():
    case = quad_case()
    s = case["setup"]
    geometry = (case["depth"] & SKY) != SKY
    mask = _mask(case, [(float("nan"), 4.0, 4.0, 1.0), (0.0, float("nan"), 0.0, 0.0)])
    assert (mask[geometry][:, :2] == 0).all()
    _, origin, _ = ref.pixel_origins(_arith(), case["depth"], case["normal"], s.inv_view, *s.fazz, 1e-3)
    y, x = np.argwhere(case["floor"])[0]
    at = tuple(float(v) for v in origin[y, x]) + (1.0,)
    mask = _mask(case, [at])
    assert mask[y, x, 0] == 0, "a light exactly at the pixel's origin: dvec = 0, facing = 0, no ray"
