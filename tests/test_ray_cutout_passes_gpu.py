"""vkr_shadow_mask_rt_cutout and vkr_reflections_rt_cutout on the GPU, byte for byte against the numpy restatement
(tests/ray_cutout_reference.py), at 8 x 8 (one wave), 17 x 9 (partial tiles on both axes), 64 x 36 and the degenerate 1 x 1, 1 x 9,
9 x 1, on the procedural scene WITH its fence (a quad whose texture has alpha-0 holes, between the ground and two of the lights and
in front of the ground's mirror rays) rasterised by the oracle, and on G-buffer content classes of tests/gbuffer_content.py (live
and dead lanes alternating per pixel, noise normals); the mask with four lights, point and directional, the reflections in both
modes; every mask channel at least the opaque entry's on the same input; PostFxChain's cutouts= option; and the frame: the two
stages against the entries called by hand, the task orders, a frame that never called set_ray_cutouts and one that called it with
enable = 0 against today's entries, the mask with cutouts on differing from the opaque one with pixels in the fence's shadow lit."""
import functools

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PostFxChain
from vk_renderer_amd.images import ImageBuf

import camera_cases as cc
import gbuffer_content as content
import ray_cutout_reference as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0xA5
SKY = 0xFFFFFF
SIZES = [(8, 8), (17, 9), (64, 36), (1, 1), (1, 9), (9, 1)]
OFFSET, TMIN = abi.SHADOW_RT_NORMAL_OFFSET, abi.SHADOW_RT_TMIN
# behind the fence as the camera sees it (the fence stands at z = 5, x in [-2.5, 3.5], y up to 2.4): the ground in front of it lies
# in the fence's shadow; the shading pass's light; a directional light through the fence; one from the side
LIGHTS = [(0.5, 2.5, 8.0, 1.0), (-1.85867, 5.81832, -0.247114, 1.0), (0.2, 1.5, 4.0, 0.0), (-6.0, 2.0, 0.5, 0.0)]


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
    sc = scn.procedural_scene(detail=8, cutout=True)
    return sc, abi.scene_triangles(sc), abi.scene_triangle_attributes(sc), abi.scene_opaque_texture_mask(sc)


@functools.lru_cache(maxsize=None)
def _device_scene():
    import torch

    sc, _, att, _ = _scene()
    rs, keep = sc.upload(device="cuda")
    nbytes = abi.accel_cutout_scratch_bytes(rs.texture_count)
    return rs, torch.from_numpy(np.ascontiguousarray(att).view(np.uint8).copy()).to("cuda"), keep, nbytes, torch.empty(nbytes, dtype=torch.uint8, device="cuda")


@functools.lru_cache(maxsize=None)
def _accel():
    return abi.Accel(_scene()[1])


@functools.lru_cache(maxsize=None)
def _raster(size):
    w, h = size
    ew, eh = w + (w & 1), h + (h & 1)
    setup = cc.frame_setup(size, ew, eh)  # the frozen camera, or the case an Extent names
    chain = PostFxChain(ew, eh, backend="oracle", setup=setup)
    chain.raster(_scene()[0])
    return chain.depth.raw(0)[:h, :w, 0].astype(np.uint32), chain.normal.raw(0)[:h, :w].copy(), setup


class _Gbuffer:
    def __init__(self, size):
        w, h = size
        words, codes, self.setup = _raster(size)
        self.depth = self.prev_depth = ImageBuf(abi.FMT_D24_UNORM_S8, w, h)
        self.normal = ImageBuf(abi.FMT_RG16_UNORM, w, h)
        self.depth.set_raw(words.reshape(h, w, 1))
        self.normal.set_raw(codes)


CLASSES = {"raster": lambda c, rng: None, "checker_px": content.checker_px, "normal_noise": content.normal_noise}


@functools.lru_cache(maxsize=None)
def _inputs(name, size):
    g = _Gbuffer(size)
    CLASSES[name](g, np.random.default_rng([0xC07, sorted(CLASSES).index(name), size[0], size[1]]))
    return g.depth.raw(0)[..., 0].copy(), g.normal.raw(0).copy(), g.setup, g.depth.to_host().copy(), g.normal.to_host().copy()


def _upload(name, size):
    w, h = size
    _, _, setup, depth_bytes, normal_bytes = _inputs(name, size)
    depth = ImageBuf(abi.FMT_D24_UNORM_S8, w, h, device="cuda")
    normal = ImageBuf(abi.FMT_RG16_UNORM, w, h, device="cuda")
    depth.upload(depth_bytes)
    normal.upload(normal_bytes)
    return depth, normal, setup


def _rows_only(out, w, h):
    host_bytes = out.to_host()
    rows = host_bytes[: out.pitch[0] * h].reshape(h, out.pitch[0])
    assert (rows[:, 4 * w:] == FILL).all() and (host_bytes[out.pitch[0] * h:] == FILL).all(), "bytes outside the image were written"
    return out.raw(0, host_bytes)


def _differing(name, got, want):
    bad = (got != want).any(axis=-1)
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} texels differ, first at {tuple(np.argwhere(bad)[0])}: "
                           f"{got[bad][:4].tolist()} != {want[bad][:4].tolist()}")


# ---- the mask -------------------------------------------------------------------------------------------------------------------------
def _mask(name, size, cutout):
    """-> RGBA8 codes [h, w, 4]; cutout None: vkr_shadow_mask_rt"""
    w, h = size
    depth, normal, setup = _upload(name, size)
    out = ImageBuf(abi.FMT_RGBA8_UNORM, w, h, device="cuda", fill=FILL)
    params = abi.shadow_rt_params(setup.inv_view, LIGHTS, *setup.fazz, normal_offset=OFFSET, tmin=TMIN)
    if cutout is None:
        abi.shadow_mask_rt(depth.desc(), normal.desc(), _accel(), params, out.desc(), _stream())
    else:
        rs, attribs, _, nbytes, scratch = _device_scene()
        abi.shadow_mask_rt_cutout(depth.desc(), normal.desc(), _accel(), attribs.data_ptr(), len(_scene()[2]), rs.textures, rs.texture_count, params,
                                  cutout, out.desc(), scratch.data_ptr(), nbytes, _stream())
    _sync()
    return _rows_only(out, w, h)


@functools.lru_cache(maxsize=None)
def _mask_expected(name, size, lod, mask):
    words, codes, setup, _, _ = _inputs(name, size)
    sc, tris, att, _ = _scene()
    return ref.shadow_mask_rt_cutout(_arith(), words, codes, setup.inv_view, *setup.fazz, LIGHTS, OFFSET, TMIN, tris, att, sc.textures, lod, mask)


# (alpha_lod, the scene's own mask of textures without holes or none)
SETTINGS = {"lod0": (0, False), "lod0_masked": (0, True), "lod3_masked": (3, True)}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", sorted(CLASSES))
def test_mask_parity(name, size, setting):
    lod, masked = SETTINGS[setting]
    mask = _scene()[3] if masked else 0
    want = _mask_expected(name, size, lod, mask)
    got = _mask(name, size, abi.ray_cutout(lod, mask))
    opaque = _mask(name, size, None)
    print(f"[ray cutout] mask {name} {size[0]}x{size[1]} {setting}: differing texels {int((got != want).any(axis=-1).sum())}, "
          f"channels lit through holes {int(((got == 255) & (opaque == 0)).sum())}")
    _differing(f"mask {name} {size} {setting}", got, want)
    assert (got >= opaque).all(), "a channel is darker than the opaque entry's"
    assert np.isin(got, (0, 255)).all()


def test_the_reference_mask_sees_the_fence():
    """not vacuous: at 64 x 36 the opaque reference and the cutout reference differ, in the channels of the lights behind the fence,
    and the right hint changes nothing"""
    import shadow_mask_rt_reference as opaque_ref

    words, codes, setup, _, _ = _inputs("raster", (64, 36))
    sc, tris, att, mask = _scene()
    opaque = opaque_ref.shadow_mask_rt(_arith(), words, codes, setup.inv_view, *setup.fazz, LIGHTS, OFFSET, TMIN, tris)
    cut = _mask_expected("raster", (64, 36), 0, 0)
    lit = (cut == 255) & (opaque == 0)
    print(f"[ray cutout] reference mask 64x36: texels lit through holes per light {lit.reshape(-1, 4).sum(axis=0).tolist()}")
    assert lit[..., 0].sum() >= 1 and lit[..., 2].sum() >= 1 and (cut >= opaque).all()
    assert np.array_equal(cut, _mask_expected("raster", (64, 36), 0, mask))
    assert mask == 0b0111


# ---- the reflections ------------------------------------------------------------------------------------------------------------------
def _rays_w(size, fill):
    w, h = size
    y, x = np.mgrid[0:h, 0:w]
    valid_codes = ((x * 7 + y * 13) % 65535).astype(np.uint16)
    return np.where(((x + y) & 1) == 0, np.uint16(65535), valid_codes).astype(np.uint16)


def _reflections(name, size, fill, texture_lod, cutout):
    import torch

    w, h = size
    depth, normal, setup = _upload(name, size)
    rays = None
    if fill:
        host_rays = ImageBuf(abi.FMT_RGBA16_UNORM, w, h)
        codes = np.full((h, w, 4), 0x1234, np.uint16)
        codes[..., 3] = _rays_w(size, fill)
        host_rays.set_raw(codes)
        rays = ImageBuf(abi.FMT_RGBA16_UNORM, w, h, device="cuda")
        rays.upload(host_rays.to_host())
    out = ImageBuf(abi.FMT_RGBA8_UNORM, w, h, device="cuda", fill=FILL)
    rs, attribs, _, nbytes, scratch = _device_scene()
    params = abi.reflect_rt_params(setup.inv_view, *setup.fazz, fill_misses=fill, normal_offset=OFFSET, tmin=TMIN, texture_lod=texture_lod)
    args = (depth.desc(), normal.desc(), rays.desc() if fill else None, _accel(), attribs.data_ptr(), len(_scene()[2]), rs.textures, rs.texture_count, params)
    if cutout is None:
        abi.reflections_rt(*args, out.desc(), scratch.data_ptr(), nbytes, _stream())
    else:
        abi.reflections_rt_cutout(*args, cutout, out.desc(), scratch.data_ptr(), nbytes, _stream())
    _sync()
    return _rows_only(out, w, h)


@functools.lru_cache(maxsize=None)
def _reflections_expected(name, size, fill, texture_lod, lod, mask):
    words, codes, setup, _, _ = _inputs(name, size)
    sc, tris, att, _ = _scene()
    before = np.full(words.shape + (4,), FILL, np.uint8)
    return ref.reflections_rt_cutout(_arith(), words, codes, _rays_w(size, fill) if fill else None, setup.inv_view, *setup.fazz, OFFSET, TMIN,
                                     float(setup.fazz[3]), texture_lod, ref.FILL_MISSES if fill else 0, tris, att, sc.textures, before, lod, mask)


@pytest.mark.parametrize("fill", [False, True], ids=["all", "fill"])
@pytest.mark.parametrize("setting", ["lod0", "lod3_masked"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", sorted(CLASSES))
def test_reflections_parity(name, size, setting, fill):
    lod, masked = SETTINGS[setting]
    mask = _scene()[3] if masked else 0
    texture_lod = 1 if fill else 0
    want, traced, index = _reflections_expected(name, size, fill, texture_lod, lod, mask)
    got = _reflections(name, size, fill, texture_lod, abi.ray_cutout(lod, mask))
    print(f"[ray cutout] reflections {name} {size[0]}x{size[1]} {setting} {'fill' if fill else 'all'}: {int(traced.sum())} rays, "
          f"{int((index != ref.MISS).sum())} hits, differing texels {int((got != want).any(axis=-1).sum())}")
    _differing(f"reflections {name} {size} {setting} fill={fill}", got, want)


def test_the_reference_reflections_see_through_the_fence():
    import reflections_rt_reference as opaque_ref

    words, codes, setup, _, _ = _inputs("raster", (64, 36))
    sc, tris, att, _ = _scene()
    before = np.zeros(words.shape + (4,), np.uint8)
    opaque = opaque_ref.reflections_rt(_arith(), words, codes, None, setup.inv_view, *setup.fazz, OFFSET, TMIN, float(setup.fazz[3]), 0, 0, tris, att,
                                       sc.textures, before)
    cut = _reflections_expected("raster", (64, 36), False, 0, 0, 0)
    fence = np.nonzero(att["albedo_index"] == 3)[0]
    through = np.isin(opaque[2], fence) & ~np.isin(cut[2], fence)
    print(f"[ray cutout] reference reflections 64x36: {int(np.isin(opaque[2], fence).sum())} mirror rays meet the fence, {int(through.sum())} pass through a hole")
    assert through.sum() >= 1 and np.isin(cut[2], fence).any()


def test_chain_options():
    """PostFxChain.shadow_mask_rt(cutouts=) and .reflections_rt(cutouts=) are the entries on the chain's own images"""
    sc, tris, att, mask = _scene()
    cw, ch = 64, 36
    setup = FrameSetup(cw, ch)
    chain = PostFxChain(cw, ch, backend="product", device="cuda", setup=setup)
    chain.raster(sc)
    chain.downsample()
    rs, attribs, _, _, _ = _device_scene()
    cut = abi.ray_cutout(0, mask)
    chain.shadow_mask_rt(_accel(), LIGHTS, cutouts=(attribs, rs, cut))
    chain.reflections_rt(_accel(), attribs, rs, cutouts=cut)
    _sync()
    words, codes = chain.depth.raw(0)[..., 0].astype(np.uint32), chain.normal.raw(0)
    want = ref.shadow_mask_rt_cutout(_arith(), words, codes, setup.inv_view, *setup.fazz, LIGHTS, OFFSET, TMIN, tris, att, sc.textures, 0, mask)
    _differing("PostFxChain.shadow_mask_rt(cutouts=)", chain.shadow_mask_out.raw(0), want)
    words, codes = chain.depth.raw(1)[..., 0].astype(np.uint32), chain.dn.raw(0)
    want = ref.reflections_rt_cutout(_arith(), words, codes, None, setup.inv_view, *setup.fazz, OFFSET, TMIN, float(setup.fazz[3]), 0, 0, tris, att,
                                     sc.textures, np.zeros(words.shape + (4,), np.uint8), 0, mask)[0]
    _differing("PostFxChain.reflections_rt(cutouts=)", chain.reflections.raw(0), want)


# ---- the frame ------------------------------------------------------------------------------------------------------------------------
W, H = 128, 72
PRE = host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH
FRAME_LIGHTS = LIGHTS[:3]


def _frame_by_hand(frame, setup, accel, sc, cutout):
    """the two entries on the frame's own images -> (mask codes, reflections codes); cutout None: the opaque entries"""
    import torch

    rs, keep = sc.upload(device="cuda")
    att = abi.scene_triangle_attributes(sc)
    attribs = torch.from_numpy(np.ascontiguousarray(att).view(np.uint8).copy()).to("cuda")
    nbytes = abi.accel_cutout_scratch_bytes(rs.texture_count)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    mask_out = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda", fill=FILL)
    refl_out = ImageBuf(abi.FMT_RGBA8_UNORM, W // 2, H // 2, device="cuda", fill=FILL)
    sp = abi.shadow_rt_params(setup.inv_view, FRAME_LIGHTS, *setup.fazz, normal_offset=OFFSET, tmin=TMIN)
    rp = abi.reflect_rt_params(setup.inv_view, *setup.fazz)
    table = (attribs.data_ptr(), len(att), rs.textures, rs.texture_count)
    if cutout is None:
        abi.shadow_mask_rt(frame.image("depth", 0, 1), frame.image("normal"), accel, sp, mask_out.desc(), _stream())
        abi.reflections_rt(frame.image("depth", 1, 1), frame.image("dn"), None, accel, *table, rp, refl_out.desc(), scratch.data_ptr(), nbytes, _stream())
    else:
        abi.shadow_mask_rt_cutout(frame.image("depth", 0, 1), frame.image("normal"), accel, *table, sp, cutout, mask_out.desc(), scratch.data_ptr(), nbytes,
                                  _stream())
        abi.reflections_rt_cutout(frame.image("depth", 1, 1), frame.image("dn"), None, accel, *table, rp, cutout, refl_out.desc(), scratch.data_ptr(), nbytes,
                                  _stream())
    _sync()
    return mask_out.raw(0), refl_out.raw(0)


def _stages(frame):
    frame.run(host.STAGE_SHADOW_MASK_RT)
    _sync()
    assert frame.last_tasks() == ["ShadowMaskRT"], frame.last_tasks()
    mask = frame.download("shadow_mask").raw(0)
    frame.run(host.STAGE_REFLECTIONS_RT)
    _sync()
    assert frame.last_tasks() == ["ReflectionsRT", "SSSR_blur"], frame.last_tasks()
    return mask, frame.download("reflections").raw(0)


def test_frame_stages():
    sc = scn.procedural_scene(detail=8, cutout=True)
    setup = FrameSetup(W, H)
    frame = host.HostFrame(setup, device="cuda")
    accel = abi.Accel.from_scene(sc)
    try:
        frame.load_scene(sc)
        frame.run(PRE)
        frame.set_shadow_rays(FRAME_LIGHTS)
        frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE)
        _sync()
        # a frame that never called set_ray_cutouts, and one that called it with enable = 0: today's entries
        opaque_mask, opaque_refl = _frame_by_hand(frame, setup, accel, sc, None)
        for what in ("never set", "enable = 0"):
            if what == "enable = 0":
                frame.set_ray_cutouts(False, alpha_lod=2)
            mask, refl = _stages(frame)
            _differing(f"shadow mask stage, {what}, against vkr_shadow_mask_rt", mask, opaque_mask)
            _differing(f"reflections stage, {what}, against vkr_reflections_rt", refl, opaque_refl)
        # cutouts on: the _cutout entries with the scene's mask of textures without holes, the same task orders
        for lod in (0, 2):
            frame.set_ray_cutouts(True, alpha_lod=lod)
            mask, refl = _stages(frame)
            want_mask, want_refl = _frame_by_hand(frame, setup, accel, sc, abi.ray_cutout(lod, abi.scene_opaque_texture_mask(sc)))
            _differing(f"shadow mask stage, cutouts at level {lod}, against vkr_shadow_mask_rt_cutout", mask, want_mask)
            _differing(f"reflections stage, cutouts at level {lod}, against vkr_reflections_rt_cutout", refl, want_refl)
            if lod == 0:
                lit = (mask == 255) & (opaque_mask == 0)
                print(f"[ray cutout] frame {W}x{H}: pixels in the fence's shadow lit through its holes, per light: {lit.reshape(-1, 4).sum(axis=0).tolist()}; "
                      f"reflection texels that changed: {int((refl != opaque_refl).any(axis=-1).sum())}")
                assert not np.array_equal(mask, opaque_mask) and lit[..., 0].sum() >= 1, "no pixel in the fence's shadow is lit"
                assert (mask >= opaque_mask).all()
                assert not np.array_equal(refl, opaque_refl), "the mirror shows the fence as a solid quad"
        # and the numpy reference of the frame's own G-buffer agrees on where the light comes through
        words = frame.download("depth").raw(0)[..., 0].astype(np.uint32)
        codes = frame.download("normal").raw(0)
        frame.set_ray_cutouts(True, alpha_lod=0)
        mask, _ = _stages(frame)
        want = ref.shadow_mask_rt_cutout(_arith(), words, codes, setup.inv_view, *setup.fazz, FRAME_LIGHTS, OFFSET, TMIN, abi.scene_triangles(sc),
                                         abi.scene_triangle_attributes(sc), sc.textures, 0, 0)
        _differing("shadow mask stage with cutouts against the numpy reference", mask, want)
        frame.set_ray_cutouts(False)
        mask, refl = _stages(frame)
        _differing("shadow mask stage, switched off again", mask, opaque_mask)
        _differing("reflections stage, switched off again", refl, opaque_refl)
    finally:
        accel.close()
        frame.close()
