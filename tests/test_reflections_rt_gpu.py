"""Program reflections_rt on the GPU: the image byte for byte against the numpy restatement (tests/reflections_rt_reference.py) at
8 x 8 (one wave), 17 x 9 (partial tiles on both axes), 64 x 36 and the degenerate 1 x 1, 1 x 9, 9 x 1, on the procedural scene
rasterised by the oracle and on the G-buffer content at which a wave-wide walk goes wrong (nothing live, live and dead lanes
alternating per pixel and per 8 x 8 tile, every normal facing away, noise and pole normals); texture_lod 0 and one beyond the chain,
no textures at all (everything grey), an empty structure (everything 0), and VKR_REFLECT_RT_FILL_MISSES with a `rays` image whose
.w alternates per pixel and per 8 x 8 tile (untouched texels keep the fill byte); the bytes outside the rows; and the frame stage
STAGE_REFLECTIONS_RT in both modes: against the entries called by hand, the task order, its refusals, the kept texels against a
plain trace + filter, and a frame without the stage.

Coverage, asserted on the reference's own output at raster 64 x 36 (measured there: of 2024 geometry pixels 1246 cast a ray, 851 hit and
395 miss; hits on all 5 draws: 165 on the ground, 338 on the wall, 129 / 88 on the textured spheres and 131 grey ones on the
untextured sphere; the level beyond the chain changes all 720 textured hits)."""
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
import reflections_rt_reference as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0xA5
SKY = 0xFFFFFF
SIZES = [(8, 8), (17, 9), (64, 36), (1, 1), (1, 9), (9, 1)]  # a wave is an 8 x 8 tile: the last three are one live lane, one live column, one live row
OFFSET, TMIN = abi.SHADOW_RT_NORMAL_OFFSET, abi.SHADOW_RT_TMIN  # the frame's defaults
GREY = 128  # rint(0.5 * 255), ties to even


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
    """-> (scene, world triangles, attribute records, draw index of every triangle)"""
    sc = scn.procedural_scene(detail=8)
    draw_of = np.concatenate([np.full(d["index_count"] // 3, i) for i, d in enumerate(sc.draws)])
    return sc, abi.scene_triangles(sc), abi.scene_triangle_attributes(sc), draw_of


@functools.lru_cache(maxsize=None)
def _device_scene():
    """the scene's textures and attribute table on the device: -> (RasterScene, attribs tensor, keep-alive)"""
    import torch

    sc, _, att, _ = _scene()
    rs, keep = sc.upload(device="cuda")
    return rs, torch.from_numpy(np.ascontiguousarray(att).view(np.uint8).copy()).to("cuda"), keep


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
    # every normal is the view direction's own: seen from behind, dot(n, dir) <= 0 wherever the camera looks along +z
    codes = np.zeros((c.normal.height, c.normal.width, 2), np.uint16)
    codes[..., 0] = 32768
    codes[..., 1] = 32768  # (0, 0, 1) up to the code's rounding
    c.normal.set_raw(codes)


CLASSES = {"raster": lambda c, rng: None, "sky_all": content.sky_all, "checker_px": content.checker_px, "checker_tile8": _checker_tile8,
           "facing_away": _facing_away, "normal_noise": content.normal_noise, "normal_poles": content.normal_poles}
# variant: (texture_lod, textures bound, empty structure, fill mode: None, "px" or "tile8")
VARIANTS = {"lod0": (0, True, False, None), "lod_beyond": (99, True, False, None), "no_textures": (0, False, False, None),
            "empty": (0, True, True, None), "fill_px": (0, True, False, "px"), "fill_tile8": (3, True, False, "tile8")}


@functools.lru_cache(maxsize=None)
def _inputs(name, size):
    g = _Gbuffer(size)
    CLASSES[name](g, np.random.default_rng([0x5EF1, sorted(CLASSES).index(name), size[0], size[1]]))
    return g.depth.raw(0)[..., 0].copy(), g.normal.raw(0).copy(), g.setup, g.depth.to_host().copy(), g.normal.to_host().copy()


def _rays_w(size, kind):
    """the .w codes of a `rays` image: 65535 (an invalid screen-space ray: traced) alternating with valid codes"""
    w, h = size
    y, x = np.mgrid[0:h, 0:w]
    invalid = ((x + y) & 1) == 0 if kind == "px" else (((x // 8) + (y // 8)) & 1) == 0 if w > 8 or h > 8 else (x & 1) == 0
    valid_codes = ((x * 7 + y * 13) % 65535).astype(np.uint16)  # 0 .. 65534: every one a valid hit
    return np.where(invalid, np.uint16(65535), valid_codes).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def _expected(name, size, variant):
    lod, textured, empty, fill = VARIANTS[variant]
    words, codes, setup, _, _ = _inputs(name, size)
    sc, tris, att, _ = _scene()
    if empty:
        tris, att = np.zeros((0, 3, 3), F32), att[:0]
    before = np.full(words.shape + (4,), FILL, np.uint8)
    return ref.reflections_rt(_arith(), words, codes, _rays_w(size, fill) if fill else None, setup.inv_view, *setup.fazz, OFFSET, TMIN,
                              float(setup.fazz[3]), lod, ref.FILL_MISSES if fill else 0, tris, att, sc.textures if textured else [], before)


@functools.lru_cache(maxsize=None)
def _accel(empty=False):
    return abi.Accel(np.zeros((0, 3, 3), F32) if empty else _scene()[1])


def _launch(name, size, variant):
    """-> the RGBA8 codes [h, w, 4] of vkr_reflections_rt on an image filled with FILL; checks that nothing outside the rows was written"""
    import torch

    lod, textured, empty, fill = VARIANTS[variant]
    w, h = size
    _, _, setup, depth_bytes, normal_bytes = _inputs(name, size)
    depth = ImageBuf(abi.FMT_D24_UNORM_S8, w, h, device="cuda")
    normal = ImageBuf(abi.FMT_RG16_UNORM, w, h, device="cuda")
    depth.upload(depth_bytes)
    normal.upload(normal_bytes)
    rays = None
    if fill:
        host_rays = ImageBuf(abi.FMT_RGBA16_UNORM, w, h)
        codes = np.full((h, w, 4), 0x1234, np.uint16)
        codes[..., 3] = _rays_w(size, fill)
        host_rays.set_raw(codes)
        rays = ImageBuf(abi.FMT_RGBA16_UNORM, w, h, device="cuda")
        rays.upload(host_rays.to_host())
    out = ImageBuf(abi.FMT_RGBA8_UNORM, w, h, device="cuda", fill=FILL)
    rs, attribs, _ = _device_scene()
    count = 0 if not textured else rs.texture_count
    nbytes = abi.reflections_rt_scratch_bytes(count)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    params = abi.reflect_rt_params(setup.inv_view, *setup.fazz, fill_misses=bool(fill), normal_offset=OFFSET, tmin=TMIN, texture_lod=lod)
    abi.reflections_rt(depth.desc(), normal.desc(), rays.desc() if fill else None, _accel(empty), None if empty else attribs.data_ptr(),
                       0 if empty else len(_scene()[2]), rs.textures if textured else None, count, params, out.desc(), scratch.data_ptr(), nbytes,
                       _stream())
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
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", sorted(CLASSES))
def test_parity(name, size, variant):
    lod, textured, empty, fill = VARIANTS[variant]
    want, traced, index = _expected(name, size, variant)
    got = _launch(name, size, variant)
    geometry = (_inputs(name, size)[0] & SKY) != SKY
    hit = index != ref.MISS
    print(f"[reflections rt] {name} {size[0]}x{size[1]} {variant}: {int(geometry.sum())} geometry pixels, {int(traced.sum())} rays, "
          f"{int(hit.sum())} hits, differing texels {int((got != want).any(axis=-1).sum())}")
    _differing(f"{name} {size} {variant}", got, want)
    if fill:
        kept = geometry & (_rays_w(size, fill) != 65535)
        assert (got[kept] == FILL).all(), "a texel with a valid screen-space ray was touched"
        assert (got[~kept][:, 3] == 0).all()
    else:
        assert (got[..., 3] == 0).all(), "alpha is 0"
        assert (got[~geometry] == 0).all() and (got[~hit] == 0).all()
    if empty:
        assert (got[got[..., 3] == 0] == 0).all() and not hit.any()
    if not textured and not fill:
        assert (got[hit][:, :3] == GREY).all(), "without textures every hit is grey"
    if name == "sky_all":
        assert not geometry.any()
    if name == "facing_away":
        assert not traced.any(), "a surface seen from behind casts no ray"


def test_the_reference_covers_what_the_pass_can_do():
    """at raster 64 x 36 the reference alone: hits and misses, hits on at least three draws, grey hits on the untextured sphere and
    coloured ones on textured draws; and the clamped level differs from level 0 (the variant is not vacuous)"""
    sc, _, att, draw_of = _scene()
    want, traced, index = _expected("raster", (64, 36), "lod0")
    hit = index != ref.MISS
    geometry = (_inputs("raster", (64, 36))[0] & SKY) != SKY
    per_draw = np.bincount(draw_of[index[hit]], minlength=len(sc.draws))
    print(f"[reflections rt] raster 64x36: {int(geometry.sum())} geometry pixels, {int(traced.sum())} rays, {int(hit.sum())} hits, "
          f"{int((traced & ~hit).sum())} misses, hits per draw {per_draw.tolist()}")
    assert hit.any() and (traced & ~hit).any(), "some geometry pixels hit and some miss"
    assert int((per_draw > 0).sum()) >= 3, "hits fall on at least three distinct draws"
    untextured = att["albedo_index"][index[hit]] == np.uint32(scn.INVALID)
    assert untextured.any() and (want[hit][untextured][:, :3] == GREY).all(), "a hit on the untextured sphere is grey"
    assert (want[hit][~untextured][:, :3] != GREY).any(axis=1).any(), "a hit on a textured draw is not grey"
    beyond, _, _ = _expected("raster", (64, 36), "lod_beyond")
    assert (beyond != want).any(), "the last level of the chain gives other colours than level 0"


def test_chain_driver_binds_the_half_resolution_set():
    """PostFxChain.reflections_rt: depth mip 1, dn and reflections of a 128 x 72 product chain, against the restatement on the
    chain's own images"""
    import torch

    sc, tris, att, _ = _scene()
    cw, ch = 128, 72
    setup = FrameSetup(cw, ch)
    chain = PostFxChain(cw, ch, backend="product", device="cuda", setup=setup)
    chain.raster(sc)
    chain.downsample()
    rs, attribs, _ = _device_scene()
    chain.reflections_rt(_accel(), attribs, rs, texture_lod=1)
    torch.cuda.synchronize()
    words, codes = chain.depth.raw(1)[..., 0].astype(np.uint32), chain.dn.raw(0)
    want, traced, index = ref.reflections_rt(_arith(), words, codes, None, setup.inv_view, *setup.fazz, OFFSET, TMIN, float(setup.fazz[3]), 1, 0,
                                             tris, att, sc.textures, np.zeros(words.shape + (4,), np.uint8))
    assert (index != ref.MISS).sum() > 100
    _differing("PostFxChain.reflections_rt", chain.reflections.raw(0), want)
    with pytest.raises(RuntimeError, match="only the product backend"):
        PostFxChain(cw, ch, backend="oracle", setup=setup).reflections_rt(_accel(), attribs, rs)


# ---- the frame stage ----------------------------------------------------------------------------------------------------------------
W, H = 256, 144
PRE = host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH


def _by_hand(frame, setup, accel, fill, before=None, **rays):
    """vkr_reflections_rt on the frame's own half-resolution images -> the RGBA8 codes; before: the content the image starts with"""
    import torch

    out = ImageBuf(abi.FMT_RGBA8_UNORM, W // 2, H // 2, device="cuda", fill=FILL)
    if before is not None:
        out.upload(before)
    rs, attribs, _ = _device_scene_of(frame.scene)
    nbytes = abi.reflections_rt_scratch_bytes(rs.texture_count)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    params = abi.reflect_rt_params(setup.inv_view, *setup.fazz, fill_misses=fill, **rays)
    abi.reflections_rt(frame.image("depth", 1, 1), frame.image("dn"), frame.image("rays") if fill else None, accel, attribs.data_ptr(),
                       attribs.numel() // 32, rs.textures, rs.texture_count, params, out.desc(), scratch.data_ptr(), nbytes, _stream())
    _sync()
    return out.raw(0)


_DEVICE_SCENES = {}


def _device_scene_of(sc):
    import torch

    if id(sc) not in _DEVICE_SCENES:
        rs, keep = sc.upload(device="cuda")
        att = abi.scene_triangle_attributes(sc)
        _DEVICE_SCENES[id(sc)] = (rs, torch.from_numpy(np.ascontiguousarray(att).view(np.uint8).copy()).to("cuda"), (keep, sc))
    return _DEVICE_SCENES[id(sc)]


def _frame(sc):
    setup = FrameSetup(W, H)
    frame = host.HostFrame(setup, device="cuda")
    frame.scene = sc
    return frame, setup


def test_frame_stage_all_mode():
    sc = scn.procedural_scene(detail=12, cutout=True)
    frame, setup = _frame(sc)
    accel = abi.Accel.from_scene(sc)
    try:
        with pytest.raises(RuntimeError, match="VKRH_STAGE_REFLECTIONS_RT without a loaded scene"):
            frame.run(host.STAGE_GBUFFER | host.STAGE_DOWNSAMPLE | host.STAGE_REFLECTIONS_RT)
        frame.load_scene(sc)
        for other in (host.STAGE_SSR, host.STAGE_SSR_CLASSIFIED, host.STAGE_SSR_RESOLVE, host.STAGE_SSR_TRACE, 1 << 18, 1 << 19):  # ..., _TRACE_HEAD, _TRACE_RESUME
            with pytest.raises(RuntimeError, match="VKRH_STAGE_REFLECTIONS_RT together with an SSR stage"):
                frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE | other | host.STAGE_REFLECTIONS_RT)
        assert "ReflectionsRT" not in frame.last_tasks()
        frame.run(PRE)
        # the defaults: every pixel traced, the offsets of the shadow rays, max_distance = zfar, level 0
        frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE | host.STAGE_REFLECTIONS_RT)
        _sync()
        tasks = frame.last_tasks()
        assert tasks[-2:] == ["ReflectionsRT", "SSSR_blur"] and "SSSR_trace" not in tasks and "SSSR_filter" not in tasks, tasks
        assert tasks.index("DownsampleGbuffer") < tasks.index("ReflectionsRT")
        d = frame.image("reflections")
        assert (d.format, d.width, d.height) == (abi.FMT_RGBA8_UNORM, W // 2, H // 2)
        staged = frame.download("reflections").raw(0)
        _differing("frame stage, defaults, against the entry called by hand", staged, _by_hand(frame, setup, accel, False))
        assert (staged[..., :3] != 0).any() and (staged[..., 3] == 0).all()
        assert (frame.download("blurred").raw(0) != 0).any(), "the blur ran on the traced image"
        # the rays of vkrh_set_reflection_rays; the stage alone, on the G-buffer of the earlier run
        rays = dict(normal_offset=5e-3, tmin=1e-4, max_distance=6.0, texture_lod=2)
        frame.set_reflection_rays(fill_misses=False, **rays)
        frame.run(host.STAGE_REFLECTIONS_RT)
        _sync()
        assert frame.last_tasks() == ["ReflectionsRT", "SSSR_blur"]
        again = frame.download("reflections").raw(0)
        _differing("frame stage, other rays, against the entry called by hand", again, _by_hand(frame, setup, accel, False, **rays))
        assert not np.array_equal(again, staged)
        with pytest.raises(RuntimeError, match="tmin is NaN"):
            frame.set_reflection_rays(tmin=float("nan"))
        with pytest.raises(RuntimeError, match="max_distance is NaN"):
            frame.set_reflection_rays(max_distance=float("nan"))
    finally:
        accel.close()
        frame.close()


def test_frame_stage_fill_mode():
    """trace -> filter -> ReflectionsRT -> blur: the texels whose screen-space ray is valid are the filter's of a plain
    STAGE_SSR_TRACE + resolve with the same randoms, the whole image is the entry called by hand on the filter's output, and what
    the trace writes for GTAO (rays, raw) is what the plain trace writes"""
    sc = scn.procedural_scene(detail=12, cutout=True)
    frame, setup = _frame(sc)
    accel = abi.Accel.from_scene(sc)
    try:
        frame.load_scene(sc)
        frame.run(PRE)
        frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE)
        frame.pin_randoms(0.25, 3, 5)
        frame.run(host.STAGE_SSR_TRACE | host.STAGE_SSR_RESOLVE)
        _sync()
        assert frame.last_tasks() == ["SSSR_trace", "SSSR_filter", "SSSR_blur"]
        plain = {n: frame.download(n).to_host().copy() for n in ("rays", "reflections", "raw")}
        filtered = frame.download("reflections").raw(0)
        frame.pin_randoms(0.25, 3, 5)
        frame.set_reflection_rays(fill_misses=True)
        frame.run(host.STAGE_REFLECTIONS_RT)
        _sync()
        assert frame.last_tasks() == ["SSSR_trace", "SSSR_filter", "ReflectionsRT", "SSSR_blur"], frame.last_tasks()
        for n in ("rays", "raw"):
            assert np.array_equal(frame.download(n).to_host(), plain[n]), f"{n} differs from the plain trace's"
        filled = frame.download("reflections").raw(0)
        valid = frame.download("rays").raw(0)[..., 3] != 65535
        geometry = (frame.download("depth").raw(1)[..., 0] & SKY) != SKY
        kept = valid & geometry
        share = 1.0 - kept.mean()
        print(f"[reflections rt] frame, fill mode: {int(kept.sum())} of {kept.size} texels keep the filter's value, {share:.3f} of the image is traced or sky")
        assert kept.any() and (~kept & geometry).any()
        assert np.array_equal(filled[kept], filtered[kept]), "a texel with a valid screen-space ray is not the filter's"
        _differing("frame stage, fill mode, against the entry called by hand on the filter's output", filled,
                   _by_hand(frame, setup, accel, True, before=plain["reflections"]))
        assert (filled[~kept] != filtered[~kept]).any(), "no texel was filled"
    finally:
        accel.close()
        frame.close()


def test_a_frame_without_the_stage_is_what_it_was():
    """the stage and its setter leave every other stage alone: a frame that traced reflections first and one that never did produce
    the same bytes from the same stages, and no task of the second run belongs to the stage"""
    sc = scn.procedural_scene(detail=12)
    stages = host.STAGE_RASTER | host.STAGE_CHAIN | host.STAGE_SHADING | host.STAGE_TAA
    outs = []
    for traced in (False, True):
        frame = host.HostFrame(FrameSetup(W, H), device="cuda")
        try:
            frame.load_scene(sc)
            frame.run(PRE)
            if traced:
                frame.set_reflection_rays(fill_misses=True, normal_offset=1e-2, tmin=1e-3, max_distance=5.0, texture_lod=1)
                frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE | host.STAGE_REFLECTIONS_RT)
                frame.set_reflection_rays(fill_misses=False)
                frame.run(host.STAGE_REFLECTIONS_RT)
            else:
                frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE)
            frame.pin_randoms(0.25, 3, 5)  # the fill-mode trace advanced the SSR counter: both frames start the chain from one state
            frame.run(stages)
            _sync()
            assert "ReflectionsRT" not in frame.last_tasks()
            outs.append((frame.last_tasks(), {n: frame.download(n).to_host().copy() for n in ("color_out", "taa_target", "acc_ao", "reflections", "blurred", "rays", "depth")}))
        finally:
            frame.close()
    assert outs[0][0] == outs[1][0]
    for n in outs[0][1]:
        assert np.array_equal(outs[0][1][n], outs[1][1][n]), f"{n} differs after a run of STAGE_REFLECTIONS_RT"
