"""Program shadow_mask and program defered_shading_shadowed on the GPU.

The mask is compared bit for bit with the numpy restatement (tests/shadow_mask_reference.py): on synthetic inputs in which every
class of the rule occurs (tests/test_shadow_mask.py builds them and checks that on the CPU), on rasterised content (maps from
vkr_default_shadow, depth from vkr_raster_gbuffer, the restatement fed the same device bytes) and on the analytic occluder
scene of the CPU test; the frame stage is compared with the entries called by hand and its refusals are checked.  The shadowed
shading: a mask of 255 gives the bytes of vkr_defered_shading, show_ao ignores the mask, the stored colour is affine in the
mask value within what the sRGB8 encode can tell, and vkrh_set_shadow_mask(apply) switches the frame to it.

Measured on an MI355X: 0 differing texels in all 27 synthetic cases (each 16 launches, twice: the second with the maps' top
bytes inverted), in the 6 rasterised cases (light A: 1428 / 939 / 672 texels of 0 and 35436 / 34571 / 33499 of 255 at 256 x 144 for
radius 0 / 1 / 2) and on the occluder scene; shading: 15223 of 36864 pixels change between mask 0 and 255 at 256 x 144 and 1038 of
2590 at 70 x 37, 0 samples off the affine combination; the frame with the mask applied: 775 texels of color_out darker."""
import ctypes as C

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PostFxChain
from vk_renderer_amd.images import ArrayImageBuf, ImageBuf

import shadow_light as sl
import shadow_mask_reference as ref
from test_shadow_mask import (BIASES, MAP_SIZES, RADII, check_occluder_mask, check_synthetic_classes, occluder_bias, occluder_case,
                              synthetic_launches)

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0xA5
D24 = abi.FMT_D24_UNORM_S8


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch

    torch.cuda.synchronize()


def _arith():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


def _upload_words(words):
    """uint32 [h, w] -> a D24_UNORM_S8 image on the device holding exactly those words"""
    h, w = words.shape
    staged = ImageBuf(D24, w, h)
    staged.set_raw(np.ascontiguousarray(words, dtype=np.uint32).reshape(h, w, 1), 0)
    dev = ImageBuf(D24, w, h, device="cuda")
    dev.upload(staged.to_host())
    return dev


def _upload_layers(maps):
    """uint32 [layers, n, n] -> a D24_UNORM_S8 array image on the device holding exactly those words"""
    import torch

    layers, n, _ = maps.shape
    staged = ArrayImageBuf(D24, n, n, layers)
    for l in range(layers):
        o = staged.layer_offset(l, 0)
        rows = staged.host[o: o + staged.pitch[0] * n].reshape(n, staged.pitch[0])
        rows[:, : 4 * n] = np.ascontiguousarray(maps[l], dtype=np.uint32).view(np.uint8).reshape(n, 4 * n)
    dev = ArrayImageBuf(D24, n, n, layers, device="cuda")
    dev.tensor.copy_(torch.from_numpy(staged.host))
    return dev


def _launch(depth_desc, layer_descs, params, w, h):
    """-> the RGBA8 codes [h, w, 4]; checks that nothing outside the rows was written"""
    out = ImageBuf(abi.FMT_RGBA8_UNORM, w, h, device="cuda", fill=FILL)
    abi.shadow_mask(depth_desc, layer_descs, params, out.desc(), _stream())
    _sync()
    host_bytes = out.to_host()
    rows = host_bytes[: out.pitch[0] * h].reshape(h, out.pitch[0])
    assert (rows[:, 4 * w:] == FILL).all() and (host_bytes[out.pitch[0] * h:] == FILL).all(), "bytes outside the image were written"
    return out.raw(0, host_bytes)


def _differing(name, got, want):
    bad = (got != want).any(axis=-1)
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} texels differ, first at {tuple(np.argwhere(bad)[0])}: "
                           f"{got[bad][:4].tolist()} != {want[bad][:4].tolist()}")


# ---- bit for bit on synthetic inputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", BIASES)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("map_n", MAP_SIZES)
def test_synthetic_parity(map_n, radius, bias):
    """every output size x layer_count 1..4 of the case: 0 differing texels, 255 in the unused channels, the row padding
    untouched, and the same bytes from maps whose top bytes are inverted"""
    total = check_synthetic_classes(map_n, radius, bias)
    differing = 0
    for launch in synthetic_launches(map_n, radius, bias):
        w, h = launch["size"]
        k = len(launch["mvps"])
        depth = _upload_words(launch["depth"])
        layers = _upload_layers(launch["maps"])
        params = abi.shadow_mask_params(launch["inverse_camera"], launch["mvps"], *launch["fazz"], radius=radius, bias=bias)
        got = _launch(depth.desc(), layers.descs(), params, w, h)
        differing += int((got != launch["expect"]).any(axis=-1).sum())
        _differing(f"{w}x{h} map {map_n} radius {radius} bias {bias} lights {launch['kinds']}", got, launch["expect"])
        assert (got[..., k:] == 255).all(), "a channel at or beyond layer_count is not 255"
        flipped = _upload_layers(launch["maps"] ^ np.uint32(0xFF000000))
        again = _launch(depth.desc(), flipped.descs(), params, w, h)
        assert np.array_equal(again, got), "the top byte of a map word is not ignored"
    print(f"[shadow mask] map {map_n} radius {radius} bias {bias}: differing texels {differing}; classes {total}")


# ---- rasterised content -------------------------------------------------------------------------------------------------------------
def _render_maps(sc, mvps, n):
    """vkr_default_shadow -> the array image on the device"""
    import torch

    s, keep = sc.upload("cuda")
    array = ArrayImageBuf(D24, n, n, len(mvps), device="cuda", fill=0x5A)
    tris = sum(d["index_count"] // 3 for d in sc.draws)
    nbytes = abi.default_shadow_scratch_bytes(n, len(mvps), tris)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    abi.default_shadow(s, mvps, [array.desc(l) for l in range(len(mvps))], scratch.data_ptr(), nbytes, _stream())
    _sync()
    return array


RASTER_BIAS = 4096  # 2.4e-4 of the depth range: small against every occluder distance of the scene, large against its slopes per texel


@pytest.mark.parametrize("size", [(256, 144), (252, 142)])
def test_rasterised_content(size):
    """procedural_scene(cutout=True): lights A, B, C in one call, 360^2 maps by vkr_default_shadow, depth by vkr_raster_gbuffer;
    the mask equals the restatement fed the same device bytes, and light A's channel holds both 0 and 255"""
    rasterised_content(FrameSetup(*size))


def rasterised_content(setup, both_in_light_a=True):
    """the body of test_rasterised_content seen through `setup` (tests/test_camera_cases_gpu.py runs it under other cameras, which
    need not see a shadow of light A)"""
    W, H = setup.width, setup.height
    sc = scn.procedural_scene(cutout=True)
    mvps = [sl.mvp(k) for k in "ABC"]
    array = _render_maps(sc, mvps, 360)
    chain = PostFxChain(W, H, backend="product", setup=setup)
    chain.raster(sc)
    chain.sync()
    depth_words = chain.depth.raw(0)[..., 0]
    map_words = array.raw()[..., 0]
    s = chain.setup
    for radius in RADII:
        chain.shadow_mask([array.desc(l) for l in range(3)], mvps, radius=radius, bias=RASTER_BIAS)
        chain.sync()
        got = chain.shadow_mask_out.raw(0)
        want = ref.shadow_mask(_arith(), depth_words, map_words, s.inv_view, mvps, *s.fazz, radius, RASTER_BIAS)
        a = got[..., 0]
        print(f"[shadow mask] raster {W}x{H} radius {radius}: differing texels {int((got != want).any(axis=-1).sum())}, light A: "
              f"{int((a == 0).sum())} texels 0, {int((a == 255).sum())} texels 255, sky {int(((depth_words & sl.D24_MAX) == sl.D24_MAX).sum())}")
        _differing(f"raster {W}x{H} radius {radius}", got, want)
        assert (got[..., 3] == 255).all()
        if both_in_light_a:
            assert (a == 0).any() and (a == 255).any(), "light A's channel does not hold both a shadowed and a lit texel"
        else:  # whatever the camera sees: geometry, and a mask that is not one value over it
            geometry = (depth_words & sl.D24_MAX) != sl.D24_MAX
            assert geometry.any() and len(np.unique(got[geometry][:, :3])) > 1, "the mask holds one value wherever there is geometry"


# ---- the analytic occluder scene ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
def test_known_answer_occluder(radius):
    case = occluder_case()
    s = case["setup"]
    h, w = case["depth"].shape
    bias = occluder_bias(case["words"], radius)
    depth = _upload_words(case["depth"])
    layers = _upload_layers(case["words"][None])
    params = abi.shadow_mask_params(s.inv_view, [case["mvp"]], *s.fazz, radius=radius, bias=bias)
    got = _launch(depth.desc(), layers.descs(), params, w, h)
    check_occluder_mask(case, radius, got[..., 0])
    _differing(f"occluder radius {radius}", got, ref.shadow_mask(_arith(), case["depth"], case["words"][None], s.inv_view, [case["mvp"]], *s.fazz, radius, bias))


# ---- the frame stage ----------------------------------------------------------------------------------------------------------------
W, H = 256, 144


def _frame_layers(frame, count):
    out = []
    for l in range(count):
        d = abi.VkrImg()
        frame._check(host.lib().vkrh_image_layer(frame.h, b"shadows", l, C.byref(d)))
        out.append(d)
    return out


def test_frame_stage():
    sc = scn.procedural_scene(detail=12, cutout=True)
    setup = FrameSetup(W, H)
    lights = [sl.mvp("A"), sl.mvp("B")]
    frame = host.HostFrame(setup, device="cuda")
    try:
        frame.load_scene(sc)
        with pytest.raises(RuntimeError, match="VKRH_STAGE_SHADOW_MASK without rendered shadow maps"):
            frame.run(host.STAGE_RASTER | host.STAGE_SHADOW_MASK)
        assert "ShadowMask" not in frame.last_tasks()
        with pytest.raises(RuntimeError, match="'shadow_mask' only exists after"):
            frame.image("shadow_mask")
        frame.set_shadow_lights(lights, 360)
        frame.set_shadow_mask(bias=RASTER_BIAS, radius=2)
        frame.run(host.STAGE_RASTER | host.STAGE_SHADOW | host.STAGE_SHADOW_MASK)
        _sync()
        tasks = frame.last_tasks()
        assert tasks == ["GbufferPass", "ShadowPass", "ShadowPass", "ShadowMask"], tasks
        d = frame.image("shadow_mask")
        assert (d.format, d.width, d.height) == (abi.FMT_RGBA8_UNORM, W, H)
        staged = frame.download("shadow_mask").raw(0)
        # by hand: the maps from vkr_default_shadow, the mask from vkr_shadow_mask on the frame's depth
        array = _render_maps(sc, lights, 360)
        params = abi.shadow_mask_params(setup.inv_view, lights, *setup.fazz, radius=2, bias=RASTER_BIAS)
        direct = _launch(frame.image("depth", 0, 1), [array.desc(0), array.desc(1)], params, W, H)
        _differing("frame stage against the entries called by hand", staged, direct)
        assert (staged[..., 2:] == 255).all() and (staged[..., 0] == 0).any() and (staged[..., 0] == 255).any()
        # the stage alone, on the maps of the earlier run; other settings give another mask
        frame.set_shadow_mask(bias=0, radius=0)
        frame.run(host.STAGE_SHADOW_MASK)
        _sync()
        assert frame.last_tasks() == ["ShadowMask"]
        params = abi.shadow_mask_params(setup.inv_view, lights, *setup.fazz, radius=0, bias=0)
        direct0 = _launch(frame.image("depth", 0, 1), _frame_layers(frame, 2), params, W, H)
        _differing("frame stage, radius 0", frame.download("shadow_mask").raw(0), direct0)
        assert not np.array_equal(direct0, direct)
        # new lights: the maps are stale until VKRH_STAGE_SHADOW runs again
        frame.set_shadow_lights([sl.mvp("C")], 360)
        with pytest.raises(RuntimeError, match="VKRH_STAGE_SHADOW_MASK without rendered shadow maps"):
            frame.run(host.STAGE_SHADOW_MASK)
        with pytest.raises(RuntimeError, match="vkrh_set_shadow_mask: radius 3"):
            frame.set_shadow_mask(radius=3)
    finally:
        frame.close()


def test_frame_stage_is_refused_on_a_tiled_frame():
    tiled = host.HostFrame(FrameSetup(W, H), device="cuda", tiled=True)
    try:
        with pytest.raises(RuntimeError, match="VKRH_STAGE_SHADOW_MASK on a tiled frame"):
            tiled.run(host.STAGE_SHADOW_MASK)
        with pytest.raises(RuntimeError, match="VKRH_STAGE_SHADOW_MASK on a tiled frame"):
            tiled.run(host.STAGE_SHADOW | host.STAGE_SHADOW_MASK)
        assert "ShadowMask" not in tiled.last_tasks()
        with pytest.raises(RuntimeError, match="vkrh_set_shadow_mask: on a tiled frame"):
            tiled.set_shadow_mask(apply=1)
    finally:
        tiled.close()


# ---- the shadowed shading -----------------------------------------------------------------------------------------------------------
class ShadingInputs:
    """random but tame G-buffer content at any extent (the flat chain driver only takes even extents): random albedo, material,
    normals, reflections and depth words (both mips), occlusion in [0.25, 1], a BRDF LUT in [0, 1]"""

    def __init__(self, w, h, seed):
        rng = np.random.default_rng(seed)
        w2, h2 = max(1, w // 2), max(1, h // 2)

        def filled(fmt, ww, hh, mips=1, arrays=None):
            staged = ImageBuf(fmt, ww, hh, mips)
            for m, a in enumerate(arrays):
                staged.set_raw(a, m)
            dev = ImageBuf(fmt, ww, hh, mips, device="cuda")
            dev.upload(staged.to_host())
            return dev

        u8 = lambda hh, ww: rng.integers(0, 256, size=(hh, ww, 4), dtype=np.uint8)  # noqa: E731
        self.w, self.h = w, h
        self.albedo = filled(abi.FMT_RGBA8_SRGB, w, h, arrays=[u8(h, w)])
        self.material = filled(abi.FMT_RGBA8_SRGB, w, h, arrays=[u8(h, w)])
        self.normal = filled(abi.FMT_RG16_UNORM, w, h, arrays=[rng.integers(0, 65536, size=(h, w, 2), dtype=np.uint16)])
        d0 = rng.integers(1 << 23, 1 << 24, size=(h, w, 1), dtype=np.uint32)
        d1 = rng.integers(1 << 23, 1 << 24, size=(h2, w2, 1), dtype=np.uint32)
        self.depth = filled(D24, w, h, 2, arrays=[d0, d1])
        self.occlusion = filled(abi.FMT_RG16_SFLOAT, w2, h2, arrays=[rng.uniform(0.25, 1.0, size=(h2, w2, 2)).astype(np.float16)])
        self.brdf = filled(abi.FMT_RG16_SFLOAT, 32, 32, arrays=[rng.uniform(0.0, 1.0, size=(32, 32, 2)).astype(np.float16)])
        self.reflections = filled(abi.FMT_RGBA8_UNORM, w2, h2, arrays=[u8(h2, w2)])
        setup = FrameSetup(w, h)
        self.consts = abi.ShadingParams()
        self.consts.inverse_camera = abi.Mat4.from_np(setup.inv_view)
        self.consts.camera = abi.Mat4.from_np(setup.view)
        self.consts.shadow_mvp = abi.Mat4.from_np(sl.mvp("A"))
        self.consts.fovy, self.consts.aspect, self.consts.znear, self.consts.zfar = [float(v) for v in setup.fazz]

    def mask(self, rgba):
        """an RGBA8_UNORM mask on the device: one value everywhere (4 codes) or an array [h, w, 4]"""
        a = np.broadcast_to(np.asarray(rgba, dtype=np.uint8), (self.h, self.w, 4))
        staged = ImageBuf(abi.FMT_RGBA8_UNORM, self.w, self.h)
        staged.set_raw(np.ascontiguousarray(a), 0)
        dev = ImageBuf(abi.FMT_RGBA8_UNORM, self.w, self.h, device="cuda")
        dev.upload(staged.to_host())
        return dev

    def shade(self, mask=None, show_ao=0):
        """-> the RGBA8_SRGB codes [h, w, 4]; mask None: vkr_defered_shading"""
        lib = abi.product()
        out = ImageBuf(abi.FMT_RGBA8_SRGB, self.w, self.h, device="cuda", fill=FILL)
        push = abi.ShadingPush((C.c_float * 2)(0.0, 1.0), show_ao)
        common = [self.albedo.desc(), self.normal.desc(), self.material.desc(), self.depth.desc(), self.consts, self.occlusion.desc(),
                  self.brdf.desc(), self.reflections.desc()]
        if mask is None:
            abi.check(lib.vkr_defered_shading(*[C.byref(v) for v in common], C.byref(out.desc()), C.byref(push), _stream()), lib)
        else:
            abi.defered_shading_shadowed(*common, mask.desc(), out.desc(), push, _stream())
        _sync()
        host_bytes = out.to_host()
        rows = host_bytes[: out.pitch[0] * self.h].reshape(self.h, out.pitch[0])
        assert (rows[:, 4 * self.w:] == FILL).all(), "bytes outside the image were written"
        return out.raw(0, host_bytes)


@pytest.mark.parametrize("size", [(256, 144), (70, 37)])
def test_shading_with_a_white_mask_is_the_plain_shading(size):
    """(a) mask 255 everywhere (in .x; the other channels are not read, whatever they hold): byte for byte vkr_defered_shading;
    (b) with show_ao = 1 no mask changes anything"""
    inputs = ShadingInputs(*size, seed=3)
    plain = inputs.shade()
    assert np.array_equal(inputs.shade(inputs.mask([255, 255, 255, 255])), plain)
    assert np.array_equal(inputs.shade(inputs.mask([255, 0, 77, 3])), plain)
    assert not np.array_equal(inputs.shade(inputs.mask([0, 255, 255, 255])), plain)
    ao = inputs.shade(show_ao=1)
    assert not np.array_equal(ao, plain)
    rng = np.random.default_rng(9)
    noise = inputs.mask(rng.integers(0, 256, size=(size[1], size[0], 4), dtype=np.uint8))
    assert np.array_equal(inputs.shade(noise, show_ao=1), ao)
    assert np.array_equal(inputs.shade(inputs.mask([0, 0, 0, 0]), show_ao=1), ao)


@pytest.mark.parametrize("size", [(256, 144), (70, 37)])
def test_shading_is_affine_in_the_mask(size):
    """(c) the linear colour is affine in the mask value v: with I(c) the set of linear values the encode stores as code c
    (shade_interval), the interval at mask code 128 must meet (1 - 128 / 255) I(code at 0) + (128 / 255) I(code at 255).  The
    combine is two products and a sum: each endpoint is widened by three float32 ulps of the larger endpoint.  The stored code
    does not rise as the mask falls, and some pixel changes between 0 and 255."""
    inputs = ShadingInputs(*size, seed=4)
    c0, c128, c255 = (inputs.shade(inputs.mask([v, 255, 255, 255]))[..., :3].astype(np.int64) for v in (0, 128, 255))
    assert (c0 <= c128).all() and (c128 <= c255).all(), "the stored colour rises as the mask falls"
    changed = int((c0 != c255).any(axis=-1).sum())
    a = 128.0 / 255.0
    (lo0, hi0), (lo128, hi128), (lo255, hi255) = (ref.shade_interval(c) for c in (c0, c128, c255))
    lo, hi = (1.0 - a) * lo0 + a * lo255, (1.0 - a) * hi0 + a * hi255
    finite = lambda v: np.where(np.isfinite(v), np.abs(v), 0.0)  # noqa: E731
    ulp = np.spacing(np.maximum(finite(lo), finite(hi)).astype(F32)).astype(np.float64)
    lo, hi = lo - 3.0 * ulp, hi + 3.0 * ulp
    disjoint = ~(np.maximum(lo, lo128) < np.minimum(hi, hi128))
    print(f"[shadow mask] shading {size}: {changed} pixels change between mask 0 and 255, {int(disjoint.sum())} samples off the affine combination, "
          f"{int((c0 != c128).any(axis=-1).sum())} pixels differ between 0 and 128")
    assert changed >= 1
    assert not disjoint.any(), f"{int(disjoint.sum())} samples: first at {tuple(np.argwhere(disjoint)[0])}"


def test_frame_applies_the_mask_when_asked():
    """(d) vkrh_set_shadow_mask(apply = 1): color_out of the frame equals vkr_defered_shading_shadowed called by hand on the frame's
    images; with the default it equals vkr_defered_shading"""
    sc = scn.procedural_scene(detail=12, cutout=True)
    setup = FrameSetup(W, H)
    frame = host.HostFrame(setup, device="cuda")
    try:
        frame.load_scene(sc)
        frame.run(host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH)
        stages = host.STAGE_RASTER | host.STAGE_SHADOW | host.STAGE_SHADOW_MASK | host.STAGE_CHAIN | host.STAGE_SHADING
        consts = abi.ShadingParams()
        consts.inverse_camera = abi.Mat4.from_np(setup.inv_view)
        consts.camera = abi.Mat4.from_np(setup.view)
        consts.shadow_mvp = abi.Mat4.from_np(frame.shadow_lights()[0])
        consts.fovy, consts.aspect, consts.znear, consts.zfar = [float(v) for v in setup.fazz]
        push = abi.ShadingPush((C.c_float * 2)(0.0, 1.0), 0)
        lib = abi.product()

        def by_hand(shadowed):
            """the entry on the images the frame's last run left behind"""
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
            frame.set_shadow_mask(bias=RASTER_BIAS, radius=1, apply=apply)
            frame.run(stages)
            _sync()
            tasks = frame.last_tasks()
            assert tasks.index("ShadowPass") < tasks.index("ShadowMask") < tasks.index("DeferedShading"), tasks
            got = frame.download("color_out").raw(0)
            plain, shadowed = by_hand(False), by_hand(True)
            want = shadowed if apply else plain
            assert np.array_equal(got, want), f"apply {apply}: {int((got != want).any(axis=-1).sum())} texels differ from the entry called by hand"
            darker = int((shadowed.astype(int) < plain.astype(int)).any(axis=-1).sum())
            print(f"[shadow mask] frame, apply {apply}: {darker} texels of color_out are darker under the mask")
            assert darker >= 1 and (shadowed <= plain).all()
        # the mask of an earlier run is not applied: without VKRH_STAGE_SHADOW_MASK in the run the shading is the plain one
        frame.run(host.STAGE_SHADING)
        _sync()
        assert np.array_equal(frame.download("color_out").raw(0), by_hand(False))
    finally:
        frame.close()
