"""Programs shadow_mask_rt_soft and shadow_mask_rt_soft_cutout on the GPU: the mask byte for byte against the numpy restatement
(tests/shadow_mask_rt_soft_reference.py) at 8 x 8 (one wave), 17 x 9 (partial tiles on both axes), 1 x 1, 1 x 9, 9 x 1 and 64 x 36, on
the procedural scene and on the G-buffer content at which a wave-wide walk goes wrong, for (S, P) = (1, 1), (3, 2), (16, 4) everywhere,
(64, 4) at the two small extents and (4, 2) at 64 x 36, with 1 to 4 lights, point and directional mixed, and one set of mixed radii;
against the shipped hard entry where the rule says they agree (every radius 0, an all-zero table) and against itself under a
permuted table; a NaN light, a light at a pixel's origin, a light inside the sphere; an empty structure; the cutout entry on the
scene with the fence (the scene, lights and settings of tests/test_ray_cutout_passes_gpu.py at its smallest extent, and once at
64 x 36 where light provably comes through); the build with the light-volume cull (the library ships without it), byte for byte;
and the frame: vkrh_set_shadow_area_lights against the entry called by hand, with cutouts, applied by the shading, switched off
again, and never called."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import LIGHT_POS, FrameSetup
from vk_renderer_amd.chain import PostFxChain
from vk_renderer_amd.images import ImageBuf

import camera_cases as cc
import gbuffer_content as content
import shadow_mask_rt_reference as hard_ref
import shadow_mask_rt_soft_reference as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0xA5
SKY = 0xFFFFFF
SMALL = [(8, 8), (17, 9)]
SIZES = SMALL + [(1, 1), (1, 9), (9, 1), (64, 36)]
POINT_A = tuple(LIGHT_POS) + (1.0,)
POINT_B = (3.0, 4.0, 2.0, 1.0)
SUN_A = (1.5, 4.5, -1.5, 0.0)
SUN_B = (-6.0, 9.0, 3.0, 0.0)
LIGHT_SETS = {1: [POINT_A], 2: [SUN_A, POINT_B], 3: [POINT_B, SUN_B, POINT_A], 4: [POINT_A, SUN_A, POINT_B, SUN_B]}
# name: (lights, radii)
SETS = {"1": (LIGHT_SETS[1], (0.5,)), "2": (LIGHT_SETS[2], (0.5, 0.5)), "3": (LIGHT_SETS[3], (0.5, 0.5, 0.5)), "4": (LIGHT_SETS[4], (0.5, 0.5, 0.5, 0.5)),
        "mixed": (LIGHT_SETS[4], (0.5, 0.0, 1.0, 0.0))}
IN_SPHERE = (0.3, 1.4, 6.0, 1.0)  # the centre of the large sphere of scene.procedural_scene
OFFSET, TMIN = abi.SHADOW_RT_NORMAL_OFFSET, abi.SHADOW_RT_TMIN


def sample_configs(size):
    """(S, P) per extent: the brute force stays near a second per case"""
    return [(1, 1), (3, 2), (16, 4)] + ([(64, 4)] if size in SMALL else []) + ([(4, 2)] if size == (64, 36) else [])


def main_config(size):
    return (4, 2) if size == (64, 36) else (16, 4)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch

    torch.cuda.synchronize()


def _arith():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


@functools.lru_cache(maxsize=None)
def _scene(cutout=False):
    sc = scn.procedural_scene(detail=8, cutout=cutout)
    return sc, abi.scene_triangles(sc)


@functools.lru_cache(maxsize=None)
def _raster(size, cutout=False):
    """the procedural scene through the oracle's rasteriser at the next even extent, cut to size"""
    w, h = size
    ew, eh = w + (w & 1), h + (h & 1)
    setup = cc.frame_setup(size, ew, eh)  # the frozen camera, or the case an Extent names
    chain = PostFxChain(ew, eh, backend="oracle", setup=setup)
    chain.raster(_scene(cutout)[0])
    return chain.depth.raw(0)[:h, :w, 0].astype(np.uint32), chain.normal.raw(0)[:h, :w].copy(), setup


class _Gbuffer:
    """what a content class of tests/gbuffer_content.py touches of a chain: host images of the two inputs of the pass"""

    def __init__(self, size, cutout=False):
        w, h = size
        words, codes, self.setup = _raster(size, cutout)
        self.depth = self.prev_depth = ImageBuf(abi.FMT_D24_UNORM_S8, w, h)
        self.normal = ImageBuf(abi.FMT_RG16_UNORM, w, h)
        self.depth.set_raw(words.reshape(h, w, 1))
        self.normal.set_raw(codes)


# the two local helpers of tests/test_shadow_mask_rt_gpu.py, restated
def _checker_tile8(c, rng):
    x, y = content._grid(c.depth)
    content._set_depth(c.depth, SKY, (((x // 8) + (y // 8)) & 1) == 1)


def _facing_away(c, rng):
    codes = np.zeros((c.normal.height, c.normal.width, 2), np.uint16)
    codes[..., 0] = 32768
    c.normal.set_raw(codes)


CLASSES = {"raster": lambda c, rng: None, "sky_all": content.sky_all, "checker_px": content.checker_px, "checker_tile8": _checker_tile8,
           "facing_away": _facing_away, "normal_noise": content.normal_noise}


@functools.lru_cache(maxsize=None)
def _inputs(name, size, cutout=False):
    g = _Gbuffer(size, cutout)
    CLASSES[name](g, np.random.default_rng([0x50F7, sorted(CLASSES).index(name), size[0], size[1]]))
    return g.depth.raw(0)[..., 0].copy(), g.normal.raw(0).copy(), g.setup, g.depth.to_host().copy(), g.normal.to_host().copy()


@functools.lru_cache(maxsize=None)
def _table(S, P, kind="disk"):
    t = ref.disk_samples(S, P)
    if kind == "zero":
        return np.zeros_like(t)
    if kind == "permuted":
        rng = np.random.default_rng([0x7AB, S, P])
        return np.stack([t[p][rng.permutation(S)] for p in range(P * P)])
    return t


@functools.lru_cache(maxsize=None)
def _expected(name, size, lights, radii, S, P, empty=False):
    words, codes, setup, _, _ = _inputs(name, size)
    tris = np.zeros((0, 3, 3), F32) if empty else _scene()[1]
    return ref.shadow_mask_rt_soft(_arith(), words, codes, setup.inv_view, *setup.fazz, list(lights), OFFSET, TMIN, tris, radii, _table(S, P))


@functools.lru_cache(maxsize=None)
def _accel(empty=False, cutout=False):
    return abi.Accel(np.zeros((0, 3, 3), F32) if empty else _scene(cutout)[1])


def _rows_only(out, w, h):
    host_bytes = out.to_host()
    rows = host_bytes[: out.pitch[0] * h].reshape(h, out.pitch[0])
    assert (rows[:, 4 * w:] == FILL).all() and (host_bytes[out.pitch[0] * h:] == FILL).all(), "bytes outside the image were written"
    return out.raw(0, host_bytes)


def _launch(name, size, lights, radii, S, P, kind="disk", empty=False, entry=None, cutout=None):
    """-> the RGBA8 codes [h, w, 4]; radii None: vkr_shadow_mask_rt; entry: a ctypes function in place of the library's soft entry
    (the build with the cull); cutout: (abi.RayCutout,) for the cutout entries on the scene with the fence.  Checks that nothing
    outside the rows was written."""
    w, h = size
    _, _, setup, depth_bytes, normal_bytes = _inputs(name, size, cutout is not None)
    depth = ImageBuf(abi.FMT_D24_UNORM_S8, w, h, device="cuda")
    normal = ImageBuf(abi.FMT_RG16_UNORM, w, h, device="cuda")
    depth.upload(depth_bytes)
    normal.upload(normal_bytes)
    out = ImageBuf(abi.FMT_RGBA8_UNORM, w, h, device="cuda", fill=FILL)
    params = abi.shadow_rt_params(setup.inv_view, list(lights), *setup.fazz, normal_offset=OFFSET, tmin=TMIN)
    accel = _accel(empty, cutout is not None)
    lib = abi.product()
    if radii is None:
        abi.shadow_mask_rt(depth.desc(), normal.desc(), accel, params, out.desc(), _stream())
    else:
        soft = abi.shadow_rt_soft(radii, S, P, device="cuda", table=_table(S, P, kind))
        if cutout is None:
            if entry is None:
                abi.shadow_mask_rt_soft(depth.desc(), normal.desc(), accel, params, soft, out.desc(), _stream())
            else:
                abi.check(entry(C.byref(depth.desc()), C.byref(normal.desc()), accel.handle, C.byref(params), C.byref(soft), C.byref(out.desc()), _stream()), lib)
        else:
            rs, attribs, count, nbytes, scratch = _device_scene()
            args = (depth.desc(), normal.desc(), accel, attribs.data_ptr(), count, rs.textures, rs.texture_count, params, cutout[0], soft, out.desc(),
                    scratch.data_ptr(), nbytes, _stream())
            if entry is None:
                abi.shadow_mask_rt_soft_cutout(*args)
            else:
                byref = [C.byref(a) if isinstance(a, C.Structure) else a for a in args]
                byref[2] = accel.handle
                abi.check(entry(*byref), lib)
    _sync()
    return _rows_only(out, w, h)


def _differing(name, got, want):
    bad = (got != want).any(axis=-1)
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} texels differ, first at {tuple(np.argwhere(bad)[0])}: "
                           f"{got[bad][:4].tolist()} != {want[bad][:4].tolist()}")


def _check_mask(name, size, lights, radii, S, got):
    geometry = (_inputs(name, size)[0] & SKY) != SKY
    assert (got[..., len(lights):] == 255).all(), "a channel at or beyond light_count is not 255"
    assert (got[~geometry] == 255).all(), "a sky texel is not 0xFFFFFFFF"
    for l, r in enumerate(radii):
        codes = set(np.unique(got[..., l][geometry]).tolist())
        assert codes <= (ref.code_set(S) if r > 0 else {0, 255}), (l, sorted(codes))
    return geometry


# ---- byte for byte against the restatement ------------------------------------------------------------------------------------------
CASES = [(name, size, sp) for name in sorted(CLASSES) for size in SIZES for sp in sample_configs(size)]


@pytest.mark.parametrize("name,size,sp", CASES, ids=[f"{n}-{s[0]}x{s[1]}-S{sp[0]}P{sp[1]}" for n, s, sp in CASES])
def test_parity(name, size, sp):
    lights, radii = SETS["4"]
    S, P = sp
    want = _expected(name, size, tuple(lights), radii, S, P)
    got = _launch(name, size, lights, radii, S, P)
    geometry = _check_mask(name, size, lights, radii, S, got)
    between = [int(((want[..., l] > 0) & (want[..., l] < 255) & geometry).sum()) for l in range(4)]
    print(f"[shadow mask rt soft] {name} {size[0]}x{size[1]} S {S} P {P}: {int(geometry.sum())} geometry pixels, strictly between per channel {between}, "
          f"differing texels {int((got != want).any(axis=-1).sum())}")
    _differing(f"{name} {size} S {S} P {P}", got, want)
    if name == "sky_all":
        assert not geometry.any()
    if name == "raster" and size == (64, 36) and S >= 4:  # not vacuous: a penumbra under every light
        assert all(b >= 1 for b in between), between
    if name == "raster" and size == (8, 8) and S == 16:
        assert all(b >= 1 for b in between), between


LIGHT_CASES = [(name, size, key) for name in ("raster", "normal_noise") for size in SIZES for key in ("1", "2", "3", "mixed")]


@pytest.mark.parametrize("name,size,key", LIGHT_CASES, ids=[f"{n}-{s[0]}x{s[1]}-{k}" for n, s, k in LIGHT_CASES])
def test_parity_light_sets(name, size, key):
    lights, radii = SETS[key]
    S, P = main_config(size)
    want = _expected(name, size, tuple(lights), radii, S, P)
    got = _launch(name, size, lights, radii, S, P)
    _check_mask(name, size, lights, radii, S, got)
    _differing(f"{name} {size} lights {key}", got, want)
    if key == "mixed":  # the lights with radius 0 read what the hard entry writes for them
        hard = _launch(name, size, lights, None, S, P)
        assert np.array_equal(got[..., 1], hard[..., 1]) and np.array_equal(got[..., 3], hard[..., 3])


# ---- metamorphic, against the shipped hard entry on the GPU -----------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["raster", "checker_px", "normal_noise"])
def test_against_the_hard_entry(name, size):
    lights = LIGHT_SETS[4]
    hard = _launch(name, size, lights, None, 0, 0)
    for S, P in sample_configs(size):
        _differing(f"every radius 0, {name} {size} S {S} P {P}", _launch(name, size, lights, (0.0, 0.0, 0.0, 0.0), S, P), hard)
        _differing(f"an all-zero table, {name} {size} S {S} P {P}", _launch(name, size, lights, (0.5, 0.5, 1.0, 0.5), S, P, kind="zero"), hard)


@pytest.mark.parametrize("size", SIZES)
def test_a_permuted_table_changes_no_byte(size):
    lights, radii = SETS["mixed"]
    for S, P in ((3, 2), (16, 4)) + (((64, 4),) if size in SMALL else ()):
        assert not np.array_equal(_table(S, P), _table(S, P, "permuted"))
        a = _launch("raster", size, lights, radii, S, P)
        _differing(f"permuted table {size} S {S} P {P}", _launch("raster", size, lights, radii, S, P, kind="permuted"), a)


@pytest.mark.parametrize("size", SIZES)
def test_nan_light_light_at_an_origin_light_inside_the_sphere(size):
    words, codes, setup, _, _ = _inputs("raster", size)
    _, origin, _ = hard_ref.pixel_origins(_arith(), words, codes, setup.inv_view, *setup.fazz, OFFSET)
    y, x = np.argwhere((words & SKY) != SKY)[len(words) // 2]
    at = tuple(float(v) for v in origin[y, x]) + (1.0,)
    lights = (IN_SPHERE, (float("nan"), 4.0, 2.0, 1.0), at, (0.0, float("nan"), 1.0, 0.0))
    radii = (0.25, 0.5, 0.5, 0.5)  # 0.25: the disk stays inside the sphere
    S, P = main_config(size)
    want = _expected("raster", size, lights, radii, S, P)
    got = _launch("raster", size, lights, radii, S, P)
    _differing(f"special lights {size}", got, want)
    geometry = (words & SKY) != SKY
    assert geometry.any() and (got[geometry][:, 0] == 0).all(), "a light inside the closed sphere reaches something"
    assert (got[geometry][:, 1] == 0).all() and (got[geometry][:, 3] == 0).all(), "a NaN light lights something"
    assert got[y, x, 2] == 0, "dvec = 0: the frame is NaN, no sample casts, the channel is 0"


@pytest.mark.parametrize("size", SIZES)
def test_empty_structure(size):
    """node_count == 0 is legal: V = the number of cast samples"""
    lights, radii = SETS["mixed"]
    S, P = main_config(size)
    for name in ("raster", "normal_noise"):
        want = _expected(name, size, tuple(lights), radii, S, P, empty=True)
        got = _launch(name, size, lights, radii, S, P, empty=True)
        _differing(f"empty structure {name} {size}", got, want)
        words, codes, setup, _, _ = _inputs(name, size)
        h, w = words.shape
        _, origin, normal = hard_ref.pixel_origins(_arith(), words, codes, setup.inv_view, *setup.fazz, OFFSET)
        o, n = origin.reshape(-1, 3), normal.reshape(-1, 3)
        geometry = ((words & SKY) != SKY).reshape(-1)
        slot = ref.pattern_slots(h, w, P)
        for l in (0, 2):
            casts = sum(ref.sample_rays(_arith(), o, n, lights[l], radii[l], _table(S, P)[slot, k])[1].astype(np.int64) for k in range(S))
            assert np.array_equal(got[..., l].reshape(-1)[geometry], ref.quantise(casts, S)[geometry])


# ---- cutouts ----------------------------------------------------------------------------------------------------------------------------
# behind the fence as the camera sees it, the shading pass's light, a directional light through the fence, one from the side
# (the lights of tests/test_ray_cutout_passes_gpu.py)
FENCE_LIGHTS = ((0.5, 2.5, 8.0, 1.0), (-1.85867, 5.81832, -0.247114, 1.0), (0.2, 1.5, 4.0, 0.0), (-6.0, 2.0, 0.5, 0.0))
FENCE_RADII = (0.5, 0.5, 0.25, 0.0)


@functools.lru_cache(maxsize=None)
def _device_scene():
    import torch

    sc = _scene(True)[0]
    att = abi.scene_triangle_attributes(sc)
    rs, keep = sc.upload(device="cuda")
    nbytes = abi.accel_cutout_scratch_bytes(rs.texture_count)
    _device_scene.keep = keep
    return rs, torch.from_numpy(np.ascontiguousarray(att).view(np.uint8).copy()).to("cuda"), len(att), nbytes, torch.empty(nbytes, dtype=torch.uint8, device="cuda")


CUTOUT_CASES = [(name, (8, 8), setting) for name in ("raster", "checker_px", "normal_noise") for setting in ("lod0", "lod0_masked", "lod3_masked")] + \
    [("raster", (64, 36), "lod0")]


@pytest.mark.parametrize("name,size,setting", CUTOUT_CASES, ids=[f"{n}-{s[0]}x{s[1]}-{k}" for n, s, k in CUTOUT_CASES])
def test_cutout_parity(name, size, setting):
    sc, tris = _scene(True)
    lod, masked = {"lod0": (0, False), "lod0_masked": (0, True), "lod3_masked": (3, True)}[setting]
    mask = abi.scene_opaque_texture_mask(sc) if masked else 0
    S, P = main_config(size)
    words, codes, setup, _, _ = _inputs(name, size, True)
    want = ref.shadow_mask_rt_soft_cutout(_arith(), words, codes, setup.inv_view, *setup.fazz, list(FENCE_LIGHTS), OFFSET, TMIN, tris, FENCE_RADII,
                                          _table(S, P), abi.scene_triangle_attributes(sc), sc.textures, lod, mask)
    got = _launch(name, size, FENCE_LIGHTS, FENCE_RADII, S, P, cutout=(abi.ray_cutout(lod, mask),))
    opaque = _launch(name, size, FENCE_LIGHTS, FENCE_RADII, S, P, cutout=(abi.ray_cutout(0, 0xFFFFFFFF),))
    print(f"[shadow mask rt soft] cutout {name} {size[0]}x{size[1]} {setting}: differing texels {int((got != want).any(axis=-1).sum())}, "
          f"channels brighter through holes {int((got > opaque).sum())}")
    _differing(f"cutout {name} {size} {setting}", got, want)
    assert (got >= opaque).all(), "a channel is darker than the opaque entry's"
    if size == (64, 36):
        assert (got > opaque).any(), "no light comes through the fence"


def test_cutout_with_every_texture_masked_is_the_opaque_soft_entry():
    """the opaque answer of the cutout entry (a mask of all ones) is vkr_shadow_mask_rt_soft's on the same input"""
    words, codes, setup, depth_bytes, normal_bytes = _inputs("raster", (64, 36), True)
    S, P = 4, 2
    got = _launch("raster", (64, 36), FENCE_LIGHTS, FENCE_RADII, S, P, cutout=(abi.ray_cutout(0, 0xFFFFFFFF),))
    want = ref.shadow_mask_rt_soft(_arith(), words, codes, setup.inv_view, *setup.fazz, list(FENCE_LIGHTS), OFFSET, TMIN, _scene(True)[1], FENCE_RADII,
                                   _table(S, P))
    _differing("cutout entry, every texture masked opaque", got, want)


# ---- the cull switch --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cull():
    """the build of csrc/shadow_mask_rt_soft.hip with the light-volume cull (the library is built without it: DESIGN.md 7.12), as
    tools/shadow_mask_rt_soft_timing.py builds it"""
    sys.path.insert(0, os.path.join(abi.ROOT, "tools"))
    import shadow_mask_rt_soft_timing as tool

    if not os.path.exists(tool.VARIANTS["cull"][1]):
        tool.build_variant("cull")
    return tool.load_variant("cull", abi.product())


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_with_and_without_the_cull_give_the_same_bytes(cull, name):
    size = (64, 36)
    for key in ("4", "mixed"):
        lights, radii = SETS[key]
        a = _launch(name, size, lights, radii, 16, 4)
        _differing(f"with the cull, {name} lights {key}", _launch(name, size, lights, radii, 16, 4, entry=cull[0]), a)
    if name in ("raster", "checker_px", "normal_noise"):
        cut = (abi.ray_cutout(0, 0),)
        a = _launch(name, size, FENCE_LIGHTS, FENCE_RADII, 16, 4, cutout=cut)
        _differing(f"with the cull, cutouts, {name}", _launch(name, size, FENCE_LIGHTS, FENCE_RADII, 16, 4, cutout=cut, entry=cull[1]), a)


# ---- the frame ----------------------------------------------------------------------------------------------------------------------------
W, H = 256, 144
FRAME_LIGHTS = [POINT_A, SUN_A, POINT_B]
FRAME_RADII = [0.5, 0.25, 0.0]


def _by_hand(frame, setup, accel, lights, radii, S, P, sc=None, cutout=None):
    """the entries on the frame's own images; radii None: vkr_shadow_mask_rt"""
    import torch

    out = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda", fill=FILL)
    params = abi.shadow_rt_params(setup.inv_view, lights, *setup.fazz, normal_offset=OFFSET, tmin=TMIN)
    depth, normal = frame.image("depth", 0, 1), frame.image("normal")
    if radii is None:
        abi.shadow_mask_rt(depth, normal, accel, params, out.desc(), _stream())
    else:
        soft = abi.shadow_rt_soft(radii, S, P, device="cuda", table=abi.shadow_disk_samples(S, P))
        if cutout is None:
            abi.shadow_mask_rt_soft(depth, normal, accel, params, soft, out.desc(), _stream())
        else:
            rs, keep = sc.upload(device="cuda")
            att = abi.scene_triangle_attributes(sc)
            attribs = torch.from_numpy(np.ascontiguousarray(att).view(np.uint8).copy()).to("cuda")
            nbytes = abi.accel_cutout_scratch_bytes(rs.texture_count)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            abi.shadow_mask_rt_soft_cutout(depth, normal, accel, attribs.data_ptr(), len(att), rs.textures, rs.texture_count, params, cutout, soft, out.desc(),
                                           scratch.data_ptr(), nbytes, _stream())
            _sync()  # before the scene's upload and the scratch go out of scope
    _sync()
    return out.raw(0)


def test_frame_stage():
    sc = scn.procedural_scene(detail=12, cutout=True)
    setup = FrameSetup(W, H)
    frame = host.HostFrame(setup, device="cuda")
    accel = abi.Accel.from_scene(sc)
    try:
        frame.load_scene(sc)
        # a frame that has not called the setter: the hard stage, the bytes of vkr_shadow_mask_rt
        frame.run(host.STAGE_RASTER | host.STAGE_SHADOW_MASK_RT)
        _sync()
        assert frame.last_tasks() == ["GbufferPass", "ShadowMaskRT"], frame.last_tasks()
        _differing("never set, against vkr_shadow_mask_rt", frame.download("shadow_mask").raw(0), _by_hand(frame, setup, accel, [POINT_A], None, 0, 0))
        with pytest.raises(RuntimeError, match="count 3, but 1 lights are set"):
            frame.set_shadow_area_lights(FRAME_RADII)
        frame.set_shadow_rays(FRAME_LIGHTS)
        hard = _by_hand(frame, setup, accel, FRAME_LIGHTS, None, 0, 0)
        for S, P in ((16, 4), (5, 2)):
            frame.set_shadow_area_lights(FRAME_RADII, S, P)
            frame.run(host.STAGE_SHADOW_MASK_RT)
            _sync()
            assert frame.last_tasks() == ["ShadowMaskRTSoft"], frame.last_tasks()
            staged = frame.download("shadow_mask").raw(0)
            _differing(f"area lights S {S} P {P}, against the entry called by hand", staged, _by_hand(frame, setup, accel, FRAME_LIGHTS, FRAME_RADII, S, P))
            assert np.array_equal(staged[..., 2], hard[..., 2]) and (staged[..., 3] == 255).all()
            between = (staged[..., 0] > 0) & (staged[..., 0] < 255)
            assert between.any(), "no penumbra under light 0"
        # with cutouts: the cutout entry, the same task name
        frame.set_shadow_area_lights(FRAME_RADII, 16, 4)
        frame.set_ray_cutouts(True, alpha_lod=0)
        frame.run(host.STAGE_SHADOW_MASK_RT)
        _sync()
        assert frame.last_tasks() == ["ShadowMaskRTSoft"], frame.last_tasks()
        cut = abi.ray_cutout(0, abi.scene_opaque_texture_mask(sc))
        with_holes = frame.download("shadow_mask").raw(0)
        _differing("area lights with cutouts, against the cutout entry called by hand", with_holes,
                   _by_hand(frame, setup, accel, FRAME_LIGHTS, FRAME_RADII, 16, 4, sc, cut))
        assert (with_holes >= _by_hand(frame, setup, accel, FRAME_LIGHTS, FRAME_RADII, 16, 4)).all(), "a channel is darker than the opaque soft entry's"
        frame.set_ray_cutouts(False)
        # every radius 0 again: the hard stage, its task name and its bytes
        frame.set_shadow_area_lights([0.0, 0.0, 0.0])
        frame.run(host.STAGE_SHADOW_MASK_RT)
        _sync()
        assert frame.last_tasks() == ["ShadowMaskRT"], frame.last_tasks()
        _differing("radii back to 0, against vkr_shadow_mask_rt", frame.download("shadow_mask").raw(0), hard)
        with pytest.raises(RuntimeError, match="sample_count 65"):
            frame.set_shadow_area_lights(FRAME_RADII, 65, 4)
    finally:
        accel.close()
        frame.close()


def test_frame_applies_the_soft_mask_when_asked():
    """vkrh_set_shadow_mask(apply = 1): color_out of a run with area lights equals vkr_defered_shading_shadowed called by hand on the
    frame's images, and some texels lie strictly between their hard-shadow and their unshadowed values"""
    sc = scn.procedural_scene(detail=12)
    setup = FrameSetup(W, H)
    frame = host.HostFrame(setup, device="cuda")
    try:
        frame.load_scene(sc)
        frame.run(host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH)
        stages = host.STAGE_RASTER | host.STAGE_SHADOW_MASK_RT | host.STAGE_CHAIN | host.STAGE_SHADING
        consts = abi.ShadingParams()
        consts.inverse_camera = abi.Mat4.from_np(setup.inv_view)
        consts.camera = abi.Mat4.from_np(setup.view)
        consts.shadow_mvp = abi.Mat4.from_np(np.eye(4))
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

        frame.set_shadow_mask(apply=1)
        frame.run(stages)  # the hard mask of the default light
        _sync()
        hard_color = frame.download("color_out").raw(0)
        frame.set_shadow_area_lights([0.5], 16, 4)
        frame.run(stages)
        _sync()
        tasks = frame.last_tasks()
        assert tasks.index("GbufferPass") < tasks.index("ShadowMaskRTSoft") < tasks.index("DeferedShading") and "ShadowMaskRT" not in tasks, tasks
        got = frame.download("color_out").raw(0)
        plain, shadowed = by_hand(False), by_hand(True)
        assert np.array_equal(got, shadowed), f"{int((got != shadowed).any(axis=-1).sum())} texels differ from vkr_defered_shading_shadowed called by hand"
        lo, hi, g = hard_color.astype(int), plain.astype(int), got.astype(int)
        between = ((g > lo) & (g < hi)).any(axis=-1)
        print(f"[shadow mask rt soft] frame: {int(between.sum())} texels of color_out strictly between their hard-shadow and their unshadowed values")
        assert between.sum() >= 1
    finally:
        frame.close()
