"""Adversarial content for the four side passes that the hostile-input work had left out: ssao, tile_regression, gtao_rt_main and
trace_probe.  Shared by tests/test_side_pass_content.py (CPU: the numpy restatements alone, class quality) and
tests/test_side_pass_content_gpu.py (each kernel against its restatement).

A Gbuffer holds the host images a content class of tests/gbuffer_content.py touches (depth, prev_depth, normal), filled from the
oracle's rasteriser of scene.procedural_scene at the next even extent and cut to size; where the pass reads depth mip 1 the
holder takes that mip from the oracle's downsample and the normal stays at twice the extent.  Nothing on the reference side
comes from the GPU.  Only texel values are adversarial: every descriptor, extent, mip count, layer count and grid size is one
its entry accepts.  Draws come from numpy.random.default_rng with a seed fixed per (pass, class, size).
"""
import functools

import numpy as np

from vk_renderer_amd import abi
from vk_renderer_amd import scene as scn
from vk_renderer_amd.chain import PostFxChain
from vk_renderer_amd.images import ImageBuf

import camera_cases as cc
import gbuffer_content as content
import gtao_rt_reference as gtao_ref
import probe_reference as probe_ref
import ssao_reference as ssao_ref
import tile_regression_reference as tile_ref
from test_probe_gpu import PMAX, PMIN, _room_cube
from test_tile_regression_gpu import HAND_CAMERA, HAND_FAZZ  # noqa: F401  (re-exported for the two test files)

F32 = np.float32
SKY = content.SKY
RASTER_DETAIL = 8  # the scene of the G-buffer (the traced AO's ray scene has a detail of its own, AO_DETAIL)


def arith():
    return gtao_ref.Arith(int(abi.product().vkr_numeric_contract()))


# ---- the G-buffer holder ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _raster(size, depth_mip):
    """-> (depth words [h, w] of the view, normal codes, setup).  depth_mip 0: size is the G-buffer's extent; depth_mip 1: size
    is the extent of depth mip 1, the G-buffer (and the normal) has twice that"""
    w, h = size
    ew, eh = (w + (w & 1), h + (h & 1)) if depth_mip == 0 else (2 * w, 2 * h)
    setup = cc.frame_setup(size, ew, eh)  # the frozen camera, or the case an Extent names
    chain = PostFxChain(ew, eh, backend="oracle", setup=setup)
    chain.raster(scn.procedural_scene(detail=RASTER_DETAIL))
    if depth_mip == 0:
        return chain.depth.raw(0)[:h, :w, 0].astype(np.uint32), chain.normal.raw(0)[:h, :w].copy(), setup
    chain.downsample()
    words = chain.depth.raw(1)[..., 0].astype(np.uint32)
    assert words.shape == (h, w)
    return words, chain.normal.raw(0).copy(), setup


class Gbuffer:
    """what a content class of tests/gbuffer_content.py touches of a chain: host images of the inputs of a side pass.  depth is
    the view the pass reads, size[0] x size[1] (depth_mip 1: the oracle's mip 1 of a G-buffer of twice the extent, whose normal
    this holds at full extent)"""

    def __init__(self, size, depth_mip=0):
        w, h = size
        words, codes, self.setup = _raster(size, depth_mip)
        self.depth = self.prev_depth = ImageBuf(abi.FMT_D24_UNORM_S8, w, h)
        self.normal = ImageBuf(abi.FMT_RG16_UNORM, codes.shape[1], codes.shape[0])
        self.depth.set_raw(words.reshape(h, w, 1))
        self.normal.set_raw(codes)


# ---- classes ----------------------------------------------------------------------------------------------------------------------
def raster(c, rng):
    pass


def checker_tile8(c, rng):
    x, y = content._grid(c.depth)
    content._set_depth(c.depth, SKY, (((x // 8) + (y // 8)) & 1) == 1)


def stencil_noise(c, rng):
    """the raster depth with a random top byte in every word: every pass must produce exactly the bytes of `raster`"""
    d = c.depth.raw(0)[..., 0]
    top = rng.integers(0, 256, size=d.shape, dtype=np.uint32) << np.uint32(24)
    c.depth.set_raw(((d & np.uint32(SKY)) | top).astype(np.uint32))


def near_codes(c, rng):
    """depth codes 0 .. 3, random per pixel: view z = -znear or one or two float steps behind it, so a sample pushed 0.05 towards
    the eye lands on the eye plane or a few ulps from it (clip.w = 0 or ~4e-9: infinite, NaN and huge finite coordinates mixed)"""
    content._set_depth(c.depth, rng.integers(0, 4, size=(c.depth.height, c.depth.width), dtype=np.uint32))


DEPTH_CLASSES = {f.__name__: f for f in (raster, content.sky_all, content.near_all, content.checker_px, content.checker_tile, checker_tile8,
                                         content.depth_noise, content.depth_stripes, stencil_noise)}
NORMAL_CLASSES = {f.__name__: f for f in (content.normal_noise, content.normal_poles)}
CLASSES = {**DEPTH_CLASSES, **NORMAL_CLASSES}
SSAO_CLASSES = {**DEPTH_CLASSES, "near_codes": near_codes}  # the issue's depth classes and one more, for the pass that divides by clip.w
_ALL = {**CLASSES, **SSAO_CLASSES}
PASSES = ("ssao", "tile_regression", "gtao_rt", "trace_probe")


def seed_of(pass_name, name, size):
    return [0x51DE_9A55, PASSES.index(pass_name), sorted(_ALL).index(name), size[0], size[1]]


@functools.lru_cache(maxsize=None)
def inputs(pass_name, name, size, depth_mip=0):
    """-> (depth words [h, w], normal codes [nh, nw, 2], setup, the depth image's bytes, the normal image's bytes): class `name`
    applied to the raster G-buffer of `size`.  Cached: treat as read-only."""
    g = Gbuffer(size, depth_mip)
    _ALL[name](g, np.random.default_rng(seed_of(pass_name, name, size)))
    out = (g.depth.raw(0)[..., 0].copy(), g.normal.raw(0).copy(), g.setup, g.depth.to_host().copy(), g.normal.to_host().copy())
    for a in (out[0], out[1], out[3], out[4]):
        a.setflags(write=False)
    return out


# ---- ssao -------------------------------------------------------------------------------------------------------------------------
# (depth extent, output extent): equal; both odd and different; a depth one texel wide (the instantiation without pair loads)
SSAO_SIZES = (((70, 38), (70, 38)), ((35, 19), (37, 21)), ((1, 19), (5, 3)))
SSAO_SAMPLE_SETS = ("fixed", "eye_plane")


def ssao_samples(which):
    """fixed: ssao_reference.fixed_samples(); eye_plane: sample 0 replaced by (0, 0, 1) and sample 1 by (0, 0, -1), so that under
    near_all (view z = -znear = -0.05, and 0.05 * 1 on top of it) the sample lands on the eye plane"""
    s = ssao_ref.fixed_samples().copy()
    if which == "eye_plane":
        s[0] = (0.0, 0.0, 1.0)
        s[1] = (0.0, 0.0, -1.0)
    return s


@functools.lru_cache(maxsize=None)
def ssao_expected(name, depth_size, out_size, which):
    """-> (codes [oh, ow] uint8, counts, stats)"""
    words, _, setup, _, _ = inputs("ssao", name, depth_size)
    stats = {}
    codes, counts = ssao_ref.ssao(arith(), words, setup.proj, *setup.fazz, ssao_samples(which), out_size[0], out_size[1], stats=stats)
    return codes, counts, stats


# ---- tile regression --------------------------------------------------------------------------------------------------------------
# depth views (mip 1 of a G-buffer of twice the extent): 5 x 3 tiles with partial right and bottom tiles; whole tiles, less than
# one block; one inside column in the last tile and one inside row in the bottom tiles
TILE_SIZES = ((35, 19), (16, 8), (33, 9))
TILE_CAMERAS = ("frame", "hand")


def tile_camera(which, setup):
    """-> (camera_to_world 4x4, (fovy, aspect, znear, zfar))"""
    if which == "hand":
        return HAND_CAMERA, HAND_FAZZ
    return setup.inv_view, tuple(float(v) for v in setup.fazz)


@functools.lru_cache(maxsize=None)
def tile_expected(name, size, which):
    words, _, setup, _, _ = inputs("tile_regression", name, size, 1)
    cam, fazz = tile_camera(which, setup)
    tw, th = tile_ref.tiles_of(*size)
    return tile_ref.tile_regression(arith(), words, cam, *fazz, tw, th)


def tile_counts(want):
    """-> (tiles with finite planes, with a NaN in the plane, with a residual of exactly 1e10)"""
    plane, res = want[..., :3], want[..., 3]
    return int(np.isfinite(plane).all(axis=-1).sum()), int(np.isnan(plane).any(axis=-1).sum()), int((res == F32(tile_ref.NAN_RESIDUAL)).sum())


# ---- traced AO --------------------------------------------------------------------------------------------------------------------
AO_SIZES = ((35, 19), (9, 5))  # 665 pixels: the last block of four waves has one live wave; 45 pixels: likewise
AO_ROTATIONS = (0.0, 0.3)
AO_DETAIL = 16
AO_SCENES = ("scene", "empty")


@functools.lru_cache(maxsize=None)
def ao_triangles(which):
    if which == "empty":
        return np.zeros((0, 3, 3), F32)
    return abi.scene_triangles(scn.procedural_scene(detail=AO_DETAIL))


@functools.lru_cache(maxsize=None)
def ao_directions():
    return gtao_ref.random_directions(64)


def ao_camera(setup):
    return setup.inv_view, float(setup.fazz[0]), float(setup.fazz[1]), float(setup.fazz[2]), float(setup.fazz[3])


@functools.lru_cache(maxsize=None)
def ao_expected(name, size, rotation, which):
    """-> float16 [h, w, 4]"""
    words, codes, setup, _, _ = inputs("gtao_rt", name, size, 1)
    return gtao_ref.gtao_rt(arith(), words, codes, ao_camera(setup), rotation, ao_directions(), ao_triangles(which), size[0], size[1])


@functools.lru_cache(maxsize=None)
def ao_sky(name, size):
    """-> [h, w] bool: the pixels whose sampled depth is >= 1 (steps 1-4 of the restatement, no ray)"""
    words, codes, setup, _, _ = inputs("gtao_rt", name, size, 1)
    return gtao_ref.pixel_setup(arith(), words, codes, *ao_camera(setup), 0.0, size[0], size[1])[0]


def ao_open_hemisphere():
    """what a live pixel with no occluder holds: 2 / 64 * sum max(dir_i.z, 0), to float16's precision"""
    return 2.0 / 64.0 * float(np.maximum(ao_directions()[:, 2].astype(np.float64), 0.0).sum())


# ---- probe trace ------------------------------------------------------------------------------------------------------------------
PROBE_SIZES = ((70, 38), (24, 12))  # dispatch extents 64 x 36 (the tail must keep its fill) and 24 x 12
PROBE_SIZE, CUBE_SIZE = 32, 16
PROBE_MIPS = 6
GRIDS = ((4, 16), (3, 16), (2, 4))  # (grid, layers): exact; more layers than the grid uses, start-probe clamp at 1; the clamp at 0
PROBE_CLASSES = ("room", "noise_pyramid", "independent_mips", "short_chain", "colour_noise")
# (G-buffer class, probe class): every G-buffer class against the room probes, every other probe class on the raster G-buffer
# and short_chain under three more G-buffers: on `raster` alone a kernel that reads the last mip's texel past the chain gives the
# same image (the rays it sends elsewhere end as MISS or UNKNOWN either way); these three each change a few texels
PROBE_CASES = (tuple((g, "room") for g in CLASSES) + tuple(("raster", p) for p in PROBE_CLASSES[1:])
               + tuple((g, "short_chain") for g in ("near_all", "depth_noise", "depth_stripes")))


def probe_positions(grid, layers):
    """probe p of the grid at probe_min + step * (p % grid, 0, p // grid); layers past grid^2 (never addressed) repeat probe 0"""
    step = (np.array(PMAX[:3], F32) - np.array(PMIN[:3], F32)) / F32(grid - 1)
    pos = [np.array(PMIN[:3], np.float64) + step.astype(np.float64) * np.array([p % grid, 0, p // grid]) for p in range(grid * grid)]
    return pos + [pos[0]] * (layers - grid * grid)


@functools.lru_cache(maxsize=None)
def room_cubes(grid, layers):
    """the analytic room of tests/test_probe_gpu.py seen from every probe: [(colour codes [6, n, n, 4], distance [6, n, n])]"""
    return [_room_cube(p, CUBE_SIZE) for p in probe_positions(grid, layers)]


@functools.lru_cache(maxsize=None)
def room_probes_host(grid, layers):
    """the room probes by the restatements of the two bake kernels (cube2oct, probe_downsample): (colour codes [L, S, S, 4],
    [depth codes [L, S >> m, S >> m] per mip]).  The GPU test bakes the same probes with the kernels and checks them equal."""
    ar = arith()
    colour, mip0 = zip(*[probe_ref.cube2oct(ar, c, d, PROBE_SIZE, PROBE_SIZE) for c, d in room_cubes(grid, layers)])
    chains = [probe_ref.probe_downsample(m, PROBE_MIPS) for m in mip0]
    return np.stack(colour), [np.stack([ch[m] for ch in chains]) for m in range(PROBE_MIPS)]


def _probe_noise(rng, shape):
    """random R16 codes over the full range, three quarters of them 65535 - floor(65535 u^4), u uniform: an octahedral depth of
    1 - 0.05 / distance lies above 0.9 from half a unit on, so uniform codes lie below almost every ray and end its march at the
    first step; these lie where the rays are, on both sides of them"""
    u = rng.random(shape)
    near_one = 65535 - np.floor(65535.0 * u ** 4).astype(np.int64)
    uniform = rng.integers(0, 65536, shape)
    return np.where(rng.random(shape) < 0.75, near_one, uniform).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def probes(name, grid, layers):
    """-> (colour codes [L, S, S, 4] uint8, [depth codes per mip]) of probe class `name`"""
    colour, depth = room_probes_host(grid, layers)
    rng = np.random.default_rng([0x9B0BE, PROBE_CLASSES.index(name), grid, layers])
    S = PROBE_SIZE
    if name == "noise_pyramid":  # mip 0 random codes, upper mips the min-pyramid of it
        mip0 = _probe_noise(rng, (layers, S, S))
        chains = [probe_ref.probe_downsample(m, PROBE_MIPS) for m in mip0]
        depth = [np.stack([ch[m] for ch in chains]) for m in range(PROBE_MIPS)]
    elif name == "independent_mips":  # no min-pyramid: the march climbs and descends wherever the comparisons send it
        depth = [_probe_noise(rng, (layers, S >> m, S >> m)) for m in range(PROBE_MIPS)]
    elif name == "short_chain":  # 3 of the 6 mips: a climb past the last one reads 0.  Noise colour, so that a hit that moves shows
        depth = depth[:3]
        colour = rng.integers(0, 256, colour.shape, dtype=np.uint8)
    elif name == "colour_noise":
        colour = rng.integers(0, 256, colour.shape, dtype=np.uint8)
    out = np.ascontiguousarray(colour), [np.ascontiguousarray(d) for d in depth]
    out[0].setflags(write=False)
    for d in out[1]:
        d.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def probe_expected(gname, size, pname, grid, layers):
    """-> (codes [th, tw, 4], result [th, tw], traced [th, tw], fetches past the last mip) on the dispatch extent"""
    words, codes, setup, _, _ = inputs("trace_probe", gname, size)
    colour, depth = probes(pname, grid, layers)
    pa = probe_ref.ProbeArrays(colour, depth)
    out, result, traced = probe_ref.trace_probe(arith(), words, codes, pa, setup.inv_view, PMIN, PMAX, grid, *[float(v) for v in setup.fazz],
                                                size[0], size[1])
    return out, result, traced, pa.past_last_mip
