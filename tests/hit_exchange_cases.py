"""Constructed strip cuts and ray images for the hit request / reply exchange (csrc/hit_exchange.hip).

The exchange's kernels decide everything from the rays' uv codes, the pending rays' raw float uv and the strip cut: which rows a
footprint touches, who owns them, how many requests a ray, a wave, a tile and a block have, and in which slot each lands.  The
geometries below are the smallest strip cuts at which each of those decisions has another outcome (three uneven strips, strips of
one half-res row, HIT_MAX_WORLD strips, one tile per block / two / five, 14-bit rows and columns); the classes fill the window's
rays, pending mask and pending data with the content that reaches them.  Draws come from numpy.random.default_rng with a seed per
(geometry, class, rank): the bytes are frozen.

HitRig is a PostFxChain that allocates only the images the exchange touches, on either backend, so that the chain's own hit_*
drivers run on a 1024 x 8192 frame without the rest of the chain's resource set.
"""
from dataclasses import dataclass

import numpy as np

import hit_exchange_reference as ref
from vk_renderer_amd import abi
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import _BACKENDS, PostFxChain
from vk_renderer_amd.images import ImageBuf

POISON = 0xA5


@dataclass(frozen=True)
class Geometry:
    name: str
    W: int
    H: int
    bounds: tuple
    halo: int
    ranks: tuple

    @property
    def world(self):
        return len(self.bounds) - 1

    def window(self, rank):
        """the full-res rows [win0, win1) rank holds: its strip and `halo` rows either side"""
        return max(0, self.bounds[rank] - self.halo), min(self.H, self.bounds[rank + 1] + self.halo)

    def rays_extent(self, rank):
        w0, w1 = self.window(rank)
        return self.W // 2, (w1 - w0) // 2


GEOMETRIES = {g.name: g for g in (
    Geometry("ragged3", 206, 226, (0, 64, 150, 226), 16, (0, 1, 2)),        # three uneven strips; extents ragged against 64 and 16
    Geometry("small3", 140, 76, (0, 20, 50, 76), 8, (1,)),                  # 70 x 23 rays
    Geometry("world16", 128, 512, tuple(range(0, 513, 32)), 8, (0, 7, 15)),  # HIT_MAX_WORLD
    Geometry("thin16", 128, 512, tuple(range(0, 31, 2)) + (512,), 8, (0, 15)),  # strips of two rows: one half-res row each
    Geometry("world1", 70, 38, (0, 38), 8, (0,)),                           # nothing to ask
    Geometry("tiles256", 2048, 480, (0, 80, 480), 60, (1,)),                # 1024 x 230 rays: 16 x (15 + 1) tiles, one per block
    Geometry("tiles257", 128, 8192, (0, 192, 8192), 180, (1,)),             # 64 x 4090 rays: 1 x (256 + 1) tiles, block 0 has two (the apron's)
    Geometry("tiles1080", 1024, 8192, (0, 4200, 8192), 64, (0,)),           # 512 x 2132 rays: 8 x (134 + 1) tiles, 56 blocks with 5, 200 with 4
    Geometry("wide", 16384, 64, (0, 32, 64), 8, (0,)),                      # x up to 16382
    Geometry("tall", 64, 16384, (0, 8192, 16384), 8, (0,)),                 # rows up to 16383
)}


class HitRig(PostFxChain):
    """the images of the exchange for one rank of a geometry: the window's rays / pending images / albedo / downsampled normals
    and the whole-frame images the scatter writes"""

    def __init__(self, geom, rank, backend="oracle", device=None):
        self.geom, self.rank = geom, rank
        self.W, self.H, self.backend = geom.W, geom.H, backend
        self.lib, self.prefix, on_device = _BACKENDS[backend]()
        self.device = (device or "cuda") if on_device else None
        self.stream = self._stream_ptr(self.device) if on_device else None
        self.setup = FrameSetup(geom.W, geom.H)
        win0, win1 = geom.window(rank)
        self.window = (0, win0, geom.W, win1 - win0)
        self.tiled = True
        W, H, wh = geom.W, geom.H, win1 - win0
        half = dict(device=self.device, full=(W // 2, H // 2), origin=(0, win0 // 2))
        self.rays = ImageBuf(abi.FMT_RGBA16_UNORM, W // 2, wh // 2, **half)
        self.dn = ImageBuf(abi.FMT_RG16_UNORM, W // 2, wh // 2, **half)
        self.albedo = ImageBuf(abi.FMT_RGBA8_SRGB, W, wh, device=self.device, full=(W, H), origin=(0, win0))
        self.frame_normals = ImageBuf(abi.FMT_RG16_UNORM, W // 2, H // 2, device=self.device, fill=POISON)
        self.frame_albedo = ImageBuf(abi.FMT_RGBA8_SRGB, W, H, device=self.device, fill=POISON)
        self._pending_images()


def _rows(img, a):
    """raw texels `a` [h, w, c] -> the bytes of a one-mip image"""
    host = np.zeros(img.nbytes, dtype=np.uint8)
    rows = np.ascontiguousarray(a).reshape(img.height, -1).view(np.uint8)
    host[: img.pitch[0] * img.height].reshape(img.height, img.pitch[0])[:, : rows.shape[1]] = rows
    return host


@dataclass
class Case:
    geom: Geometry
    rank: int
    name: str
    rays: np.ndarray      # [h2, w2, 4] uint16
    mask: np.ndarray      # [h2, w2] uint8
    data: np.ndarray      # [h2, w2, 8] float32: pending data (R and, at [4:6], the hit uv)
    albedo: np.ndarray    # [H, W] uint32: the frame's albedo texels (every owner's rows)
    normals: np.ndarray   # [H / 2, W / 2] uint32

    @property
    def hit_uv(self):
        return self.data[..., 4:6]

    def requests(self, rules=ref.EXACT):
        win0, win1 = self.geom.window(self.rank)
        return ref.emit(self.rays, self.mask, self.hit_uv, self.geom.W, self.geom.H, win0, win1, self.geom.bounds, rules)

    def fill(self, rig):
        """the case's bytes into a rig of its rank"""
        rig.rays.upload(_rows(rig.rays, self.rays))
        rig.pend_mask.upload(_rows(rig.pend_mask, self.mask))
        rig.pend_data.upload(_rows(rig.pend_data, self.data))
        fill_owner(rig, self.albedo, self.normals)

    def frame_images(self):
        """what the whole-frame images hold before the scatter: the rank's own rows, poison elsewhere (uint32 texels)"""
        return poisoned_frames(self.geom, self.rank, self.albedo, self.normals)


def poisoned_frames(g, rank, albedo, normals):
    win0, win1 = g.window(rank)
    fa = np.full(albedo.shape, POISON * 0x01010101, dtype=np.uint32)
    fn = np.full(normals.shape, POISON * 0x01010101, dtype=np.uint32)
    fa[win0: win1], fn[win0 // 2: win1 // 2] = albedo[win0: win1], normals[win0 // 2: win1 // 2]
    return fa, fn


def fill_owner(rig, albedo, normals):
    """the rig's window rows of the frame's albedo and downsampled normals, as an owner answers from them; the whole-frame images:
    the own rows, poison elsewhere"""
    win0, win1 = rig.geom.window(rig.rank)
    rig.albedo.upload(_rows(rig.albedo, albedo[win0: win1]))
    rig.dn.upload(_rows(rig.dn, normals[win0 // 2: win1 // 2]))
    fa, fn = poisoned_frames(rig.geom, rig.rank, albedo, normals)
    rig.frame_albedo.upload(_rows(rig.frame_albedo, fa))
    rig.frame_normals.upload(_rows(rig.frame_normals, fn))


def window_texels(rig, which):
    """(uint32 texels [rows, width], first frame row) of an owner's albedo ("albedo") or downsampled normals ("dn")"""
    img = getattr(rig, which)
    return np.ascontiguousarray(img.raw(0)).view(np.uint32).reshape(img.height, img.width), img.origin[1]


def frame_texels(rig):
    return tuple(np.ascontiguousarray(img.raw(0)).view(np.uint32).reshape(img.height, img.width) for img in (rig.frame_albedo, rig.frame_normals))


# ---- aiming ------------------------------------------------------------------------------------------------------------
_TABLES = {}


def index_table(extent):
    if extent not in _TABLES:
        _TABLES[extent] = ref.code_index_table(extent)
    return _TABLES[extent]


def codes_for(index, extent):
    """(smallest, largest) UNORM16 uv code whose y0 / x0 on an image of `extent` texels is `index`, or () if there is none"""
    c = np.nonzero(index_table(extent) == index)[0]
    return (int(c[0]), int(c[-1])) if c.size else ()


def floats_for(index, extent):
    """(smallest, largest) float32 uv whose y0 / x0 is `index`, found by stepping nextafter from (index + 0.5) / extent and
    (index + 1.5) / extent, and their outer neighbours (whose index is index - 1 and index + 1)"""
    def settle(u, step, want):
        u = np.float32(u)
        for _ in range(8):  # towards the inside until the index is `want` ...
            if int(ref.texel_index(u, extent)) == want:
                break
            u = np.nextafter(u, np.float32(step))
        for _ in range(8):  # ... then outwards as long as it stays
            o = np.nextafter(u, np.float32(-step))
            if int(ref.texel_index(o, extent)) != want:
                break
            u = o
        assert int(ref.texel_index(u, extent)) == want
        return u
    lo, hi = settle((index + 0.5) / extent, np.inf, index), settle((index + 1.5) / extent, -np.inf, index)
    return np.array([lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))], dtype=np.float32)


def rows_of_interest(g, rank):
    """y0 values around frame rows 0 and ah - 1, the window's ends and every strip boundary, offsets -2 .. +1"""
    win0, win1 = g.window(rank)
    rows = set()
    for r in {0, g.H - 1, win0, win1} | set(g.bounds):
        rows.update(r + d for d in (-2, -1, 0, 1))
    return sorted(r for r in rows if -1 <= r <= g.H - 1)


def half_rows_of_interest(g, rank):
    win0, win1 = g.window(rank)
    rows = set()
    for r in {0, g.H // 2 - 1, win0 // 2, win1 // 2} | {b // 2 for b in g.bounds}:
        rows.update(r + d for d in (-2, -1, 0, 1))
    return sorted(r for r in rows if -1 <= r <= g.H // 2 - 1)


def foreign_rows(g, rank):
    win0, win1 = g.window(rank)
    return np.array([r for r in range(g.H) if r < win0 or r >= win1], dtype=np.int64)


def code_aimed_at(rows, extent):
    """a uv code whose y0 is each of `rows` (the smallest one)"""
    t = index_table(extent)
    first = np.full(extent + 1, -1, dtype=np.int64)  # first code of y0 = -1 .. extent - 1
    index, code = np.unique(t, return_index=True)
    first[index + 1] = code
    got = first[np.asarray(rows) + 1]
    assert (got >= 0).all(), "a frame taller than 65536 / 2 rows has rows no uv code reaches"
    return got.astype(np.uint16)


def float_aimed_at(rows, extent, frac):
    """a float32 uv whose f = row + frac"""
    return ((np.asarray(rows, dtype=np.float64) + 0.5 + frac) / extent).astype(np.float32)


# ---- the classes: (geometry, rank, rng, blank case) -> fills rays / mask / data ------------------------------------------------------
def misses(c, rng):
    c.rays[..., 3] = 0xFFFF
    c.mask[:] = 0


def _cycle(c, ycodes, xcodes, hys, hxs):
    """The uv.y codes laid through the window cyclically, the uv.x codes beside them shifted by one per cycle (so that a y code
    meets another x code every time round), every fifth cycle all misses; the same for the pending rays' (hit uv.y, hit uv.x),
    every fourth cycle not pending.  The first cycle of each is complete and live: every y code is on a hit ray and every hit
    uv.y on a pending ray (tests/test_hit_exchange_cases.py asserts it, and that every x value is on a ray that asks)."""
    h2, w2 = c.mask.shape
    i = np.arange(h2 * w2)
    ycodes, xcodes = np.asarray(ycodes, dtype=np.uint16), np.asarray(xcodes, dtype=np.uint16)
    hys, hxs = np.asarray(hys, dtype=np.float32), np.asarray(hxs, dtype=np.float32)
    assert i.size >= max(ycodes.size, hys.size), "the window is too small to carry every code once"
    k = i // ycodes.size
    c.rays[..., 1] = ycodes[i % ycodes.size].reshape(h2, w2)
    c.rays[..., 0] = xcodes[(i + k) % xcodes.size].reshape(h2, w2)
    c.rays[..., 3] = np.where(k % 5 == 4, 0xFFFF, c.rays[..., 3].reshape(-1) & 0xFFFE).reshape(h2, w2)
    k = i // hys.size
    c.mask[:] = np.where(k % 4 == 3, 0, np.array([1, 0x80, 0xFF], dtype=np.uint8)[i % 3]).reshape(h2, w2)
    c.data[..., 5] = hys[i % hys.size].reshape(h2, w2)
    c.data[..., 4] = hxs[(i + k) % hxs.size].reshape(h2, w2)


def edge_lists(g, rank):
    """(uv.y codes, uv.x codes, hit uv.y floats, hit uv.x floats) of `edge_rows`: the smallest and the largest code / float of every
    row of interest and its outer neighbours, x codes 0, 1, 65534, 65535 and those around x0 = w - 2"""
    ycodes = [code for r in rows_of_interest(g, rank) for code in codes_for(r, g.H)]
    xcodes = [0, 1, 65534, 65535] + [code for x in (g.W - 4, g.W - 3, g.W - 2, g.W - 1) for code in codes_for(x, g.W)]
    hys = np.concatenate([floats_for(r, g.H // 2) for r in half_rows_of_interest(g, rank)])
    hxs = np.concatenate([np.array([0.0, 1.0], dtype=np.float32)] + [floats_for(x, g.W // 2) for x in (0, g.W // 2 - 3, g.W // 2 - 2, g.W // 2 - 1)])
    return ycodes, xcodes, hys, hxs


def edge_rows(c, rng):
    _cycle(c, *edge_lists(c.geom, c.rank))


def foreign_pairs(g, rank):
    """the strip boundaries whose two rows either side — full-res, and half-res for the normals — all lie outside the rank's window:
    a footprint across one is split between two owners that are both foreign"""
    win0, win1 = g.window(rank)
    return [b for b in g.bounds[1:-1] if (b - 1 < win0 or b - 1 >= win1) and (b < win0 or b >= win1)
            and ((b >> 1) - 1 < win0 // 2 or (b >> 1) - 1 >= win1 // 2) and ((b >> 1) < win0 // 2 or (b >> 1) >= win1 // 2)]


def four(c, rng):
    g = c.geom
    cuts = np.array(foreign_pairs(g, c.rank), dtype=np.int64)
    assert cuts.size, "needs a boundary between two foreign strips"
    shape = c.mask.shape
    c.rays[..., 1] = code_aimed_at(rng.choice(cuts, size=shape) - 1, g.H)
    c.rays[..., 3] &= 0xFFFE
    c.mask[:] = rng.choice(np.array([0, 1, 0xFF], dtype=np.uint8), size=shape)
    c.data[..., 5] = float_aimed_at((rng.choice(cuts, size=shape) >> 1) - 1, g.H // 2, rng.uniform(0.01, 0.99, size=shape))


def owner_salad(c, rng):
    """lane i of every wave aims its albedo footprint at strip (7 i) mod world and its normal footprint at strip (7 i + 3) mod world"""
    g = c.geom
    b = np.asarray(g.bounds, dtype=np.int64)
    h2, w2 = c.mask.shape
    lane = np.broadcast_to(np.arange(w2) % 64, (h2, w2))
    sa, sn = (7 * lane) % g.world, (7 * lane + 3) % g.world
    mid = lambda s: b[s] + ((b[s + 1] - b[s]) // 2 - 1).clip(0)
    c.rays[..., 1] = code_aimed_at(mid(sa), g.H)
    c.rays[..., 3] &= 0xFFFE
    c.mask[:] = 1
    c.data[..., 5] = float_aimed_at(mid(sn) >> 1, g.H // 2, 0.25)


def tile_checker(c, rng):
    g = c.geom
    h2, w2 = c.mask.shape
    y, x = np.mgrid[0:h2, 0:w2]
    tx, ty = x // 64, y // 16
    loud = ((tx + ty) & 1) == 0
    rows = foreign_rows(g, c.rank)
    c.rays[..., 1] = code_aimed_at(rng.choice(rows, size=(h2, w2)), g.H)
    c.data[..., 5] = float_aimed_at(rng.choice(rows, size=(h2, w2)) >> 1, g.H // 2, 0.5)
    c.mask[:] = rng.choice(np.array([0, 1], dtype=np.uint8), size=(h2, w2))
    # silent tiles, in turn: nothing; one ray at lane 0 / wave 0; one at the tile's last texel (lane 63 / wave 15, or the last texel
    # of a ragged tile); one pending ray there
    turn = ((ty * (-(-w2 // 64)) + tx) // 2) % 4
    first = (x % 64 == 0) & (y % 16 == 0)
    last = (x == np.minimum(tx * 64 + 63, w2 - 1)) & (y == np.minimum(ty * 16 + 15, h2 - 1))
    one = ((turn == 1) & first) | ((turn >= 2) & last)
    c.rays[..., 3] = np.where(loud | (one & (turn != 3)), c.rays[..., 3] & 0xFFFE, 0xFFFF)
    c.mask[:] = np.where(loud, c.mask, np.where(one & (turn == 3), 1, 0))


def every_code(c, rng):
    h2, w2 = c.mask.shape
    i = np.arange(h2 * w2, dtype=np.int64)
    assert i.size >= 65536
    c.rays[..., 1] = (i % 65536).reshape(h2, w2)
    c.rays[..., 0] = ((i * 7919 + i // 65536) % 65536).reshape(h2, w2)  # (odd multiplier: a bijection on every run of 65536 rays)
    c.rays[..., 3] &= 0xFFFE
    c.mask[:] = (i % 5 == 0).reshape(h2, w2)
    c.data[..., 5] = ref.unorm16_to_float((i * 40503) % 65536).reshape(h2, w2)
    c.data[..., 4] = ref.unorm16_to_float((i * 12345 + 1) % 65536).reshape(h2, w2)


def pending_floats(c, rng):
    g = c.geom
    wild = np.array([0.0, -0.0, 1.0, -0.25, 1.25, 1e30, -1e30, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, -1e-39], dtype=np.float32)
    hys = np.concatenate([wild] + [floats_for(r, g.H // 2) for r in half_rows_of_interest(g, c.rank)])
    hxs = np.concatenate([wild] + [floats_for(x, g.W // 2) for x in (0, g.W // 2 - 2, g.W // 2 - 1)])
    c.rays[..., 3] = 0xFFFF  # no albedo request but the apron's: every request below comes from a raw float
    c.mask[:] = rng.choice(np.array([1, 0x80, 0xFF], dtype=np.uint8), size=c.mask.shape)
    c.data[..., 5] = rng.choice(hys, size=c.mask.shape)
    c.data[..., 4] = rng.choice(hxs, size=c.mask.shape)


def noise(c, rng):
    shape = c.mask.shape
    c.rays[..., 3] = np.where(rng.integers(0, 2, size=shape) == 1, 0xFFFF, c.rays[..., 3])
    c.mask[:] = rng.choice(np.array([0, 1, 0x80, 0xFF], dtype=np.uint8), size=shape)
    c.data[..., 4:6] = rng.uniform(-0.25, 1.25, size=shape + (2,)).astype(np.float32)


CLASSES = {f.__name__: f for f in (misses, edge_rows, four, owner_salad, tile_checker, every_code, pending_floats, noise)}
_ON = {
    "ragged3": ("misses", "edge_rows", "four", "tile_checker", "pending_floats", "noise"),
    "small3": ("misses", "edge_rows", "tile_checker", "pending_floats", "noise"),
    "world16": ("edge_rows", "four", "owner_salad", "pending_floats", "noise"),
    "thin16": ("edge_rows", "owner_salad", "noise"),
    "world1": ("misses", "noise"),
    "tiles256": ("tile_checker", "noise"),
    "tiles257": ("tile_checker", "noise"),
    "tiles1080": ("every_code", "tile_checker", "noise"),
    "wide": ("edge_rows", "noise"),
    "tall": ("edge_rows", "noise"),
}
# (geometry, rank, class).  `four` needs a boundary between two strips that are both foreign: not on the middle rank of three
CASES = [(g, r, k) for g, ks in _ON.items() for r in GEOMETRIES[g].ranks for k in ks if not (k == "four" and not foreign_pairs(GEOMETRIES[g], r))]


def case_id(case):
    return "-".join(str(v) for v in case)


def seed_of(geom, rank, name):
    return [0x417E_C4A, list(GEOMETRIES).index(geom), rank, list(CLASSES).index(name)]


_FRAMES = {}


def frame_noise(geom):
    """noise albedo / downsampled-normal texels of the whole frame (every owner answers from its rows of them)"""
    if geom not in _FRAMES:
        g = GEOMETRIES[geom]
        rng = np.random.default_rng([0x417E_C4A, list(GEOMETRIES).index(geom)])
        _FRAMES[geom] = (rng.integers(0, 1 << 32, size=(g.H, g.W), dtype=np.uint32), rng.integers(0, 1 << 32, size=(g.H // 2, g.W // 2), dtype=np.uint32))
    return _FRAMES[geom]


def make(geom, rank, name):
    g = GEOMETRIES[geom]
    rng = np.random.default_rng(seed_of(geom, rank, name))
    w2, h2 = g.rays_extent(rank)
    albedo, normals = frame_noise(geom)
    c = Case(g, rank, name, rng.integers(0, 1 << 16, size=(h2, w2, 4), dtype=np.uint16), np.zeros((h2, w2), dtype=np.uint8),
             rng.uniform(-1.0, 1.0, size=(h2, w2, 8)).astype(np.float32), albedo, normals)
    c.data[..., 4:6] = rng.uniform(0.0, 1.0, size=(h2, w2, 2)).astype(np.float32)
    CLASSES[name](c, rng)
    return c


def capacity_vectors(counts):
    """the rooms of the bounded pass, per owner, from the exact counts: fits exactly, one short wherever there is a request, none,
    roomy, and a mix of all of them"""
    mixed = [(c, max(c - 1, 0), 0, c + 100)[(o + 1) % 4] for o, c in enumerate(counts)]
    return {"exact": list(counts), "one_short": [max(c - 1, 0) for c in counts], "none": [0] * len(counts),
            "roomy": [c + 100 for c in counts], "mixed": mixed}
