"""The rules of the hit request / reply exchange, restated in numpy: integers and exact fp32, no tolerance anywhere.

Written from include/vkr_postfx.h ("hit colours and hit normals by request / reply"), DESIGN_MULTIGPU.md and the comments of
csrc/hit_exchange.hip — not from the kernels' code: which footprint rows a ray asks for and from whom (emit), how many per owner
(pass 1), in which slot each request lands (pass 2: block, tile, wave, request k of the ray, lane), what a segment of fixed room
keeps (the first `cap` in that order), what the owner answers (reply) and where the answer goes (scatter), and the room the next
frame's segments get (hit_capacities).  Vectorised over rays: the largest case of tests/hit_exchange_cases.py has 1.1 M of them.

`Rules` switches single rules to a wrong variant (the mutants of tests/test_hit_exchange_cases.py); Rules() is the contract.
"""
from dataclasses import dataclass

import numpy as np

BOTH_ROWS, NORMAL, NO_REQUEST = 0x10000000, 0x20000000, 0xFFFFFFFF
MAX_BLOCKS, TILE_W, TILE_H = 256, 64, 16
# kinds of a request: both rows from one owner; the upper row alone (the lower is held); the lower row alone; the two halves of a
# footprint whose rows belong to two owners
KIND_BOTH, KIND_ROW0, KIND_ROW1, KIND_SPLIT0, KIND_SPLIT1 = 0, 1, 2, 3, 4


@dataclass(frozen=True)
class Rules:
    owner_gt: bool = False          # ownership: boundaries BELOW the row instead of at or below it
    normal_unshifted: bool = False  # the half-res row compared with the full-res boundaries as it is
    x_clamp_w1: bool = False        # the left texel clamped to w - 1 instead of w - 2
    r1_unclamped: bool = False      # the lower row not clamped to the frame
    both_across: bool = False       # BOTH_ROWS also where the rows have two owners
    no_apron: bool = False          # the apron request omitted
    w_eq_zero: bool = False         # a ray counts as a hit where w == 0 instead of w != 0xFFFF
    lane_then_k: bool = False       # slots within a wave by lane, then request k
    keep_last: bool = False         # a bounded segment keeps the last `cap` requests instead of the first


EXACT = Rules()


# ---- footprint ---------------------------------------------------------------------------------------------------------
def unorm16_to_float(v):
    """x = v * 2^-16 (exact), then fma(x, 2^-16 + 2^-32, x) rounded once: product and sum are exact in float64"""
    x = np.asarray(v).astype(np.float64) * 2.0 ** -16
    return (x * (2.0 ** -16 + 2.0 ** -32) + x).astype(np.float32)


def texel_floor(uv, extent):
    """floor(fma(uv, extent, -0.5)) as a float32: a 24-bit times a 14-bit number and the -0.5 are exact in float64 wherever the
    result is not far outside every frame (there one rounding more cannot move it back in)"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = (np.asarray(uv, dtype=np.float32).astype(np.float64) * float(extent) - 0.5).astype(np.float32)
        return np.floor(f)


def float_to_int(f):
    """the kernels' float -> int: saturating (here at +-2^30, far outside every frame), NaN -> 0"""
    f = np.asarray(f, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        g = np.where(np.isnan(f), np.float32(0), np.clip(f, np.float32(-2.0 ** 30), np.float32(2.0 ** 30)))
    return g.astype(np.int64)


def texel_index(uv, extent):
    """x0 / y0 of the bilinear footprint of texture(image, uv) before the clamps (int64)"""
    return float_to_int(texel_floor(uv, extent))


def code_index_table(extent):
    """y0 (or x0) of every UNORM16 uv code on an image of `extent` texels: [65536] int64"""
    return texel_index(unorm16_to_float(np.arange(65536, dtype=np.uint32)), extent)


def owner_of(row, bounds, rules=EXACT):
    """how many strip boundaries (bounds[1 .. world - 1]) lie at or below the full-res row"""
    inner = np.asarray(bounds[1:-1], dtype=np.int64)
    return np.searchsorted(inner, row, side="left" if rules.owner_gt else "right").astype(np.int64)


def _footprint(y0, x0, w, h, lo, hi, tag, shift, bounds, rules):
    """-> (valid [n, 2], code [n, 2], owner [n, 2], kind [n, 2]): the first and the second request of one surface per ray"""
    r0 = np.clip(y0, 0, h - 1)
    r1 = y0 + 1 if rules.r1_unclamped else np.clip(y0 + 1, 0, h - 1)
    x = np.clip(x0, 0, w - 1 if rules.x_clamp_w1 else w - 2)
    want0 = (r0 < lo) | (r0 >= hi)
    want1 = (r1 != r0) & ((r1 < lo) | (r1 >= hi))
    s = 0 if rules.normal_unshifted else shift
    o0, o1 = owner_of(r0 << s, bounds, rules), owner_of(r1 << s, bounds, rules)
    both = want0 & want1 & ((o0 == o1) | rules.both_across)
    base = ((x & 0x3FFF) << 14) | tag
    c0, c1 = (r0 & 0x3FFF) | base, (r1 & 0x3FFF) | base
    two = want0 & want1 & ~both
    first_is_r1 = want1 & ~want0
    valid = np.stack([want0 | want1, two], axis=1)
    code = np.stack([np.where(both, c0 | BOTH_ROWS, np.where(first_is_r1, c1, c0)), c1], axis=1)
    owner = np.stack([np.where(first_is_r1, o1, o0), o1], axis=1)
    kind = np.stack([np.where(both, KIND_BOTH, np.where(two, KIND_SPLIT0, np.where(first_is_r1, KIND_ROW1, KIND_ROW0))),
                     np.full(y0.shape, KIND_SPLIT1)], axis=1)
    return valid, code, owner, kind


@dataclass
class Requests:
    """every request of one window, in the order pass 2 hands out the slots of each owner's segment"""
    world: int
    code: np.ndarray    # [n] uint32
    owner: np.ndarray   # [n]
    kind: np.ndarray    # [n]
    ray: np.ndarray     # [n] index of the ray in the window, row-major; the apron request: rays.size
    k: np.ndarray       # [n] request index of the ray
    block: np.ndarray   # [n] block that writes it
    tile: np.ndarray
    wave: np.ndarray
    per_ray: np.ndarray  # [rays + 1] requests of each ray (last: the apron)
    tiles: int
    blocks: int

    @property
    def counts(self):  # pass 1
        return [int(v) for v in np.bincount(self.owner, minlength=self.world)[: self.world]]

    def of_owner(self, o):
        return self.code[self.owner == o]


def emit(rays, mask, hit_uv, aw, ah, win0, win1, bounds, rules=EXACT):
    """rays: [h2, w2, 4] uint16 (the rank's half-res window); mask: [h2, w2] uint8 or None (no normal requests); hit_uv: [h2, w2, 2]
    float32 (pending data, texel 1, xy); frame aw x ah, the rank holds full-res rows [win0, win1) and half-res rows at half of
    them; strip o owns full-res rows [bounds[o], bounds[o + 1])."""
    h2, w2 = rays.shape[:2]
    n = h2 * w2
    world = len(bounds) - 1
    nw, nh, nrow0, nrow1 = aw // 2, ah // 2, win0 // 2, win1 // 2
    flat = rays.reshape(n, 4)
    # the apron request: one albedo footprint of uv (0, 0), standing in the tile row below the window, tile column 0, thread 0
    u = np.append(unorm16_to_float(flat[:, 0]), np.float32(0))
    v = np.append(unorm16_to_float(flat[:, 1]), np.float32(0))
    hit = np.append((flat[:, 3] == 0) if rules.w_eq_zero else (flat[:, 3] != 0xFFFF), not rules.no_apron)
    va, ca, oa, ka = _footprint(texel_index(v, ah), texel_index(u, aw), aw, ah, win0, win1, 0, 0, bounds, rules)
    va &= hit[:, None]
    if mask is None:
        vn, cn, on, kn = np.zeros_like(va), ca, oa, ka
    else:
        pend = np.append(mask.reshape(n) != 0, False)
        huv = np.concatenate([np.asarray(hit_uv, dtype=np.float32).reshape(n, 2), np.zeros((1, 2), dtype=np.float32)])
        vn, cn, on, kn = _footprint(texel_index(huv[:, 1], nh), texel_index(huv[:, 0], nw), nw, nh, nrow0, nrow1, NORMAL, 1, bounds, rules)
        vn &= pend[:, None]
    valid = np.concatenate([va, vn], axis=1)              # [n + 1, 4]: albedo first, second; normal first, second
    k_of = np.cumsum(valid, axis=1) - 1                   # the ray's request index of each
    ray, col = np.nonzero(valid)
    code = np.concatenate([ca, cn], axis=1)[ray, col].astype(np.uint32)
    owner = np.concatenate([oa, on], axis=1)[ray, col]
    kind = np.concatenate([ka, kn], axis=1)[ray, col]
    k = k_of[ray, col]
    # the walk: tiles of 64 x 16 ray texels plus one apron row of tiles; block b of G takes tiles b, b + G, ...
    tiles_x, tiles_y = -(-w2 // TILE_W), -(-h2 // TILE_H) + 1
    tiles = tiles_x * tiles_y
    blocks = min(tiles, MAX_BLOCKS)
    ly, lx = ray // w2, ray % w2
    apron = ray == n
    tile = np.where(apron, tiles_x * (tiles_y - 1), (ly // TILE_H) * tiles_x + lx // TILE_W)
    wave = np.where(apron, 0, ly % TILE_H)
    lane = np.where(apron, 0, lx % TILE_W)
    block = tile % blocks
    within = (k, lane) if rules.lane_then_k else (lane, k)  # (np.lexsort: the LAST key is the primary one)
    order = np.lexsort(within + (wave, tile // blocks, block, owner))
    pick = lambda a: a[order]
    return Requests(world, pick(code), pick(owner), pick(kind), pick(ray), pick(k), pick(block), pick(tile), pick(wave),
                    valid.sum(axis=1), tiles, blocks)


# ---- pass 2 ------------------------------------------------------------------------------------------------------------
def layout(req):
    """-> (segments [world + 1], buffer): owner o's requests at [segments[o], segments[o + 1]) in slot order"""
    seg = np.concatenate([[0], np.cumsum(req.counts)]).astype(np.int64)
    return [int(s) for s in seg], req.code.copy()  # (emit sorted by owner first)


def layout_bounded(req, caps, rules=EXACT):
    """segments of fixed room: -> (segments, buffer, dropped).  Slot i of owner o is written iff i < caps[o]; the rest of the
    segment stays NO_REQUEST; dropped = 1 iff some owner's count exceeds its room."""
    seg = [0]
    for c in caps:
        seg.append(seg[-1] + int(c))
    buf = np.full(seg[-1], NO_REQUEST, dtype=np.uint32)
    dropped = 0
    for o, cap in enumerate(caps):
        mine = req.of_owner(o)
        if mine.size > cap:
            dropped = 1
            mine = mine[mine.size - cap:] if rules.keep_last else mine[:cap]
        buf[seg[o]: seg[o] + mine.size] = mine
    return seg, buf, dropped


# ---- reply / scatter ---------------------------------------------------------------------------------------------------
def reply(requests, albedo, albedo_row0, normals, normals_row0):
    """albedo / normals: the owner's window as uint32 texels [rows, width] whose first row is frame row *_row0 (normals may be
    None: no normal request can be answered) -> (replies [n, 4] uint32, errors)"""
    r = np.asarray(requests, dtype=np.uint32).astype(np.int64)
    out = np.zeros((r.size, 4), dtype=np.uint32)
    live = r != NO_REQUEST
    nrm, both = (r & NORMAL) != 0, (r & BOTH_ROWS) != 0
    row, x = r & 0x3FFF, (r >> 14) & 0x3FFF
    errors = 0
    for surface, img, row0 in ((False, albedo, albedo_row0), (True, normals, normals_row0)):
        sel = live & (nrm == surface)
        if img is None:
            errors += int(sel.sum())
            continue
        ly = row - row0
        ok = sel & (ly >= 0) & (ly + both < img.shape[0]) & (x + 1 < img.shape[1])
        errors += int((sel & ~ok).sum())
        i = np.nonzero(ok)[0]
        ly0, ly1, xi = ly[i], ly[i] + both[i], x[i]
        out[i, 0], out[i, 1], out[i, 2], out[i, 3] = img[ly0, xi], img[ly0, xi + 1], img[ly1, xi], img[ly1, xi + 1]
    return out, errors


def scatter(requests, replies, frame_albedo, frame_normals):
    """writes the replies into the whole-frame images (uint32 texels [rows, width], changed in place) at their frame positions"""
    r = np.asarray(requests, dtype=np.uint32).astype(np.int64)
    replies = np.asarray(replies, dtype=np.uint32).reshape(-1, 4)
    for i in np.nonzero(r != NO_REQUEST)[0]:  # in order: a later request for the same texel overwrites an earlier one
        img = frame_normals if r[i] & NORMAL else frame_albedo
        row, x = r[i] & 0x3FFF, (r[i] >> 14) & 0x3FFF
        img[row, x: x + 2] = replies[i, 0:2]
        if r[i] & BOTH_ROWS:
            img[row + 1, x: x + 2] = replies[i, 2:4]


def scatter_unordered(requests, replies, frame_albedo, frame_normals):
    """the same for lists in which every texel is only ever given one value (replies of the texels' owners): vectorised"""
    r = np.asarray(requests, dtype=np.uint32).astype(np.int64)
    replies = np.asarray(replies, dtype=np.uint32).reshape(-1, 4)
    live = r != NO_REQUEST
    row, x = r & 0x3FFF, (r >> 14) & 0x3FFF
    for surface, img in ((0, frame_albedo), (NORMAL, frame_normals)):
        sel = live & ((r & NORMAL) == surface)
        img[row[sel], x[sel]], img[row[sel], x[sel] + 1] = replies[sel, 0], replies[sel, 1]
        sel &= (r & BOTH_ROWS) != 0
        img[row[sel] + 1, x[sel]], img[row[sel] + 1, x[sel] + 1] = replies[sel, 2], replies[sel, 3]


# ---- the room of the next frame's segments -------------------------------------------------------------------------------
def hit_capacities(counts, world, percent=125):
    """host/frame.cpp: count * percent / 100, rounded up to a step of 64, plus 64; adjacent strips always keep a segment, a distant
    pair that asked for nothing keeps none, a rank asks itself for nothing.  counts: world x world, row = asking rank."""
    caps = []
    for r in range(world):
        for o in range(world):
            c = int(counts[r * world + o])
            adjacent = abs(r - o) == 1
            if r == o or (c == 0 and not adjacent):
                caps.append(0)
            else:
                caps.append(((c * percent // 100 + 63) // 64 * 64 + 64) & 0xFFFFFFFF)
    return caps
