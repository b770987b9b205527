"""Constructed geometry for the three compute rasterisers (gbuf_opaque_taa, default_shadow, cubemap_probe): named classes in the
style of gbuffer_content.py and degenerate_extents.py.  Each class is a function of the target extent returning a Case: the
triangles in submission order, how they are grouped into draws, and a dict `contains` of what the class is meant to hold, which
tests/test_raster_geometry.py checks against the exact reference (raster_rules_reference.py) on the CPU, so that the GPU tests
cannot go vacuous.

Geometry is given in pixels (a 1/256 grid survives the trip to clip space and back exactly; every class asserts that through the
reference's snap) or directly in clip space.  A draw's matrix is the identity with the last row (0, 0, k, c): clip w = k z + c,
exact for the dyadic z used where k != 0.  For the cube bake the same triangles are placed in world space on face -Z of a probe at
the origin (place_on_cube), and the reference is fed the clip positions that the vertex stage of cubemap_reference computes.
"""
import numpy as np

from vk_renderer_amd import scene as scn

import raster_rules_reference as rr

F32 = np.float32
BIG_PX = float(2 ** 20 - 4096)  # far outside, inside the guard band, differences of two of them at most 2^29 / 256
PALETTE_W = 16  # the palette texture: 16 x 16 texels of distinct opaque colours, triangle i samples texel i mod 256 at its centre


class Case:
    def __init__(self, name, width, height):
        self.name, self.width, self.height = name, width, height
        self.pos = []        # per triangle float32 [3, 3]: what goes into the vertex buffer
        self.draw_of = []    # per triangle: index into self.draws
        self.draws = []      # per draw: dict(k, c, textured)
        self.contains = {}
        self.zmax = 1.0      # largest |z / w| of a corner: scales the depth bound

    def draw(self, k=0.0, c=1.0, textured=True):
        self.draws.append(dict(k=float(k), c=float(c), textured=textured))
        return len(self.draws) - 1

    def tri(self, p, draw=None):
        if draw is None:
            draw = len(self.draws) - 1 if self.draws else self.draw()
        self.pos.append(np.asarray(p, F32).reshape(3, 3))
        self.draw_of.append(draw)
        return len(self.pos) - 1

    def px(self, pts, z):
        """three (x, y) in pixels and one z or three -> clip-space corners through an identity matrix"""
        pts = np.asarray(pts, np.float64).reshape(3, 2)
        out = np.empty((3, 3), np.float64)
        out[:, 0] = pts[:, 0] * 2.0 / self.width - 1.0
        out[:, 1] = pts[:, 1] * 2.0 / self.height - 1.0
        out[:, 2] = z
        return out.astype(F32)

    # ---- what the programs and the reference are given ----
    def clip(self):
        """float32 [T, 3, 4]: the vertex stage of an identity view-projection and the draw's matrix"""
        if getattr(self, "world_clip", None) is not None:
            return self.world_clip  # a case given in world space round the probe: what cubemap_reference's vertex stage computes
        pos = np.asarray(self.pos, F32).reshape(-1, 3, 3)
        k = np.array([self.draws[d]["k"] for d in self.draw_of], F32)[:, None]
        c = np.array([self.draws[d]["c"] for d in self.draw_of], F32)[:, None]
        with np.errstate(all="ignore"):
            w = (k * pos[..., 2] + c).astype(F32)
            w64 = k.astype(np.float64) * pos[..., 2].astype(np.float64) + c.astype(np.float64)
            # NaN and infinities spread through the zero entries of a matrix row: 0 * inf is NaN
            poison = ~np.isfinite(pos).all(axis=-1)
        assert np.all((w64 == w) | poison), "clip w is not exact: the result would depend on the numeric contract"
        out = np.concatenate([pos, w[..., None]], axis=-1)
        out[poison] = np.nan
        return out.astype(F32)

    def model(self, d):
        m = np.eye(4, dtype=F32)
        m[3, 2], m[3, 3] = self.draws[d]["k"], self.draws[d]["c"]
        m[0, 3] = self.draws[d].get("tx", 0.0)  # a translation that a layer's matrix takes back (the four-layer shadow test)
        return m

    def scene(self, textured=None):
        """scene.Scene: three vertices of its own per triangle (normal and uv constant over the triangle), one draw per group"""
        sc = scn.Scene()
        tex = sc.add_texture(palette())
        T = len(self.pos)
        runs = []  # a draw call per run of consecutive triangles of one draw: submission order is the order of the list
        for i in range(T):
            if runs and runs[-1][0] == self.draw_of[i]:
                runs[-1][1].append(i)
            else:
                runs.append((self.draw_of[i], [i]))
        for d, ids in runs:
            info = self.draws[d]
            pos = np.asarray([self.pos[i] for i in ids], F32).reshape(-1, 3)
            nrm = np.repeat(np.asarray([tri_normal(i) for i in ids], F32).reshape(-1, 3), 3, axis=0)
            uv = np.repeat(np.asarray([tri_uv(i) for i in ids], F32).reshape(-1, 2), 3, axis=0)
            mesh = sc.add_mesh(pos, nrm, uv, np.arange(3 * len(ids), dtype=np.uint32))
            t = sc.add_transform(self.model(d))
            use_tex = info["textured"] if textured is None else textured
            sc.add_draw(t, mesh, tex if use_tex else scn.INVALID)
        return sc

    def reference(self):
        """the exact reference's result on the near-clipped triangles"""
        tris, owners = clip_near_all(self.clip())
        r = rr.rasterise(tris, self.width, self.height, owner_ids=owners)
        r.kept_submission = np.bincount(owners[r.kept], minlength=len(self.pos)) > 0  # some part of the submitted triangle is set up
        return r


def palette():
    i = np.arange(PALETTE_W * PALETTE_W)
    tex = np.empty((PALETTE_W, PALETTE_W, 4), np.uint8)
    tex[..., 0] = ((i * 37) % 256).reshape(PALETTE_W, PALETTE_W)
    tex[..., 1] = i.reshape(PALETTE_W, PALETTE_W)
    tex[..., 2] = ((i * 101 + 50) % 256).reshape(PALETTE_W, PALETTE_W)
    tex[..., 3] = 255
    return tex


def tri_uv(i):
    i = i % (PALETTE_W * PALETTE_W)
    return ((i % PALETTE_W + 0.5) / PALETTE_W, (i // PALETTE_W + 0.5) / PALETTE_W)


def tri_color(i):
    """the sRGB codes triangle i shows: its texel of the palette (a constant uv has no footprint: level 0, at a texel centre)"""
    i = np.asarray(i) % (PALETTE_W * PALETTE_W)
    return palette().reshape(-1, 4)[i]


def tri_normal(i):
    """a unit normal per triangle, 1024 distinct directions on the upper hemisphere"""
    i = i % 1024
    a, b = (i % 32 + 0.5) / 32.0 * 2.0 * np.pi, (i // 32 + 0.5) / 32.0 * 0.45 * np.pi
    return (np.cos(a) * np.sin(b), np.sin(a) * np.sin(b), np.cos(b))


# ---- the near clip: plain Sutherland-Hodgman in fp32, the crossing from the inside vertex ----
def clip_near(tri):
    """tri float32 [3, 4] -> list of 0, 3 or 4 clip positions float32 [4]"""
    poly = []
    with np.errstate(all="ignore"):
        for k in range(3):
            p, q = tri[k], tri[(k + 1) % 3]
            pin, qin = bool(p[2] >= 0), bool(q[2] >= 0)
            if pin:
                poly.append(p)
            if pin != qin:
                s, e = (p, q) if pin else (q, p)
                t = F32(s[2] / F32(s[2] - e[2]))
                poly.append((s + (t * (e - s)).astype(F32)).astype(F32))
    return poly


def clip_near_all(clip):
    tris, owners = [], []
    for i, tri in enumerate(np.asarray(clip, F32).reshape(-1, 3, 4)):
        poly = clip_near(tri)
        for sub in range(len(poly) - 2):
            tris.append([poly[0], poly[1 + sub], poly[2 + sub]])
            owners.append(i)
    return np.asarray(tris, F32).reshape(-1, 3, 4), np.asarray(owners, np.int64)


def inside_mask(tri):
    z = np.asarray(tri)[:, 2]
    return sum((1 << k) for k in range(3) if z[k] >= 0)


def centre_blocks(case, i):
    """8 x 8 blocks touched by the pixel centres inside the extent of triangle i's snapped corners, clipped to the viewport"""
    X, Y, _, kept = rr.snap(case.clip()[i:i + 1], case.width, case.height)
    if not kept[0]:
        return 0
    cx = [c for c in range(case.width) if X.min() <= c * 256 + 128 <= X.max()]
    cy = [c for c in range(case.height) if Y.min() <= c * 256 + 128 <= Y.max()]
    if not cx or not cy:
        return 0
    return (cx[-1] // 8 - cx[0] // 8 + 1) * (cy[-1] // 8 - cy[0] // 8 + 1)


def _assert_pixel_exact(case, ids=None):
    """every corner given in pixels on the 1/256 grid snaps to exactly that"""
    clip = case.clip()
    X, Y, _, kept = rr.snap(clip, case.width, case.height)
    ids = range(len(clip)) if ids is None else ids
    for i in ids:
        if not kept[i]:
            continue
        want_x = (clip[i, :, 0].astype(np.float64) / clip[i, :, 3] + 1.0) * 0.5 * case.width * 256.0
        want_y = (clip[i, :, 1].astype(np.float64) / clip[i, :, 3] + 1.0) * 0.5 * case.height * 256.0
        assert np.abs(X[i] - want_x).max() < 0.26 and np.abs(Y[i] - want_y).max() < 0.26, (case.name, i)


def _zgrid(n, rng, lo=0.125, step=2.0 ** -12):
    """n distinct flat depths on a 2^-12 grid, in shuffled order"""
    z = lo + step * np.arange(n)
    assert z.max() < 0.95
    rng.shuffle(z)
    return z


# ---- the classes ----
def centre_lattice(width, height):
    """Two closed meshes: one with every vertex on a pixel centre, one with every vertex on a pixel corner.  Columns 4, 2, 3 px
    wide and rows 2, 4, 3 px high, every cell cut by a diagonal (alternating): horizontal and vertical edges, 45 degrees (3 x 3),
    2:1 (4 x 2) and 1:2 (2 x 4), plus the slopes of the other cells; both windings, shuffled submission order, a flat z of its own
    per triangle."""
    case = Case("centre_lattice", width, height)
    rng = np.random.default_rng(11)
    tris = []
    half = (width - 16) // 2
    regions = []
    for origin, x_start in ((0.5, 8), (0.0, 8 + half)):
        xs, ys = [x_start + origin], [8 + origin]
        cw, ch = [4, 2, 3], [2, 4, 3]
        while xs[-1] + cw[(len(xs) - 1) % 3] <= x_start + half - 2:
            xs.append(xs[-1] + cw[(len(xs) - 1) % 3])
        while ys[-1] + ch[(len(ys) - 1) % 3] <= min(height - 8, 8 + 54):
            ys.append(ys[-1] + ch[(len(ys) - 1) % 3])
        regions.append((xs[0], ys[0], xs[-1], ys[-1]))
        for i in range(len(xs) - 1):
            for j in range(len(ys) - 1):
                a, b, c, d = (xs[i], ys[j]), (xs[i + 1], ys[j]), (xs[i + 1], ys[j + 1]), (xs[i], ys[j + 1])
                pair = [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
                for t in pair:
                    tris.append(t if rng.random() < 0.5 else (t[0], t[2], t[1]))
    order = rng.permutation(len(tris))
    z = _zgrid(len(tris), rng, lo=0.0625)
    case.draw()
    for n, i in enumerate(order):
        case.tri(case.px(tris[i], z[n]))
    _assert_pixel_exact(case)
    case.regions = regions
    case.contains = {"min_on_edge_centres": 300, "every_edge_kind": True, "single_cover_regions": regions}
    return case


def exact_ties(width, height, coplanar=True, on_cube=False):
    """One triangle six times inside one draw and one five times across five draws (both windings alternating), and two pairs of
    different coplanar triangles, submitted in either order, whose depths tie exactly where they overlap: vertices on pixel
    centres, legs of 16 and 32 px (area2 a power of two) and z on a 2^-6 grid, so every fp32 step of the depth is exact and a
    tie of the rational depths is a tie of the D24 codes."""
    case = Case("exact_ties", width, height)
    d = case.draw()
    a = [(8.5, 8.5), (40.5, 10.5), (12.5, 30.5)]
    for n in range(6):
        case.tri(case.px(a if n % 2 == 0 else [a[0], a[2], a[1]], 0.5), d)
    b = [(48.5, 6.5), (60.5, 30.5), (44.5, 28.5)]
    for n in range(5):
        case.tri(case.px(b, [0.25, 0.5, 0.75])[[0, 1, 2] if n % 2 == 0 else [0, 2, 1]], case.draw())

    d = case.draw()
    pairs = []
    for ox, first_small in ((8.5, True), (52.5, False)) if coplanar else ():
        def pl(p):  # the plane z = 1/4 + (x - ox) / 128 + (y - 40.5) / 64: on the 2^-7 grid at pixel centres
            return [0.25 + (x - ox) / 128.0 + (y - 40.5) / 64.0 for x, y in p]
        small = [(ox + 4, 44.5), (ox + 20, 44.5), (ox + 4, 60.5)]
        large = [(ox, 40.5), (ox + 32, 40.5), (ox, 72.5)]
        seq = (small, large) if first_small else (large, small)
        # on the cube a plane of NDC is none; there both lie in the plane of one distance whose z / w is exactly 0.5
        ids = [case.tri(case.px(p, 0.40625 if on_cube else pl(p)), d) for p in seq]
        pairs.append(ids)
        if on_cube:
            case.cube_distance = getattr(case, "cube_distance", {})
            case.cube_distance.update({i: tie_distance() for i in ids})
    assert height >= 74 and width >= 86
    _assert_pixel_exact(case)
    case.contains = {"same_in_draw": list(range(0, 6)), "same_across_draws": list(range(6, 11)), "coplanar_pairs": pairs,
                     "min_tied_centres_per_pair": 100}
    return case


def block_split(width, height):
    """Bounding boxes of exactly 1, 64 (the aligned 64 x 64 px box), 72 (that box moved by one pixel), 65 (13 x 5 blocks: a last
    chunk of one block) blocks, and nine pixels wide inside one block row; the extent is no multiple of 8."""
    assert width % 8 and height % 8 and width >= 136 and height >= 110
    case = Case("block_split", width, height)
    case.draw()
    z = 0.5 - 2.0 ** -10 * np.arange(10)  # the later the nearer: every triangle shows
    want = []
    def add(pts, blocks, zi):
        i = case.tri(case.px(pts, z[zi]))
        want.append((i, blocks))
    add([(9, 9), (15, 10), (10, 15)], 1, 0)
    add([(64, 32), (128, 32), (64, 96)], 64, 1)
    add([(128, 96), (64, 96), (128, 32)], 64, 2)          # the other half of the box, other winding
    add([(65, 32), (129, 32), (65, 96)], 72, 3)
    add([(0, 48), (104, 48), (0, 88)], 65, 4)
    add([(104, 88), (0, 88), (104, 48)], 65, 5)
    add([(20, 8.25), (29, 8.25), (24, 15.75)], 2, 6)      # nine pixels wide, one block row
    add([(64, 33), (128, 33), (64, 97)], 72, 7)           # moved down instead
    _assert_pixel_exact(case)
    for i, blocks in want:
        assert centre_blocks(case, i) == blocks, (i, centre_blocks(case, i), blocks)
    case.contains = {"blocks": sorted(set(b for _, b in want))}
    return case


def offscreen_reach(width, height):
    """Triangles that cover part of the viewport from vertices far outside on one, two and all four sides (up to +-(2^20 - 4096)
    px), triangles wholly outside on every side and at every corner (some with a bounding box that overlaps the viewport), and one
    that surrounds the viewport."""
    case = Case("offscreen_reach", width, height)
    case.draw()
    z = np.concatenate([0.25 + 2.0 ** -10 * np.arange(7), [0.9 + 2.0 ** -12, 0.9], 0.125 + 2.0 ** -10 * np.arange(15)])
    B, W, H = BIG_PX, float(width), float(height)
    inside = [
        [(-B, H / 2), (W * 0.6, H * 0.2), (W * 0.6, H * 0.8)],                # left
        [(W + B, H / 3), (W * 0.3, H * 0.1), (W * 0.3, H * 0.7)],             # right
        [(W / 2, -B), (W * 0.2, H * 0.5), (W * 0.8, H * 0.6)],                # top
        [(W / 3, H + B), (W * 0.1, H * 0.4), (W * 0.7, H * 0.3)],             # bottom
        [(-B, -B), (W * 0.9, H * 0.3), (W * 0.4, H * 0.9)],                   # two sides
        [(W + B, H + B), (W * 0.1, H * 0.6), (W * 0.5, H * 0.1)],
        [(-B, H * 0.4), (W + B, H * 0.5), (W * 0.5, H * 0.9)],                # left and right
        [(-B, -B), (W + B, -B / 2), (W / 2, H + B)],                          # all four sides: surrounds the viewport
        [(-B, -B), (W / 2, H + B), (W + B, -B / 2)],                          # the same, other winding
    ]
    outside = []
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            if sx or sy:
                cx, cy = W / 2 + sx * (W / 2 + 30), H / 2 + sy * (H / 2 + 30)
                outside.append([(cx - 20, cy - 10), (cx + 20, cy - 5), (cx, cy + 15)])
    # bounding boxes that overlap the viewport's corners although the triangle stays outside
    outside += [[(-30, 20), (20, -30), (-30, -30)], [(W + 30, H - 20), (W - 20, H + 30), (W + 30, H + 30)]]
    for n, pts in enumerate(inside + outside):
        case.tri(case.px(pts, z[n]))
    case.contains = {"covering": list(range(len(inside))), "outside": list(range(len(inside), len(inside) + len(outside))),
                     "surrounding": [7, 8]}
    return case


def _guard_ndc(extent, sign):
    """(the float32 NDC coordinate whose screen coordinate is exactly sign * 2^20, the next float32 beyond it whose screen
    coordinate exceeds the guard band) for a power-of-two extent"""
    assert extent & (extent - 1) == 0
    def xs(v):
        return (F32(v) * F32(0.5) + F32(0.5)) * F32(extent)
    on = F32(sign * (2.0 ** 21) / extent - 1.0)
    assert abs(xs(on)) == rr.GUARD_PX
    v = on
    for _ in range(8):
        v = np.nextafter(v, F32(sign * np.inf))
        if abs(xs(v)) > rr.GUARD_PX:
            return on, v
    raise AssertionError("no float32 just beyond the guard band")


def guard_band(width, height):
    """Power-of-two extents, so that a screen coordinate of exactly +-2^20 exists.  Kept triangles have one vertex on the guard
    band; the dropped ones (nearer, so they would show) have it on the next float32 beyond, or w = 0, w < 0, w = 2^-25, or one
    coordinate of one vertex NaN, +Inf or -Inf between two ordinary neighbours in the same draw."""
    case = Case("guard_band", width, height)
    d = case.draw()
    kept, dropped = [], []
    for axis in (0, 1):
        extent = (width, height)[axis]
        for sign in (1, -1):
            on, beyond = _guard_ndc(extent, sign)
            for far, z, into in ((on, 0.5, kept), (beyond, 0.25, dropped)):
                # a wedge from the far vertex on the axis to +-0.4 on the other axis through the middle of the viewport
                tri = np.array([[0.0, 0.0, z], [0.0, -0.4, z], [0.0, 0.4, z]], np.float64)
                if axis == 1:
                    tri = tri[:, [1, 0, 2]]
                t = tri.astype(F32)
                t[0, axis] = far
                into.append(case.tri(t, d))
    # w = k z + c with k = -1, c = 1/2: 0 at z = 1/2, negative beyond, 2^-25 just before
    dw = case.draw(k=-1.0, c=0.5)
    for z in (0.5, 0.75, float(F32(0.5) - F32(2.0 ** -25))):
        dropped.append(case.tri(np.array([[0.0, -0.5, z], [-0.5, 0.5, z], [0.5, 0.5, z]], F32), dw))
    # a tiny w with an ordinary x: the screen coordinate is far beyond the guard band
    dropped.append(case.tri(np.array([[0.25, 0.0, 0.49999997], [0.0, 0.25, 0.49999997], [-0.25, 0.0, 0.49999997]], F32), dw))
    dn = case.draw()
    neighbours = []
    n = 0
    for comp in (0, 1, 2):
        for bad in (np.nan, np.inf, -np.inf):
            x0 = -0.9 + 0.2 * n
            good = np.array([[x0, -0.9, 0.375], [x0 + 0.15, -0.9, 0.375], [x0, -0.6, 0.375]], F32)
            neighbours.append(case.tri(good, dn))
            t = np.array([[x0, -0.9, 0.125], [x0 + 0.15, -0.9, 0.125], [x0, -0.6, 0.125]], F32)
            t[n % 3, comp] = bad
            dropped.append(case.tri(t, dn))
            n += 1
    neighbours.append(case.tri(np.array([[0.9, -0.9, 0.375], [0.95, -0.9, 0.375], [0.9, -0.6, 0.375]], F32), dn))
    case.contains = {"kept": kept, "dropped": dropped, "neighbours": neighbours}
    return case


SLIVER_TEMPLATES = [  # corners inside a 2 x 2 px cell; a bounding box with centres in it, none of them covered
    [(0.1, 0.2), (1.9, 1.6), (1.9, 1.7)],
    [(1.9, 0.2), (0.1, 1.6), (0.1, 1.7)],
    [(0.2, 0.1), (1.6, 1.9), (1.7, 1.9)],
    [(0.2, 1.9), (1.6, 0.1), (1.7, 0.1)],
]


def slivers(width, height, count, needles=0):
    """`count` diagonal slivers thinner than a pixel whose bounding box holds pixel centres but which cover none, tiled over 2 x 2
    px cells around (and over) one ordinary triangle, all nearer than it; a few slivers that cover exactly one centre; three
    vertices inside one 1/256 cell; collinear after the snap; two coincident vertices.  needles: that many more small triangles,
    one inside each of the first pixels in raster order, each covering exactly its pixel's centre and nothing else.  Which records
    end up last in a rasteriser's small list is not determined; with more needles than the list loop's first turn has waves, and
    fewer invisible records than the last turn has records, the last turn draws pixels that nothing else draws."""
    case = Case("slivers", width, height)
    case.draw()
    ordinary = case.tri(case.px([(4, 4), (width - 4, 6), (6, height - 4)], 0.75))
    cells_x, cells_y = (width - 2) // 2, (height - 2) // 2
    listed = 0
    n = 0
    while listed < count:
        cx, cy = n % cells_x, (n // cells_x) % cells_y
        tpl = SLIVER_TEMPLATES[(n + n // (cells_x * cells_y)) % 4]
        z = 0.125 + (n % 256) * 2.0 ** -12
        case.tri(case.px([(1 + 2 * cx + x, 1 + 2 * cy + y) for x, y in tpl], z))
        listed += 1
        n += 1
    first_other = len(case.pos)
    needle_ids = []
    for n in range(needles):
        cx, cy = n % width + 0.5, n // width + 0.5
        needle_ids.append(case.tri(case.px([(cx - 0.4, cy - 0.3), (cx + 0.45, cy), (cx - 0.4, cy + 0.3)], 0.0625)))
    assert needles <= width * height
    one = []
    for k in range(4):  # thinner than a pixel, exactly one centre: a needle round the centre of pixel (9 + 4k, 3)
        c = (9.5 + 4 * k, 3.5)
        one.append(case.tri(case.px([(c[0] - 0.4, c[1] - 0.2), (c[0] + 1.3, c[1] + 0.1), (c[0] - 0.4, c[1] + 0.2)], 0.03125)))
    nothing = []
    e = 1.0 / 1024.0
    nothing.append(case.tri(case.px([(20.5 + e, 9.5 + e), (20.5 + 2 * e, 9.5 + e), (20.5 + e, 9.5 + 2 * e)], 0.0625)))  # one cell
    nothing.append(case.tri(case.px([(10, 10), (20, 20), (30, 30)], 0.0625)))                                          # collinear
    nothing.append(case.tri(case.px([(10, 10), (20.001, 20.001), (30, 30)], 0.0625)))                                  # ... after the snap
    nothing.append(case.tri(case.px([(12, 14), (12, 14), (30, 20)], 0.0625)))                                          # coincident
    case.contains = {"ordinary": ordinary, "slivers": list(range(1, first_other)), "one_centre": one, "nothing": nothing,
                     "listed_slivers": count, "needles": needle_ids}
    return case


def large_flood(width, height, count=130):
    """`count` triangles whose bounding box is the whole viewport, at distinct flat depths 2^-12 apart, submitted in ascending,
    descending and shuffled order of depth, with a small nearer triangle after every one of them (so list order and submission
    order differ).  They are nested: all share the corner (-1, -1) of NDC, and the nearer a triangle the shorter its legs, from
    1.6 times the viewport down to just over once (the nearest covers the half before the diagonal).  So EVERY one of them owns a band along its hypotenuse that crosses the block rows of the whole viewport: whichever
    records end up last in a rasteriser's large list, the chunks of the last turn of its loop draw pixels that nothing else
    draws.  (Full-viewport triangles of which the nearest owns every pixel would hide that turn: the image would not depend on
    it.)"""
    case = Case("large_flood", width, height)
    rng = np.random.default_rng(3)
    third = count // 3
    rank = np.arange(count)
    order = np.concatenate([rank[third:2 * third], rank[2 * third:][::-1], rng.permutation(rank[:third])])  # ascending, descending, shuffled
    assert len(order) == count
    case.draw()
    large = []
    for n, r in enumerate(order):
        if n == count // 2:
            case.draw()
        leg = 4.0 * (0.52 + 0.28 * (r + 1) / count)  # in NDC: 2 is the viewport
        z = 0.25 + 2.0 ** -12 * r
        t = np.array([[-1, -1, z], [-1 + leg, -1, z], [-1, -1 + leg, z]], np.float64)
        large.append(case.tri((t if n % 2 == 0 else t[[0, 2, 1]]).astype(F32)))
        x, y = 4 + (n * 7) % (width - 16), 4 + (n * 5) % (height - 16)
        case.tri(case.px([(x, y), (x + 7.5, y + 1), (x + 2, y + 8.25)], 0.125 + 2.0 ** -12 * n))
    blocks = ((width + 7) // 8) * ((height + 7) // 8)
    for i in (large[0], large[-1], large[int(np.argmin(order))]):
        assert centre_blocks(case, i) == blocks, "the bounding box of every nested triangle is the whole viewport"
    case.contains = {"large": large, "min_owned_per_large": 60, "chunks": count * ((blocks + 15) // 16)}
    return case


def near_plane(width, height):
    """All eight inside masks of the near clip in both windings, with w = 1 and with w = 1 + z / 2; corners exactly on z = +0.0 and
    z = -0.0, two corners on the plane; pairs of triangles sharing an edge that crosses the plane at several slopes."""
    case = Case("near_plane", width, height)
    d1, d2 = case.draw(), case.draw(k=0.5, c=1.0)
    cell = 24.0
    per_row = int((width - 8) // cell)
    slot = [0]

    def place(zs, winding, draw, shape=((2, 2), (21, 5), (7, 20)), at=None, scale=1.0):
        if at is None:
            cx, cy = 4 + cell * (slot[0] % per_row), 4 + cell * (slot[0] // per_row)
            slot[0] += 1
        else:
            cx, cy = at
        pts = [(cx + scale * x, cy + scale * y) for x, y in shape]
        p = case.px(pts, zs).astype(np.float64)
        w = case.draws[draw]["k"] * p[:, 2] + case.draws[draw]["c"]
        p[:, 0] *= w
        p[:, 1] *= w  # so that x / w lands where it was meant; not exact for w != 1 and need not be
        if winding:
            p = p[[0, 2, 1]]
        return case.tri(p.astype(F32), draw)

    masks = {}
    for draw in (d1, d2):
        for mask in range(8):
            for winding in (0, 1):
                zs = [(0.25 + 0.0625 * k) if mask >> k & 1 else -(0.125 + 0.0625 * k) for k in range(3)]
                i = place(zs, winding, draw)
                masks[(draw, inside_mask(case.pos[i]), winding)] = i
    on_plane = [place([0.0, 0.5, 0.25], 0, d1), place([-0.0, 0.5, 0.25], 1, d1), place([0.0, -0.0, 0.5], 0, d1),
                place([0.0, -0.5, -0.25], 0, d1), place([-0.0, -0.5, 0.25], 1, d2), place([0.0, 0.0, -0.5], 0, d2)]
    pairs = []
    pairs_y = 4 + cell * ((slot[0] + per_row - 1) // per_row) + 4
    for n, (za, zb) in enumerate([(0.5, -0.5), (0.25, -0.75), (0.75, -0.125), (-0.5, 0.5), (0.375, -0.0625), (-0.25, 0.625)]):
        draw = (d1, d2)[n % 2]
        # the shared edge runs from corner a (z = za) to corner b (z = zb) and crosses the plane; both triangles get the very
        # same floats for it (the same expression on the same inputs), the outer corners lie in front of the plane
        # Large enough (70 px) that the one-pixel band along the outline and the cut is a small share of the union.
        a, b = (3, 2 + 3 * (n % 3)), (21, 20 - 2 * (n % 4))
        at = (4 + 82.0 * (n % 3), pairs_y + 80.0 * (n // 3))
        i = place([za, zb, 0.5], 0, draw, shape=(a, b, (4, 21)), at=at, scale=3.4)
        j = place([zb, za, 0.25], n % 2, draw, shape=(b, a, (20, 2)), at=at, scale=3.4)
        pairs.append((i, j))
    assert height >= pairs_y + 160 and width >= 4 + 3 * 82
    case.contains = {"masks": masks, "on_plane": on_plane, "pairs": pairs, "max_band_share": 0.10}
    return case


def depth_range(width, height):
    """z exactly 0 and exactly 1 over whole triangles, a triangle whose z runs from 0.5 to 1.5 (the per-fragment far clip cuts it
    along a line), and a corner at z = -0.0."""
    case = Case("depth_range", width, height)
    case.draw()
    w, h = float(width), float(height)
    ids = {
        "z0": case.tri(case.px([(2, 2), (w * 0.45, 3), (3, h * 0.45)], 0.0)),
        "z1": case.tri(case.px([(w * 0.5, 2), (w - 2, 3), (w * 0.55, h * 0.45)], 1.0)),
        "far_cut": case.tri(case.px([(2, h * 0.5), (w * 0.45, h * 0.55), (3, h - 2)], [0.5, 1.5, 1.0])),
        "minus_zero": case.tri(case.px([(w * 0.5, h * 0.5), (w - 2, h * 0.55), (w * 0.55, h - 2)], [-0.0, 0.5, 0.25])),
        "z1_other_winding": case.tri(case.px([(w * 0.5, 2), (w * 0.55, h * 0.45), (w * 0.3, h * 0.3)], 1.0)),
    }
    case.zmax = 1.5
    case.contains = ids
    return case


def tiny_targets(width, height):
    """a full-target triangle and a few small ones, for targets down to 1 x 1"""
    case = Case("tiny_targets", width, height)
    case.draw()
    case.tri(np.array([[-1, -1, 0.75], [3, -1, 0.75], [-1, 3, 0.75]], F32))
    w, h = float(width), float(height)
    case.tri(case.px([(0, 0), (w * 0.75, 0), (0, h * 0.75)], 0.5))
    case.tri(case.px([(w, h), (w * 0.5, h), (w, h * 0.25)], 0.25))
    case.tri(case.px([(w * 0.25, h * 0.25), (w * 0.25 + 1, h * 0.25), (w * 0.25, h * 0.25 + 1)], 0.125))
    case.draw()
    case.tri(case.px([(w * 0.5 - 0.5, -1), (w * 0.5 + 0.75, h * 0.5), (w * 0.5 - 0.5, h + 1)], 0.375))
    case.contains = {"full": 0}
    return case


def tables(width, height, draws=17, cube=False, textures=5):
    """`draws` draws of one triangle each plus draws of 0, 1 and 2 indices first, in the middle and last, an index count that is no
    multiple of 3, and non-zero vertex and index offsets (every mesh is appended to one vertex and one index buffer); textures of
    1 x 1, 3 x 5 and 7 x 1 texels (five of them, or the first `textures`), uv negative and of several thousand.  cube: every draw's model matrix carries its NDC x, y to
    face CUBE_FACE of a probe at the origin, at a distance of its own.  Returns (scene, clip [T, 3, 4] under an identity
    view-projection, textured [T])."""
    sc = scn.Scene()
    rng = np.random.default_rng(23)
    texs = []
    for n, (tw, th, all_mips) in enumerate([(1, 1, True), (3, 5, True), (7, 1, True), (3, 5, False), (7, 1, False)][:textures]):
        img = rng.integers(1, 255, size=(th, tw, 4)).astype(np.uint8)
        img[..., 3] = 255
        t = sc.add_texture(img)
        if not all_mips:
            sc.textures[t] = sc.textures[t][:1]
        texs.append(t)
    ident = sc.add_transform(np.eye(4, dtype=F32))

    def transform(n):
        if not cube:
            return ident
        dist = 0.0625 + 2.0 ** -9 * n
        m = np.zeros((4, 4), F32)
        m[0, 0] = m[1, 1] = -dist
        m[2, 3], m[3, 3] = -dist, 1.0
        m[2, 2] = 2.0 ** -20  # so that the matrix has an inverse for the normal matrix; z of a vertex moves the distance by 2^-20 z
        return sc.add_transform(m)

    helper = Case("tables", width, height)
    clip, textured = [], []
    z = _zgrid(draws + 4, rng)

    def stub(nidx):  # a draw of fewer than three indices, with vertices of its own in the buffers
        pos = helper.px([(1, 1), (5, 1), (1, 5)], 0.0625)
        mesh = sc.add_mesh(pos, np.array([[0, 0, 1]] * 3, F32), np.zeros((3, 2), F32), np.arange(3, dtype=np.uint32))
        sc.add_draw(ident, (mesh[0], mesh[1], nidx), texs[0])

    stub(0)
    for n in range(draws):
        if n == draws // 2:
            stub(1)
            stub(2)
        x, y = 4 + (n * 11) % (width - 24), 4 + (n * 7) % (height - 24)
        pos = helper.px([(x, y), (x + 18.5, y + 3), (x + 4, y + 17.25)], z[n])
        uvs = [np.array([[0, 0], [1, 0], [0, 1]], F32), np.array([[-3.25, -7.5], [-1.0, -7.5], [-3.25, -2.0]], F32),
               np.array([[4000.0, 3000.0], [4003.0, 3000.0], [4000.0, 3009.0]], F32), np.array([[0, 0], [64, 0], [0, 64]], F32)][n % 4]
        extra = [0, 1, 2, 1][n % 4]  # index_count % 3 != 0: the trailing indices draw nothing
        idx = np.concatenate([np.arange(3), np.zeros(extra)]).astype(np.uint32)
        mesh = sc.add_mesh(pos, np.array([tri_normal(n)] * 3, F32), uvs, idx)
        tex = texs[n % len(texs)] if n % 6 != 5 else scn.INVALID
        sc.add_draw(transform(n), mesh, tex)
        clip.append(np.concatenate([pos, np.ones((3, 1), F32)], axis=1))
        textured.append(tex != scn.INVALID)
    stub(2)
    return sc, np.asarray(clip, F32), np.asarray(textured, bool)


# ---- the cube bake: the same triangles on face -Z of a probe at the origin ----
CUBE_FACE = 5  # forward (0, 0, -1), up (0, -1, 0): view x = -world x, view y = -world y, clip w = -world z


def place_on_cube(case, depth_of):
    """scene.Scene whose triangle i has the NDC x, y of case triangle i on face CUBE_FACE at the distance depth_of(i) (clip w) from
    a probe at the origin; exact where x, y and the distance are dyadic with few bits.  Textured draws, grouped as in the case."""
    sc = scn.Scene()
    tex = sc.add_texture(palette())
    ident = sc.add_transform(np.eye(4, dtype=F32))
    clip = case.clip()
    runs = []
    for i in range(len(case.pos)):
        if runs and runs[-1][0] == case.draw_of[i]:
            runs[-1][1].append(i)
        else:
            runs.append((case.draw_of[i], [i]))
    for d, ids in runs:
        pos = []
        for i in ids:
            dist = np.asarray(depth_of(i), np.float64).reshape(-1) * np.ones(3)
            ndc = clip[i, :, :2].astype(np.float64) / clip[i, :, 3:4]
            pos.append(np.stack([-ndc[:, 0] * dist, -ndc[:, 1] * dist, -dist], axis=1))
        pos = np.asarray(pos).reshape(-1, 3).astype(F32)
        uv = np.repeat(np.asarray([tri_uv(i) for i in ids], F32).reshape(-1, 2), 3, axis=0)
        mesh = sc.add_mesh(pos, np.array([[0, 0, 1]] * len(pos), F32), uv, np.arange(len(pos), dtype=np.uint32))
        sc.add_draw(ident, mesh, tex)
    return sc


def world_scene(case):
    """scene.Scene of a case whose `pos` are world positions (a probe at the origin): textured with the palette, an identity model,
    a draw per run of triangles of one draw"""
    sc = scn.Scene()
    tex = sc.add_texture(palette())
    ident = sc.add_transform(np.eye(4, dtype=F32))
    runs = []
    for i in range(len(case.pos)):
        if runs and runs[-1][0] == case.draw_of[i]:
            runs[-1][1].append(i)
        else:
            runs.append((case.draw_of[i], [i]))
    for d, ids in runs:
        pos = np.asarray([case.pos[i] for i in ids], F32).reshape(-1, 3)
        uv = np.repeat(np.asarray([tri_uv(i) for i in ids], F32).reshape(-1, 2), 3, axis=0)
        mesh = sc.add_mesh(pos, np.array([[0, 0, 1]] * len(pos), F32), uv, np.arange(len(pos), dtype=np.uint32))
        sc.add_draw(ident, mesh, tex)
    return sc


class WorldCase(Case):
    """A case for the cube bake alone, given in world space on face CUBE_FACE of a probe at the origin: a corner at pixel (x, y) of
    the face and distance D (its clip w) is the world point (-ndc_x D, -ndc_y D, -D).  The near plane lies at D = 0.05, the far
    plane at D = 80, and z / w = 1.0006254 - 0.05003127 / D."""
    world = True
    NEAR, FAR = 0.05, 80.0

    def at(self, pts, dist):
        pts = np.asarray(pts, np.float64).reshape(3, 2)
        d = np.asarray(dist, np.float64).reshape(-1) * np.ones(3)
        nx, ny = pts[:, 0] * 2.0 / self.width - 1.0, pts[:, 1] * 2.0 / self.height - 1.0
        return np.stack([-nx * d, -ny * d, -d], axis=1).astype(F32)

    def ndc(self, xy, dist):
        """corners given in NDC (exact for a distance that is a power of two)"""
        xy = np.asarray(xy, np.float64).reshape(3, 2)
        d = np.asarray(dist, np.float64).reshape(-1) * np.ones(3)
        return np.stack([-xy[:, 0] * d, -xy[:, 1] * d, -d], axis=1).astype(F32)


def cube_near_plane(size):
    """The near clip on the cube bake (cubemap.hip's own instantiation of clip_near: view position and uv are interpolated at the
    crossing too): the eight inside masks in both windings -- a corner is inside at a distance beyond 0.05 -- and six pairs
    sharing an edge that crosses the plane.  Not placed: a corner exactly on the plane (clip z of a placed vertex is a rounded
    expression of its distance, m22 * z + m23, and is not exactly +-0 for any float32 distance)."""
    case = WorldCase("near_plane", size, size)
    case.draw()
    cell = 24.0
    per_row = int((size - 8) // cell)
    slot = 0
    masks = {}
    for mask in range(8):
        for winding in (0, 1):
            d = [(0.1 + 0.02 * k) if mask >> k & 1 else (0.02 + 0.005 * k) for k in range(3)]
            cx, cy = 4 + cell * (slot % per_row), 4 + cell * (slot // per_row)
            slot += 1
            p = case.at([(cx + 2, cy + 2), (cx + 21, cy + 5), (cx + 7, cy + 20)], d)
            i = case.tri(p[[0, 2, 1]] if winding else p)
            masks[(mask, winding)] = i
    pairs = []
    pairs_y = 4 + cell * ((slot + per_row - 1) // per_row) + 4
    for n, (da, db) in enumerate([(0.2, 0.02), (0.1, 0.01), (0.4, 0.04), (0.03, 0.3), (0.07, 0.045), (0.02, 0.09)]):
        a, b = (3, 2 + 3 * (n % 3)), (21, 20 - 2 * (n % 4))
        ox, oy = 4 + 82.0 * (n % 3), pairs_y + 80.0 * (n // 3)
        def sc(p):
            return (ox + 3.4 * p[0], oy + 3.4 * p[1])
        i = case.tri(case.at([sc(a), sc(b), sc((4, 21))], [da, db, 0.15]))
        pj = case.at([sc(b), sc(a), sc((20, 2))], [db, da, 0.12])
        j = case.tri(pj[[0, 2, 1]] if n % 2 else pj)
        pairs.append((i, j))
    assert size >= pairs_y + 160 and size >= 4 + 3 * 82
    case.contains = {"masks": masks, "pairs": pairs, "max_band_share": 0.10}
    return case


def cube_guard_band(size):
    """The guard band and non-numbers on the cube bake.  With a distance that is a power of two the placement is exact, so a screen
    coordinate of exactly +-2^20 px exists: kept; the next float32 beyond (nearer, so it would show): dropped; for x and y, both
    signs.  One coordinate of one world position NaN, +Inf or -Inf between two ordinary neighbours in the same draw: dropped,
    the neighbours drawn.  Not placed: w = 0, w < 0 and w just above 0 with clip z >= 0 (on the cube clip w is the distance and
    clip z = 1.0006 w - 0.05: a corner nearer than 0.05 is behind the near plane and is clipped away before the snap sees it)."""
    case = WorldCase("guard_band", size, size)
    d = case.draw()
    kept, dropped = [], []
    for axis in (0, 1):
        for sign in (1, -1):
            on, beyond = _guard_ndc(size, sign)
            # each kept wedge at a power of two of its own (they overlap in the middle of the face: no near-ties)
            for far, dist, into in ((on, 0.125 * 2.0 ** len(kept), kept), (beyond, 0.0625, dropped)):
                xy = np.array([[0.0, 0.0], [0.0, -0.4], [0.0, 0.4]], np.float64)
                if axis == 1:
                    xy = xy[:, [1, 0]]
                xy[0, axis] = float(far)
                into.append(case.tri(case.ndc(xy, dist), d))
    dn = case.draw()
    neighbours = []
    n = 0
    for comp in (0, 1, 2):
        for bad in (np.nan, np.inf, -np.inf):
            x0 = -0.9 + 0.2 * n
            xy = [(x0, -0.9), (x0 + 0.15, -0.9), (x0, -0.6)]
            neighbours.append(case.tri(case.ndc(xy, 0.09375), dn))
            t = case.ndc(xy, 0.078125)
            t[n % 3, comp] = bad
            dropped.append(case.tri(t, dn))
            n += 1
    neighbours.append(case.tri(case.ndc([(0.9, -0.9), (0.95, -0.9), (0.9, -0.6)], 0.09375), dn))
    case.contains = {"kept": kept, "dropped": dropped, "neighbours": neighbours}
    return case


def cube_depth_range(size):
    """The limits of the depth range on the cube bake, near the middle of the face (the stored distance stays clear of the clear
    value 100): a triangle that straddles the far distance 80 (the per-fragment far clip cuts it along a line), one wholly beyond
    it (draws nothing), one just before it, one just beyond the near distance.  Not placed: z exactly 0, -0.0 or exactly 1 over a
    whole triangle (z / w = 1.0006254 - 0.05003127 / w takes neither value exactly for a float32 w)."""
    case = WorldCase("depth_range", size, size)
    case.draw()
    s = float(size)
    ids = {
        "far_cut": case.tri(case.at([(s * 0.36, s * 0.36), (s * 0.49, s * 0.38), (s * 0.37, s * 0.49)], [40.0, 120.0, 90.0])),
        "beyond": case.tri(case.at([(s * 0.51, s * 0.36), (s * 0.64, s * 0.38), (s * 0.52, s * 0.49)], [81.0, 90.0, 100.0])),
        "before_far": case.tri(case.at([(s * 0.36, s * 0.51), (s * 0.49, s * 0.53), (s * 0.37, s * 0.64)], 79.5)),
        "after_near": case.tri(case.at([(s * 0.51, s * 0.51), (s * 0.64, s * 0.53), (s * 0.52, s * 0.64)], 0.0501)),
    }
    case.zmax = 1.001
    case.contains = ids
    return case


def tie_distance():
    """a distance D on the cube face whose z / w is exactly 0.5 in fp32 under both numeric contracts: the weights of the tie class
    are dyadic with few bits, so every fp32 step of a depth interpolated between corners at z / w = 0.5 is exact"""
    import cubemap_reference as cref

    proj = cref.projection()
    d0 = F32(float(-proj[2, 3]) / (float(-proj[2, 2]) - 0.5))
    cand = d0 + (np.arange(-4096, 4096) * np.spacing(d0)).astype(F32)
    ok = np.ones(len(cand), bool)
    zc = []
    for contract in (1, 2):
        c = cref.mat_vec(cref.Arith(contract), proj, np.zeros_like(cand), np.zeros_like(cand), -cand, np.ones_like(cand))
        ok &= (c[2] / c[3]).astype(F32) == F32(0.5)
        zc.append(np.asarray(c[2], F32))
    ok &= zc[0] == zc[1]
    assert ok.any(), "no float32 distance with z / w == 0.5"
    return float(cand[np.nonzero(ok)[0][0]])


def cube_clip(ar, sc, face=CUBE_FACE, pos=(0.0, 0.0, 0.0)):
    """float32 [T, 3, 4]: the clip positions of every triangle of the textured draws of `sc` on `face`, as the vertex stage of
    cubemap_reference computes them"""
    import cubemap_reference as cref

    proj = cref.projection()
    out = []
    for d in sc.draws:
        if d["albedo"] == scn.INVALID or d["index_count"] < 3:
            continue
        n = d["index_count"] // 3 * 3
        idx = sc.indices[d["index_offset"]:d["index_offset"] + n].astype(np.int64) + d["vertex_offset"]
        v = sc.vertices[idx].astype(F32)
        view_model = cref.mat_mul(cref.face_view(face, pos), np.asarray(sc.transforms[d["transform"]][0], F32))
        vp = cref.mat_vec(ar, view_model, v[:, 0], v[:, 1], v[:, 2], np.ones(len(v), F32))
        c = cref.mat_vec(ar, proj, vp[0], vp[1], vp[2], vp[3])
        out.append(np.stack(c, -1).astype(F32).reshape(-1, 3, 4))
    return np.concatenate(out) if out else np.zeros((0, 3, 4), F32)


def shadow_small_waves(triangles):
    """waves per layer of default_shadow's small-list kernel for a scene of that many triangles (shadow.hip: one wave per record,
    2 per triangle, in blocks of 4, plus a block, at most 2048 blocks)"""
    return 4 * min(2 * triangles // 4 + 1, 2048)


def cube_small_waves(triangles):
    """waves of cubemap_probe's small-list kernel (cubemap.hip: 12 records per triangle, blocks of 4, plus one, at most 1024)"""
    return 4 * min(12 * triangles // 4 + 1, 1024)


RASTER_LARGE_WAVES = 4 * 2048  # gbuf_opaque_taa's large kernel: a fixed grid


# ---- the registry: class name -> (builder arguments per program) ----
# gbuf_opaque_taa takes any extent; default_shadow and cubemap_probe square ones.  The slivers of the square programs outnumber the
# waves of their small-list kernels (asserted in tests/test_raster_geometry.py from the grid formulas above).
SHADOW_NEEDLES = 8192 + 128  # with 40 invisible slivers: the last turn of the small-list loop holds at least 88 needles
CUBE_NEEDLES = 4096 + 128
CLASSES = {
    "centre_lattice": dict(gbuf=[(203, 117), (204, 118)],  # the even extent: HostFrame's
                            shadow=(117, 117), cube=(64, 64)),
    "exact_ties": dict(gbuf=(203, 117), shadow=(117, 117), cube=(128, 128, True, True)),
    "block_split": dict(gbuf=(203, 117), shadow=(203, 203), cube=(203, 203)),
    "offscreen_reach": dict(gbuf=(203, 117), shadow=(117, 117), cube=(117, 117)),
    "guard_band": dict(gbuf=(64, 32), shadow=(64, 64), cube=("world", 64)),
    "slivers": dict(gbuf=(64, 48, 3000), shadow=(92, 92, 40, SHADOW_NEEDLES), cube=(72, 72, 40, CUBE_NEEDLES)),
    "large_flood": dict(gbuf=(328, 200), shadow=(136, 136, 30), cube=(136, 136, 30)),
    "near_plane": dict(gbuf=(251, 291), shadow=(291, 291), cube=("world", 256)),
    "depth_range": dict(gbuf=(203, 117), shadow=(117, 117), cube=("world", 117)),
    "tiny_targets": dict(gbuf=[(1, 1), (3, 2), (8, 8), (9, 7)], shadow=[(1, 1), (7, 7), (9, 9)], cube=[(1, 1), (7, 7), (9, 9)]),
}
TABLES = dict(gbuf=[(203, 117, 1), (203, 117, 8, False, 4), (203, 117, 9), (203, 117, 17)], shadow=[(117, 117, 9), (117, 117, 33)],
              cube=[(64, 64, 1, True), (64, 64, 9, True), (64, 64, 17, True)])
_CACHE = {}


def tables_case(program, args):
    """(scene, reference result, drawn triangles) of the tables class for a program -- cached"""
    key = ("tables", program, tuple(args))
    if key not in _CACHE:
        import cubemap_reference as cref

        sc, clip, textured = tables(*args)
        if program == "cube":
            clip = cube_clip(cref.Arith(2), sc)  # the textured draws only
            assert len(clip) == int(textured.sum())
            assert np.array_equal(clip, cube_clip(cref.Arith(1), sc))
            ids = np.nonzero(textured)[0]
        else:
            ids = np.arange(len(clip))
        tris, owners = clip_near_all(clip)
        r = rr.rasterise(tris, args[0], args[1], owner_ids=ids[owners])
        _CACHE[key] = (sc, r, len(ids))
    return _CACHE[key]


def get(name, args):
    """(case, reference result) of class `name` built with `args`, computed once per process and never changed"""
    key = (name, tuple(args))
    if key not in _CACHE:
        case = build(name, args)
        _CACHE[key] = (case, case.reference())
    return _CACHE[key]


def build(name, args):
    """the case alone (cached), for a test that needs no reference"""
    key = ("case", name, tuple(args))
    if key not in _CACHE:
        if args and args[0] == "world":  # a class of its own for the cube bake, given in world space
            _CACHE[key] = globals()["cube_" + name](*args[1:])
        else:
            _CACHE[key] = globals()[name](*args)
    return _CACHE[key]


def cube_distances(case):
    """per triangle the three distances (clip w on the cube face) that keep its order in depth: the rank of a corner's z among all
    z of the case on a 2^-13 grid from 1/16; more than 2^-12 of NDC depth apart there (d z_ndc / d w = 0.05 / w^2 >= 3.2)"""
    z = np.asarray(case.pos, F32)[..., 2]
    z = np.where(np.isfinite(z), z, F32(0.5))
    uniq = np.unique(z)
    d = 0.0625 + 2.0 ** -13 * np.searchsorted(uniq, z)
    assert d.max() < 0.125, "more distinct depths than the cube placement has room for"
    return d


def cube_case(name, args):
    """(scene on the cube, reference result from the clip positions of cubemap_reference's vertex stage) -- cached"""
    key = ("cube", name, tuple(args))
    if key not in _CACHE:
        import cubemap_reference as cref

        case = build(name, args)
        if getattr(case, "world", False):
            # placed in world space by the class; not exact, so the reference is fed what the vertex stage of the contract in
            # use computes (contract 2: what the libraries are built with; the GPU test asserts that)
            sc = world_scene(case)
            with np.errstate(invalid="ignore"):  # 0 * inf of the non-numbers among the positions
                clip = case.world_clip = cube_clip(cref.Arith(2), sc)
        else:
            dist = cube_distances(case)
            for i, d in getattr(case, "cube_distance", {}).items():
                dist[i] = d
            sc = place_on_cube(case, lambda i: dist[i])
            clip = cube_clip(cref.Arith(2), sc)
            # the placement is exact, so the clip positions do not depend on the numeric contract
            assert np.array_equal(clip, cube_clip(cref.Arith(1), sc), equal_nan=True)
        tris, owners = clip_near_all(clip)
        r = rr.rasterise(tris, case.width, case.height, owner_ids=owners)
        r.kept_submission = np.bincount(owners[r.kept], minlength=len(case.pos)) > 0
        _CACHE[key] = (case, sc, r)
    return _CACHE[key]


# ---- comparing a program's output with the exact reference ----
def compare(label, case, ref, d24=None, albedo=None, covered=None, zmax=None):
    """Asserts coverage (as a set), owner and depth of one program's output against the exact reference `ref`.
    d24: the 24-bit depth codes [H, W] (0xFFFFFF: cleared), or None for a program that stores no depth (then `covered` is given).
    albedo: sRGB codes [H, W, 4] of a program that shades with the palette, or None.
    Returns (covered texels, largest deviation from the exact depth in codes)."""
    bound = rr.depth_bound_codes(case.zmax if zmax is None else zmax)
    # the line along which the depth clip cuts a triangle (depth_range's far cut): fp32 rounding decides within the depth bound of it
    edge = ref.clip_band.copy()
    if covered is None:
        covered = d24 != 0xFFFFFF
        edge |= ref.coverage & (ref.d24 == 0xFFFFFF)  # a depth-only program stores the cleared word for a fragment on the far plane
    elif albedo is not None and d24 is not None:
        assert ((d24 != 0xFFFFFF) <= covered).all(), f"{label}: a depth without a colour"
    diff = (covered != ref.coverage) & ~edge
    assert not diff.any(), f"{label}: coverage differs on {int(diff.sum())} texels, first (y, x) {np.argwhere(diff)[:5].tolist()}"
    both = covered & ref.coverage
    worst = 0
    if d24 is not None:
        dev = np.abs(d24.astype(np.int64) - ref.d24)[both]
        worst = int(dev.max(initial=0))
        print(f"[raster-geometry] {label}: covered {int(both.sum())}, depth within {worst} codes of the exact depth (bound {bound})")
        assert worst <= bound, f"{label}: depth {worst} codes from the exact depth of the reference's owner, bound {bound}"
    if albedo is not None:
        want = tri_color(np.where(ref.owner >= 0, ref.owner, 0))
        wrong = both & (albedo != want).any(axis=-1)
        assert not wrong.any(), f"{label}: wrong owner on {int(wrong.sum())} texels, first (y, x) {np.argwhere(wrong)[:5].tolist()}"
    return int(both.sum()), worst


# ---- running gbuf_opaque_taa at any extent (PostFxChain wants even ones: the chain behind the G-buffer works at half size) ----
class Gbuf:
    """the five attachments of one extent and the raster_gbuffer entry of a registered backend ("oracle": host memory, no stream;
    "product": the HIP library on `device`), with an identity view-projection unless one is given"""
    NAMES = ("albedo", "normal", "material", "velocity", "depth")

    def __init__(self, width, height, backend, device=None):
        from vk_renderer_amd import abi, chain
        from vk_renderer_amd.images import ImageBuf

        self.lib, self.prefix, on_device = chain._BACKENDS[backend]()
        self.backend, self.device = backend, (device or "cuda") if on_device else None
        self.width, self.height = width, height
        fmts = (abi.FMT_RGBA8_SRGB, abi.FMT_RG16_UNORM, abi.FMT_RGBA8_SRGB, abi.FMT_RG16_SFLOAT, abi.FMT_D24_UNORM_S8)
        self.images = {n: ImageBuf(f, width, height, device=self.device, fill=0x5A) for n, f in zip(self.NAMES, fmts)}

    def raster(self, scene, view_projection=None, keep_scratch=False):
        """-> {name: raw texels}; depth as the whole 32-bit words [H, W]"""
        import ctypes as C

        from vk_renderer_amd import abi

        rs, keep = scene.upload(self.device)
        c = abi.GbufConst()
        m = np.eye(4, dtype=F32) if view_projection is None else np.asarray(view_projection, F32)
        c.view_projection, c.prev_view_projection = abi.Mat4.from_np(m), abi.Mat4.from_np(m)
        img = self.images
        args = [C.byref(rs), C.byref(c)] + [C.byref(img[n].desc()) for n in self.NAMES]
        fn = getattr(self.lib, self.prefix + "raster_gbuffer")
        if self.device is None:
            rc = fn(*args, C.c_void_p(0), 0)
        else:
            import torch

            nbytes = int(self.lib.vkr_raster_scratch_bytes(self.width, self.height, sum(d["index_count"] // 3 for d in scene.draws)))
            scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
            rc = fn(*args, C.c_void_p(scratch.data_ptr()), nbytes, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
            torch.cuda.synchronize(self.device)
            self._scratch = scratch
        abi.check(rc, self.lib if self.backend == "product" else None)
        out = {n: img[n].raw(0).copy() for n in self.NAMES}
        out["depth"] = out["depth"][..., 0].astype(np.uint32)
        if keep_scratch:
            out["scratch"] = self._scratch
        out["decoded"] = {n: img[n].decode() for n in self.NAMES[:4]}  # what a texelFetch returns, for the rule of parity.py
        return out


def oracle_shadow(scene, m, n):
    """the expected shadow map, as shadow_light.expected() defines it (the oracle's depth attachment under the light's matrix, no
    textures), at any extent: uint32 [n, n]"""
    import shadow_light as sl

    return Gbuf(n, n, "oracle").raster(sl.strip(scene), m)["depth"] & 0xFFFFFF
