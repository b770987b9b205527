"""Constructed scenes and far rays for the ray query (csrc/accel_traverse.hpp, the host build of csrc/accel.hip), shared by
tests/test_ray_scene_cases.py (no GPU: the layout invariants, the reach property of tests/ray_walk_reference.py, the mutants) and
tests/test_ray_scene_cases_gpu.py (the entries against the brute force).

The rays of tests/test_accel_occluded_gpu.py are adversarial; its scenes live within a few units of the origin, where the widening
of the triangle boxes, (s + 1) * 2^-12, is thousands of times larger than any rounding of the slab term.  The scenes here go where
that stops: far from the origin, at 2^-40 and 2^40 times the size, with boxes of wildly different area, with vertices that are not
finite, and down to the builder's depth cap.

Scenes (`procedural` is abi.scene_triangles(procedural_scene(detail=3)), 112 triangles; `box` the 12 triangles of
test_accel_occluded_gpu.py; transformed in float64 and rounded once):
  offset_2p13, offset_2p20   procedural translated by (2^13, -2^13, 2^13) and (2^20, 2^20, -2^20); at 2^20 the float grid is 1/8 wide
                             and vertices collapse: 36 triangles lose their area, no two become duplicates (counted in the CPU test)
  scale_2m40, scale_2p40     procedural times 2^-40 and 2^40 (exact)
  mixed_scale                the first half of procedural shrunk by 2^-10 around its first vertex, the second half as it is, and the
                             8 faces of an octahedron with vertices 2^12 from the scene's centre around everything
  slivers                    256 triangles from a corner of the scene box to the opposite one, 64 per diagonal, each 1e-3 wide
  duplicates_reversed        procedural followed by procedural in reverse order: every hit is an exact tie
  deep                       see below
  area_overflow              box interleaved with 12 small triangles at +-2^70 on each axis: area() of every node that holds two of
                             them is infinite, the SAH cost NaN, and the range is halved in its present order
  nonfinite_vertices         procedural with 24 triangles changed: one coordinate NaN, +inf, -inf; all three x +inf; a whole NaN
                             triangle (in turn)

`deep`: 50 small triangles at 2^e on alternating axes, e falling by 5 from one triangle to the next of the same axis (59, 57, 55,
54, 52, 50, ... -23), each centred on 0 in the two other coordinates, and a clump of 12 distinct triangles at 2^-30.  The centroid bins
are 16 wide, so with a step of 2^5 everything but the outermost triangle falls into bin 0 of every axis and each level peels exactly
one triangle; a triangle that is not centred on the other axes shares a bin with the next one and the depth halves.  After 48 peels
the builder is at ACCEL_MAX_DEPTH and makes a leaf of the 2 triangles left over and the clump: the maximum depth is exactly 48 and
that leaf holds 14 > ACCEL_MAX_LEAF triangles (asserted from the layout in tests/test_ray_scene_cases.py).  Every extent stays below
2^60, so area() is finite everywhere.

Rays of a scene: test_accel_occluded_gpu._rays(tris, rng), unchanged, then four classes (`ext`, `centre` as _rays computes them
from the root box; k in K = 8, 13, 16, 20, 24; targets are triangle centroids, vertices, edge midpoints and `beside` points just
outside a corner of the scene box, which a ray may pass without hitting anything):
  far_origin    origins at centre + u * 2^k * ext on random unit vectors u; per target one ray ending there (d = target - o) and one
                passing through (d = 2 (target - o))
  far_axis      the same, with the origin moved onto an axis through the target: two direction components are exactly 0
  far_end       origins in the scene box (every fourth one in the shell of 0.25 ext around it, so that a closed scene has misses),
                directions of length 2^k * max(ext), half of them aimed at a target: the hits sit at t of about 2^-k
  last_subtree  test_accel_closest_gpu._last_subtree_rays, where the root is interior and its first child's box is finite
The rays of nonfinite_vertices are built around procedural (the boxes of a scene with infinite vertices are infinite, and a class
"around the box" means nothing there); its far classes aim at the unchanged geometry as well.  Those of area_overflow are built
around box: around a root box of 2^71 nothing would ever meet the 12 triangles in the middle.  _rays alone makes 6800 to 9600 rays
of a scene, so a case has 8400 to 11300 rays.

What the cases are (brute force, t in [0, 1]; hits of the 72 rays of a far class per k = 8 / 13 / 16 / 20 / 24):
  scene               tris nodes depth  rays  hits   far_origin      far_axis        far_end
  offset_2p13          112   39    6    9576  4312   55/54/52/54/46  52/53/52/54/36  44/36/34/39/37
  offset_2p20          112   37    6    9576  2250   52/51/53/54/52  53/49/52/51/54  28/27/28/28/28
  scale_2m40           112   33    5    9576  2293   52/50/66/72/70  52/48/52/46/46  27/28/28/28/28
  scale_2p40           112   99    8    9576   488   0/0/0/0/0       14/0/0/0/0      0/0/0/0/0
  mixed_scale          120   79    9    9672  4517   49/54/56/53/18  53/53/50/48/45  40/37/44/38/41
  slivers              256   63    5   11304  3575   47/20/20/24/26  54/50/53/52/46  28/28/28/28/28
  duplicates_reversed  224  143    9   10920  6112   55/50/47/35/24  51/52/50/42/14  42/45/41/41/38
  deep                  62   97   48    8976   992   42/50/48/46/5   16/20/12/16/12  5/10/8/6/6
  area_overflow         24    7    2    8352  4624   53/58/47/52/16  54/50/46/45/27  65/63/62/61/63
  nonfinite_vertices   112   49    7    9320  2971   49/32/27/14/16  50/46/48/36/14  34/31/32/32/29
At scale_2p40 the products of the frozen test overflow for every far ray but a few on an axis: a miss for both sides.  At k = 24 the
grid of the origin is coarser than the scene and the frozen test's own box clause decides what is a hit; the counts fall on most scenes.
"""
import functools

import numpy as np

from vk_renderer_amd import abi
from vk_renderer_amd import scene as scn

import closest_hit_reference as closest
from test_accel_closest_gpu import _last_subtree_rays
from test_accel_occluded_gpu import SCENES as OLD_SCENES
from test_accel_occluded_gpu import _box, _nodes, _rays

F32 = np.float32
F64 = np.float64
MISS = closest.MISS
NODE = np.dtype([("lo", "<f4", 3), ("first", "<u4"), ("hi", "<f4", 3), ("count", "<u4")])
TRI = np.dtype([("v0", "<f4", 3), ("index", "<u4"), ("e1", "<f4", 3), ("e2", "<f4", 3), ("lo", "<f4", 3), ("hi", "<f4", 3)])
MAX_DEPTH, MAX_LEAF, STACK = 48, 8, 64  # ACCEL_MAX_DEPTH, ACCEL_MAX_LEAF, ACCEL_STACK
K = (8, 13, 16, 20, 24)
FAR = ("far_origin", "far_axis", "far_end")
# the parameter ranges of the new scenes; exact_range() adds tmin == tmax at the t of a far_origin hit
RANGES = ((0.0, 1.0), (1e-12, 1.0), (0.25, 0.75), (0.0, 1e10))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _procedural64():
    return np.asarray(abi.scene_triangles(scn.procedural_scene(detail=3)), F64)


def _procedural():
    return _procedural64().astype(F32)


def _offset(x, y, z):
    return (_procedural64() + np.array([x, y, z], F64)).astype(F32)


def _mixed_scale():
    p = _procedural64()
    half = len(p) // 2
    pivot = p[0, 0]
    small = pivot + (p[:half] - pivot) * 2.0 ** -10
    c = 0.5 * (p.reshape(-1, 3).min(0) + p.reshape(-1, 3).max(0))
    r = 2.0 ** 12
    octa = [[c + [sx * r, 0, 0], c + [0, sy * r, 0], c + [0, 0, sz * r]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    return np.concatenate([small, p[half:], np.array(octa, F64)]).astype(F32)


def _slivers():
    p = _procedural64().reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    out = []
    for corner in range(4):
        a = np.array([(lo, hi)[(corner >> k) & 1][k] for k in range(3)])
        a[2] = lo[2]
        b = lo + hi - a
        along = (b - a) / np.linalg.norm(b - a)
        side = np.cross(along, [0.0, 0.0, 1.0])
        side /= np.linalg.norm(side)
        for i in range(64):
            turn = np.cos(i * 0.1) * side + np.sin(i * 0.1) * np.cross(along, side)
            out.append([a, b, a + (b - a) * ((i + 1) / 65.0) + turn * 1e-3])
    return np.array(out, F64).astype(F32)


def _deep(levels=50, top=59, gap=5, clump=12, size=2.0 ** -6, inner=-30):
    out = []
    for k in range(levels):
        axis, j = k % 3, k // 3
        e = top - gap * j - 2 * axis
        c = np.zeros(3)
        c[axis] = 2.0 ** e
        s = 2.0 ** e * size
        u, w = np.roll([s, 0.0, 0.0], (axis + 1) % 3), np.roll([s, 0.0, 0.0], (axis + 2) % 3)
        out.append([c - u - w, c + u, c + w])  # -s, +s, 0 and -s, 0, +s on the other axes: centred on 0 there
    rng = np.random.default_rng(3)
    for _ in range(clump):
        c = rng.uniform(-1, 1, 3) * 2.0 ** inner
        out.append([c, c + [2.0 ** (inner - 1), 0, 0], c + [0, 2.0 ** (inner - 1), 0]])
    return np.array(out, F64).astype(F32)


def _area_overflow():
    box = np.asarray(_box(), F64)
    far = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            for turn in range(2):
                c = np.zeros(3)
                c[axis] = sign * 2.0 ** 70
                u, w = np.roll([2.0 ** 50, 0.0, 0.0], (axis + 1 + turn) % 3), np.roll([2.0 ** 50, 0.0, 0.0], (axis + 2 - turn) % 3)
                far.append([c, c + u, c + w])
    far = np.array(far, F64)
    out = np.empty((24, 3, 3), F64)
    out[0::2], out[1::2] = box, far
    return out.astype(F32)


NONFINITE_COUNT = 24


def nonfinite_changed():
    """the input indices of the triangles of nonfinite_vertices that are changed"""
    n = len(_procedural64())
    return np.random.default_rng(41).permutation(n)[:NONFINITE_COUNT]


def _nonfinite_vertices():
    t = _procedural()
    for j, i in enumerate(nonfinite_changed()):
        kind, vertex, axis = j % 5, (j // 5) % 3, (j // 2) % 3
        if kind < 3:
            t[i, vertex, axis] = (np.nan, np.inf, -np.inf)[kind]
        elif kind == 3:
            t[i, :, 0] = np.inf
        else:
            t[i] = np.nan
    return t


NEW_SCENES = {
    "offset_2p13": lambda: _offset(2.0 ** 13, -2.0 ** 13, 2.0 ** 13),
    "offset_2p20": lambda: _offset(2.0 ** 20, 2.0 ** 20, -2.0 ** 20),
    "scale_2m40": lambda: (_procedural64() * 2.0 ** -40).astype(F32),
    "scale_2p40": lambda: (_procedural64() * 2.0 ** 40).astype(F32),
    "mixed_scale": _mixed_scale,
    "slivers": _slivers,
    "duplicates_reversed": lambda: np.concatenate([_procedural(), _procedural()[::-1]]),
    "deep": _deep,
    "area_overflow": _area_overflow,
    "nonfinite_vertices": _nonfinite_vertices,
}
# what the rays of a scene are built around, where that is not the scene itself
RAY_GEOMETRY = {"nonfinite_vertices": _procedural, "area_overflow": lambda: np.asarray(_box(), F32)}
ALL_SCENES = dict(OLD_SCENES, **NEW_SCENES)


# ---- the records and the layout -------------------------------------------------------------------------------------------------
def host_records(tris):
    """gtao_rt_reference.triangle_records with the NaN rules of the host's std::min / std::max (`b < a ? b : a`: a NaN second
    argument is never taken, a NaN first one stays), which is what make_record computes for vertices that are not finite; for
    finite input the two are the same bits (asserted in tests/test_ray_scene_cases.py)"""
    t = np.asarray(tris, F32).reshape(-1, 3, 3)
    smin = lambda a, b: np.where(b < a, b, a)
    smax = lambda a, b: np.where(a < b, b, a)
    with np.errstate(all="ignore"):
        s = np.zeros(len(t), F32)
        for v in np.abs(t.reshape(-1, 9)).T:
            s = smax(s, v)
        margin = ((s + F32(1.0)) * F32(2.0 ** -12)).astype(F32)[:, None]
        return {"v0": t[:, 0], "e1": t[:, 1] - t[:, 0], "e2": t[:, 2] - t[:, 0],
                "lo": smin(smin(t[:, 0], t[:, 1]), t[:, 2]) - margin, "hi": smax(smax(t[:, 0], t[:, 1]), t[:, 2]) + margin}


class Layout:
    """vkr_accel_layout's arrays with what the tests derive from them: parent and depth per node, the leaf of every input
    triangle; nodes are stored parents first"""

    def __init__(self, tris):
        raw_nodes, raw_tris = abi.accel_layout(tris)
        self.bytes = raw_nodes.tobytes() + raw_tris.tobytes()
        self.nodes = raw_nodes.view(NODE).reshape(-1)
        self.recs = raw_tris.view(TRI).reshape(-1)
        n = len(self.nodes)
        self.parent = np.full(n, -1, np.int64)
        self.depth = np.zeros(n, np.int64)
        self.leaf_of = np.full(len(self.recs), -1, np.int64)  # input index -> node
        for i in range(n):
            nd = self.nodes[i]
            first, count = int(nd["first"]), int(nd["count"])
            if count == 0:
                assert i < first and first + 1 < n, "children are stored behind their parent"
                self.parent[first], self.parent[first + 1] = i, i
                self.depth[first], self.depth[first + 1] = self.depth[i] + 1, self.depth[i] + 1
            else:
                self.leaf_of[self.recs["index"][first:first + count]] = i

    @property
    def max_depth(self):
        return int(self.depth.max()) if len(self.depth) else 0

    def subtree_records(self, node):
        """record positions below a node, in record order"""
        nd = self.nodes[node]
        if nd["count"]:
            return list(range(int(nd["first"]), int(nd["first"]) + int(nd["count"])))
        return self.subtree_records(int(nd["first"])) + self.subtree_records(int(nd["first"]) + 1)


def _union(lo, hi):
    """the box box_of makes of boxes: std::min / std::max from +-inf, so a NaN bound is dropped"""
    with np.errstate(all="ignore"):
        return np.fmin.reduce(np.concatenate([np.full((1, 3), np.inf, F32), lo]), axis=0), np.fmax.reduce(np.concatenate([np.full((1, 3), -np.inf, F32), hi]), axis=0)


def check_layout(tris):
    """The assertions of test_accel.py::test_layout_hierarchy, with `nested` sharpened to `the exact union` and stated so that they
    hold for vertices that are not finite too (a NaN bound of a record is in no node box; everything finite is held as there).
    -> Layout"""
    tris = np.asarray(tris, F32)
    n = len(tris)
    lay = Layout(tris)
    nodes, recs = lay.nodes, lay.recs
    assert 1 <= len(nodes) <= max(1, 2 * n - 1)
    assert len(recs) == n
    want = host_records(tris)
    idx = recs["index"].astype(np.int64)
    assert sorted(idx.tolist()) == list(range(n)), "every input triangle has exactly one record"
    for f in ("v0", "e1", "e2", "lo", "hi"):
        got, exp = recs[f], want[f][idx]
        same = (got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))
        assert same.all(), f
    covered = np.zeros(n, np.int64)
    seen = np.zeros(len(nodes), np.int64)
    stack = [(0, 0)]
    max_depth = 0
    while stack:
        i, depth = stack.pop()
        seen[i] += 1
        max_depth = max(max_depth, depth)
        nd = nodes[i]
        if nd["count"] == 0:
            ch = nodes[[int(nd["first"]), int(nd["first"]) + 1]]
            ulo, uhi = _union(ch["lo"], ch["hi"])
            assert np.array_equal(ulo.view(np.uint32), nd["lo"].view(np.uint32)) and np.array_equal(uhi.view(np.uint32), nd["hi"].view(np.uint32)), \
                f"node {i} is not the union of its children"
            for c in (int(nd["first"]), int(nd["first"]) + 1):
                assert np.all(nodes[c]["lo"] >= nd["lo"]) and np.all(nodes[c]["hi"] <= nd["hi"]), f"child {c} leaves parent {i}"
                stack.append((c, depth + 1))
        else:
            first, count = int(nd["first"]), int(nd["count"])
            r = recs[first:first + count]
            assert len(r) == count
            covered[first:first + count] += 1
            ulo, uhi = _union(r["lo"], r["hi"])
            assert np.array_equal(ulo.view(np.uint32), nd["lo"].view(np.uint32)) and np.array_equal(uhi.view(np.uint32), nd["hi"].view(np.uint32)), \
                f"leaf {i} is not the union of its triangles' boxes"
            assert np.all((r["lo"] >= nd["lo"]) | np.isnan(r["lo"])) and np.all((r["hi"] <= nd["hi"]) | np.isnan(r["hi"])), f"leaf {i} does not contain its triangles"
            with np.errstate(all="ignore"):
                v = np.stack([r["v0"], r["v0"] + r["e1"], r["v0"] + r["e2"]], 1)
            fin = np.isfinite(v) & np.isfinite(tris[r["index"]])
            assert np.all((v >= nd["lo"][None, None]) | ~fin) and np.all((v <= nd["hi"][None, None]) | ~fin)
    assert not np.isnan(nodes["lo"]).any() and not np.isnan(nodes["hi"]).any(), "a node box holds a NaN"
    assert np.all(seen == 1), "a node is unreachable or shared"
    assert np.all(covered == 1), "a triangle is in no leaf or in two"
    assert max_depth <= MAX_DEPTH and max_depth == lay.max_depth
    assert Layout(tris).bytes == lay.bytes, "the same input gives the same bytes"
    return lay


# ---- rays -----------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def far_rays(tris, rng, per_kind=9):
    """-> (origins, directions, tag, k) of far_origin, far_axis and far_end, built around finite triangles"""
    lo, hi, _ = _nodes(tris)
    slo, shi = lo.min(0), hi.max(0)
    ext = np.maximum(shi - slo, F32(1.0)).astype(F64)
    centre = ((slo + shi) * F32(0.5)).astype(F64)
    slo, shi = slo.astype(F64), shi.astype(F64)
    verts = tris.reshape(-1, 3)
    mids = np.concatenate([(tris[:, 0] + tris[:, 1]), (tris[:, 1] + tris[:, 2]), (tris[:, 2] + tris[:, 0])]) * F32(0.5)
    cents = tris.astype(F64).mean(axis=1).astype(F32)
    o, d, tag, ks = [], [], [], []

    def add(oo, dd, name, k):
        o.append(np.asarray(oo, F32))
        d.append(np.asarray(dd, F32))
        tag.extend([name] * len(oo))
        ks.extend([k] * len(oo))

    def targets():
        corner = np.where(rng.integers(0, 2, size=(per_kind, 3)) == 1, shi, slo)
        beside = centre + (corner - centre) * rng.uniform(1.02, 1.3, size=(per_kind, 1))
        return np.concatenate([cents[rng.integers(0, len(cents), per_kind)], verts[rng.integers(0, len(verts), per_kind)],
                               mids[rng.integers(0, len(mids), per_kind)], beside.astype(F32)]).astype(F32)

    for k in K:
        t = targets()
        oo = (centre + _unit(rng, len(t)) * ext * 2.0 ** k).astype(F32)
        add(oo, t - oo, "far_origin", k)
        add(oo, (t - oo) * F32(2.0), "far_origin", k)
        t = targets()
        oo = (centre + _unit(rng, len(t)) * ext * 2.0 ** k).astype(F32)
        axis = np.arange(len(t)) % 3
        on = t.copy()
        on[np.arange(len(t)), axis] = oo[np.arange(len(t)), axis]
        add(on, t - on, "far_axis", k)
        add(on, (t - on) * F32(2.0), "far_axis", k)
        t = np.concatenate([targets(), targets()])
        inside = rng.uniform(slo, shi, size=(len(t), 3))
        shell = rng.uniform(slo - 0.25 * ext, shi + 0.25 * ext, size=(len(t), 3))
        oo = np.where((np.arange(len(t)) % 4 == 3)[:, None], shell, inside).astype(F32)
        aim = t.astype(F64) - oo.astype(F64)
        aim /= np.maximum(np.linalg.norm(aim, axis=1, keepdims=True), 1e-300)
        dirs = np.where((np.arange(len(t)) % 2 == 0)[:, None], aim, _unit(rng, len(t)))
        add(oo, (dirs * ext.max() * 2.0 ** k).astype(F32), "far_end", k)
    return np.concatenate(o), np.concatenate(d), np.array(tag), np.array(ks)


class Case:
    """a scene with its rays: tris, o, d, tag, k (per ray; -1 outside the far classes), rec (host_records), last_set"""


@functools.lru_cache(maxsize=None)
def case(name):
    c = Case()
    c.name = name
    c.tris = np.ascontiguousarray(ALL_SCENES[name](), F32)
    geometry = np.ascontiguousarray(RAY_GEOMETRY[name](), F32) if name in RAY_GEOMETRY else c.tris
    rng = np.random.default_rng([53, sorted(ALL_SCENES).index(name)])
    with np.errstate(all="ignore"):
        o, d, tag = _rays(geometry, rng)
        k = np.full(len(o), -1, np.int64)
        if len(geometry):
            fo, fd, ftag, fk = far_rays(geometry, rng)
            o, d, tag, k = np.concatenate([o, fo]), np.concatenate([d, fd]), np.concatenate([tag, ftag]), np.concatenate([k, fk])
        lo, hi, _ = _nodes(c.tris)
        # the class starts from the box of the root's first child, which an infinite vertex below it makes infinite
        last = _last_subtree_rays(c.tris, rng) if len(lo) > 1 and np.isfinite(lo[1]).all() and np.isfinite(hi[1]).all() else None
    c.last_set = set()
    if last is not None:
        o, d = np.concatenate([o, last[0]]), np.concatenate([d, last[1]])
        tag, k = np.concatenate([tag, np.array(["last_subtree"] * len(last[0]))]), np.concatenate([k, np.full(len(last[0]), -1, np.int64)])
        c.last_set = last[2]
    c.o, c.d, c.tag, c.k = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32), tag, k
    c.rec = host_records(c.tris)
    return c


@functools.lru_cache(maxsize=None)
def base_closest(name):
    """the brute-force closest hits of a case for t in [0, 1], computed once"""
    c = case(name)
    return closest.brute_force_closest(c.o, c.d, 0.0, 1.0, c.rec)


def exact_range(name):
    """(t, t) with t the t of a far_origin hit of the case (the median of those that are > 0); where no far_origin ray hits
    (scale_2p40 and area_overflow: the products of the frozen test overflow for such rays) of a hit of any class; None where
    nothing is hit at all"""
    c, base = case(name), base_closest(name)
    hit = (base["index"] != MISS) & (base["t"] > 0)
    i = np.nonzero((c.tag == "far_origin") & hit)[0]
    if len(i) == 0:
        i = np.nonzero(hit)[0]
    if len(i) == 0:
        return None
    t = float(np.sort(base["t"][i])[len(i) // 2])
    return (t, t)


def ranges(name):
    e = exact_range(name)
    return list(RANGES) + ([e] if e else [])


def candidates(o, d, tmin, tmax, rec, chunk=2048):
    """every (ray, input triangle) the frozen test accepts in [tmin, tmax], with no prefilter at all: -> (ray [m], triangle [m], t [m])"""
    from gtao_rt_reference import frozen_hit_tuv

    ri, ti, tt = [], [], []
    if len(rec["lo"]):
        for s in range(0, len(o), chunk):
            so, sd = o[s:s + chunk, None, :], d[s:s + chunk, None, :]
            ok, t, _, _ = frozen_hit_tuv(so, sd, tmin, tmax, rec["v0"][None], rec["e1"][None], rec["e2"][None], rec["lo"][None], rec["hi"][None])
            r, i = np.nonzero(ok)
            ri.append(r + s)
            ti.append(i)
            tt.append(t[r, i])
    if not ri:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, F32)
    return np.concatenate(ri), np.concatenate(ti), np.concatenate(tt)
