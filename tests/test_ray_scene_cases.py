"""The ray query on constructed scenes and far rays, without a GPU (tests/ray_scene_cases.py has the scenes and the rays,
tests/ray_walk_reference.py the node test restated; tests/test_ray_scene_cases_gpu.py holds the kernels to the brute force on the
same cases).

  - vkr_accel_layout on every new scene: the assertions of test_accel.py::test_layout_hierarchy with `nested` sharpened to `the exact
    union` (ray_scene_cases.check_layout), `deep` at the depth cap with a leaf of more than ACCEL_MAX_LEAF triangles there,
    area_overflow halved, the float grid of offset_2p20 making zero-area triangles, nonfinite_vertices deterministic.
  - the reach property: no triangle the frozen test accepts lies below a node the node test refuses, on every scene, ray class and
    range, under the segment box alone, with the slab term up to tmax, and with the slab term up to the winner's t.
  - the classes are not vacuous (hit counts per class and k are printed), and the mutants of the restatement.
  - the restatement decides as LaneRay::enters compiled for the host does, on 64 hand-picked (ray, node) pairs.

What the mutants show.  A mutant is UNSOUND when the reach property catches it losing a hit, and merely NOT THE CODE when it
loses none but decides differently from the compiled enters on a named pair of the 64.
  1  margin = 0 and no outward step   unsound: far_origin loses hits from k = 13 on a scene of a few units (duplicates_reversed; k = 16
                                      on procedural, 20 on box, 8 on mixed_scale, every k on deep), far_axis from k = 13.  No class of
                                      tests/test_accel_occluded_gpu.py catches it on its scenes.
  7  node boxes from unwidened boxes  unsound: vertex_tmax, edge_tmax and the far classes at every k.
  2  margin = 0 alone                 not the code (pair graze_2p5, graze_1p5).  No hit is lost on any case here, and none can be where
  3  no outward step alone            not the code (pair far_just_below_tmin, graze_2p5).  the rounding is absolute: an accepted hit point
                                      lies on its triangle to a few ulps of the RAY's coordinates, the node box is wider than the triangle
                                      by 2^-12 of the TRIANGLE's, and once the ray's are 2^12 times larger the ray is long, t d_k is of the
                                      size of o_k, the error is relative to t and either protection alone covers it (6 u against 16 u
                                      and 8 u).  Mutant 1 shows that one of the two is needed; these two that either one suffices.
  4  slab_reciprocal without its gate not the code (pair huge_components_disjoint_slabs: it culls a true miss the code visits).  1 / 0 = inf
                                      gives (x - margin) * inf = +-inf on the right side (the margin keeps x - margin from 0), and an
                                      infinity on the wrong side turns into NaN in the outward step: the gate makes the proof short,
                                      the NaN rule makes the walk safe.
  5  rejects on tn >= tf              not the code (pair far_16_ulps_below_tmin).  After the outward step tn == tf needs the raw sides to
                                      be 32 u apart while a hit keeps them within 12.4 u (steps 4 - 5 of the proof).
  6  NaN-propagating segment corners  not the code (pair nan_corner_infinite_box).  A corner is NaN only for a NaN or infinite origin
                                      or direction, and the frozen test accepts nothing for such a ray.
  8  reach as a maximum               not the code (pair graze_2p5).  Step 3 of the proof needs margin >= 6.2 u M and the maximum still
                                      gives 8 u M; the sum is there for the infinities and NaN it hands to the margin.
  9  entry side from the sign of d    EXEMPT, the one equivalent mutant: the two signs differ only where the reciprocal is NaN, and then
                                      both slab parameters of the axis are NaN whichever side was chosen.  No input separates them.
So two mutants are unsound, six are sound and pinned to the code by a named pair, one is equivalent; the rule "killed by a ray class
or exempt, at most two exempt" cannot be met by lost hits alone, because six of the nine steps are redundant protections.
"""
import functools
import shutil
import subprocess

import numpy as np
import pytest

import gtao_rt_reference as gref
import ray_scene_cases as cs
import ray_walk_reference as rw
from ray_scene_cases import F32, MISS

NEW = sorted(cs.NEW_SCENES)
ALL = sorted(cs.ALL_SCENES)
# the ranges of tests/test_accel_occluded_gpu.py that RANGES does not hold, on its own scenes
OLD_RANGES = ((0.5, 0.5), (1.0, 1.0), (0.75, 0.25), (-0.5, 1.5))
NON_VACUOUS = ("box", "procedural", "offset_2p13", "mixed_scale", "duplicates_reversed")


@functools.lru_cache(maxsize=None)
def _layout(name):
    return cs.check_layout(cs.case(name).tris)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- the build ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW)
def test_layout_invariants(name):
    c = cs.case(name)
    lay = _layout(name)
    leaves = lay.nodes["count"] > 0
    print(f"[ray scenes] {name}: {len(c.tris)} triangles, {len(lay.nodes)} nodes, depth {lay.max_depth}, largest leaf {int(lay.nodes['count'].max())}, {len(c.o)} rays")
    assert lay.max_depth <= cs.MAX_DEPTH < cs.STACK
    assert (lay.leaf_of >= 0).all() and leaves[lay.leaf_of].all()
    if np.isfinite(c.tris).all():  # the host's records are those of the shared reference wherever it defines them
        want = gref.triangle_records(c.tris)
        for f in ("v0", "e1", "e2", "lo", "hi"):
            assert np.array_equal(_bits(c.rec[f]), _bits(want[f])), f


def test_deep_reaches_the_depth_cap():
    lay = _layout("deep")
    assert lay.max_depth == cs.MAX_DEPTH == 48
    at_cap = np.nonzero((lay.depth == cs.MAX_DEPTH) & (lay.nodes["count"] > 0))[0]
    counts = lay.nodes["count"][at_cap]
    print(f"[ray scenes] deep: leaves at depth 48 hold {counts.tolist()} triangles; one stack entry per level: 48 of {cs.STACK}")
    assert (counts > cs.MAX_LEAF).any(), "no leaf at the cap holds more than ACCEL_MAX_LEAF triangles"
    assert (lay.nodes["count"][lay.depth < cs.MAX_DEPTH] <= cs.MAX_LEAF).all(), "above the cap no leaf is larger than ACCEL_MAX_LEAF"
    tris = cs.case("deep").tris
    assert len(np.unique(tris.reshape(-1, 9), axis=0)) == len(tris), "the triangles are distinct"


def test_area_overflow_is_halved():
    """every node whose area() overflows holds its records in their order of arrival, cut at n / 2"""
    c, lay = cs.case("area_overflow"), _layout("area_overflow")
    halved = 0
    for i in range(len(lay.nodes)):
        nd = lay.nodes[i]
        with np.errstate(all="ignore"):
            e = np.maximum(nd["hi"] - nd["lo"], F32(0))
            area = e[0] * e[1] + e[1] * e[2] + e[2] * e[0]
        if not np.isinf(area):
            continue
        recs = lay.subtree_records(i)
        n = len(recs)
        if nd["count"]:
            assert n <= cs.MAX_LEAF
            continue
        halved += 1
        assert len(lay.subtree_records(int(nd["first"]))) == n // 2, f"node {i} of {n} triangles is not cut at n / 2"
    assert halved >= 3 and np.isinf(area_of_root(lay))
    # at the root the order of arrival is the input order
    assert lay.recs["index"].tolist() == list(range(len(c.tris)))


def area_of_root(lay):
    with np.errstate(all="ignore"):
        e = lay.nodes["hi"][0] - lay.nodes["lo"][0]
        return e[0] * e[1] + e[1] * e[2] + e[2] * e[0]


def test_offset_2p20_collapses_onto_the_float_grid():
    tris = cs.case("offset_2p20").tris
    e1, e2 = (tris[:, 1] - tris[:, 0]).astype(np.float64), (tris[:, 2] - tris[:, 0]).astype(np.float64)
    zero_area = int((np.linalg.norm(np.cross(e1, e2), axis=1) == 0).sum())
    duplicates = len(tris) - len(np.unique(tris.reshape(-1, 9), axis=0))
    print(f"[ray scenes] offset_2p20: {zero_area} zero-area triangles, {duplicates} duplicates of {len(tris)}")
    # 36 of 112 collapse to zero area; no two triangles of this mesh collapse onto each other (duplicates_reversed has the duplicates)
    assert zero_area > 0 and duplicates == 0


def test_nonfinite_vertices_are_what_the_scene_says():
    c = cs.case("nonfinite_vertices")
    bad = ~np.isfinite(c.tris).all(axis=(1, 2))
    assert int(bad.sum()) == cs.NONFINITE_COUNT and set(np.nonzero(bad)[0]) == set(cs.nonfinite_changed().tolist())
    assert np.isnan(c.tris).any() and np.isposinf(c.tris).any() and np.isneginf(c.tris).any()
    assert np.isnan(c.tris[bad]).all(axis=(1, 2)).any(), "a whole NaN triangle"
    base = cs.base_closest("nonfinite_vertices")
    won = np.isin(base["index"], np.nonzero(bad)[0])
    print(f"[ray scenes] nonfinite_vertices: {int(won.sum())} rays are won by a triangle with a vertex that is not finite")
    assert not np.isin(base["index"], np.nonzero(np.isnan(c.tris).any(axis=(1, 2)))[0]).any(), "NaN is a miss"


# ---- the reach property -----------------------------------------------------------------------------------------------------------
def _ranges(name):
    return cs.ranges(name) + (list(OLD_RANGES) if name in cs.OLD_SCENES else [])


def _winner_t(ri, tt, n):
    """per accepted pair, whether its t is the smallest of its ray (==, so -0 == +0), and that t per ray"""
    key = (tt + F32(0.0)).astype(F32)
    best = np.full(n, np.inf, F32)
    np.minimum.at(best, ri, key)
    return key == best[ri], best


def _lost(name, tmin, tmax, variant=rw.CODE, node_boxes=None):
    """the accepted (ray, triangle) pairs of a case whose leaf the node test does not reach -> (box, slab to tmax, slab to the winner's
    t) as arrays of ray numbers, and the Reach of the rays that hit anything"""
    c, lay = cs.case(name), cs.Layout(cs.case(name).tris)
    ri, ti, tt = cs.candidates(c.o, c.d, tmin, tmax, c.rec)
    if len(ri) == 0:
        return (np.zeros(0, np.int64),) * 3, None
    rays, inv = np.unique(ri, return_inverse=True)
    wins, best = _winner_t(inv, tt, len(rays))
    lo, hi = (lay.nodes["lo"], lay.nodes["hi"]) if node_boxes is None else node_boxes(lay, c.tris)
    reach = rw.Reach(lo, hi, lay.parent, rw.Rays(c.o[rays], c.d[rays], tmin, tmax, variant), [F32(tmax), best])
    lost = (rays[inv[rw.violations(reach.box, lay.leaf_of, inv, ti)]], rays[inv[rw.violations(reach.slab[0], lay.leaf_of, inv, ti)]],
            rays[inv[wins][rw.violations(reach.slab[1], lay.leaf_of, inv[wins], ti[wins])]])
    return lost, reach


@pytest.mark.parametrize("name", ALL)
def test_reach_property(name):
    """0 violations of the unmutated restatement: a violation would be a defect of the cull itself"""
    c = cs.case(name)
    for tmin, tmax in _ranges(name):
        lost, reach = _lost(name, tmin, tmax)
        if reach is not None:
            print(f"[ray scenes] {name} t in [{tmin}, {tmax}]: {reach.box.shape[1]} rays hit; of {reach.tests} node tests the slab term rejects "
                  f"{reach.slab_rejects}, NaN accepts {reach.nan_accepts}, axes off {reach.axes_off}")
        for what, rays in zip(("the segment box", "the slab term to tmax", "the slab term to the winner's t"), lost):
            assert len(rays) == 0, f"{name}, t in [{tmin}, {tmax}]: {what} loses {len(rays)} hits, e.g. {[(int(r), str(c.tag[r]), int(c.k[r])) for r in rays[:6]]}"
        if tmin > tmax:
            assert reach is None, "an empty parameter range hits nothing"


def test_the_winner_is_the_reference_winner():
    """the candidates the property is checked on are those of the shared brute force: same winners, prefilter or not"""
    for name in ("nonfinite_vertices", "offset_2p20", "deep"):
        c, base = cs.case(name), cs.base_closest(name)
        ri, ti, tt = cs.candidates(c.o, c.d, 0.0, 1.0, c.rec)
        wins, best = _winner_t(ri, tt, len(c.o))
        index = np.full(len(c.o), MISS, np.uint32)
        np.minimum.at(index, ri[wins], ti[wins].astype(np.uint32))
        assert np.array_equal(index, base["index"]), name
        hit = index != MISS
        assert np.array_equal(best[hit], (base["t"][hit] + F32(0.0)).astype(F32)), name


# ---- the classes are not vacuous ------------------------------------------------------------------------------------------------
def _counts(name, hit):
    c = cs.case(name)
    return {cl: {k: (int(hit[(c.tag == cl) & (c.k == k)].sum()), int(((c.tag == cl) & (c.k == k)).sum())) for k in cs.K} for cl in cs.FAR}


@pytest.mark.parametrize("name", [n for n in ALL if n != "empty"])
def test_far_classes_hit_and_miss(name):
    c, base = cs.case(name), cs.base_closest(name)
    hit = base["index"] != MISS
    counts = _counts(name, hit)
    for cl in cs.FAR:
        print(f"[ray scenes] {name} {cl}: hits / rays per k " + ", ".join(f"{k}: {h}/{n}" for k, (h, n) in counts[cl].items()))
    if name in NON_VACUOUS:
        for cl in cs.FAR:
            for k in (8, 13):
                h, n = counts[cl][k]
                assert 0 < h < n, f"{name} {cl} k = {k}: {h} hits of {n} rays"
    # k = 24: the origin's grid is coarser than the scene, and the frozen test's own box clause decides; recorded, not required
    far_end_t = base["t"][hit & (c.tag == "far_end")]
    if name in NON_VACUOUS:
        assert (far_end_t < 2.0 ** -6).any(), "far_end hits sit at small t"


def test_duplicates_reversed_ties():
    c, base = cs.case("duplicates_reversed"), cs.base_closest("duplicates_reversed")
    n = len(c.tris) // 2
    ri, ti, tt = cs.candidates(c.o, c.d, 0.0, 1.0, c.rec)
    wins, _ = _winner_t(ri, tt, len(c.o))
    ties = np.bincount(ri[wins], minlength=len(c.o))
    hit = base["index"] != MISS
    assert hit.sum() > 1000 and (ties[hit] >= 2).all(), "every hit is a tie"
    assert (base["index"][hit] < n).all(), "the winner is the copy with the lower input index"
    # its twin lies at 2 n - 1 - index, elsewhere in the tree
    lay = _layout("duplicates_reversed")
    twin = 2 * n - 1 - base["index"][hit].astype(np.int64)
    apart = lay.leaf_of[twin] != lay.leaf_of[base["index"][hit]]
    first = np.array([int(np.nonzero(lay.recs["index"] == i)[0][0]) for i in range(2 * n)])
    before = first[base["index"][hit]] < first[twin]
    print(f"[ray scenes] duplicates_reversed: {int(hit.sum())} hits, all ties; {int(apart.sum())} with the twin in another leaf, {int(before.sum())} with the winner's record first")
    # Recorded: equal boxes have equal centroids, which no plane parts and the stable partition keeps in input order, so the twins share
    # a leaf with the lower index first.  What the scene holds the walks to is the tie rule itself (t == t_best never replaces a lower
    # index, and with cutouts a hole in the lower copy hands the hit to the higher one: tests/test_ray_scene_cases_gpu.py).
    assert not apart.any() and before.all()


def _all_ray_reach(name, tmin=0.0, tmax=1.0, sel=None):
    c, lay = cs.case(name), _layout(name)
    sel = np.ones(len(c.o), bool) if sel is None else sel
    return rw.Reach(lay.nodes["lo"], lay.nodes["hi"], lay.parent, rw.Rays(c.o[sel], c.d[sel], tmin, tmax), [F32(tmax)])


def test_slab_counters():
    """on slivers every node box covers the scene and the cull rejects little; under far_origin on the offset scenes it works"""
    got = {}
    for name in ("slivers", "procedural", "offset_2p13", "offset_2p20"):
        c = cs.case(name)
        r = _all_ray_reach(name, sel=c.tag == "long")
        f = _all_ray_reach(name, sel=c.tag == "far_origin")
        got[name] = (r.slab_rejects / max(r.tests, 1), f.slab_rejects)
        print(f"[ray scenes] {name}: the slab term rejects {r.slab_rejects} of {r.tests} node tests of `long` the segment box accepts, {f.slab_rejects} of {f.tests} of far_origin")
    assert got["slivers"][0] < 0.25 * got["procedural"][0], "the cull rejects little where every box covers the scene"
    assert got["offset_2p13"][1] > 0 and got["offset_2p20"][1] > 0


# ---- the mutants ------------------------------------------------------------------------------------------------------------------
def _tight_boxes(lay, tris):
    """node boxes recomputed from the triangles' own boxes, without the widening"""
    n = len(lay.nodes)
    lo, hi = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    for i in range(n - 1, -1, -1):
        nd = lay.nodes[i]
        if nd["count"]:
            v = tris[lay.recs["index"][nd["first"]:nd["first"] + nd["count"]]].reshape(-1, 3)
            lo[i], hi[i] = np.fmin.reduce(v, axis=0), np.fmax.reduce(v, axis=0)
        else:
            f = int(nd["first"])
            lo[i], hi[i] = np.fmin(lo[f], lo[f + 1]), np.fmax(hi[f], hi[f + 1])
    return lo, hi


MUTANTS = {
    1: (rw.Variant(margin=False, outward=False), None),
    2: (rw.Variant(margin=False), None),
    3: (rw.Variant(outward=False), None),
    4: (rw.Variant(guard=False), None),
    5: (rw.Variant(strict=False), None),
    6: (rw.Variant(fmin_rule=False), None),
    7: (rw.CODE, _tight_boxes),
    8: (rw.Variant(reach_sum=False), None),
    9: (rw.Variant(side_of_reciprocal=False), None),
}
UNSOUND = {1: {("far_origin", 13), ("far_origin", 16), ("far_axis", 13)}, 7: {("vertex_tmax", -1), ("edge_tmax", -1), ("far_origin", 8), ("far_axis", 8)}}
NOT_THE_CODE = {2: ("graze_2p5", "graze_1p5"), 3: ("far_just_below_tmin", "graze_2p5"), 4: ("huge_components_disjoint_slabs",), 5: ("far_16_ulps_below_tmin",),
                6: ("nan_corner_infinite_box",), 8: ("graze_2p5",)}
EXEMPT = {9: "equivalent: the signs of d and of its reciprocal differ only where the reciprocal is NaN, and then the axis is off for either side"}
MUTANT_SCENES = ("box", "procedural", "offset_2p13", "offset_2p20", "scale_2m40", "mixed_scale", "duplicates_reversed", "deep", "nonfinite_vertices")


@functools.lru_cache(maxsize=None)
def _kills(number):
    """the (class, k) of the rays whose hits the mutant loses under a slab walk, per scene, for t in [0, 1]"""
    variant, boxes = MUTANTS[number]
    out = {}
    for name in MUTANT_SCENES:
        c = cs.case(name)
        lost, _ = _lost(name, 0.0, 1.0, variant, boxes)
        rays = np.concatenate(lost[1:]) if boxes is None else np.concatenate(lost)
        out[name] = sorted(set((str(c.tag[r]), int(c.k[r])) for r in rays))
    return out


def test_partition_of_the_mutants():
    assert sorted(list(UNSOUND) + list(NOT_THE_CODE) + list(EXEMPT)) == list(range(1, 10)) and len(EXEMPT) <= 2
    assert all(EXEMPT.values())


@pytest.mark.parametrize("number", sorted(UNSOUND))
def test_unsound_mutants_lose_hits(number):
    kills = _kills(number)
    killed = set().union(*kills.values())
    for name, classes in kills.items():
        print(f"[ray scenes] mutant {number} on {name}: loses hits of {classes}")
    assert UNSOUND[number] <= killed, f"mutant {number} survives {sorted(UNSOUND[number] - killed)}"
    if number == 1:
        # what proves the far classes sharp: the classes of tests/test_accel_occluded_gpu.py alone do not catch it on a scene near the origin
        old = {cl for name in ("box", "procedural", "duplicates_reversed") for cl, k in kills[name] if cl not in cs.FAR}
        assert not old, old
        first = {name: min((k for cl, k in classes if cl == "far_origin"), default=None) for name, classes in kills.items()}
        print(f"[ray scenes] mutant 1: the smallest k at which far_origin loses a hit, |o| = 2^k scene extents: {first}")
        assert first["duplicates_reversed"] == 13 and first["procedural"] in (13, 16) and first["deep"] == 8


@pytest.mark.parametrize("number", sorted(list(NOT_THE_CODE) + list(EXEMPT)))
def test_sound_mutants_lose_no_hit(number):
    """recorded, not wished for: these mutants pass the reach property on every scene (the module docstring says why), so what
    pins their step of the restatement to the code is the compiled node test below"""
    kills = _kills(number)
    assert not any(kills.values()), f"mutant {number} does lose hits: {kills}: move it to UNSOUND"


# ---- the restatement is the code ------------------------------------------------------------------------------------------------
ENTERS_CPP = r"""
// LaneRay<SLAB>::enters of csrc/accel_traverse.hpp as plain host C++; reads 17 hex words per line (o, d, tmin, tmax, lo, hi, t_far)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
struct f3 { float x, y, z; };
struct node { float lo[3], hi[3]; };
static float as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static float slab_reciprocal(float d) { const float m = fabsf(d); return (m >= 0x1p-100f && m <= 0x1p100f) ? 1.0f / d : as_float(0x7FC00000u); }
static float slab_keep_max(float acc, float x) { return x > acc ? x : acc; }
static float slab_keep_min(float acc, float x) { return x < acc ? x : acc; }
template <bool SLAB> struct LaneRay {
  float lox, loy, loz, hix, hiy, hiz; f3 o; float tmin, ix, iy, iz, mx, my, mz; bool px, py, pz;
  LaneRay(f3 o_, f3 d, float tmin_, float tmax) {
    const float ax = o_.x + tmin_ * d.x, ay = o_.y + tmin_ * d.y, az = o_.z + tmin_ * d.z;
    const float bx = o_.x + tmax * d.x, by = o_.y + tmax * d.y, bz = o_.z + tmax * d.z;
    lox = fminf(ax, bx); loy = fminf(ay, by); loz = fminf(az, bz);
    hix = fmaxf(ax, bx); hiy = fmaxf(ay, by); hiz = fmaxf(az, bz);
    o = o_; tmin = tmin_;
    const float reach = (((fabsf(o.x) + fabsf(o.y)) + (fabsf(o.z) + fabsf(ax))) + ((fabsf(ay) + fabsf(az)) + (fabsf(bx) + fabsf(by)))) + fabsf(bz);
    const float margin = reach * 0x1p-21f + 0x1p-126f;
    ix = slab_reciprocal(d.x); iy = slab_reciprocal(d.y); iz = slab_reciprocal(d.z);
    px = ix > 0.0f; py = iy > 0.0f; pz = iz > 0.0f;
    mx = px ? margin : -margin; my = py ? margin : -margin; mz = pz ? margin : -margin;
  }
  bool enters(const node nd, bool live, float t_far) const {
    bool overlap = live && lox <= nd.hi[0] && hix >= nd.lo[0] && loy <= nd.hi[1] && hiy >= nd.lo[1] && loz <= nd.hi[2] && hiz >= nd.lo[2];
    if (SLAB) {
      const float nx = (((px ? nd.lo[0] : nd.hi[0]) - o.x) - mx) * ix, fx = (((px ? nd.hi[0] : nd.lo[0]) - o.x) + mx) * ix;
      const float ny = (((py ? nd.lo[1] : nd.hi[1]) - o.y) - my) * iy, fy = (((py ? nd.hi[1] : nd.lo[1]) - o.y) + my) * iy;
      const float nz = (((pz ? nd.lo[2] : nd.hi[2]) - o.z) - mz) * iz, fz = (((pz ? nd.hi[2] : nd.lo[2]) - o.z) + mz) * iz;
      float tn = slab_keep_max(slab_keep_max(slab_keep_max(tmin, nx), ny), nz);
      float tf = slab_keep_min(slab_keep_min(slab_keep_min(t_far, fx), fy), fz);
      tn = tn - (fabsf(tn) * 0x1p-20f + 0x1p-126f);
      tf = tf + (fabsf(tf) * 0x1p-20f + 0x1p-126f);
      if (tn > tf) overlap = false;
    }
    return overlap;
  }
};
int main() {
  uint32_t w[17];
  for (;;) {
    for (int i = 0; i < 17; i++) if (scanf("%x", &w[i]) != 1) return 0;
    float v[17];
    for (int i = 0; i < 17; i++) v[i] = as_float(w[i]);
    const f3 o = {v[0], v[1], v[2]}, d = {v[3], v[4], v[5]};
    const node nd = {{v[8], v[9], v[10]}, {v[11], v[12], v[13]}};
    printf("%d %d\n", (int)LaneRay<true>(o, d, v[6], v[7]).enters(nd, true, v[16]), (int)LaneRay<false>(o, d, v[6], v[7]).enters(nd, true, v[16]));
  }
}
"""

NAN, INF = float("nan"), float("inf")
UNIT = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def _pair(o=(0.25, 0.5, -0.25), d=(1.0, 2.0, 3.0), tmin=0.0, tmax=1.0, box=UNIT, t_far=None):
    return dict(o=o, d=d, tmin=tmin, tmax=tmax, lo=box[0], hi=box[1], t_far=tmax if t_far is None else t_far)


def _graze(gap):
    """the ray from 0 along (1024, 1024, 0) beside a box that ends `gap` * 2^-10 below the line in y where the ray enters it in x at
    t = 1 / 2: margin is 2^-10 as a sum and 2^-11 as a maximum, and the outward step is worth 2^-10 here"""
    return _pair(o=(0.0, 0.0, 0.0), d=(1024.0, 1024.0, 0.0), box=((512.0, 500.0, -1.0), (513.0, 512.0 - gap * 2.0 ** -10, 1.0)))


def pairs():
    """the 64 hand-picked (ray, node) pairs, by name"""
    p = {"base": _pair(), "away": _pair(d=(-1.0, -2.0, -3.0), o=(3.0, 3.0, 3.0), tmax=0.5)}
    for name, v in (("nan", NAN), ("inf", INF), ("minus_inf", -INF), ("zero", 0.0), ("minus_zero", -0.0), ("denormal", 1e-41), ("minus_denormal", -1e-41),
                    ("below_the_gate", 2.0 ** -101), ("at_the_gate", 2.0 ** -100), ("top_of_the_gate", 2.0 ** 100)):
        p[f"dx_{name}"] = _pair(d=(v, 2.0, 3.0))
        if "gate" not in name:
            p[f"dz_{name}_from_outside"] = _pair(o=(0.25, -3.0, 0.5), d=(0.125, 4.0, v))
    for name, v in (("nan", NAN), ("inf", INF), ("minus_inf", -INF), ("zero", 0.0), ("minus_zero", -0.0)):
        p[f"oy_{name}"] = _pair(o=(0.25, v, -0.25))
    # the origin on a slab plane with a zero component: 0 * inf without the gate and the margin
    p["on_plane_zero"] = _pair(o=(-1.0, 0.0, 0.0), d=(0.0, 1.0, 0.0))
    p["on_plane_minus_zero"] = _pair(o=(1.0, 0.0, 0.0), d=(-0.0, 1.0, 0.0))
    p["beside_plane_zero"] = _pair(o=(-1.0 - 2.0 ** -10, 0.0, 0.0), d=(0.0, 1.0, 0.0))
    p["zero_direction_inside"] = _pair(d=(0.0, 0.0, 0.0))
    p["zero_direction_outside"] = _pair(o=(2.0, 0.0, 0.0), d=(0.0, 0.0, -0.0))
    # two components above the gate whose slabs are disjoint (t in [2^-109, 2^-108] and in [2^-111, 2^-110]): both axes are off
    p["huge_components_disjoint_slabs"] = _pair(o=(3.0, -3.0, 0.0), d=(-2.0 ** 110, 2.0 ** 112, 0.0), tmax=2.0 ** -100)
    p["huge_component"] = _pair(o=(-3.0, 0.0, 0.0), d=(2.0 ** 101, 1.0, 0.0))
    p["overflowed_corner"] = _pair(d=(1e30, -1e30, 1.0), tmax=1e10)
    # the range
    p["tmin_above_tmax"] = _pair(tmin=0.75, tmax=0.25)
    p["tmin_is_tmax"] = _pair(tmin=0.5, tmax=0.5)
    p["far_is_tmin"] = _pair(tmin=0.25, t_far=0.25)
    p["far_just_below_tmin"] = _pair(o=(0.0, 0.0, 0.0), d=(0.25, 0.25, 0.25), tmin=1.0, tmax=2.0, t_far=1.0 - 2.0 ** -24)
    p["far_16_ulps_below_tmin"] = _pair(o=(0.0, 0.0, 0.0), d=(0.25, 0.25, 0.25), tmin=1.0, tmax=2.0, t_far=1.0 - 2.0 ** -19)
    p["far_well_below_tmin"] = _pair(o=(0.0, 0.0, 0.0), d=(0.25, 0.25, 0.25), tmin=1.0, tmax=2.0, t_far=0.5)
    p["far_zero_from_zero"] = _pair(t_far=0.0)
    p["tmin_nan"] = _pair(tmin=NAN)
    p["tmax_nan"] = _pair(tmax=NAN)
    p["far_nan"] = _pair(t_far=NAN)
    p["tmax_inf"] = _pair(tmax=INF)
    p["negative_range"] = _pair(tmin=-0.5, tmax=1.5)
    # the box
    flat = ((-1.0, -1.0, 0.5), (1.0, 1.0, 0.5))
    p["flat_box_crossed"] = _pair(box=flat)
    p["flat_box_in_its_plane"] = _pair(o=(-2.0, 0.0, 0.5), d=(4.0, 0.0, 0.0), box=flat)
    p["flat_box_beside_its_plane"] = _pair(o=(-2.0, 0.0, 0.5 + 2.0 ** -8), d=(4.0, 0.0, 0.0), box=flat)
    p["flat_box_missed"] = _pair(o=(-2.0, 3.0, 0.0), d=(4.0, 0.0, 1.0), box=flat)
    p["point_box"] = _pair(o=(-1.0, -1.0, -1.0), d=(2.0, 2.0, 2.0), box=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))
    p["empty_box"] = _pair(box=((INF, INF, INF), (-INF, -INF, -INF)))
    p["infinite_box"] = _pair(box=((-INF, -INF, -INF), (INF, INF, INF)))
    p["half_infinite_box_missed"] = _pair(o=(0.0, 5.0, 0.0), d=(1.0, 0.0, 0.0), box=((-1.0, -1.0, -1.0), (INF, 1.0, 1.0)))
    p["nan_corner_infinite_box"] = _pair(o=(0.0, 0.0, 0.0), d=(INF, 0.5, 0.5), box=((-1.0, -1.0, -1.0), (INF, 1.0, 1.0)))
    p["nan_corner_finite_box"] = _pair(o=(0.0, 0.0, 0.0), d=(INF, 0.5, 0.5))
    # beside a box by less and by more than the protections cover
    for gap in (0.5, 1.5, 2.5, 3.5):
        p["graze_" + str(gap).replace(".", "p")] = _graze(gap)
    # far origins and far ends
    p["far_origin_hits"] = _pair(o=(2.0 ** 20, 2.0 ** 19, -2.0 ** 20), d=(-2.0 ** 20, -2.0 ** 19, 2.0 ** 20))
    p["far_origin_ends_short"] = _pair(o=(2.0 ** 20, 2.0 ** 19, -2.0 ** 20), d=(-2.0 ** 20, -2.0 ** 19, 2.0 ** 20), tmax=1.0 - 2.0 ** -18)
    p["far_origin_on_axis"] = _pair(o=(0.5, -2.0 ** 24, 0.5), d=(0.0, 2.0 ** 24, 0.0))
    p["far_origin_passes"] = _pair(o=(2.0 ** 20, 2.0 ** 19, -2.0 ** 20), d=(-2.0 ** 20, -2.0 ** 19 + 8.0, 2.0 ** 20))
    p["far_end"] = _pair(d=(2.0 ** 24, 2.0 ** 25, -2.0 ** 24))
    p["tiny_box_tiny_ray"] = _pair(o=(0.0, 0.0, 0.0), d=(2.0 ** -120, 2.0 ** -121, 0.0), box=((2.0 ** -121, 0.0, -0.0), (2.0 ** -120, 2.0 ** -122, 0.0)))
    return p


@functools.lru_cache(maxsize=None)
def _compiled_enters(tmp):
    cxx = shutil.which("g++")
    if cxx is None:
        return None
    src, exe = f"{tmp}/enters.cpp", f"{tmp}/enters"
    open(src, "w").write(ENTERS_CPP)
    subprocess.run([cxx, "-std=c++17", "-O0", "-ffp-contract=off", "-o", exe, src], check=True)
    return exe


def _words(p):
    v = np.array([*p["o"], *p["d"], p["tmin"], p["tmax"], *p["lo"], *p["hi"], 0.0, 0.0, p["t_far"]], np.float64)
    with np.errstate(all="ignore"):
        w = v.astype(F32).view(np.uint32)
    nan = np.isnan(v)
    w[nan] = 0x7FC00000
    return w


def _restated(p, variant=rw.CODE):
    rays = rw.Rays(np.array([p["o"]], F32), np.array([p["d"]], F32), p["tmin"], p["tmax"], variant)
    lo, hi = np.array(p["lo"], F32), np.array(p["hi"], F32)
    return bool(rw.enters(rays, lo, hi, F32(p["t_far"]))[0]), bool(rw.enters(rays, lo, hi, F32(p["t_far"]), slab=False)[0])


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    exe = _compiled_enters(str(tmp_path_factory.mktemp("enters")))
    if exe is None:
        pytest.skip("no g++ to compile the node test with")
    cases = pairs()
    text = "\n".join(" ".join(f"{int(x):08x}" for x in _words(p)) for p in cases.values())
    out = subprocess.run([exe], input=text + "\n", capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == 2 * len(cases)
    return {name: (out[2 * i] == "1", out[2 * i + 1] == "1") for i, name in enumerate(cases)}


def test_the_restatement_decides_as_the_compiled_node_test(compiled):
    cases = pairs()
    assert len(cases) == 64
    for name, p in cases.items():
        assert _restated(p) == compiled[name], f"{name}: the restatement says {_restated(p)}, the compiled enters {compiled[name]} (slab, segment box)"
    slab = [v[0] for v in compiled.values()]
    print(f"[ray scenes] the compiled node test enters {sum(slab)} of {len(slab)} pairs; the segment box alone {sum(v[1] for v in compiled.values())}")
    assert 16 <= sum(slab) <= 48
    # what the named pairs are there for
    assert compiled["graze_0p5"][0] and compiled["graze_2p5"][0] and not compiled["graze_3p5"][0] and compiled["graze_3p5"][1]
    assert compiled["far_just_below_tmin"][0] and compiled["far_16_ulps_below_tmin"][0] and not compiled["far_well_below_tmin"][0]
    assert compiled["huge_components_disjoint_slabs"][0] and compiled["nan_corner_infinite_box"][0] and not compiled["nan_corner_finite_box"][0]
    assert not compiled["tmin_above_tmax"][0] and compiled["tmin_nan"][0] == compiled["tmin_nan"][1]


@pytest.mark.parametrize("number", sorted(NOT_THE_CODE))
def test_sound_mutants_are_not_the_code(compiled, number):
    cases = pairs()
    for name in NOT_THE_CODE[number]:
        assert _restated(cases[name], MUTANTS[number][0])[0] != compiled[name][0], f"mutant {number} decides as the code on {name}"


def test_the_equivalent_mutant_is_equivalent(compiled):
    cases = pairs()
    for name, p in cases.items():
        assert _restated(p, MUTANTS[9][0]) == compiled[name], name
