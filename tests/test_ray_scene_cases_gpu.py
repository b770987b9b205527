"""The ray-level entries of the ray query on the constructed scenes and far rays of tests/ray_scene_cases.py, on the GPU: every answer
must be that of the numpy brute force of the frozen triangle test, bit for bit.

Which entry runs which walk (csrc/accel_traverse.hpp):
  vkr_accel_query            wave_any_hit        the any-hit walk under the segment box alone
  vkr_accel_occluded         wave_any_hit_ray    the any-hit walk with the slab term up to tmax
  vkr_accel_closest          wave_closest_hit    the closest-hit walk, children in stored order, the slab term up to t_best
  vkr_accel_occluded_cutout  wave_any_hit_walk<true, CutoutFilter>
  vkr_accel_closest_cutout   wave_closest_hit_walk<false, CutoutFilter>
wave_closest_hit_ordered (children ordered by the lanes that enter them) is reached by no entry of the library: only
tools/reflections_rt_timing.py builds csrc/accel_closest.hip a second time on it, and checks there that both walks give the same
bytes.  It is not run here.

Per new scene, over all its rays (those of tests/test_accel_occluded_gpu.py, far_origin, far_axis, far_end, last_subtree) and the
ranges (0, 1), (1e-12, 1), (0.25, 0.75), (0, 1e10) and tmin == tmax at the t of a far_origin hit: the any hit of both entries equals
the brute force for every ray; all four words of every closest record equal; `index != miss` equals the any-hit answer; a miss is
(0, 0, 0, 0xFFFFFFFF); guard words behind the last ray stay.  The cutout entries on offset_2p13 and duplicates_reversed against
tests/ray_cutout_reference.py, with the textures and attribute conventions of tests/ray_cutout_cases.py; on duplicates_reversed a hole
in the lower-index copy hands the hit to the higher one at the same t.  Batches of 1, 63, 64, 65 and 257 rays on deep and offset_2p20.

One structure per scene is built once per module.  Before anything is launched the layout is checked on the host: its depth, one
stack entry per level, stays below the 64 entries of a wave's stack (deep: 48).
"""
import numpy as np
import pytest

from vk_renderer_amd import abi

import closest_hit_reference as closest
import gtao_rt_reference as gref
import ray_cutout_cases as cut
import ray_cutout_reference as cutref
import ray_scene_cases as cs
from test_accel_closest_gpu import _compare as _compare_closest
from test_accel_closest_gpu import _run
from test_accel_occluded_gpu import _both
from test_accel_occluded_gpu import _compare as _compare_any
from test_ray_cutout_gpu import _arith, _same_bits, _textures
from test_ray_cutout_gpu import _run as _run_cutout

pytestmark = pytest.mark.gpu

F32 = np.float32
MISS = closest.MISS
NEW = sorted(cs.NEW_SCENES)


@pytest.fixture(scope="module")
def accels():
    """name -> abi.Accel, built on first use after the host check of the stack bound, closed with the module"""
    made = {}

    def get(name):
        if name not in made:
            tris = cs.case(name).tris
            depth = cs.Layout(tris).max_depth
            assert depth <= cs.MAX_DEPTH < cs.STACK, f"{name}: a walk would need {depth} stack entries"
            made[name] = abi.Accel(tris)
            assert made[name].info()[1] == len(tris)
        return made[name]

    yield get
    for a in made.values():
        a.close()


def _any(o, d, tmin, tmax, rec):
    with np.errstate(all="ignore"):
        return gref.brute_force_any_hit(o, d, tmin, tmax, rec)


@pytest.mark.parametrize("name", NEW)
def test_entries_equal_the_brute_force(name, accels):
    c = cs.case(name)
    accel = accels(name)
    exact = cs.exact_range(name)
    differing = 0
    for tmin, tmax in cs.ranges(name):
        want = cs.base_closest(name) if (tmin, tmax) == (0.0, 1.0) else closest.brute_force_closest(c.o, c.d, tmin, tmax, c.rec)
        want_any = _any(c.o, c.d, tmin, tmax, c.rec)
        hits = want["index"] != MISS
        assert np.array_equal(hits, want_any), "the two brute forces disagree"
        per_class = {k: int(hits[c.tag == k].sum()) for k in cs.FAR + ("last_subtree",)}
        print(f"[ray scenes gpu] {name} ({len(c.tris)} triangles) t in [{tmin}, {tmax}]: {len(c.o)} rays, {int(hits.sum())} hits {per_class}")
        got_any, query = _both(accel, c.o, c.d, tmin, tmax)
        _compare_any(name, f"t in [{tmin}, {tmax}]", got_any, query, want_any, c.tag)
        got, occluded = _run(accel, c.o, c.d, tmin, tmax)
        differing += int((got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)).any(axis=1).sum())
        _compare_closest(name, f"t in [{tmin}, {tmax}]", got, occluded, want, c.tag)
        assert np.array_equal(occluded, got_any)
        if (tmin, tmax) == exact:
            assert hits.any() and (want["t"][hits] == F32(tmin)).all(), "the degenerate range holds exactly the hits at its t"
    assert differing == 0


def test_duplicates_reversed_goes_to_the_lower_index(accels):
    c = cs.case("duplicates_reversed")
    got, _ = _run(accels("duplicates_reversed"), c.o, c.d, 0.0, 1.0)
    hit = got["index"] != MISS
    assert hit.sum() > 1000 and (got["index"][hit] < len(c.tris) // 2).all()


def _attributes(name):
    """the attribute conventions of ray_cutout_cases (uvs (0, 0), (2, 0), (0, 2): uv_hit = (2 u, 2 v)).  offset_2p13: every kind of
    albedo index in turn.  duplicates_reversed: the lower-index copy wears the checker, a 1 x 1 hole or the 3 x 5 texture in turn,
    the higher-index copy is solid"""
    n = len(cs.case(name).tris)
    if name == "duplicates_reversed":
        lower = np.array([cut.CHECKER, cut.HOLE, cut.ODD], np.int64)[np.arange(n // 2) % 3]
        return cut.attributes(np.concatenate([lower, np.full(n - n // 2, cut.SOLID, np.int64)]))
    kinds = np.array([cut.CHECKER, cut.SOLID, cut.HOLE, cut.MIPPED, cut.ODD, cut.EDGE, cut.MISS, cut.TEXTURE_COUNT + 1], np.int64)
    return cut.attributes(kinds[np.arange(n) % len(kinds)])


@pytest.mark.parametrize("name", ["offset_2p13", "duplicates_reversed"])
def test_cutout_entries_equal_the_brute_force(name, accels):
    c = cs.case(name)
    attribs = _attributes(name)
    textures = _textures()[0]
    opaque = cs.base_closest(name)
    for tmin, tmax in ((0.0, 1.0), cs.exact_range(name)):
        want = cutref.brute_force_closest_cutout(_arith(), c.o, c.d, tmin, tmax, c.rec, attribs, textures, 0, 0)
        want_any = cutref.brute_force_any_hit_cutout(_arith(), c.o, c.d, tmin, tmax, c.rec, attribs, textures, 0, 0)
        got, got_any = _run_cutout(c.tris, attribs, c.o, c.d, tmin, tmax, 0, 0, accel=accels(name))
        _same_bits(got, want, f"{name}, t in [{tmin}, {tmax}]")
        assert np.array_equal(got_any, want_any) and np.array_equal(got_any, got["index"] != MISS)
        miss = got[got["index"] == MISS]
        assert (miss["t"] == 0).all() and (miss["u"] == 0).all() and (miss["v"] == 0).all()
        if (tmin, tmax) != (0.0, 1.0):
            continue
        changed = got["index"] != opaque["index"]
        lost = changed & (got["index"] == MISS)
        print(f"[ray scenes gpu] {name} cutouts: {int((opaque['index'] != MISS).sum())} opaque hits, {int(changed.sum())} change, {int(lost.sum())} miss")
        assert changed.sum() > 100, "the holes change answers"
        if name == "duplicates_reversed":
            n = len(c.tris)
            was = opaque["index"].astype(np.int64)
            handed = changed & (got["index"].astype(np.int64) == n - 1 - was)
            assert handed.sum() > 100, "no hole in a lower-index copy hands the hit to its twin"
            assert np.array_equal(got["t"][handed].view(np.uint32), opaque["t"][handed].view(np.uint32)), "the twin is hit at the same t"
            assert (got["index"][handed] >= n // 2).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_partial_waves_and_blocks(n, accels):
    """the first n rays of a shuffle of every class, on deep and on offset_2p20"""
    for name in ("deep", "offset_2p20"):
        c = cs.case(name)
        order = np.random.default_rng([59, n]).permutation(len(c.o))[:n]
        o, d = c.o[order], c.d[order]
        want = closest.brute_force_closest(o, d, 0.0, 1.0, c.rec)
        got_any, query = _both(accels(name), o, d, 0.0, 1.0)
        _compare_any(name, f"{n} rays", got_any, query, _any(o, d, 0.0, 1.0, c.rec), c.tag[order])
        got, occluded = _run(accels(name), o, d, 0.0, 1.0)
        _compare_closest(name, f"{n} rays", got, occluded, want, c.tag[order])
