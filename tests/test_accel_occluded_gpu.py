"""vkr_accel_occluded (the walk with the per-ray cull, csrc/accel_traverse.hpp wave_any_hit_ray) on the GPU: its answers must be
those of vkr_accel_query and of the numpy brute force of the frozen triangle test (tests/gtao_rt_reference.py), bit for bit,
on small hierarchies and on the rays at which a slab test goes wrong: rays lying in the plane of an axis-aligned face with zero
direction components and the origin on a slab plane (0 * inf), rays through shared vertices and edges, direction components of
1e-30, of denormal size and of 1e30, a zero direction, tmin == tmax, tmin > tmax, NaN and inf in origin or direction, rays that
stay inside one leaf box, rays that point away from everything, and seeded random long rays across the scene box.  Ray counts
of 1, 63, 64, 65 and 257 make partial waves and partial blocks."""
import functools

import numpy as np
import pytest

from vk_renderer_amd import abi
from vk_renderer_amd import scene as scn

import gtao_rt_reference as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 9  # the value of out_hit entries no ray owns


def _box():
    """the axis-aligned box [-1, 1]^3 as 12 triangles"""
    p = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], F32)
    faces = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    return np.array([[p[a], p[b], p[c]] for f in faces for a, b, c in ((f[0], f[1], f[2]), (f[0], f[2], f[3]))], F32)


def _zero_area():
    rng = np.random.default_rng(5)
    a = rng.uniform(-2, 2, size=(12, 3)).astype(F32)
    b = a + rng.uniform(-0.5, 0.5, size=(12, 3)).astype(F32)
    return np.concatenate([np.stack([a, a, b], 1), np.stack([a, b, (a + b) * F32(0.5)], 1), np.stack([a, a, a], 1)]).astype(F32)


ONE = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F32)
SCENES = {
    "empty": lambda: np.zeros((0, 3, 3), F32),
    "one_triangle": lambda: ONE,
    "nine_in_one_spot": lambda: np.repeat(ONE, 9, axis=0),  # more than a leaf holds and no plane to split at
    "zero_area": _zero_area,
    "box": _box,
    "procedural": lambda: abi.scene_triangles(scn.procedural_scene(detail=3)),
}


def _nodes(tris):
    """(lo [n, 3], hi [n, 3], count [n]) of vkr_accel_layout's nodes"""
    raw, _ = abi.accel_layout(tris)
    if len(raw) == 0:
        return np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, np.uint32)
    words = raw.view(np.uint32).reshape(len(raw), 8)
    return words[:, 0:3].view(F32), words[:, 4:7].view(F32), words[:, 7]


def _rays(tris, rng):
    """-> (origins, directions, tag per ray) of every class, built around the scene's own boxes, vertices and edges"""
    o, d, tag = [], [], []

    def add(oo, dd, name):
        oo, dd = np.asarray(oo, F32).reshape(-1, 3), np.asarray(dd, F32).reshape(-1, 3)
        oo, dd = np.broadcast_arrays(oo, dd) if len(oo) != len(dd) else (oo, dd)
        o.append(np.array(oo, F32))
        d.append(np.array(dd, F32))
        tag.extend([name] * len(oo))

    lo, hi, count = _nodes(tris)
    if len(lo) == 0:  # the empty scene: the classes need boxes of some kind
        lo, hi, count = np.array([[-1, -1, -1]], F32), np.array([[1, 1, 1]], F32), np.array([1], np.uint32)
        verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
        mids = verts
    else:
        verts = tris.reshape(-1, 3)
        mids = np.concatenate([(tris[:, 0] + tris[:, 1]), (tris[:, 1] + tris[:, 2]), (tris[:, 2] + tris[:, 0])]) * F32(0.5)
    slo, shi = lo.min(0), hi.max(0)
    ext = np.maximum(shi - slo, F32(1.0))
    # (a) in the plane of an axis-aligned face of a node box, origin on a slab plane, one or two zero direction components
    pick = rng.integers(0, len(lo), 240)
    for k, i in enumerate(pick):
        axis, side = k % 3, (k // 3) % 2
        p = rng.uniform(lo[i], np.maximum(hi[i], lo[i])).astype(F32)
        p[axis] = (lo[i], hi[i])[side][axis]           # in the face's plane
        other = (axis + 1 + (k // 6) % 2) % 3
        p[other] = (lo[i], hi[i])[(k // 12) % 2][other]  # and on a second slab plane
        dd = np.zeros(3, F32)
        dd[other] = F32(rng.choice([-1.5, 1.5])) * ext[other]
        if k % 2:
            third = 3 - axis - other
            dd[third] = F32(rng.uniform(-1, 1)) * ext[third]  # one zero component; else two
        add(p - dd * F32(0.5) * F32(k % 4 == 0), dd, "in_plane")
    # the box scene's own faces: exactly in the plane of the triangles
    for axis in range(3):
        for s in (-1.0, 1.0):
            p = rng.uniform(-1.5, 1.5, size=(20, 3)).astype(F32)
            p[:, axis] = s
            dd = rng.uniform(-3, 3, size=(20, 3)).astype(F32)
            dd[:, axis] = 0
            dd[::2, (axis + 1) % 3] = 0
            add(p, dd, "in_plane")
    # (b) at every vertex and edge midpoint from a common point: ending there (t = tmax) and passing through
    eye = (shi + ext * F32(0.75)).astype(F32)
    for target, name in ((verts, "vertex"), (mids, "edge")):
        add(eye, target - eye, name + "_tmax")
        add(eye, (target - eye) * F32(2.0), name + "_through")
    # (c) tiny, denormal and huge direction components
    base_o = rng.uniform(slo - ext * F32(0.2), shi + ext * F32(0.2), size=(120, 3)).astype(F32)
    base_d = rng.uniform(-1, 1, size=(120, 3)).astype(F32) * ext * F32(2.0)
    for value, name in ((1e-30, "tiny"), (1e-41, "denormal"), (1e30, "huge")):
        for axis in range(3):
            dd = base_d.copy()
            dd[:, axis] = F32(value) * np.where(np.arange(120) % 2, F32(-1), F32(1))
            add(base_o, dd, name)
        add(base_o[:40], np.full((40, 3), value, F32), name)
    add(verts[: min(len(verts), 60)], np.zeros((min(len(verts), 60), 3), F32), "zero_direction")
    add(base_o[:40], np.zeros((40, 3), F32), "zero_direction")
    # (d) NaN and inf in the origin or the direction
    for value in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            oo, dd = base_o[:30].copy(), base_d[:30].copy()
            oo[:, axis] = value
            add(oo, dd, "nonfinite")
            oo, dd = base_o[:30].copy(), base_d[:30].copy()
            dd[:, axis] = value
            add(oo, dd, "nonfinite")
    # (e) inside one leaf box from start to end
    leaves = np.nonzero(count > 0)[0]
    li = leaves[rng.integers(0, len(leaves), 400)]
    a = rng.uniform(lo[li], np.maximum(hi[li], lo[li])).astype(F32)
    b = rng.uniform(lo[li], np.maximum(hi[li], lo[li])).astype(F32)
    add(a, b - a, "inside_leaf")
    # (f) pointing away from everything
    out = rng.normal(size=(200, 3)).astype(F32)
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    centre = (slo + shi) * F32(0.5)
    add(centre + out * ext * F32(2.0), out * ext * F32(3.0), "away")
    # (g) long rays across the whole scene box
    a = rng.uniform(slo - ext * F32(0.25), shi + ext * F32(0.25), size=(4096, 3)).astype(F32)
    b = rng.uniform(slo - ext * F32(0.25), shi + ext * F32(0.25), size=(4096, 3)).astype(F32)
    add(a, b - a, "long")
    return np.concatenate(o), np.concatenate(d), np.array(tag)


@functools.lru_cache(maxsize=None)
def _case(name):
    tris = np.ascontiguousarray(SCENES[name](), F32)
    o, d, tag = _rays(tris, np.random.default_rng([17, sorted(SCENES).index(name)]))
    return tris, o, d, tag, ref.triangle_records(tris)


def _both(accel, o, d, tmin, tmax):
    """-> (vkr_accel_occluded, vkr_accel_query) answers as bool arrays; the entries past the rays must stay untouched"""
    import torch

    n = len(o)
    to, td = torch.from_numpy(np.ascontiguousarray(o)).to("cuda"), torch.from_numpy(np.ascontiguousarray(d)).to("cuda")
    got = []
    for fn in (accel.occluded, accel.query):
        out = torch.full((n + 64,), GUARD, dtype=torch.int32, device="cuda")
        fn(to, td, tmin, tmax, out, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        h = out.cpu().numpy()
        assert (h[n:] == GUARD).all(), "entries past the last ray were written"
        assert set(np.unique(h[:n]).tolist()) <= {0, 1}
        got.append(h[:n].astype(bool))
    return got


def _compare(name, what, got, query, want, tag):
    for label, other in (("vkr_accel_query", query), ("the brute force", want)):
        bad = np.nonzero(got != other)[0]
        assert len(bad) == 0, (f"{name}, {what}: {len(bad)} of {len(got)} rays differ from {label}, e.g. "
                               f"{[(int(i), str(tag[i]), bool(got[i]), bool(other[i])) for i in bad[:8]]}")


@pytest.mark.parametrize("name", sorted(SCENES))
def test_occluded_equals_query_and_brute_force(name):
    tris, o, d, tag, rec = _case(name)
    accel = abi.Accel(tris)
    try:
        assert accel.info()[1] == len(tris)
        # (0, 1e10): tmax * d overflows for the components of 1e30, and the segment's far corner is infinite
        for tmin, tmax in ((0.0, 1.0), (1e-12, 1.0), (0.25, 0.75), (0.5, 0.5), (1.0, 1.0), (0.75, 0.25), (-0.5, 1.5), (0.0, 1e10)):
            got, query = _both(accel, o, d, tmin, tmax)
            want = ref.brute_force_any_hit(o, d, tmin, tmax, rec)
            hits = {k: int(want[tag == k].sum()) for k in np.unique(tag)}
            print(f"[accel occluded] {name} ({len(tris)} triangles) t in [{tmin}, {tmax}]: {len(o)} rays, {int(want.sum())} hits {hits}")
            _compare(name, f"t in [{tmin}, {tmax}]", got, query, want, tag)
            if tmin > tmax:
                assert not got.any(), "an empty parameter range hits nothing"
        if name in ("box", "procedural"):  # the adversarial classes are not vacuous where there is something to hit
            want = ref.brute_force_any_hit(o, d, 0.0, 1.0, rec)
            for k in ("in_plane", "inside_leaf", "long", "tiny", "denormal", "huge"):
                assert 0 < int(want[tag == k].sum()) < int((tag == k).sum()), k
            assert int(want[tag == "vertex_tmax"].sum()) > 0 and int(want[tag == "edge_tmax"].sum()) > 0
            assert int(want[tag == "away"].sum()) == 0 and int(want[tag == "zero_direction"].sum()) == 0
    finally:
        accel.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_partial_waves_and_blocks(n):
    """the first n rays of a shuffle of every class, on the box and on the procedural scene"""
    for name in ("box", "procedural", "empty"):
        tris, o, d, tag, rec = _case(name)
        order = np.random.default_rng([23, n]).permutation(len(o))[:n]
        accel = abi.Accel(tris)
        try:
            got, query = _both(accel, o[order], d[order], 0.0, 1.0)
            want = ref.brute_force_any_hit(o[order], d[order], 0.0, 1.0, rec)
            _compare(name, f"{n} rays", got, query, want, tag[order])
        finally:
            accel.close()
