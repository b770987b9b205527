"""numpy restatement of the refit rule (include/vkr_postfx.h vkr_accel_refit, csrc/accel_refit.hip), with the scenes and motions of
tests/test_accel_refit.py (no GPU) and tests/test_accel_refit_gpu.py.

The rule: the topology (every node's first and count, every record's slot and index) is kept; a record becomes
ray_scene_cases.host_records of its input triangle at the new position; a node box becomes ray_scene_cases._union of what lies
below it — a leaf's records, an interior node's two children — level by level over the heights that Layout's parents give, always
from scratch.

refit(..., mutant=) restates it wrongly in five ways; tests/test_accel_refit.py names the case that catches each:
  grow        a box is the union of the old box and the new one
  skip_level  the nodes of height 1 keep their old boxes
  drop_last   a leaf of more than one record ignores its last one
  nan_min     the union propagates a NaN (np.minimum / np.maximum instead of fmin / fmax)
  old_margin  the margin of a record comes from the vertices before the move

Scenes (tris (n, 3, 3) float32): tri1, tri2, tri3, tri9 (a root leaf, two triangles that may not be split, the first legal
split, the first forced split), box, procedural, deep, area_overflow, duplicates_reversed of ray_scene_cases, and detail24:
abi.scene_triangles(procedural_scene(detail=24)), 6916 triangles — the one whose leaf level is wider than the tail of the device
schedule.  Motions: see MOTIONS; each maps the built triangles to the pose(s) refitted in turn.
"""
import functools

import numpy as np

from vk_renderer_amd import abi
from vk_renderer_amd import scene as scn

import ray_scene_cases as cs

F32 = np.float32
F64 = np.float64
NODE, TRI = cs.NODE, cs.TRI
MUTANTS = ("grow", "skip_level", "drop_last", "nan_min", "old_margin")


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def heights(nodes):
    """height per node: 0 for a leaf, 1 + the larger height of the two children; children are stored behind their parent"""
    h = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes) - 1, -1, -1):
        if nodes["count"][i] == 0:
            f = int(nodes["first"][i])
            h[i] = 1 + max(h[f], h[f + 1])
    return h


def _records_old_margin(tris, old):
    """host_records with the margin of the triangles before the move (the mutant)"""
    new = cs.host_records(tris)
    smin = lambda a, b: np.where(b < a, b, a)
    smax = lambda a, b: np.where(a < b, b, a)
    with np.errstate(all="ignore"):
        s = np.zeros(len(new["v0"]), F32)
        for v in np.abs(np.asarray(old, F32).reshape(-1, 9)).T:
            s = smax(s, v)
        margin = ((s + F32(1.0)) * F32(2.0 ** -12)).astype(F32)[:, None]
        n = np.asarray(tris, F32).reshape(-1, 3, 3)
        new["lo"] = smin(smin(n[:, 0], n[:, 1]), n[:, 2]) - margin
        new["hi"] = smax(smax(n[:, 0], n[:, 1]), n[:, 2]) + margin
    return new


def _union_nan(lo, hi):
    with np.errstate(all="ignore"):
        return np.minimum.reduce(np.concatenate([np.full((1, 3), np.inf, F32), lo]), axis=0), np.maximum.reduce(np.concatenate([np.full((1, 3), -np.inf, F32), hi]), axis=0)


def refit(nodes, recs, tris, mutant=None, old_tris=None):
    """nodes (NODE [n]) and recs (TRI [m]) refitted to tris ((m, 3, 3) float32, input order) -> new (nodes, recs)"""
    assert mutant is None or mutant in MUTANTS
    nodes, recs = nodes.copy(), recs.copy()
    tris = np.asarray(tris, F32).reshape(-1, 3, 3)
    rec = _records_old_margin(tris, old_tris) if mutant == "old_margin" else cs.host_records(tris)
    idx = recs["index"].astype(np.int64)
    for f in ("v0", "e1", "e2", "lo", "hi"):
        recs[f] = rec[f][idx]
    union = _union_nan if mutant == "nan_min" else cs._union
    h = heights(nodes)
    for level in range(int(h.max()) + 1 if len(h) else 0):
        if mutant == "skip_level" and level == 1:
            continue
        for i in np.nonzero(h == level)[0]:
            first, count = int(nodes["first"][i]), int(nodes["count"][i])
            if count == 0:
                lo, hi = union(nodes["lo"][first:first + 2], nodes["hi"][first:first + 2])
            else:
                last = first + count - (1 if mutant == "drop_last" and count > 1 else 0)
                lo, hi = union(recs["lo"][first:last], recs["hi"][first:last])
            if mutant == "grow":
                lo, hi = union(np.stack([nodes["lo"][i], lo]), np.stack([nodes["hi"][i], hi]))
            nodes["lo"][i], nodes["hi"][i] = lo, hi
    return nodes, recs


def same_bytes(a, b):
    """two structured arrays (NODE or TRI) are the same bytes, where a NaN equals any NaN"""
    if a.shape != b.shape:
        return False
    wa, wb = np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1), np.ascontiguousarray(b).view(np.uint32).reshape(len(b), -1)
    fa, fb = wa.view(F32), wb.view(F32)
    isf = np.ones(wa.shape[1], bool)
    isf[3] = False  # `first` of a node, `index` of a record: word 3 of both
    if a.dtype == NODE:
        isf[7] = False  # `count`
    return bool(np.all((wa == wb) | (isf[None] & np.isnan(fa) & np.isnan(fb))))


def view(raw_nodes, raw_tris):
    """the uint8 arrays of abi.accel_layout / accel_refit_layout / Accel.download as (NODE [n], TRI [m])"""
    return np.ascontiguousarray(raw_nodes).view(NODE).reshape(-1), np.ascontiguousarray(raw_tris).view(TRI).reshape(-1)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def _small(n):
    rng = np.random.default_rng([71, n])
    c = rng.uniform(-4, 4, size=(n, 1, 3)) * np.array([4.0, 1.0, 1.0])  # spread along x: a split is cheaper than a leaf
    return (c + rng.uniform(-0.3, 0.3, size=(n, 3, 3))).astype(F32)


@functools.lru_cache(maxsize=None)
def _detail24():
    return np.ascontiguousarray(abi.scene_triangles(scn.procedural_scene(detail=24)), F32)


SCENES = {
    "tri1": lambda: _small(1), "tri2": lambda: _small(2), "tri3": lambda: _small(3), "tri9": lambda: _small(9),
    "box": cs.ALL_SCENES["box"], "procedural": cs.ALL_SCENES["procedural"], "deep": cs.ALL_SCENES["deep"],
    "area_overflow": cs.ALL_SCENES["area_overflow"], "duplicates_reversed": cs.ALL_SCENES["duplicates_reversed"],
    "detail24": _detail24,
}


@functools.lru_cache(maxsize=None)
def scene(name):
    t = np.ascontiguousarray(SCENES[name](), F32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def built(name):
    """-> (NODE [n], TRI [m]) of vkr_accel_layout on the scene as built, read-only"""
    nodes, recs = view(*abi.accel_layout(scene(name)))
    nodes.setflags(write=False)
    recs.setflags(write=False)
    return nodes, recs


# ---- motions ----------------------------------------------------------------------------------------------------------------------
def _jitter(t):
    rng = np.random.default_rng(83)
    with np.errstate(all="ignore"):
        size = np.linalg.norm(t[:, 1].astype(F64) - t[:, 0], axis=1) + np.linalg.norm(t[:, 2].astype(F64) - t[:, 0], axis=1)
        return (t.astype(F64) + rng.normal(size=t.shape) * 0.5 * size[:, None, None]).astype(F32)


def _swap(t):
    return np.concatenate([t[len(t) // 2:], t[:len(t) // 2]])


def poison(t):
    """up to 24 triangles made non-finite as ray_scene_cases._nonfinite_vertices does"""
    t = t.copy()
    for j, i in enumerate(np.random.default_rng(41).permutation(len(t))[:cs.NONFINITE_COUNT]):
        kind, vertex, axis = j % 5, (j // 5) % 3, (j // 2) % 3
        if kind < 3:
            t[i, vertex, axis] = (np.nan, np.inf, -np.inf)[kind]
        elif kind == 3:
            t[i, :, 0] = np.inf
        else:
            t[i] = np.nan
    return t


def _scaled(t, k):
    with np.errstate(all="ignore"):
        return (t.astype(F64) * 2.0 ** k).astype(F32)


# name -> the poses refitted one after the other, from the triangles as built
MOTIONS = {
    "identity": lambda t: [t.copy()],
    "translation": lambda t: [(t.astype(F64) + np.array([2.0 ** 13, -2.0 ** 13, 2.0 ** 13])).astype(F32)],
    "scale_2m40": lambda t: [_scaled(t, -40)],
    "scale_2p40": lambda t: [_scaled(t, 40)],
    "jitter": lambda t: [_jitter(t)],
    "collapse": lambda t: [np.broadcast_to(t[:1, :1], t.shape).copy()],
    "cluster_swap": lambda t: [_swap(t)],
    "poison_heal": lambda t: [poison(t), t.copy()],
}


@functools.lru_cache(maxsize=None)
def poses(name, motion):
    out = [np.ascontiguousarray(p, F32) for p in MOTIONS[motion](scene(name))]
    for p in out:
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, motion):
    """the restatement's (nodes, recs) after every pose of the motion, read-only"""
    nodes, recs = built(name)
    out = []
    for p in poses(name, motion):
        nodes, recs = refit(nodes, recs, p)
        nodes.setflags(write=False)
        recs.setflags(write=False)
        out.append((nodes, recs))
    return out


# ---- the numpy twin of vkr_scene_triangles ----------------------------------------------------------------------------------------
def scene_triangles_twin(vertices, indices, models, draws):
    """vkr_scene_triangles' rule on plain arrays: vertices (n, >= 3) float32, indices uint32, models: list of 4 x 4 float32
    (maths convention, as scene.Scene keeps them), draws: dicts of transform, index_offset, index_count, vertex_offset -> (m, 3, 3)
    float32; a triangle with an index outside the vertex buffer is NaN"""
    out = []
    for d in draws:
        m = np.asarray(models[d["transform"]], F32)
        n = d["index_count"] // 3 * 3
        idx = indices[d["index_offset"]:d["index_offset"] + n].astype(np.int64) + d["vertex_offset"]
        ok = idx < len(vertices)
        p = vertices[np.where(ok, idx, 0), :3].astype(F32)
        w = np.empty_like(p)
        for r in range(3):
            w[:, r] = ((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3]
        w = w.reshape(-1, 3, 3)
        w[~ok.reshape(-1, 3).all(axis=1)] = np.nan
        out.append(w)
    return np.concatenate(out) if out else np.zeros((0, 3, 3), F32)
