"""vkr_accel_closest (csrc/accel_traverse.hpp wave_closest_hit) on the GPU: its answers must be those of the numpy brute force
(tests/closest_hit_reference.py) bit for bit in all four words — t, u, v as uint32 views and the index — and `index != miss` must
be vkr_accel_occluded's answer for every ray.

The rays are those of tests/test_accel_occluded_gpu.py (in the plane of node-box faces with zero direction components, through
shared vertices and edges, direction components of 1e-30, denormal size and 1e30, a zero direction, NaN and inf, inside one leaf
box, pointing away, seeded long rays) and two classes a walk with a shrinking interval adds: rays whose nearest triangle lies in
the subtree the walk visits LAST (built from the layout: they start just in front of a triangle below the root's second child
and run on through the first child's box, so the walk meets farther hits first and must still replace them), and parameter ranges
with tmin == tmax exactly at a hit's t.  Ray counts of 1, 63, 64, 65 and 257 make partial waves and partial blocks; the records
behind the last ray keep a guard value."""
import functools

import numpy as np
import pytest

from vk_renderer_amd import abi

import closest_hit_reference as ref
from test_accel_occluded_gpu import SCENES, _nodes, _rays

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 0x0BADBEEF  # every word of a record no ray owns


def _last_subtree_rays(tris, rng, count=256):
    """-> (origins, directions, record positions of the root's second subtree) or None where the root is a leaf"""
    raw_nodes, raw_tris = abi.accel_layout(tris)
    if len(raw_nodes) == 0:
        return None
    nodes = raw_nodes.view(np.uint32).reshape(len(raw_nodes), 8)
    if nodes[0, 7] != 0:
        return None
    order = raw_tris.view(np.uint32).reshape(len(raw_tris), 16)[:, 3]  # record position -> input index
    lo, hi, _ = _nodes(tris)

    def records(node):
        first, n = int(nodes[node, 3]), int(nodes[node, 7])
        return list(range(first, first + n)) if n else records(first) + records(first + 1)

    left, right = int(nodes[0, 3]), int(nodes[0, 3]) + 1
    last = order[np.array(records(right))]
    pick = last[rng.integers(0, len(last), count)]
    c = tris[pick].mean(axis=1).astype(F32)
    target = rng.uniform(lo[left], np.maximum(hi[left], lo[left]), size=(count, 3)).astype(F32)
    d = ((target - c) * F32(2.0)).astype(F32)
    return (c - d * F32(0.01)).astype(F32), d, set(int(i) for i in last)


@functools.lru_cache(maxsize=None)
def _case(name):
    tris = np.ascontiguousarray(SCENES[name](), F32)
    rng = np.random.default_rng([29, sorted(SCENES).index(name)])
    o, d, tag = _rays(tris, rng)
    last = _last_subtree_rays(tris, rng)
    last_set = set()
    if last is not None:
        o, d, tag = np.concatenate([o, last[0]]), np.concatenate([d, last[1]]), np.concatenate([tag, np.array(["last_subtree"] * len(last[0]))])
        last_set = last[2]
    return tris, o, d, tag, ref.triangle_records(tris), last_set


def _run(accel, o, d, tmin, tmax):
    """-> (vkr_accel_closest's records as HIT_DTYPE [n], vkr_accel_occluded's answers as bool [n]); records past n stay untouched"""
    import torch

    n = len(o)
    to, td = torch.from_numpy(np.ascontiguousarray(o)).to("cuda"), torch.from_numpy(np.ascontiguousarray(d)).to("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full((n + 64, 4), GUARD, dtype=torch.int32, device="cuda")
    accel.closest(to, td, tmin, tmax, out, stream)
    occ = torch.full((n + 64,), 9, dtype=torch.int32, device="cuda")
    accel.occluded(to, td, tmin, tmax, occ, stream)
    torch.cuda.synchronize()
    h = out.cpu().numpy().view(np.uint32)
    assert (h[n:] == GUARD).all(), "records past the last ray were written"
    return np.ascontiguousarray(h[:n]).view(ref.HIT_DTYPE).reshape(n), occ.cpu().numpy()[:n].astype(bool)


def _compare(name, what, got, occluded, want, tag):
    g, w = got.view(np.uint32).reshape(-1, 4), want.view(np.uint32).reshape(-1, 4)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, (f"{name}, {what}: {len(bad)} of {len(got)} rays differ from the brute force, e.g. "
                           f"{[(int(i), str(tag[i]), got[i].tolist(), want[i].tolist()) for i in bad[:6]]}")
    bad = np.nonzero((got["index"] != ref.MISS) != occluded)[0]
    assert len(bad) == 0, f"{name}, {what}: {len(bad)} rays hit here and not for vkr_accel_occluded (or the reverse), e.g. {bad[:8].tolist()}"
    miss = got["index"] == ref.MISS
    assert (g[miss, :3] == 0).all(), "a miss is (0, 0, 0, 0xFFFFFFFF)"


@pytest.mark.parametrize("name", sorted(SCENES))
def test_closest_equals_brute_force_bit_for_bit(name):
    tris, o, d, tag, rec, last_set = _case(name)
    accel = abi.Accel(tris)
    try:
        assert accel.info()[1] == len(tris)
        ranges = [(0.0, 1.0), (1e-12, 1.0), (0.25, 0.75), (0.5, 0.5), (1.0, 1.0), (0.75, 0.25), (-0.5, 1.5), (0.0, 1e10)]
        base = ref.brute_force_closest(o, d, 0.0, 1.0, rec)
        # tmin == tmax exactly at a hit's t: the t of a few rays that hit, one of each class that has one
        exact = []
        for k in np.unique(tag):
            i = np.nonzero((tag == k) & (base["index"] != ref.MISS) & (base["t"] > 0))[0]
            if len(i):
                exact.append(float(base["t"][i[len(i) // 2]]))
        ranges += [(t, t) for t in exact[:6]]
        for tmin, tmax in ranges:
            got, occluded = _run(accel, o, d, tmin, tmax)
            want = base if (tmin, tmax) == (0.0, 1.0) else ref.brute_force_closest(o, d, tmin, tmax, rec)
            hits = want["index"] != ref.MISS
            print(f"[accel closest] {name} ({len(tris)} triangles) t in [{tmin}, {tmax}]: {len(o)} rays, {int(hits.sum())} hits")
            _compare(name, f"t in [{tmin}, {tmax}]", got, occluded, want, tag)
            if tmin > tmax:
                assert not hits.any(), "an empty parameter range hits nothing"
            if tmin == tmax and (tmin, tmax) in [(t, t) for t in exact[:6]]:
                assert hits.any() and (want["t"][hits] == F32(tmin)).all(), "the degenerate range holds exactly the hits at its t"
        if name in ("box", "procedural"):  # the adversarial classes are not vacuous where there is something to hit
            hit = base["index"] != ref.MISS
            for k in ("in_plane", "inside_leaf", "long", "tiny", "denormal", "huge"):
                assert 0 < int(hit[tag == k].sum()) < int((tag == k).sum()), k
            assert int(hit[tag == "vertex_tmax"].sum()) > 0 and int(hit[tag == "edge_tmax"].sum()) > 0
            assert not hit[tag == "away"].any() and not hit[tag == "zero_direction"].any()
            # ties: rays through shared vertices and edges are accepted by more than one triangle at one t
            through = np.nonzero((tag == "edge_through") & hit)[0][:64]
            tied = 0
            for i in through:
                ok, t, _, _ = ref.frozen_hit_tuv(o[i][None], d[i][None], 0.0, 1.0, rec["v0"], rec["e1"], rec["e2"], rec["lo"], rec["hi"])
                tied += int((ok & (t == base["t"][i])).sum() > 1)
            assert tied > 0, "no ray of the edge class is a tie"
            # the last subtree: the winner lies below the root's second child although the ray also hits below the first
            sel = tag == "last_subtree"
            wins_last = np.array([int(i) in last_set for i in base["index"][sel]]) & hit[sel]
            first_only = np.array([k for k in range(len(tris)) if k not in last_set])
            other = ref.brute_force_closest(o[sel], d[sel], 0.0, 1.0, ref.triangle_records(tris[first_only]))
            both = wins_last & (other["index"] != ref.MISS)
            print(f"[accel closest] {name}: {int(sel.sum())} last-subtree rays, {int(wins_last.sum())} won there, {int(both.sum())} also hit the first subtree")
            assert int(both.sum()) > 0, "no ray whose nearest triangle lies in the subtree visited last and that hits the other one too"
    finally:
        accel.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_partial_waves_and_blocks(n):
    """the first n rays of a shuffle of every class, on the box, the procedural scene and the empty one"""
    for name in ("box", "procedural", "empty"):
        tris, o, d, tag, rec, _ = _case(name)
        order = np.random.default_rng([31, n]).permutation(len(o))[:n]
        accel = abi.Accel(tris)
        try:
            got, occluded = _run(accel, o[order], d[order], 0.0, 1.0)
            want = ref.brute_force_closest(o[order], d[order], 0.0, 1.0, rec)
            _compare(name, f"{n} rays", got, occluded, want, tag[order])
        finally:
            accel.close()
