"""Numpy restatement of the node test of the ray query, LaneRay<SLAB>::enters (csrc/accel_traverse.hpp; DESIGN_NUMERICS.md, "Ray
query, the per-ray cull"), and of nothing else about the walks — the checker of tests/test_ray_scene_cases.py.

Test infrastructure, like the oracle: the product package never imports it.  Every operation is one float32 numpy operation, in
the source's order: the segment-box corners mul-then-add with the fminf / fmaxf rule (a NaN corner gives way to the other one),
slab_reciprocal with its range gate, `reach` as the source's tree of sums, margin, the entry side per axis from the sign of the
RECIPROCAL, slab_keep_max / slab_keep_min (a NaN candidate is never taken, a NaN held stays), the outward step, and the one
comparison that rejects, tn > tf.  Vectorised over rays; Reach loops over the nodes of a layout.

What it is for is the property the two proofs claim, which does not depend on the order of the visit: for every ray and every
triangle the frozen test accepts in [tmin, tmax], every node from the root to the leaf that holds the triangle is entered
  - under the segment box alone (the short-ray walk),
  - under the segment box and the slab term with t_far = tmax (the any-hit walk for long rays),
  - under both with t_far = the t of the closest-hit winner: the tightest far bound the closest walk can hold while the winner is
    unvisited (the slab test is monotone in t_far).

A Variant switches single steps of the restatement to a wrong form (the mutants of tests/test_ray_scene_cases.py); the default is
the code.  Counters: `slab_rejects` (node, ray) pairs the segment box accepted and the slab term rejected, `axes_off` axes of rays
whose reciprocal is NaN, `nan_accepts` pairs the segment box accepted whose tn or tf was NaN at the compare.
"""
import dataclasses

import numpy as np

F32 = np.float32
QNAN = np.array([0x7FC00000], np.uint32).view(F32)[0]


@dataclasses.dataclass(frozen=True)
class Variant:
    margin: bool = True          # False: margin = 0
    outward: bool = True         # False: no outward step
    guard: bool = True           # False: slab_reciprocal is 1 / d for every d
    strict: bool = True          # False: rejects on tn >= tf
    fmin_rule: bool = True       # False: np.minimum / np.maximum for the segment-box corners (a NaN corner wins)
    reach_sum: bool = True       # False: reach is the maximum of the nine magnitudes
    side_of_reciprocal: bool = True  # False: the entry side from the sign of d


CODE = Variant()


class Rays:
    """what LaneRay's constructor keeps of rays (o, d) [n, 3] and the range [tmin, tmax]"""

    def __init__(self, o, d, tmin, tmax, variant=CODE):
        o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
        tmin, tmax = F32(tmin), F32(tmax)
        self.variant, self.n = variant, len(o)
        with np.errstate(all="ignore"):
            a = (o + (tmin * d).astype(F32)).astype(F32)
            b = (o + (tmax * d).astype(F32)).astype(F32)
            lo_of, hi_of = (np.fmin, np.fmax) if variant.fmin_rule else (np.minimum, np.maximum)
            self.lo, self.hi = lo_of(a, b), hi_of(a, b)
            self.o, self.tmin = o, np.full(len(o), tmin, F32)
            ab = np.abs
            if variant.reach_sum:
                reach = (((ab(o[:, 0]) + ab(o[:, 1])) + (ab(o[:, 2]) + ab(a[:, 0]))) + ((ab(a[:, 1]) + ab(a[:, 2])) + (ab(b[:, 0]) + ab(b[:, 1])))) + ab(b[:, 2])
            else:
                reach = np.fmax.reduce(np.concatenate([ab(o), ab(a), ab(b)], axis=1), axis=1)
            margin = (reach * F32(2.0 ** -21)).astype(F32) + F32(2.0 ** -126)
            if not variant.margin:
                margin = np.zeros(len(o), F32)
            m = ab(d)
            inv = (F32(1.0) / d).astype(F32)
            self.inv = np.where((m >= F32(2.0 ** -100)) & (m <= F32(2.0 ** 100)), inv, QNAN).astype(F32) if variant.guard else inv
            self.positive = (self.inv > 0) if variant.side_of_reciprocal else (d > 0)
            self.m = np.where(self.positive, margin[:, None], -margin[:, None]).astype(F32)
        self.axes_off = int(np.isnan(self.inv).sum())


def _keep_max(acc, x):
    return np.where(x > acc, x, acc)


def _keep_min(acc, x):
    return np.where(x < acc, x, acc)


def slab_terms(rays, lo, hi):
    """the part of enters that does not depend on t_far, for every ray against one node box [lo, hi] (3 floats each)
    -> (segment-box overlap [n] bool, the near accumulator before the outward step [n], the three far parameters)"""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    with np.errstate(all="ignore"):
        box = np.ones(rays.n, bool)
        for k in range(3):
            box &= (rays.lo[:, k] <= hi[k]) & (rays.hi[:, k] >= lo[k])
        tn = rays.tmin
        far = []
        for k in range(3):
            p, o, m, inv = rays.positive[:, k], rays.o[:, k], rays.m[:, k], rays.inv[:, k]
            tn = _keep_max(tn, ((((np.where(p, lo[k], hi[k]) - o).astype(F32)) - m).astype(F32) * inv).astype(F32))
            far.append(((((np.where(p, hi[k], lo[k]) - o).astype(F32)) + m).astype(F32) * inv).astype(F32))
    return box, tn, far


def decide(rays, box, tn, far, t_far):
    """the rest of enters: t_far a float or one per ray -> (enters [n] bool, NaN at the compare [n] bool)"""
    with np.errstate(all="ignore"):
        tf = np.broadcast_to(np.asarray(t_far, F32), (rays.n,))
        for k in range(3):
            tf = _keep_min(tf, far[k])
        if rays.variant.outward:
            tn = (tn - ((np.abs(tn) * F32(2.0 ** -20)).astype(F32) + F32(2.0 ** -126)).astype(F32)).astype(F32)
            tf = (tf + ((np.abs(tf) * F32(2.0 ** -20)).astype(F32) + F32(2.0 ** -126)).astype(F32)).astype(F32)
        reject = (tn > tf) if rays.variant.strict else (tn >= tf)
    return box & ~reject, np.isnan(tn) | np.isnan(tf)


def enters(rays, lo, hi, t_far, slab=True):
    """LaneRay<slab>::enters of every ray (live) against one node box -> [n] bool"""
    box, tn, far = slab_terms(rays, lo, hi)
    return decide(rays, box, tn, far, t_far)[0] if slab else box


class Reach:
    """reach[node, ray] = enters[node, ray] & reach[parent, ray] in one pass over the nodes (parents stored first): `box` under the
    segment box alone, `slab[j]` under the segment box and the slab term with t_fars[j]; the counters of the module docstring are
    those of t_fars[0]"""

    def __init__(self, node_lo, node_hi, parent, rays, t_fars):
        n = len(node_lo)
        self.box = np.zeros((n, rays.n), bool)
        self.slab = [np.zeros((n, rays.n), bool) for _ in t_fars]
        self.slab_rejects = self.nan_accepts = self.tests = 0
        self.axes_off = rays.axes_off
        for i in range(n):
            box, tn, far = slab_terms(rays, node_lo[i], node_hi[i])
            up = parent[i]
            self.box[i] = box if up < 0 else box & self.box[up]
            for j, t_far in enumerate(t_fars):
                e, nan = decide(rays, box, tn, far, t_far)
                self.slab[j][i] = e if up < 0 else e & self.slab[j][up]
                if j == 0:
                    self.tests += int(box.sum())
                    self.slab_rejects += int((box & ~e).sum())
                    self.nan_accepts += int((box & nan).sum())


def violations(table, leaf_of, ray, tri):
    """of the accepted (ray, input triangle) pairs, those whose leaf is not reached -> indices into the pairs"""
    if len(ray) == 0:
        return np.zeros(0, np.int64)
    return np.nonzero(~table[leaf_of[tri], ray])[0]
