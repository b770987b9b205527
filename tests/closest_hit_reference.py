"""Numpy restatement of the closest-hit ray query (csrc/accel_traverse.hpp wave_closest_hit, entry vkr_accel_closest;
DESIGN_NUMERICS.md, "Ray query, closest hit") — the checker of tests/test_accel_closest.py and tests/test_accel_closest_gpu.py,
and the ray query of tests/reflections_rt_reference.py.

Test infrastructure, like the oracle: the product package never imports it.  No hierarchy here: the frozen triangle test of
tests/gtao_rt_reference.py (frozen_hit_tuv: it hands back the t, u, v it computes) against ALL triangles, then the smallest t
and of equal t (==, so -0 == +0) the smallest input index.
"""
import numpy as np

from gtao_rt_reference import F32, frozen_hit_tuv, segment_boxes, triangle_records  # noqa: F401

MISS = 0xFFFFFFFF
HIT_DTYPE = np.dtype([("t", F32), ("u", F32), ("v", F32), ("index", np.uint32)])  # vkr_accel_hit


def brute_force_closest(o, d, tmin, tmax, rec, chunk=512):
    """closest hit of every ray against every triangle: -> HIT_DTYPE [n]; a miss is (0, 0, 0, MISS).  A triangle whose widened
    box misses the ray's segment box is skipped: by the test's own definition it cannot be hit (its hit point lies in both
    boxes), so this is the exact answer."""
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    out = np.zeros(len(o), HIT_DTYPE)
    out["index"] = MISS
    lo, hi = rec["lo"], rec["hi"]
    if len(lo) == 0:
        return out
    for s in range(0, len(o), chunk):
        so, sd = o[s:s + chunk], d[s:s + chunk]
        with np.errstate(all="ignore"):
            slo, shi = segment_boxes(so, sd, tmin, tmax)
        cand = np.ones((len(so), len(lo)), dtype=bool)
        for k in range(3):
            cand &= (slo[:, None, k] <= hi[None, :, k]) & (shi[:, None, k] >= lo[None, :, k])
        ri, ti = np.nonzero(cand)
        if len(ri) == 0:
            continue
        ok, t, u, v = frozen_hit_tuv(so[ri], sd[ri], tmin, tmax, rec["v0"][ti], rec["e1"][ti], rec["e2"][ti], lo[ti], hi[ti])
        ri, ti, t, u, v = ri[ok], ti[ok], t[ok], u[ok], v[ok]
        if len(ri) == 0:
            continue
        key = t + F32(0.0)  # -0 -> +0: equal t in the sense of ==
        order = np.lexsort((ti, key, ri))  # by ray, then t, then input index
        first = order[np.concatenate([[True], ri[order][1:] != ri[order][:-1]])]
        dst = s + ri[first]
        out["t"][dst], out["u"][dst], out["v"][dst], out["index"][dst] = t[first], u[first], v[first], ti[first]
    return out
