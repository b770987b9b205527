"""Numpy restatement of alpha cutouts in the ray query (csrc/ray_cutout.hpp, csrc/accel_cutout.hip; DESIGN_NUMERICS.md, "Ray
query, cutouts") — the checker of tests/test_ray_cutout.py, tests/test_ray_cutout_gpu.py and tests/test_ray_cutout_passes_gpu.py.

Test infrastructure, like the oracle: the product package never imports it.  No hierarchy here: the frozen triangle test of
tests/gtao_rt_reference.py against ALL triangles gives every candidate (ray, triangle, t, u, v); a candidate is dropped when it is
transparent (its triangle's albedo texture exists, is not masked opaque, and the alpha of the bilinear REPEAT sample of tests/
cubemap_reference.py at the uv of tests/reflections_rt_reference.py is exactly 0); the any hit is "a candidate is left", the closest
hit the smallest t and of equal t (==) the smallest input index among those left.  The two passes are those of
tests/shadow_mask_rt_reference.py and tests/reflections_rt_reference.py with these queries in the place of the opaque ones.
"""
import numpy as np

from closest_hit_reference import HIT_DTYPE, MISS
from cubemap_reference import _sample_level
from gtao_rt_reference import Arith, F32, frozen_hit_tuv, segment_boxes, triangle_records  # noqa: F401
from reflections_rt_reference import FILL_MISSES, pixel_rays, shade
from shadow_mask_rt_reference import light_rays, pixel_origins


def hit_uv(attribs, index, u, v):
    """uv_hit of candidates (index, u, v): w = (1 - u) - v, (w uv0 + u uv1) + v uv2 per component, every operation rounded"""
    a = attribs["uv"][index]
    with np.errstate(all="ignore"):
        w = (F32(1.0) - u) - v
        return [((w * a[:, 0, c] + u * a[:, 1, c]) + v * a[:, 2, c]).astype(F32) for c in range(2)]


def transparent(ar, index, u, v, attribs, textures, alpha_lod, opaque_mask):
    """bool [n]: candidate k (triangle index[k] at (u[k], v[k])) is a hole.  textures: a list of mip chains (lists of uint8
    [h, w, 4] levels); an albedo_index at or beyond len(textures) (0xFFFFFFFF too) and a set mask bit are opaque; alpha == 0 is
    False for a NaN"""
    index = np.asarray(index, np.int64)
    out = np.zeros(len(index), bool)
    if len(index) == 0:
        return out
    ti = attribs["albedo_index"][index]
    uv = hit_uv(attribs, index, np.asarray(u, F32), np.asarray(v, F32))
    for t in np.unique(ti):
        if int(t) >= len(textures) or (int(opaque_mask) >> int(t)) & 1:
            continue
        sel = np.nonzero(ti == t)[0]
        levels = textures[int(t)]
        level = levels[min(int(alpha_lod), len(levels) - 1)]
        with np.errstate(all="ignore"):
            alpha = _sample_level(ar, level, uv[0][sel], uv[1][sel])[:, 3]
        out[sel] = alpha == F32(0.0)
    return out


def _candidates(o, d, tmin, tmax, rec):
    """every (ray, triangle) the frozen test accepts: -> (ray [m], triangle [m], t, u, v)"""
    lo, hi = rec["lo"], rec["hi"]
    with np.errstate(all="ignore"):
        slo, shi = segment_boxes(o, d, tmin, tmax)
    cand = np.ones((len(o), len(lo)), dtype=bool)
    for k in range(3):
        cand &= (slo[:, None, k] <= hi[None, :, k]) & (shi[:, None, k] >= lo[None, :, k])
    ri, ti = np.nonzero(cand)  # outside the segment box the test's own last clause fails: the exact answer
    if len(ri) == 0:
        z = np.zeros(0, F32)
        return ri, ti, z, z, z
    ok, t, u, v = frozen_hit_tuv(o[ri], d[ri], tmin, tmax, rec["v0"][ti], rec["e1"][ti], rec["e2"][ti], lo[ti], hi[ti])
    return ri[ok], ti[ok], t[ok], u[ok], v[ok]


def brute_force_closest_cutout(ar, o, d, tmin, tmax, rec, attribs, textures, alpha_lod=0, opaque_mask=0, chunk=512):
    """the closest hit that sees holes, of every ray against every triangle: -> HIT_DTYPE [n]; a miss is (0, 0, 0, MISS)"""
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    out = np.zeros(len(o), HIT_DTYPE)
    out["index"] = MISS
    if len(rec["lo"]) == 0:
        return out
    for s in range(0, len(o), chunk):
        ri, ti, t, u, v = _candidates(o[s:s + chunk], d[s:s + chunk], tmin, tmax, rec)
        keep = ~transparent(ar, ti, u, v, attribs, textures, alpha_lod, opaque_mask)
        ri, ti, t, u, v = ri[keep], ti[keep], t[keep], u[keep], v[keep]
        if len(ri) == 0:
            continue
        key = t + F32(0.0)  # -0 -> +0: equal t in the sense of ==
        order = np.lexsort((ti, key, ri))  # by ray, then t, then input index
        first = order[np.concatenate([[True], ri[order][1:] != ri[order][:-1]])]
        dst = s + ri[first]
        out["t"][dst], out["u"][dst], out["v"][dst], out["index"][dst] = t[first], u[first], v[first], ti[first]
    return out


def brute_force_any_hit_cutout(ar, o, d, tmin, tmax, rec, attribs, textures, alpha_lod=0, opaque_mask=0, chunk=512):
    """the any hit that sees holes: bool [n]"""
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    out = np.zeros(len(o), bool)
    if len(rec["lo"]) == 0:
        return out
    for s in range(0, len(o), chunk):
        ri, ti, t, u, v = _candidates(o[s:s + chunk], d[s:s + chunk], tmin, tmax, rec)
        keep = ~transparent(ar, ti, u, v, attribs, textures, alpha_lod, opaque_mask)
        out[s + ri[keep]] = True
    return out


def shadow_mask_rt_cutout(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, lights, normal_offset, tmin, tris, attribs,
                          textures, alpha_lod=0, opaque_mask=0):
    """vkr_shadow_mask_rt_cutout: uint8 [h, w, 4]; shadow_mask_rt_reference.shadow_mask_rt with the any hit that sees holes"""
    h, w = depth_words.shape
    sky, origin, normal = pixel_origins(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, normal_offset)
    rec = triangle_records(tris)
    out = np.full((h * w, 4), 255, np.uint8)
    live = ~sky.reshape(-1)
    o, n = origin.reshape(-1, 3), normal.reshape(-1, 3)
    for l, light in enumerate(lights):
        dvec, cast = light_rays(ar, o, n, light)
        cast &= live
        idx = np.nonzero(cast)[0]
        hit = np.zeros(h * w, dtype=bool)
        if len(idx) and len(rec["lo"]):
            hit[idx] = brute_force_any_hit_cutout(ar, o[idx], dvec[idx], tmin, 1.0, rec, attribs, textures, alpha_lod, opaque_mask)
        out[:, l] = np.where(live, np.where(cast & ~hit, 255, 0), 255).astype(np.uint8)
    return out.reshape(h, w, 4)


def reflections_rt_cutout(ar, depth_words, normal_codes, rays_w, inverse_camera, fovy, aspect, znear, zfar, normal_offset, tmin, max_distance,
                          texture_lod, flags, tris, attribs, textures, before, alpha_lod=0, opaque_mask=0):
    """vkr_reflections_rt_cutout: reflections_rt_reference.reflections_rt with the closest hit that sees holes -> (image, traced
    [h, w] bool, hit index [h, w] uint32)"""
    h, w = depth_words.shape
    sky, origin, direction, cast = pixel_rays(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, normal_offset)
    keep = np.zeros((h, w), bool)
    if flags & FILL_MISSES:
        keep = ~sky & (np.asarray(rays_w) != 65535)
    out = np.where(keep[..., None], np.asarray(before, np.uint8), np.uint8(0)).astype(np.uint8).reshape(h * w, 4)
    traced = (cast & ~sky & ~keep).reshape(-1)
    index = np.full(h * w, MISS, np.uint32)
    idx = np.nonzero(traced)[0]
    if len(idx) and len(tris):
        hits = brute_force_closest_cutout(ar, origin.reshape(-1, 3)[idx], direction.reshape(-1, 3)[idx], tmin, max_distance, triangle_records(tris),
                                          attribs, textures, alpha_lod, opaque_mask)
        found = hits["index"] != MISS
        index[idx[found]] = hits["index"][found]
        if found.any():
            out[idx[found]] = shade(ar, hits[found], attribs, textures, texture_lod)
    return out.reshape(h, w, 4), traced.reshape(h, w), index.reshape(h, w)
