"""Numpy restatement of program reflections_rt_lit (csrc/reflections_rt_lit.hip; DESIGN_NUMERICS.md, Reflections, ray traced,
lit) — the checker of tests/test_reflections_rt_lit.py and tests/test_reflections_rt_lit_gpu.py.

Test infrastructure, like the oracle: the product package never imports it.  Everything up to the closest hit is
tests/reflections_rt_reference.py's (pixel_rays, the fill mode, brute_force_closest) or, with a cutout, tests/ray_cutout_reference.py's
(brute_force_closest_cutout); the shadow rays go through brute_force_any_hit / brute_force_any_hit_cutout.  What is restated here is
the lighting of a hit: its position, its interpolated normal turned towards the ray, the offset origin of the shadow rays, one
diffuse term per visible light with the falloff of a point light, and the albedo times ambient plus the sum.

`mutant` names one deliberate departure from the rule (MUTANTS): tests/test_reflections_rt_lit.py shows that each changes the image,
so the inputs there can tell the rule from its neighbours.
"""
import numpy as np

from closest_hit_reference import MISS, brute_force_closest
from cubemap_reference import _sample_level
from gtao_rt_reference import Arith, F32, brute_force_any_hit, triangle_records  # noqa: F401
from probe_reference import float_to_unorm
from ray_cutout_reference import brute_force_any_hit_cutout, brute_force_closest_cutout
from reflections_rt_reference import FILL_MISSES, pixel_rays

MUTANTS = ("no_flip", "shadow_from_p", "facing_ge", "no_falloff", "falloff_directional", "reverse_order", "ndl_unclamped", "no_shadows",
           "unnormalised")


def albedo(ar, hits, attribs, textures, texture_lod):
    """step 6's albedo for the rays that hit, as reflections_rt_reference.shade computes it before it quantises: float32 [n, 3]"""
    a = attribs[hits["index"]]
    u, v = hits["u"], hits["v"]
    w = (F32(1.0) - u) - v
    uv = [(w * a["uv"][:, 0, c] + u * a["uv"][:, 1, c]) + v * a["uv"][:, 2, c] for c in range(2)]
    out = np.full((len(hits), 3), 0.5, F32)
    for ti in np.unique(a["albedo_index"]):
        if int(ti) >= len(textures):  # 0xFFFFFFFF or beyond the table: grey
            continue
        sel = np.nonzero(a["albedo_index"] == ti)[0]
        levels = textures[int(ti)]
        level = levels[min(int(texture_lod), len(levels) - 1)]
        out[sel] = _sample_level(ar, level, uv[0][sel].astype(F32), uv[1][sel].astype(F32))[:, :3]
    return out


def light_hits(ar, hits, origin, direction, normals, lights, colours, ambient, shadow_offset, shadow_tmin, occluded, mutant=None):
    """steps 1-5 for the rays that hit: hits HIT_DTYPE [n] (no misses) of rays (origin [n, 3], direction [n, 3]); normals:
    hit_normal records of every input triangle; lights: 0..4 of (x, y, z, w), colours as many rgb; occluded(o [m, 3], d [m, 3]) ->
    bool [m]: the any hit of the segments o + t d, t in [shadow_tmin, 1].
    -> (acc float32 [n, 3], stats: flipped bool [n], per light (away, shadowed, lit) bool [n] each)"""
    n = len(hits)
    with np.errstate(all="ignore"):
        t, u, v = hits["t"], hits["u"], hits["v"]
        P = ar.cfma(np.broadcast_to(t[:, None], direction.shape), direction, origin).astype(F32)
        nr = normals["n"][hits["index"]][:, :, :3].astype(F32)
        w = (F32(1.0) - u) - v
        Ni = ((w[:, None] * nr[:, 0] + u[:, None] * nr[:, 1]) + v[:, None] * nr[:, 2]).astype(F32)
        Ns = Ni if mutant == "unnormalised" else ar.normalize(Ni).astype(F32)
        flipped = ar.dot(Ns, direction) > 0  # NaN > 0 is False: a NaN normal stays
        if mutant == "no_flip":
            flipped = np.zeros(n, bool)
        N = np.where(flipped[:, None], -Ns, Ns).astype(F32)
        Po = ar.madd(P, F32(shadow_offset), N).astype(F32)
        acc = np.broadcast_to(np.asarray(ambient, F32)[:3], (n, 3)).astype(F32).copy()
        stats = []
        order = range(len(lights))
        if mutant == "reverse_order":
            order = reversed(order)
        for l in order:
            light, colour = lights[l], np.asarray(colours[l], F32)
            point = float(light[3]) != 0.0
            xyz = np.asarray(light[:3], F32)
            dvec = (xyz[None, :] - Po).astype(F32) if point else np.broadcast_to(xyz, Po.shape).astype(F32)
            facing = ar.dot(N, dvec)
            live = (facing >= 0) if mutant == "facing_ge" else (facing > 0)
            shadowed = np.zeros(n, bool)
            idx = np.nonzero(live)[0]
            if len(idx) and mutant != "no_shadows":
                shadowed[idx] = occluded((P if mutant == "shadow_from_p" else Po)[idx], dvec[idx])
            lit = live & ~shadowed
            ld2 = ar.dot(dvec, dvec)
            L = ar.normalize(dvec).astype(F32)
            ndl = ar.dot(N, L).astype(F32)
            if mutant != "ndl_unclamped":
                ndl = np.where(ndl > 0, ndl, F32(0.0)).astype(F32)
            q = (F32(1.0) / ld2).astype(F32)
            fall = np.where(q < F32(1.0), q, F32(1.0)).astype(F32)
            with_falloff = (point and mutant != "no_falloff") or (not point and mutant == "falloff_directional")
            k = (ndl * fall).astype(F32) if with_falloff else ndl
            for c in range(3):
                acc[:, c] = np.where(lit, ar.cfma(k, np.broadcast_to(colour[c], k.shape), acc[:, c]), acc[:, c])
            stats.append((~live, live & shadowed, lit))
        if mutant == "reverse_order":
            stats.reverse()
    return acc, flipped, stats


def reflections_rt_lit(ar, depth_words, normal_codes, rays_w, inverse_camera, fovy, aspect, znear, zfar, normal_offset, tmin, max_distance,
                       texture_lod, flags, tris, attribs, normals, textures, before, lights, colours, ambient, shadow_offset, shadow_tmin,
                       cutout=None, mutant=None):
    """the whole pass: uint8 [h, w, 4] as vkr_reflections_rt_lit leaves out_reflections, whose content before the call is `before`;
    the arguments of reflections_rt_reference.reflections_rt, then the hit_normal records, the lights and the shadow ray's offsets.
    cutout: None, or (alpha_lod, opaque_mask): vkr_reflections_rt_lit_cutout.
    -> (image, traced [h, w] bool, hit index [h, w] uint32, info: dict of flat pixel indices `hits` and, aligned with it, `flipped`,
    `lights` [(away, shadowed, lit)] and the float `acc`)"""
    h, w = depth_words.shape
    sky, origin, direction, cast = pixel_rays(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, normal_offset)
    keep = np.zeros((h, w), bool)
    if flags & FILL_MISSES:
        keep = ~sky & (np.asarray(rays_w) != 65535)
    out = np.where(keep[..., None], np.asarray(before, np.uint8), np.uint8(0)).astype(np.uint8).reshape(h * w, 4)
    traced = (cast & ~sky & ~keep).reshape(-1)
    index = np.full(h * w, MISS, np.uint32)
    idx = np.nonzero(traced)[0]
    info = {"hits": np.zeros(0, np.int64), "flipped": np.zeros(0, bool), "lights": [], "acc": np.zeros((0, 3), F32)}
    if len(idx) and len(tris):
        rec = triangle_records(tris)
        o, d = origin.reshape(-1, 3)[idx], direction.reshape(-1, 3)[idx]
        if cutout is None:
            hits = brute_force_closest(o, d, tmin, max_distance, rec)
            occluded = lambda so, sd: brute_force_any_hit(so, sd, shadow_tmin, 1.0, rec)
        else:
            hits = brute_force_closest_cutout(ar, o, d, tmin, max_distance, rec, attribs, textures, *cutout)
            occluded = lambda so, sd: brute_force_any_hit_cutout(ar, so, sd, shadow_tmin, 1.0, rec, attribs, textures, *cutout)
        found = hits["index"] != MISS
        index[idx[found]] = hits["index"][found]
        if found.any():
            acc, flipped, stats = light_hits(ar, hits[found], o[found], d[found], normals, lights, colours, ambient, shadow_offset, shadow_tmin,
                                             occluded, mutant)
            with np.errstate(all="ignore"):
                rgb = (albedo(ar, hits[found], attribs, textures, texture_lod) * acc).astype(F32)
            out[idx[found], :3] = float_to_unorm(rgb, 8)
            info = {"hits": idx[found], "flipped": flipped, "lights": stats, "acc": acc}
    return out.reshape(h, w, 4), traced.reshape(h, w), index.reshape(h, w), info
