"""Numpy restatement of program reflections_rt (csrc/reflections_rt.hip; DESIGN_NUMERICS.md, Reflections, ray traced) — the
checker of tests/test_reflections_rt_gpu.py.

Test infrastructure, like the oracle: the product package never imports it.  The arithmetic (Arith, the storage decodes,
decode_normal) is that of tests/gtao_rt_reference.py, the ray query the brute force of tests/closest_hit_reference.py, the
texture sampler (REPEAT, bilinear, sRGB decode through the library's table) that of tests/cubemap_reference.py; what is restated
here is the pass: the surface of a pixel (tests/shadow_mask_rt_reference.py pixel_surface: depth and normal read by index, the
view -> world transform, the offset origin), the mirror direction about the normal, the closest hit, the interpolated uv and the
albedo there.
"""
import numpy as np

from closest_hit_reference import MISS, brute_force_closest
from cubemap_reference import _sample_level
from gtao_rt_reference import Arith, F32, triangle_records  # noqa: F401
from probe_reference import float_to_unorm
from shadow_mask_rt_reference import pixel_surface

FILL_MISSES = 1


def pixel_rays(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, normal_offset):
    """steps 1-12 for every pixel: -> (sky [h, w] bool, origin [h, w, 3], dir [h, w, 3], cast [h, w] bool: dot(n, dir) > 0).
    depth_words: raw D24S8 texels [h, w] (the top byte is ignored); normal_codes: raw RG16_UNORM texels [h, w, 2];
    inverse_camera: 4x4 maths convention."""
    sky, world, normal, origin = pixel_surface(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, normal_offset)
    with np.errstate(all="ignore"):
        eye = np.asarray(inverse_camera, F32)[:3, 3]  # the translation column, read
        view = (world - eye[None, None, :]).astype(F32)
        s = -(F32(2.0) * ar.dot(normal, view))
        refl = ar.cfma(np.broadcast_to(s[..., None], normal.shape), normal, view)  # reflect(): V + (-(2 n.V)) n, one multiply-add each
        direction = ar.normalize(refl.astype(F32)).astype(F32)
        cast = ar.dot(normal, direction) > 0  # NaN > 0 is False
    return sky, origin, direction, cast


def shade(ar, hits, attribs, textures, texture_lod):
    """step 15 for the rays that hit: hits HIT_DTYPE [n] (no misses), attribs hit_attrib records of every input triangle, textures a
    list of mip chains (lists of uint8 [h, w, 4] levels) -> uint8 [n, 4] (alpha 0)"""
    a = attribs[hits["index"]]
    u, v = hits["u"], hits["v"]
    w = (F32(1.0) - u) - v
    uv = [(w * a["uv"][:, 0, c] + u * a["uv"][:, 1, c]) + v * a["uv"][:, 2, c] for c in range(2)]
    out = np.zeros((len(hits), 4), np.uint8)
    out[:, :3] = float_to_unorm(np.full(3, 0.5, F32), 8)
    for ti in np.unique(a["albedo_index"]):
        if int(ti) >= len(textures):  # 0xFFFFFFFF or beyond the table: grey
            continue
        sel = np.nonzero(a["albedo_index"] == ti)[0]
        levels = textures[int(ti)]
        level = levels[min(int(texture_lod), len(levels) - 1)]
        rgba = _sample_level(ar, level, uv[0][sel].astype(F32), uv[1][sel].astype(F32))
        out[sel, :3] = float_to_unorm(rgba[:, :3], 8)
    return out


def reflections_rt(ar, depth_words, normal_codes, rays_w, inverse_camera, fovy, aspect, znear, zfar, normal_offset, tmin, max_distance,
                   texture_lod, flags, tris, attribs, textures, before):
    """the whole pass: uint8 [h, w, 4] as vkr_reflections_rt leaves out_reflections, whose content before the call is `before`
    (uint8 [h, w, 4]; only fill mode keeps any of it).  rays_w: the .w codes of `rays` [h, w] uint16 (None without the flag);
    tris: the world-space triangles (n, 3, 3) the structure was built from, attribs their records.  -> (image, traced [h, w] bool:
    the pixels that cast a ray, hit index [h, w] uint32)"""
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
        hits = brute_force_closest(origin.reshape(-1, 3)[idx], direction.reshape(-1, 3)[idx], tmin, max_distance, triangle_records(tris))
        found = hits["index"] != MISS
        index[idx[found]] = hits["index"][found]
        if found.any():
            out[idx[found]] = shade(ar, hits[found], attribs, textures, texture_lod)
    return out.reshape(h, w, 4), traced.reshape(h, w), index.reshape(h, w)
