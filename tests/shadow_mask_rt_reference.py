"""Numpy restatement of program shadow_mask_rt (csrc/shadow_mask_rt.hip; DESIGN_NUMERICS.md, Shadow mask, ray traced) — the
checker of tests/test_shadow_mask_rt.py and tests/test_shadow_mask_rt_gpu.py.

Test infrastructure, like the oracle: the product package never imports it.  The arithmetic (Arith, the storage decodes,
decode_normal, the frozen triangle test and its brute force) is that of tests/gtao_rt_reference.py; what is restated here is
the pass: depth and normal read by index, the view -> world transform, the offset origin, one ray per light.
"""
import numpy as np

from gtao_rt_reference import (_LIBM, Arith, F32, brute_force_any_hit, d24_to_float, decode_normal, triangle_records,  # noqa: F401
                               unorm16_to_float)


def pixel_surface(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, normal_offset):
    """steps 1-4 for every pixel: -> (sky [h, w] bool, world [h, w, 3], normal [h, w, 3], origin [h, w, 3]).  depth_words: raw
    D24S8 texels [h, w] (the top byte is ignored); normal_codes: raw RG16_UNORM texels [h, w, 2]; inverse_camera: 4x4 maths
    convention.  Shared with tests/reflections_rt_reference.py (csrc/rt_surface.hpp is what the two kernels share)."""
    h, w = depth_words.shape
    gy, gx = np.mgrid[0:h, 0:w]
    uvx = ((gx.astype(F32) + F32(0.5)) / F32(w)).astype(F32)
    uvy = ((gy.astype(F32) + F32(0.5)) / F32(h)).astype(F32)
    d = d24_to_float(np.asarray(depth_words, np.uint32))
    sky = d >= F32(1.0)
    tg = F32(_LIBM.tanf(float(F32(fovy) / F32(2.0))))
    n_, f_ = F32(znear), F32(zfar)
    with np.errstate(all="ignore"):
        z = (n_ * f_) / ar.cfma(d, f_ - n_, -f_)
        xd = ar.cfma(F32(2.0), uvx, F32(-1.0))
        yd = ar.cfma(F32(2.0), uvy, F32(-1.0))
        vx = -xd * ((z * F32(aspect)) * tg)
        vy = -yd * (z * tg)
        M = np.asarray(inverse_camera, F32)
        world = np.stack([ar.cfma(M[r, 3], F32(1.0), ar.cfma(M[r, 2], z, ar.cfma(M[r, 1], vy, M[r, 0] * vx))) for r in range(3)], axis=-1).astype(F32)
        normal = decode_normal(ar, unorm16_to_float(np.asarray(normal_codes))).astype(F32)
        origin = ar.madd(world, F32(normal_offset), normal).astype(F32)
    return sky, world, normal, origin


def pixel_origins(*args):
    """pixel_surface as the shadow pass needs it: -> (sky, origin, normal)"""
    sky, _, normal, origin = pixel_surface(*args)
    return sky, origin, normal


def light_rays(ar, origin, normal, light):
    """step 5 for one light (x, y, z, w) and P pixels: -> (dvec [P, 3], cast [P] bool: facing > 0)"""
    xyz = np.asarray(light[:3], F32)
    with np.errstate(all="ignore"):
        dvec = (xyz[None, :] - origin) if float(light[3]) != 0.0 else np.broadcast_to(xyz, origin.shape).astype(F32)
        facing = ar.dot(normal, dvec.astype(F32))
    return dvec.astype(F32), facing > 0  # NaN > 0 is False


def shadow_mask_rt(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, lights, normal_offset, tmin, tris):
    """the whole pass: uint8 [h, w, 4] as vkr_shadow_mask_rt writes out_mask.  lights: 1..4 of (x, y, z, w); tris: the
    world-space triangles (n, 3, 3) the structure was built from."""
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
            hit[idx] = brute_force_any_hit(o[idx], dvec[idx], tmin, 1.0, rec)
        out[:, l] = np.where(live, np.where(cast & ~hit, 255, 0), 255).astype(np.uint8)
    return out.reshape(h, w, 4)
