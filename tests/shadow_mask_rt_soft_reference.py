"""Numpy restatement of program shadow_mask_rt_soft (csrc/shadow_mask_rt_soft.hip; DESIGN_NUMERICS.md, Shadow mask, ray traced,
area lights) — the checker of tests/test_shadow_mask_rt_soft.py and tests/test_shadow_mask_rt_soft_gpu.py — and of the table
generator vkr_shadow_disk_samples.

Test infrastructure, like the oracle: the product package never imports it.  Steps 1-4 and 6 are those of
tests/shadow_mask_rt_reference.py (pixel_origins, light_rays); the tangent frame is that of tests/gtao_rt_reference.py::pixel_setup
around the normalised direction to the light; every ray is decided by the brute force over all triangles (opaque:
gtao_rt_reference.brute_force_any_hit; with cutouts: ray_cutout_reference.brute_force_any_hit_cutout).
"""
import numpy as np

from gtao_rt_reference import Arith, F32, brute_force_any_hit, triangle_records  # noqa: F401
from shadow_mask_rt_reference import light_rays, pixel_origins

GOLDEN_ANGLE = 2.399963229728653


def disk_samples(S, P):
    """the formula of vkr_shadow_disk_samples in float64, rounded to float32: [P * P, S, 2]"""
    k = np.arange(S, dtype=np.float64)
    rho = np.sqrt((k + 0.5) / float(S))
    out = np.zeros((P * P, S, 2), F32)
    for p in range(P * P):
        phi = k * GOLDEN_ANGLE + 2.0 * np.pi * float((7 * p) % (P * P)) / float(P * P)
        out[p, :, 0] = (rho * np.cos(phi)).astype(F32)
        out[p, :, 1] = (rho * np.sin(phi)).astype(F32)
    return out


def quantise(V, S):
    """(510 V + S) / (2 S) in unsigned integers: 255 V / S rounded half up"""
    V = np.asarray(V, np.int64)
    return ((510 * V + int(S)) // (2 * int(S))).astype(np.uint8)


def code_set(S):
    """every code a light with a radius can write"""
    return set(int(c) for c in quantise(np.arange(S + 1), S))


def tangent_frame(ar, n):
    """vkr_device.hpp tangent_frame(n, &T, &B) for n [.., 3]: as gtao_rt_reference.pixel_setup builds it around the normal"""
    with np.errstate(all="ignore"):
        max_xy = np.maximum(np.abs(n[..., 0]), np.abs(n[..., 1]))
        small = (max_xy < F32(0.00001))[..., None]
        t0 = np.where(small, np.array([1, 0, 0], F32), np.stack([n[..., 1], -n[..., 0], np.zeros_like(n[..., 0])], axis=-1))
        tangent = ar.normalize(t0.astype(F32))
        bitangent = ar.normalize(ar.cross(n, tangent))
        tangent = ar.normalize(ar.cross(bitangent, n))
    return tangent.astype(F32), bitangent.astype(F32)


def pattern_slots(h, w, P):
    gy, gx = np.mgrid[0:h, 0:w]
    return ((gy & (P - 1)) * P + (gx & (P - 1))).reshape(-1)


def sample_rays(ar, origin, normal, light, radius, uv):
    """step 5 for one light with a radius and one sample per pixel: uv [N, 2] -> (dvec_k [N, 3], cast [N])"""
    dvec, _ = light_rays(ar, origin, normal, light)
    with np.errstate(all="ignore"):
        T, B = tangent_frame(ar, ar.normalize(dvec).astype(F32))
        u, v = uv[:, 0:1].astype(F32), uv[:, 1:2].astype(F32)
        shape = dvec.shape
        e = ar.cfma(np.broadcast_to(v, shape), B, np.broadcast_to(u, shape) * T).astype(F32)
        dk = ar.cfma(np.broadcast_to(F32(radius), shape), e, dvec).astype(F32)
        facing = ar.dot(normal, dk)
    return dk, facing > 0  # NaN > 0 is False


def shadow_mask_rt_soft(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, lights, normal_offset, tmin, tris, radii,
                        samples, any_hit=None):
    """the whole pass: uint8 [h, w, 4] as vkr_shadow_mask_rt_soft writes out_mask.  radii: one per light; samples: float32
    [P * P, S, 2]; any_hit(o, d, tmin, tmax, rec) -> bool [n]: the decision of a ray (default: the opaque brute force)."""
    if any_hit is None:
        any_hit = brute_force_any_hit
    samples = np.asarray(samples, F32)
    PP, S, _ = samples.shape
    P = {1: 1, 4: 2, 16: 4}[PP]
    h, w = depth_words.shape
    sky, origin, normal = pixel_origins(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, normal_offset)
    rec = triangle_records(tris)
    out = np.full((h * w, 4), 255, np.uint8)
    live = ~sky.reshape(-1)
    o, n = origin.reshape(-1, 3), normal.reshape(-1, 3)
    slot = pattern_slots(h, w, P)

    def visible(dvec, cast):
        idx = np.nonzero(cast)[0]
        hit = np.zeros(h * w, dtype=bool)
        if len(idx) and len(rec["lo"]):
            hit[idx] = any_hit(o[idx], dvec[idx], tmin, 1.0, rec)
        return cast & ~hit

    for l, light in enumerate(lights):
        if float(radii[l]) == 0.0:  # the hard pass's step 5
            dvec, cast = light_rays(ar, o, n, light)
            code = np.where(visible(dvec, cast & live), 255, 0).astype(np.uint8)
        else:
            V = np.zeros(h * w, np.int64)
            for k in range(S):
                dk, cast = sample_rays(ar, o, n, light, radii[l], samples[slot, k])
                V += visible(dk, cast & live)
            code = quantise(V, S)
        out[:, l] = np.where(live, code, 255).astype(np.uint8)
    return out.reshape(h, w, 4)


def shadow_mask_rt_soft_cutout(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, lights, normal_offset, tmin, tris, radii,
                               samples, attribs, textures, alpha_lod=0, opaque_mask=0):
    """vkr_shadow_mask_rt_soft_cutout: the same with the any hit that sees holes (tests/ray_cutout_reference.py)"""
    from ray_cutout_reference import brute_force_any_hit_cutout

    def any_hit(o, d, tmin_, tmax, rec):
        return brute_force_any_hit_cutout(ar, o, d, tmin_, tmax, rec, attribs, textures, alpha_lod, opaque_mask)

    return shadow_mask_rt_soft(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, lights, normal_offset, tmin, tris, radii,
                               samples, any_hit)
