"""Numpy restatement of vkr_shadow_mask_filter (csrc/shadow_mask_filter.hip; DESIGN_NUMERICS.md, Shadow mask, filter) — the checker
of tests/test_shadow_mask_filter.py and tests/test_shadow_mask_filter_gpu.py.

Test infrastructure, like the oracle: the product package never imports it.  The surface point of a pixel (world position and
normal) is tests/shadow_mask_rt_reference.py's pixel_surface, the arithmetic its Arith(contract); what is restated here is the
pass: the view depth of the pixel, the accept test of a tap in its frozen order, and the integer mean."""
import numpy as np

from shadow_mask_rt_reference import Arith, F32, d24_to_float, pixel_surface  # noqa: F401


def view_z(ar, depth_words, znear, zfar):
    """view_g.z of reconstruct_view_vec: (n * f) / fma(d, f - n, -f)"""
    d = d24_to_float(np.asarray(depth_words, np.uint32))
    n_, f_ = F32(znear), F32(zfar)
    with np.errstate(all="ignore"):
        return ((n_ * f_) / ar.cfma(d, f_ - n_, -f_)).astype(F32)


def tap_weight(reach, dx, dy):
    return (reach - abs(dx)) * (reach - abs(dy))


def accept_sets(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, reach, normal_min_dot, plane_tolerance):
    """-> {(dx, dy): bool [h, w]}: whether pixel g accepts tap g + (dx, dy), for every |dx|, |dy| < reach; sky [h, w]"""
    h, w = depth_words.shape
    sky, world, normal, _ = pixel_surface(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, 0.0)
    with np.errstate(all="ignore"):
        bound = (F32(plane_tolerance) * np.abs(view_z(ar, depth_words, znear, zfar))).astype(F32)
    taps = {}
    B = reach - 1
    for dy in range(-B, B + 1):
        for dx in range(-B, B + 1):
            acc = np.zeros((h, w), bool)
            if dx == 0 and dy == 0:
                acc[:] = True  # the centre, whatever its values are
            else:
                # the pixels g whose tap lies inside the image, and that tap
                gy0, gy1, gx0, gx1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
                if gy0 < gy1 and gx0 < gx1:
                    g = (slice(gy0, gy1), slice(gx0, gx1))
                    t = (slice(gy0 + dy, gy1 + dy), slice(gx0 + dx, gx1 + dx))
                    with np.errstate(all="ignore"):
                        ndot = ar.dot(normal[g], normal[t])
                        diff = (world[t] - world[g]).astype(F32)  # three subtractions
                        pdot = ar.dot(normal[g], diff)
                        ok = ~sky[t] & (ndot >= F32(normal_min_dot)) & (np.abs(pdot) <= bound[g])  # a compare with a NaN is false
                    acc[g] = ok
            taps[(dx, dy)] = acc
    return taps, sky


def shadow_mask_filter(ar, depth_words, normal_codes, mask, inverse_camera, fovy, aspect, znear, zfar, reach, normal_min_dot, plane_tolerance,
                       with_range=False):
    """the whole pass: uint8 [h, w, 4] as vkr_shadow_mask_filter writes out_mask.  depth_words: raw D24S8 texels [h, w];
    normal_codes: raw RG16_UNORM texels [h, w, 2]; mask: uint8 [h, w, 4].  with_range: also the smallest and the largest accepted
    tap per pixel and channel, and the sum of the accepted weights."""
    h, w = depth_words.shape
    mask = np.asarray(mask, np.uint8)
    taps, sky = accept_sets(ar, depth_words, normal_codes, inverse_camera, fovy, aspect, znear, zfar, reach, normal_min_dot, plane_tolerance)
    A = np.zeros((h, w), np.uint64)
    V = np.zeros((h, w, 4), np.uint64)
    lo = np.full((h, w, 4), 255, np.uint8)
    hi = np.zeros((h, w, 4), np.uint8)
    padded = np.zeros((h + 2 * reach, w + 2 * reach, 4), np.uint8)
    padded[reach:reach + h, reach:reach + w] = mask
    for (dx, dy), acc in taps.items():
        wgt = np.uint64(tap_weight(reach, dx, dy))
        tap = padded[reach + dy:reach + dy + h, reach + dx:reach + dx + w]
        A += wgt * acc.astype(np.uint64)
        V += wgt * (acc[..., None] * tap.astype(np.uint64))
        lo = np.where(acc[..., None], np.minimum(lo, tap), lo)
        hi = np.where(acc[..., None], np.maximum(hi, tap), hi)
    assert (A >= np.uint64(reach * reach)).all()
    out = ((np.uint64(2) * V + A[..., None]) // (np.uint64(2) * A[..., None])).astype(np.uint8)
    out[sky] = mask[sky]
    if with_range:
        lo[sky] = mask[sky]
        hi[sky] = mask[sky]
        return out, lo, hi, A
    return out
