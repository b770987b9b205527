"""Numpy restatement of program "shadow_mask" (csrc/shadow_mask.hip; DESIGN_NUMERICS.md, Shadow mask) — the checker of
tests/test_shadow_mask.py and tests/test_shadow_mask_gpu.py — and shade_interval(), the sRGB8 decode the linearity test of the
shadowed shading uses.

Test infrastructure, like tests/ssao_reference.py, whose fp32 helpers it shares: every operation in the kernel's order, a fused
multiply-add of numeric contract 2 one rounding, divisions numpy's IEEE float32, the float -> int rule of vkr_device.hpp.  The
host's part of the rule is restated too: M_l = mvps[l] * inverse_camera accumulated in double from 0.0 in the order k = 0..3
and rounded once.  The compare is done on int64: nothing wraps.  Maps and depth are raw D24S8 words; their top bytes are masked
off here as the kernel masks them."""
import numpy as np

from gtao_rt_reference import _LIBM, Arith, d24_to_float  # noqa: F401
from ssao_reference import encode_unorm8, f2i

F32 = np.float32
D24_MAX = 0x00FFFFFF


def light_matrix(mvp, inverse_camera):
    """mvp * inverse_camera (4x4, maths convention) as the entry takes it: products and sums in double, acc = 0.0, k = 0..3, one
    rounding to float32.  Infinities and NaNs fall as IEEE makes them (inf * 0 = NaN)."""
    a = np.asarray(mvp, F32).astype(np.float64)
    b = np.asarray(inverse_camera, F32).astype(np.float64)
    out = np.zeros((4, 4), F32)
    with np.errstate(all="ignore"):
        for r in range(4):
            for c in range(4):
                acc = np.float64(0.0)
                for k in range(4):
                    acc = acc + a[r, k] * b[k, c]
                out[r, c] = F32(acc)
    return out


def project(ar, depth_bits, inverse_camera, mvps, fovy, aspect, znear, zfar, size):
    """Steps 1-8 for every pixel and light -> dict of arrays: sky [h, w] (d >= 1); per light l (first axis): lit (no taps: steps
    2 and 6), code, tx, ty (meaningful where not lit), and the classes of step 6 one by one: behind (w <= 0), left / right / top /
    bottom (w > 0 and ndc.x < -1, > 1, ndc.y < -1, > 1), far (ndc.z > 1), near (tapped with ndc.z < 0), nan (any NaN)."""
    bits = np.asarray(depth_bits).astype(np.uint32)
    h, w = bits.shape
    d = d24_to_float(bits)
    sky = d >= F32(1.0)
    gy, gx = np.mgrid[0:h, 0:w]
    out = {"sky": sky}
    per = {k: [] for k in ("lit", "code", "tx", "ty", "behind", "left", "right", "top", "bottom", "far", "near", "nan")}
    with np.errstate(all="ignore"):
        uvx = ((gx.astype(F32) + F32(0.5)) / F32(w)).astype(F32)
        uvy = ((gy.astype(F32) + F32(0.5)) / F32(h)).astype(F32)
        # reconstruct_view_vec
        tg = F32(_LIBM.tanf(float(F32(fovy) / F32(2.0))))
        n_, f_ = F32(znear), F32(zfar)
        z = ((n_ * f_) / ar.cfma(d, f_ - n_, -f_)).astype(F32)
        xd = ar.cfma(F32(2.0), uvx, F32(-1.0))
        yd = ar.cfma(F32(2.0), uvy, F32(-1.0))
        view = [(-xd * ((z * F32(aspect)) * tg)).astype(F32), (-yd * (z * tg)).astype(F32), z]
        one = np.ones_like(z)
        for mvp in mvps:
            M = light_matrix(mvp, inverse_camera)
            clip = [ar.cfma(M[r, 3], one, ar.cfma(M[r, 2], view[2], ar.cfma(M[r, 1], view[1], M[r, 0] * view[0]))) for r in range(4)]
            nx, ny, nz = ((clip[i] / clip[3]).astype(F32) for i in range(3))
            behind = clip[3] <= 0
            nan = np.isnan(nx) | np.isnan(ny) | np.isnan(nz) | np.isnan(clip[3])
            left, right, top, bottom = nx < -1, nx > 1, ny < -1, ny > 1
            far = nz > 1
            lit = sky | behind | ~((nx >= -1) & (nx <= 1)) | ~((ny >= -1) & (ny <= 1)) | ~(nz <= 1)
            code = np.rint((np.clip(nz, F32(0.0), F32(1.0)).astype(F32) * F32(16777215.0)).astype(F32))
            code = np.where(lit, 0, np.nan_to_num(code)).astype(np.int64)
            fs = F32(size)
            tx = np.clip(f2i(np.floor((ar.cfma(F32(0.5), nx, F32(0.5)) * fs).astype(F32))), 0, size - 1)
            ty = np.clip(f2i(np.floor((ar.cfma(F32(0.5), ny, F32(0.5)) * fs).astype(F32))), 0, size - 1)
            live = ~sky
            vals = dict(lit=lit, code=code, tx=tx, ty=ty, behind=live & behind & ~nan, left=live & ~behind & left, right=live & ~behind & right,
                        top=live & ~behind & top, bottom=live & ~behind & bottom, far=live & ~behind & far, near=~lit & (nz < 0), nan=live & nan)
            for k, v in vals.items():
                per[k].append(v)
    for k, v in per.items():
        out[k] = np.stack(v)
    return out


def resolve(proj, maps, radius, bias, stats=None):
    """Steps 9-10 on the result of project() -> RGBA8 codes [h, w, 4] uint8.  maps: raw D24S8 words [layers >= lights, size, size].
    stats: a dict that receives `equal` and `one_above` (taps inside the map with code == d24 + bias, code == d24 + bias + 1),
    `outside_taps` and `taps` (of the pixels that take taps)."""
    lights = proj["lit"].shape[0]
    h, w = proj["sky"].shape
    words = np.asarray(maps).astype(np.int64) & D24_MAX
    size = words.shape[-1]
    out = np.full((h, w, 4), 255, np.uint8)
    taps = (2 * radius + 1) ** 2
    counts = dict(equal=0, one_above=0, outside_taps=0, taps=0)
    for l in range(lights):
        lit, code, tx, ty = proj["lit"][l], proj["code"][l], proj["tx"][l], proj["ty"][l]
        passes = np.zeros((h, w), np.int64)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                x, y = tx + dx, ty + dy
                inside = (x >= 0) & (x < size) & (y >= 0) & (y < size)
                word = words[l][np.clip(y, 0, size - 1), np.clip(x, 0, size - 1)]
                passes += ~inside | (code <= word + int(bias))
                t = inside & ~lit
                counts["equal"] += int((t & (code == word + int(bias))).sum())
                counts["one_above"] += int((t & (code == word + int(bias) + 1)).sum())
                counts["outside_taps"] += int((~inside & ~lit).sum())
        counts["taps"] += taps * int((~lit).sum())
        value = encode_unorm8(passes.astype(F32) / F32(taps))
        out[..., l] = np.where(lit, 255, value)
    if stats is not None:
        stats.update(counts)
    return out


def shadow_mask(ar, depth_bits, maps, inverse_camera, mvps, fovy, aspect, znear, zfar, radius, bias, stats=None):
    """the ten steps -> RGBA8 codes [h, w, 4]: channel l = light l for l < len(mvps), 255 beyond"""
    size = np.asarray(maps).shape[-1]
    return resolve(project(ar, depth_bits, inverse_camera, mvps, fovy, aspect, znear, zfar, size), maps, radius, bias, stats)


# ---- sRGB8 -> linear intervals (the shading's output encode: the largest code whose threshold is <= x) ----
def _srgb_thresholds():
    """the 256 float32 thresholds of csrc/srgb_tables.inc (k_srgb_thresh_bits): code i is stored for thresh[i] <= x < thresh[i + 1]"""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "vk-renderer_amd", "csrc", "srgb_tables.inc")).read()
    body = txt[txt.index("k_srgb_thresh_bits"):]
    body = body[body.index("{") + 1: body.index("}")]
    bits = np.array([int(v, 16) for v in re.findall(r"0x[0-9a-fA-F]+", body)], np.uint32)
    assert bits.size == 256
    return bits.view(F32).astype(np.float64)


_THRESH = None


def shade_interval(code):
    """(lo, hi) float64 arrays: the half-open set [lo, hi) of linear values the shading stores as sRGB8 `code`.  Code 0 takes
    everything below thresh[1] (lo = -inf); code 255 is open above (hi = +inf)."""
    global _THRESH
    if _THRESH is None:
        _THRESH = _srgb_thresholds()
    c = np.asarray(code).astype(np.int64)
    lo = np.where(c == 0, -np.inf, _THRESH[c])
    hi = np.where(c == 255, np.inf, _THRESH[np.minimum(c + 1, 255)])
    return lo, hi
