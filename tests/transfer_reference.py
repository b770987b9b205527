"""Numpy restatement of the image transfers (csrc/transfer.hip: vkr_clear_image, vkr_blit_image, vkr_gen_mipmaps) — the checker
of tests/test_transfer.py, tests/test_transfer_gpu.py and, on the constructed cases of tests/transfer_cases.py,
tests/test_transfer_cases.py (which also replaces the helpers below one at a time by wrong rules) and tests/test_transfer_cases_gpu.py.

Test infrastructure, like the oracle: the product package never imports it.  Every fp32 operation is written in the order
DESIGN_NUMERICS.md ("Image transfers") gives; the fused multiply-adds of numeric contract 2 (the accumulation of the bilinear
mix) go through Arith / fma32 of gtao_rt_reference.py.  Texels are arrays [h, w, channels] of the storage type (RAW_DTYPE).
The sRGB tables are the ones the kernels are built with (csrc/srgb_tables.inc)."""
import os
import re

import numpy as np

from gtao_rt_reference import Arith, fma32

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

(FMT_D24_UNORM_S8, FMT_RG16_UNORM, FMT_RG16_SFLOAT, FMT_RGBA8_SRGB, FMT_RGBA8_UNORM, FMT_RGBA16_UNORM, FMT_RGBA16_SFLOAT, FMT_R16_SFLOAT,
 FMT_R32_SFLOAT, FMT_R8_UNORM, FMT_RGBA32_SFLOAT, FMT_R16_UNORM) = range(1, 13)
NEAREST, LINEAR = 0, 1

# format: (storage dtype, channels)
RAW_DTYPE = {
    FMT_D24_UNORM_S8: (np.uint32, 1), FMT_RG16_UNORM: (np.uint16, 2), FMT_RG16_SFLOAT: (np.float16, 2), FMT_RGBA8_SRGB: (np.uint8, 4),
    FMT_RGBA8_UNORM: (np.uint8, 4), FMT_RGBA16_UNORM: (np.uint16, 4), FMT_RGBA16_SFLOAT: (np.float16, 4), FMT_R16_SFLOAT: (np.float16, 1),
    FMT_R32_SFLOAT: (np.float32, 1), FMT_R8_UNORM: (np.uint8, 1), FMT_RGBA32_SFLOAT: (np.float32, 4), FMT_R16_UNORM: (np.uint16, 1),
}
COLOR_FORMATS = sorted(f for f in RAW_DTYPE if f != FMT_D24_UNORM_S8)
MIP_FORMATS = [FMT_RGBA8_SRGB, FMT_RGBA8_UNORM, FMT_RGBA16_SFLOAT, FMT_RG16_SFLOAT, FMT_R16_SFLOAT, FMT_R32_SFLOAT, FMT_R8_UNORM]


def _table(name):
    txt = open(os.path.join(ROOT, "vk-renderer_amd", "csrc", "srgb_tables.inc")).read()
    body = re.search(name + r"\[256\] = \{(.*?)\};", txt, re.S).group(1)
    return np.array([int(v.rstrip("u"), 16) for v in re.findall(r"0x[0-9a-fA-F]+u?", body)], dtype=np.uint32).view(F32)


SRGB_DECODE = _table("k_srgb_decode_bits")
SRGB_THRESH = _table("k_srgb_thresh_bits")
assert SRGB_DECODE.shape == (256,) and SRGB_THRESH.shape == (256,)


# ---- codecs ---------------------------------------------------------------------------------------------------------------
def unorm_to_float(v, bits):
    """the correctly rounded k / (2^bits - 1), as the kernels compute it: x = k * 2^-bits, fma(x, C, x)"""
    c = {8: np.array([0x3B808081], np.uint32).view(F32)[0], 16: F32(2.0 ** -16 + 2.0 ** -32)}[bits]
    x = np.asarray(v).astype(F32) * F32(2.0 ** -bits)
    return fma32(x, c, x)


def float_to_unorm(f, bits):
    """rint(clamp(f, 0, 1) * (2^bits - 1)); fmaxf(NaN, 0) is 0"""
    f = np.asarray(f, F32)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(f), F32(0.0), np.minimum(np.maximum(f, F32(0.0)), F32(1.0))).astype(F32)
    return np.rint(c * F32(2 ** bits - 1)).astype(np.uint32)


def float_to_srgb8(x):
    """largest code whose threshold is <= x (NaN -> 0); threshold 0 is never compared"""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        code = np.searchsorted(SRGB_THRESH[1:], x, side="right")
    return np.where(np.isnan(x), 0, code).astype(np.uint32)


def half_to_float(h):
    """fp16 -> fp32: exact, denormals included"""
    return np.asarray(h, np.float16).astype(F32)


def float_to_half(x):
    """fp32 -> fp16: round to nearest even, denormals kept, overflow (65520 and above) to infinity"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, F32).astype(np.float16)


ABSENT_ALPHA = F32(1.0)  # the alpha a format without an alpha channel decodes to (absent r, g, b: 0)


def decode(fmt, raw):
    """texels [h, w, c] of the storage type -> float32 RGBA [h, w, 4], absent channels 0, 0, 0, 1"""
    raw = np.asarray(raw)
    h, w = raw.shape[:2]
    out = np.zeros((h, w, 4), F32)
    out[..., 3] = ABSENT_ALPHA
    if fmt in (FMT_RG16_UNORM, FMT_RGBA16_UNORM, FMT_R16_UNORM):
        out[..., :raw.shape[2]] = unorm_to_float(raw, 16)
    elif fmt in (FMT_RGBA8_UNORM, FMT_R8_UNORM):
        out[..., :raw.shape[2]] = unorm_to_float(raw, 8)
    elif fmt == FMT_RGBA8_SRGB:
        out[..., :3] = SRGB_DECODE[raw[..., :3]]
        out[..., 3] = unorm_to_float(raw[..., 3], 8)
    elif fmt in (FMT_RG16_SFLOAT, FMT_RGBA16_SFLOAT, FMT_R16_SFLOAT, FMT_R32_SFLOAT, FMT_RGBA32_SFLOAT):
        out[..., :raw.shape[2]] = half_to_float(raw) if raw.dtype == np.float16 else raw
    else:
        raise ValueError(fmt)
    return out


def encode(fmt, rgba):
    """float32 RGBA [h, w, 4] -> texels [h, w, c] of the storage type, by the format's store rule"""
    rgba = np.asarray(rgba, F32)
    dt, c = RAW_DTYPE[fmt]
    if fmt in (FMT_RG16_UNORM, FMT_RGBA16_UNORM, FMT_R16_UNORM):
        return float_to_unorm(rgba[..., :c], 16).astype(dt)
    if fmt in (FMT_RGBA8_UNORM, FMT_R8_UNORM):
        return float_to_unorm(rgba[..., :c], 8).astype(dt)
    if fmt == FMT_RGBA8_SRGB:
        out = np.empty(rgba.shape[:2] + (4,), np.uint8)
        out[..., :3] = float_to_srgb8(rgba[..., :3])
        out[..., 3] = float_to_unorm(rgba[..., 3], 8)
        return out
    if fmt in (FMT_RG16_SFLOAT, FMT_RGBA16_SFLOAT, FMT_R16_SFLOAT):
        return float_to_half(rgba[..., :c])
    if fmt in (FMT_R32_SFLOAT, FMT_RGBA32_SFLOAT):
        return rgba[..., :c].copy()
    raise ValueError(fmt)


# ---- clear ----------------------------------------------------------------------------------------------------------------
def depth_to_d24(depth):
    """rint(clamp(depth, 0, 1) * 16777215), the product in fp32; NaN -> 0 (fmaxf(NaN, 0) is 0), as for every UNORM store"""
    return int(float_to_unorm(depth, 24))


def clear_texel(fmt, color=(0.0, 0.0, 0.0, 0.0), depth=1.0, stencil=0):
    """the stored texel [c] every texel of every mip holds after vkr_clear_image"""
    if fmt == FMT_D24_UNORM_S8:
        return np.array([depth_to_d24(depth) | ((int(stencil) & 0xFF) << 24)], np.uint32)
    return encode(fmt, np.array(color, F32).reshape(1, 1, 4))[0, 0]


# ---- blit -----------------------------------------------------------------------------------------------------------------
def _coords(dst_n, src_n):
    scale = F32(src_n) / F32(dst_n)                       # one IEEE division on the host
    return (np.arange(dst_n).astype(F32) + F32(0.5)) * scale  # u = (i + 0.5) * scale: an add and a multiply, nothing fused


def linear_coords(dst_n, src_n):
    """x = u - 0.5: a subtraction of its own, not fused with the multiply of u"""
    return _coords(dst_n, src_n) - F32(0.5)


floor = np.floor  # step 3 and step 4: floor, not truncation (x is negative in the first texels of a magnifying blit)


def mix(ar, a, b, t):
    """the sampler's mixf; every tap is multiplied, a weight of 0 included (0 * inf is NaN)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return ar.mixf(a, b, t)


def bilinear(ar, t00, t10, t01, t11, wx, wy):
    """rows first, then columns"""
    return mix(ar, mix(ar, t00, t10, wx), mix(ar, t01, t11, wx), wy)


def blit(src_raw, src_fmt, dst_w, dst_h, dst_fmt, filt, contract=2):
    """vkr_blit_image: whole `src_raw` [h, w, c] onto a dst_w x dst_h image of dst_fmt -> texels [dst_h, dst_w, c']"""
    src_raw = np.asarray(src_raw)
    sh, sw = src_raw.shape[:2]
    u, v = _coords(dst_w, sw), _coords(dst_h, sh)
    if src_fmt == FMT_D24_UNORM_S8:
        assert dst_fmt == FMT_D24_UNORM_S8 and filt == NEAREST and (sw, sh) == (dst_w, dst_h)
        return src_raw.copy()
    img = decode(src_fmt, src_raw)
    if filt == NEAREST:
        sx = np.clip(floor(u).astype(np.int64), 0, sw - 1)
        sy = np.clip(floor(v).astype(np.int64), 0, sh - 1)
        return encode(dst_fmt, img[sy][:, sx])
    ar = Arith(contract)
    xf, yf = linear_coords(dst_w, sw), linear_coords(dst_h, sh)
    x0f, y0f = floor(xf), floor(yf)
    fx, fy = (xf - x0f).astype(F32), (yf - y0f).astype(F32)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    xa, xb = np.clip(x0, 0, sw - 1), np.clip(x0 + 1, 0, sw - 1)
    ya, yb = np.clip(y0, 0, sh - 1), np.clip(y0 + 1, 0, sh - 1)
    t00, t10, t01, t11 = img[ya][:, xa], img[ya][:, xb], img[yb][:, xa], img[yb][:, xb]
    wx = np.broadcast_to(fx[None, :, None], t00.shape)
    wy = np.broadcast_to(fy[:, None, None], t00.shape)
    # mixf(a, b, t) = cfma(b, t, a * (1 - t)): the accumulation is the fused step
    return encode(dst_fmt, bilinear(ar, t00, t10, t01, t11, wx, wy))


# ---- the mip chain --------------------------------------------------------------------------------------------------------
def mip_taps(lin):
    """the four taps a, b, c, d of every destination texel: (2X, 2Y), (x1, 2Y), (2X, y1), (x1, y1), x1 and y1 clamped to the edge"""
    sh, sw = lin.shape[:2]
    dh, dw = max(1, sh // 2), max(1, sw // 2)
    y0, y1 = np.minimum(2 * np.arange(dh), sh - 1), np.minimum(2 * np.arange(dh) + 1, sh - 1)
    x0, x1 = np.minimum(2 * np.arange(dw), sw - 1), np.minimum(2 * np.arange(dw) + 1, sw - 1)
    return lin[y0][:, x0], lin[y0][:, x1], lin[y1][:, x0], lin[y1][:, x1]


def avg4(a, b, c, d):
    """((a + b) + (c + d)) * 0.25 in fp32, denormals kept"""
    with np.errstate(over="ignore", invalid="ignore"):
        return ((a + b) + (c + d)) * F32(0.25)


def mip_level(fmt, src_raw):
    """one level of the project's mip rule from the STORED previous level"""
    return encode(fmt, avg4(*mip_taps(decode(fmt, np.asarray(src_raw)))))


def mip_count(w, h):
    return int(np.floor(np.log2(max(w, h)))) + 1


def mip_chain(fmt, level0, levels=None):
    """[level 0, level 1, ...]: floor(log2(max(w, h))) + 1 levels unless `levels` says otherwise"""
    out = [np.ascontiguousarray(level0)]
    h, w = out[0].shape[:2]
    n = mip_count(w, h) if levels is None else levels
    for _ in range(1, n):
        out.append(mip_level(fmt, out[-1]))
    return out


# ---- test inputs ----------------------------------------------------------------------------------------------------------
def random_texels(fmt, w, h, seed):
    """texels that exercise the whole code range of the format; floats finite, some outside [0, 1] and some negative"""
    rng = np.random.default_rng(seed)
    dt, c = RAW_DTYPE[fmt]
    if dt == np.uint8:
        return rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
    if dt == np.uint16:
        return rng.integers(0, 65536, size=(h, w, c)).astype(np.uint16)
    if dt == np.uint32:
        return rng.integers(0, 2 ** 32, size=(h, w, c), dtype=np.uint64).astype(np.uint32)
    vals = rng.uniform(-0.25, 1.5, size=(h, w, c)).astype(F32)
    vals[rng.random((h, w, c)) < 0.05] *= F32(40.0)
    return vals.astype(dt)
