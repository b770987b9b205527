"""Numpy restatement of the backbuffer texdraw pass (csrc/texdraw.hip: vkr_texdraw; texdraw/shader.{vert,frag}) — the checker of
tests/test_texdraw.py and tests/test_texdraw_gpu.py.

Test infrastructure, like the oracle: the product package never imports it.  Every fp32 operation is written in the order
DESIGN_NUMERICS.md ("Texdraw") gives, on Arith of gtao_rt_reference.py (the fused steps of numeric contract 2: the sampler's
texel coordinate and the accumulation of the bilinear mix); texels are decoded and stored with the helpers of
transfer_reference.py.  Run as a script it prints, per test size, how many pixel centres have a non-zero bilinear fraction."""
import numpy as np

from gtao_rt_reference import Arith
from transfer_reference import FMT_RGBA8_SRGB, FMT_RGBA8_UNORM, decode, encode

F32 = np.float32
SHOW_ALL, SHOW_R, SHOW_G, SHOW_B, SHOW_A = 0, 1, 2, 4, 8


def pixel_centre_uv(n):
    """uv of the centres of the n pixels of an axis: the IEEE quotient (g + 0.5) / n"""
    return (np.arange(n).astype(F32) + F32(0.5)) / F32(n)


def footprint(ar, dst_n, src_n):
    """one axis of texture(): -> (first tap, second tap, fraction) per destination pixel; taps clamped to the edge"""
    x = ar.cfma(pixel_centre_uv(dst_n), F32(src_n), F32(-0.5))
    x0f = np.floor(x)
    f = (x - x0f).astype(F32)
    x0 = x0f.astype(np.int64)
    return np.clip(x0, 0, src_n - 1), np.clip(x0 + 1, 0, src_n - 1), f


def shown_channel(flags):
    """the shader's four ifs in order: the last set bit of R, G, B, A wins; None = all channels; bits above 8 are ignored"""
    shown = None
    for bit, ch in ((SHOW_R, 0), (SHOW_G, 1), (SHOW_B, 2), (SHOW_A, 3)):
        if flags & bit:
            shown = ch
    return shown


def texdraw(src_raw, src_fmt, dst_w, dst_h, dst_fmt=FMT_RGBA8_SRGB, flags=SHOW_ALL, contract=2):
    """vkr_texdraw: `src_raw` [h, w, c] of src_fmt drawn onto a dst_w x dst_h backbuffer of dst_fmt -> uint8 [dst_h, dst_w, 4]"""
    assert dst_fmt in (FMT_RGBA8_SRGB, FMT_RGBA8_UNORM)
    src_raw = np.asarray(src_raw)
    sh, sw = src_raw.shape[:2]
    ar = Arith(contract)
    img = decode(src_fmt, src_raw)
    xa, xb, fx = footprint(ar, dst_w, sw)
    ya, yb, fy = footprint(ar, dst_h, sh)
    t00, t10, t01, t11 = img[ya][:, xa], img[ya][:, xb], img[yb][:, xa], img[yb][:, xb]
    wx = np.broadcast_to(fx[None, :, None], t00.shape)
    wy = np.broadcast_to(fy[:, None, None], t00.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        top = ar.mixf(t00, t10, wx)  # rows first
        bot = ar.mixf(t01, t11, wx)
        c = ar.mixf(top, bot, wy)    # then columns; all four channels
    ch = shown_channel(int(flags))
    if ch is not None:
        c = np.repeat(c[..., ch:ch + 1], 4, axis=-1)
    return encode(dst_fmt, c)


def nonzero_fractions(dst_w, dst_h, src_w, src_h, contract=2):
    """-> (pixels whose footprint has a non-zero fraction on either axis, columns with fx != 0, rows with fy != 0)"""
    ar = Arith(contract)
    fx, fy = footprint(ar, dst_w, src_w)[2], footprint(ar, dst_h, src_h)[2]
    nx, ny = int((fx != 0).sum()), int((fy != 0).sum())
    return dst_w * dst_h - (dst_w - nx) * (dst_h - ny), nx, ny


# (source extent, backbuffer extent) of the cases of tests/test_texdraw_gpu.py
TEST_SIZES = [((64, 36), (64, 36)), ((250, 142), (250, 142)), ((256, 144), (128, 72)), ((128, 72), (256, 144)), ((257, 129), (100, 77)),
              ((1, 1), (5, 3)), ((1, 9), (4, 9)), ((3, 3), (1, 1))]


def fraction_report(contract=2):
    lines = []
    for (sw, sh), (dw, dh) in TEST_SIZES + [((1920, 1080), (1920, 1080)), ((3840, 2160), (3840, 2160))]:
        n, nx, ny = nonzero_fractions(dw, dh, sw, sh, contract)
        lines.append(f"{sw}x{sh} -> {dw}x{dh}: {n} of {dw * dh} pixel centres with a non-zero fraction ({nx} of {dw} columns, {ny} of {dh} rows)")
    return lines


if __name__ == "__main__":
    print("\n".join(fraction_report()))
