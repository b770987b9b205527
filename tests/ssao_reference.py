"""Numpy restatement of program "ssao" (ssao/shader.frag:21-41, csrc/ssao.hip) — the checker of tests/test_ssao.py and
tests/test_ssao_gpu.py.

Test infrastructure, like tests/gtao_rt_reference.py, whose fp32 arithmetic (Arith, fma32, d24_to_float) it is built on: every
operation is written in the order the kernel uses, a fused multiply-add of numeric contract 2 is one rounding, divisions and
sums are numpy's IEEE float32.  The sampler is restated here and not taken from gtao_rt_reference.sample, because this pass
feeds it coordinates that are infinite, NaN or beyond 2^63 (a sample on or next to the eye plane): the texel index follows the
kernel's float -> int rule (truncate, NaN -> 0, saturate at +-2^30) instead of numpy's undefined cast.  A sample whose
coordinate is NaN or infinite has a NaN weight, its depth is NaN and the compare is false: it does not count.

The result is a count of 16 threshold tests per pixel, many of which lie within a few 1e-7 of the threshold (sky and distant
ground): kernel and restatement agree because both are one IEEE sequence, not because the counts are robust."""
import numpy as np

from gtao_rt_reference import _LIBM, Arith, d24_to_float, fma32  # noqa: F401  (fma32: re-exported for the tests)

F32 = np.float32
SAMPLES = 16


def f2i(x):
    """vkr_device.hpp f2i: v_cvt_i32_f32 (truncate, NaN -> 0, saturating) narrowed to +-2^30"""
    lim = 1073741824.0
    with np.errstate(invalid="ignore"):
        c = np.clip(np.nan_to_num(np.asarray(x, F32).astype(np.float64), nan=0.0, posinf=lim, neginf=-lim), -lim, lim)
    return np.trunc(c).astype(np.int64)


def sample_depth(ar, depth, uv_x, uv_y):
    """sample<FmtD24>(tex, uv): bilinear, clamp-to-edge, on a whole image depth[h, w] of decoded float32"""
    h, w = depth.shape
    with np.errstate(all="ignore"):
        x = ar.cfma(uv_x, F32(w), F32(-0.5))
        y = ar.cfma(uv_y, F32(h), F32(-0.5))
        x0f, y0f = np.floor(x), np.floor(y)
        fx, fy = (x - x0f).astype(F32), (y - y0f).astype(F32)
        x0, y0 = f2i(x0f), f2i(y0f)
        cx0, cx1 = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
        cy0, cy1 = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
        top = ar.mixf(depth[cy0, cx0], depth[cy0, cx1], fx)
        bot = ar.mixf(depth[cy1, cx0], depth[cy1, cx1], fx)
        return ar.mixf(top, bot, fy)


def encode_unorm8(x):
    """float_to_unorm8: rint(clamp(x, 0, 1) * 255), ties to even"""
    return np.rint(np.clip(np.asarray(x, F32), F32(0.0), F32(1.0)) * F32(255.0)).astype(np.uint8)


CODES = encode_unorm8(np.arange(SAMPLES + 1, dtype=F32) / F32(SAMPLES))  # the 17 values a texel can hold; 8 / 16 -> 128


def quirk_packed(samples16x3):
    """the 16 x 4 sample slots the shader reads when the host packs vec3 at a 12-byte stride into 272 bytes (ssao.cpp:15-22):
    slot i = floats [4i .. 4i + 3] of the flat 48-float array, zero past its end"""
    flat = np.zeros(64, F32)
    flat[:48] = np.asarray(samples16x3, F32).reshape(-1)
    return flat.reshape(16, 4)


def ssao(ar, depth_bits, proj, fovy, aspect, znear, zfar, samples16x4, out_w, out_h, stats=None):
    """-> (R8 codes [out_h, out_w] uint8, counts [out_h, out_w]).  depth_bits: raw D24S8 words [h, w] of the view's base mip;
    proj: 4x4 in maths convention; samples16x4: the block's slots ([16, 3] works too), .w unused.  stats: a dict that receives
    `offscreen_taps` (sample_uv outside [0, 1]^2, NaN included), `nonfinite_sample_uv` (taps with an infinite or NaN sample_uv
    component: a sample on or next to the eye plane) and `taps`."""
    M = np.asarray(proj, F32)
    S = np.asarray(samples16x4, F32)
    depth = d24_to_float(np.asarray(depth_bits).astype(np.uint32))
    gy, gx = np.mgrid[0:out_h, 0:out_w]
    with np.errstate(all="ignore"):
        uvx = ((gx.astype(F32) + F32(0.5)) / F32(out_w)).astype(F32)
        uvy = ((gy.astype(F32) + F32(0.5)) / F32(out_h)).astype(F32)
        frag_depth = sample_depth(ar, depth, uvx, uvy)
        # reconstruct_view_vec
        tg = F32(_LIBM.tanf(float(F32(fovy) / F32(2.0))))
        n_, f_ = F32(znear), F32(zfar)
        z = ((n_ * f_) / ar.cfma(frag_depth, f_ - n_, -f_)).astype(F32)
        xd = ar.cfma(F32(2.0), uvx, F32(-1.0))
        yd = ar.cfma(F32(2.0), uvy, F32(-1.0))
        cam = [-xd * ((z * F32(aspect)) * tg), -yd * (z * tg), z]
        counts = np.zeros((out_h, out_w), np.int64)
        offscreen = nonfinite = 0
        one = np.ones_like(z)
        for i in range(SAMPLES):
            pos = [ar.cfma(F32(0.05), np.broadcast_to(S[i, c], z.shape), cam[c]) for c in range(3)]  # madd(camera_pos, 0.05, sample)
            ndc = [ar.cfma(M[r, 3], one, ar.cfma(M[r, 2], pos[2], ar.cfma(M[r, 1], pos[1], M[r, 0] * pos[0]))) for r in range(4)]
            nx, ny, nz = (ndc[0] / ndc[3]).astype(F32), (ndc[1] / ndc[3]).astype(F32), (ndc[2] / ndc[3]).astype(F32)
            su, sv = ar.cfma(F32(0.5), nx, F32(0.5)), ar.cfma(F32(0.5), ny, F32(0.5))
            sample = sample_depth(ar, depth, su, sv)
            counts += nz < (sample + F32(0.0000001)).astype(F32)
            offscreen += int((~((su >= 0) & (su <= 1) & (sv >= 0) & (sv <= 1))).sum())
            nonfinite += int((~(np.isfinite(su) & np.isfinite(sv))).sum())
        codes = encode_unorm8(counts.astype(F32) / F32(SAMPLES))
    if stats is not None:
        stats["offscreen_taps"] = offscreen
        stats["nonfinite_sample_uv"] = nonfinite
        stats["taps"] = SAMPLES * out_w * out_h
    return codes, counts


def fixed_samples(min_abs_z=0.0):
    """the fixed sample set of the tests: rng(11) normals, normalised in float64, cast to float32 (w = 0 is the caller's);
    min_abs_z: |v.z| forced up to that value, sign kept (the constant-depth known answer needs every sample clear of the plane)"""
    v = np.random.default_rng(11).normal(size=(16, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if min_abs_z:
        v[:, 2] = np.where(np.abs(v[:, 2]) < min_abs_z, np.copysign(min_abs_z, v[:, 2]), v[:, 2])
    return v.astype(F32)
