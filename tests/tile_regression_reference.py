"""Numpy restatement of program "tile_regression" (advanced_ssr/regression.comp, csrc/tile_regression.hip) — the checker of
tests/test_tile_regression.py and tests/test_tile_regression_gpu.py.

Test infrastructure, like tests/gtao_rt_reference.py, whose fp32 arithmetic (Arith, fma32, d24_to_float) it is built on.  Two
modes.  "fp32" follows DESIGN_NUMERICS.md (Tile regression) operation for operation: the kernel must equal it bit for bit, and
nothing looser would mean anything, because the 3 x 3 normal matrix of an 8 x 8 tile is badly conditioned in fp32 (condition
numbers of a few thousand at 128 x 72, growing with resolution: the fitted coefficients differ from a float64 fit in the second
digit).  "fp64" evaluates the same formula in float64, with no claim on its rounding: it is what the formula is checked with
against np.linalg.lstsq.

Lane order: a tile's 64 lanes are i = ly * 8 + lx (gl_LocalInvocationIndex); the sums follow the shader's shared-memory tree
s[i] += s[i + off], off = 32 .. 1, which the kernel performs as an xor butterfly over the wave (xor_butterfly below)."""
import math

import numpy as np

from gtao_rt_reference import _LIBM, Arith, d24_to_float, fma32  # noqa: F401  (fma32: re-exported for the tests)

F32 = np.float32
F64 = np.float64
TILE = 8
LANES = TILE * TILE
NAN_RESIDUAL = 1e10


def tiles_of(w, h):
    """the tile grid of a w x h depth view: (ceil(w / 8), ceil(h / 8))"""
    return (w + TILE - 1) // TILE, (h + TILE - 1) // TILE


def tree_sum(v):
    """[n, 64] -> [n]: the reference's shared-memory tree, s[i] += s[i + off] for i < off, off = 32, 16, 8, 4, 2, 1; s[0]"""
    s = np.array(v, copy=True)
    off = LANES // 2
    while off:
        s[:, :off] = s[:, :off] + s[:, off:2 * off]
        off //= 2
    return s[:, 0]


def xor_butterfly(v):
    """[n, 64] -> [n, 64]: what the kernel does instead, every lane adds the value of lane i ^ off, off = 32 .. 1"""
    s = np.array(v, copy=True)
    lane = np.arange(LANES)
    off = LANES // 2
    while off:
        s = s + s[:, lane ^ off]
        off //= 2
    return s


class _Mode:
    """the arithmetic of one mode: the float type, the contract's fused multiply-add and the host's tanf(fovy / 2)"""

    def __init__(self, ar, mode):
        if mode not in ("fp32", "fp64"):
            raise ValueError(mode)
        self.fp32 = mode == "fp32"
        self.T = F32 if self.fp32 else F64
        self.ar = ar

    def cfma(self, a, b, c):
        if self.fp32:
            return self.ar.cfma(a, b, c)
        return np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)

    def tan_half(self, fovy):
        if self.fp32:
            return F32(_LIBM.tanf(float(F32(fovy) / F32(2.0))))
        return F64(math.tan(float(fovy) / 2.0))

    def depth(self, bits):
        bits = np.asarray(bits).astype(np.uint32)
        if self.fp32:
            return d24_to_float(bits)
        return (bits & 0xFFFFFF).astype(F64) / F64(16777215.0)


def tile_points(ar, depth_bits, camera_to_world, fovy, aspect, znear, zfar, mode="fp32"):
    """-> r [tiles_h, tiles_w, 64, 3]: every lane's point of every tile of the depth view (raw D24S8 words [h, w]); lanes whose
    pixel lies outside the view hold 0.  camera_to_world: 4x4 in maths convention."""
    m = _Mode(ar, mode)
    T = m.T
    M = np.asarray(camera_to_world, T)
    h, w = np.asarray(depth_bits).shape
    tw, th = tiles_of(w, h)
    py, px = np.mgrid[0:th * TILE, 0:tw * TILE]
    inside = (px < w) & (py < h)
    cx, cy = np.minimum(px, w - 1), np.minimum(py, h - 1)
    with np.errstate(all="ignore"):
        d = m.depth(np.asarray(depth_bits)[cy, cx])
        uvx = (cx.astype(T) / T(w)).astype(T)
        uvy = (cy.astype(T) / T(h)).astype(T)
        # reconstruct_view_vec
        tg = m.tan_half(fovy)
        n_, f_, asp = T(znear), T(zfar), T(aspect)
        z = ((n_ * f_) / m.cfma(d, f_ - n_, -f_)).astype(T)
        xd = m.cfma(T(2.0), uvx, T(-1.0))
        yd = m.cfma(T(2.0), uvy, T(-1.0))
        v = [-xd * ((z * asp) * tg), -yd * (z * tg), z]
        one, zero = np.ones_like(z), np.zeros_like(z)
        # mul(M, (v, 1)) and mul(M, (0, 0, 0, 1)), xyz
        world = [m.cfma(M[r, 3], one, m.cfma(M[r, 2], v[2], m.cfma(M[r, 1], v[1], M[r, 0] * v[0]))) for r in range(3)]
        origin = [m.cfma(M[r, 3], one, m.cfma(M[r, 2], zero, m.cfma(M[r, 1], zero, M[r, 0] * zero))) for r in range(3)]
        r = np.stack([np.where(inside, (world[c] - origin[c]).astype(T), T(0.0)) for c in range(3)], axis=-1).astype(T)
    return r.reshape(th, TILE, tw, TILE, 3).transpose(0, 2, 1, 3, 4).reshape(th, tw, LANES, 3)


def inverse_adjugate(m):
    """inverse(mat3) as GLM lays it out, m[..., c, r] column-major, nothing fused (vkr_device.hpp inverse_adjugate)"""
    m00, m01, m02 = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    m10, m11, m12 = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    m20, m21, m22 = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    c00 = m11 * m22 - m21 * m12
    c01 = m01 * m22 - m21 * m02
    c02 = m01 * m12 - m11 * m02
    inv_det = m.dtype.type(1.0) / ((m00 * c00 - m10 * c01) + m20 * c02)
    inv = np.empty_like(m)
    inv[..., 0, 0] = c00 * inv_det
    inv[..., 0, 1] = -c01 * inv_det
    inv[..., 0, 2] = c02 * inv_det
    inv[..., 1, 0] = -(m10 * m22 - m20 * m12) * inv_det
    inv[..., 1, 1] = (m00 * m22 - m20 * m02) * inv_det
    inv[..., 1, 2] = -(m00 * m12 - m10 * m02) * inv_det
    inv[..., 2, 0] = (m10 * m21 - m20 * m11) * inv_det
    inv[..., 2, 1] = -(m00 * m21 - m20 * m01) * inv_det
    inv[..., 2, 2] = (m00 * m11 - m10 * m01) * inv_det
    return inv


def normal_matrix(r):
    """r [n, 64, 3] -> (equ [n, 3, 3] indexed [c, r] as the shader's mat3 constructor fills it, sum r [n, 3]); tree sums"""
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    s1 = [tree_sum(c) for c in (x, y, z)]
    s2 = [tree_sum(c * c) for c in (x, y, z)]
    sxy, sxz, syz = tree_sum(x * y), tree_sum(x * z), tree_sum(y * z)
    equ = np.empty((r.shape[0], 3, 3), r.dtype)
    equ[:, 0, 0], equ[:, 0, 1], equ[:, 0, 2] = s2[0], sxy, sxz
    equ[:, 1, 0], equ[:, 1, 1], equ[:, 1, 2] = sxy, s2[1], syz
    equ[:, 2, 0], equ[:, 2, 1], equ[:, 2, 2] = sxz, syz, s2[2]
    return equ, np.stack(s1, axis=-1)


def fit(ar, r, mode="fp32"):
    """r [n, 64, 3] (dtype of the mode) -> (plane [n, 3], mean squared residual [n]): regression.comp:40-101"""
    m = _Mode(ar, mode)
    T = m.T
    r = np.asarray(r, T)
    with np.errstate(all="ignore"):
        equ, s1 = normal_matrix(r)
        inv = inverse_adjugate(equ)
        # inverse(equ) * s1: row i of the inverse, (inv[0][i] * s.x + inv[1][i] * s.y) + inv[2][i] * s.z, unfused
        plane = np.stack([(inv[:, 0, i] * s1[:, 0] + inv[:, 1, i] * s1[:, 1]) + inv[:, 2, i] * s1[:, 2] for i in range(3)], axis=-1).astype(T)
        p = plane[:, None, :]
        # dot(plane, r) - 1 with the contract's dot, squared; NaN -> 1e10
        e = m.cfma(p[..., 2], r[..., 2], m.cfma(p[..., 1], r[..., 1], p[..., 0] * r[..., 0])) - T(1.0)
        sse = (e * e).astype(T)
        sse = np.where(np.isnan(sse), T(NAN_RESIDUAL), sse).astype(T)
        mean = (tree_sum(sse) / T(LANES)).astype(T)
    return plane, mean


def tile_regression(ar, depth_bits, camera_to_world, fovy, aspect, znear, zfar, out_w, out_h, mode="fp32"):
    """the whole pass: [out_h, out_w, 4] = (plane.xyz, mean squared residual) as vkr_tile_regression writes out_planes"""
    r = tile_points(ar, depth_bits, camera_to_world, fovy, aspect, znear, zfar, mode)
    th, tw = r.shape[:2]
    assert out_w <= tw and out_h <= th, "the entry refuses an output beyond the tile grid"
    r = r[:out_h, :out_w].reshape(out_h * out_w, LANES, 3)
    plane, mean = fit(ar, r, mode)
    return np.concatenate([plane, mean[:, None]], axis=-1).reshape(out_h, out_w, 4)


def mat4_to_np(m):
    """abi.Mat4 (column-major) -> 4x4 float32 in maths convention"""
    return np.array(list(m.m), F32).reshape(4, 4).T.copy()


def plane_depth_bits(w, h, normal, k, fovy, aspect, znear, zfar):
    """D24S8 words [h, w] of the view-space plane normal . p = -k seen through the regression's own pixel -> ray map
    (uv = pixel / size): z = -k / (normal . (a, b, 1)) with (a, b) the ray's slopes, encoded with encode_depth and rounded to
    24 bits.  Evaluated in float64; the plane must lie inside (znear, zfar) on every pixel."""
    py, px = np.mgrid[0:h, 0:w].astype(F64)
    tg = math.tan(float(fovy) / 2.0)
    a = -(2.0 * px / w - 1.0) * float(aspect) * tg
    b = -(2.0 * py / h - 1.0) * tg
    z = -float(k) / (normal[0] * a + normal[1] * b + normal[2])
    n_, f_ = float(znear), float(zfar)
    assert (z < -n_).all() and (z > -f_).all(), "the plane leaves the depth range"
    d = f_ / (f_ - n_) + f_ * n_ / (z * (f_ - n_))
    return np.rint(d * 16777215.0).astype(np.uint32)
