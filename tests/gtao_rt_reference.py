"""Numpy restatement of the ray-traced AO pass (program gtao_rt_main, gtao/rt_main.frag) and of the frozen fp32 triangle
test of the acceleration structure (csrc/accel.hip, DESIGN_NUMERICS.md) — the checker of tests/test_accel_gpu.py and
tests/test_gtao_rt_gpu.py, and the independent reproduction of GTAO's 64 random directions for tests/test_accel.py.

Test infrastructure, like the oracle: the product package never imports it.  Every fp32 operation is written in the order
the kernels use; a fused multiply-add of numeric contract 2 is emulated exactly (fma32: one rounding of a * b + c).  The
host-side transcendentals (tanf of the projection, cosf / sinf of the 16 rotation angles) are taken from the C library
through ctypes, as the C-ABI's host code takes them.
"""
import ctypes as C

import numpy as np

F32 = np.float32
_LIBM = C.CDLL("libm.so.6")
for _n in ("tanf", "cosf", "sinf"):
    getattr(_LIBM, _n).argtypes = [C.c_float]
    getattr(_LIBM, _n).restype = C.c_float


# ---- fp32 arithmetic ----------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays: a * b is exact in float64; the float64 sum is corrected where rounding it to float32
    would round a second time at a tie."""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    cd = c.astype(np.float64)
    s = p + cd
    bb = s - p
    err = (p - (s - bb)) + (cd - bb)  # exact: p + c == s + err
    r = s.astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        other = np.nextafter(r, np.where(s > r.astype(np.float64), F32(np.inf), F32(-np.inf)).astype(F32))
        mid = (r.astype(np.float64) + other.astype(np.float64)) * 0.5
        tie = (s == mid) & (err != 0) & np.isfinite(s)
        up = np.maximum(r, other)
        dn = np.minimum(r, other)
        r = np.where(tie, np.where(err > 0, up, dn), r)
    return r.astype(F32)


class Arith:
    """the helpers of vkr_device.hpp under numeric contract `contract` (2: cfma fuses, 1: it does not)"""

    def __init__(self, contract=2):
        self.contract = contract

    def cfma(self, a, b, c):
        if self.contract >= 2:
            return fma32(a, b, c)
        return (np.asarray(a, F32) * np.asarray(b, F32)) + np.asarray(c, F32)

    def dot(self, a, b):  # cfma(a.z, b.z, cfma(a.y, b.y, a.x * b.x))
        return self.cfma(a[..., 2], b[..., 2], self.cfma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))

    def normalize(self, v):  # v * (1 / sqrt(v . v)), both correctly rounded
        d = self.dot(v, v)
        return v * (F32(1.0) / np.sqrt(d))[..., None]

    def cross(self, a, b):
        x = self.cfma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1]))
        y = self.cfma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2]))
        z = self.cfma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))
        return np.stack([x, y, z], axis=-1)

    def madd(self, a, s, b):  # a + s * b
        return self.cfma(np.broadcast_to(np.asarray(s, F32)[..., None] if np.ndim(s) else F32(s), b.shape), b, a)

    def mixf(self, a, b, t):  # cfma(b, t, a * (1 - t))
        return self.cfma(b, t, a * (F32(1.0) - t))


# ---- storage decodes (exact: the correctly rounded k / (2^b - 1)) ----------------------------------------------------------------
def d24_to_float(bits):
    x = (bits & 0xFFFFFF).astype(F32) * F32(2.0 ** -24)
    return fma32(x, F32(np.frombuffer(np.array([0x33800001], np.uint32).tobytes(), F32)[0]), x)  # 0x1.000002p-24


def unorm16_to_float(v):
    x = v.astype(F32) * F32(2.0 ** -16)
    return fma32(x, F32(2.0 ** -16 + 2.0 ** -32), x)


def sample(ar, img, uv_x, uv_y, lerp_channels):
    """texture(): bilinear, clamp-to-edge on a whole-frame image img[h, w, c] (float32 after decoding); uv arrays"""
    h, w = img.shape[:2]
    x = ar.cfma(uv_x, F32(w), F32(-0.5))
    y = ar.cfma(uv_y, F32(h), F32(-0.5))
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = x - x0f, y - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    cx0, cx1 = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    cy0, cy1 = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    t00, t10, t01, t11 = img[cy0, cx0], img[cy0, cx1], img[cy1, cx0], img[cy1, cx1]
    fxc, fyc = fx[..., None], fy[..., None]
    top = ar.mixf(t00, t10, np.broadcast_to(fxc, t00.shape))
    bot = ar.mixf(t01, t11, np.broadcast_to(fxc, t01.shape))
    return ar.mixf(top, bot, np.broadcast_to(fyc, top.shape))[..., :lerp_channels]


def decode_normal(ar, e):
    u = ar.cfma(F32(2.0), e[..., 0], F32(-1.0))
    v = ar.cfma(F32(2.0), e[..., 1], F32(-1.0))
    z = (F32(1.0) - np.abs(u)) - np.abs(v)
    sgn = lambda k: np.where(k >= 0, F32(1.0), F32(-1.0)).astype(F32)
    nx = np.where(z < 0, (F32(1.0) - np.abs(v)) * sgn(u), u)
    ny = np.where(z < 0, (F32(1.0) - np.abs(u)) * sgn(v), v)
    return ar.normalize(np.stack([nx, ny, z], axis=-1).astype(F32))


# ---- the frozen triangle test ---------------------------------------------------------------------------------------------
def triangle_records(tris):
    """(n, 3, 3) float32 world triangles -> dict of the record fields vkr_accel_layout computes (v0, e1, e2, lo, hi)"""
    t = np.asarray(tris, dtype=F32).reshape(-1, 3, 3)
    s = np.abs(t.reshape(-1, 9)).max(axis=1) if len(t) else np.zeros(0, F32)
    margin = (s + F32(1.0)) * F32(2.0 ** -12)
    return {"v0": t[:, 0], "e1": t[:, 1] - t[:, 0], "e2": t[:, 2] - t[:, 0],
            "lo": np.minimum(np.minimum(t[:, 0], t[:, 1]), t[:, 2]) - margin[:, None],
            "hi": np.maximum(np.maximum(t[:, 0], t[:, 1]), t[:, 2]) + margin[:, None]}


def frozen_hit_tuv(o, d, tmin, tmax, v0, e1, e2, lo, hi):
    """element-wise: ray (o, d) of [.., 3] against triangle records of [.., 3] (broadcast); the operation order of
    csrc/accel_traverse.hpp ray_triangle_closest, no fused multiply-add: -> (ok, t, u, v)"""
    tmin, tmax = F32(tmin), F32(tmax)
    with np.errstate(all="ignore"):
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        e1x, e1y, e1z = e1[..., 0], e1[..., 1], e1[..., 2]
        e2x, e2y, e2z = e2[..., 0], e2[..., 1], e2[..., 2]
        px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
        det = (e1x * px + e1y * py) + e1z * pz
        inv = F32(1.0) / det
        tx, ty, tz = o[..., 0] - v0[..., 0], o[..., 1] - v0[..., 1], o[..., 2] - v0[..., 2]
        u = ((tx * px + ty * py) + tz * pz) * inv
        qx, qy, qz = ty * e1z - tz * e1y, tz * e1x - tx * e1z, tx * e1y - ty * e1x
        v = ((dx * qx + dy * qy) + dz * qz) * inv
        t = ((e2x * qx + e2y * qy) + e2z * qz) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tmin) & (t <= tmax)
        hx, hy, hz = o[..., 0] + t * dx, o[..., 1] + t * dy, o[..., 2] + t * dz
        ok &= (hx >= lo[..., 0]) & (hx <= hi[..., 0]) & (hy >= lo[..., 1]) & (hy <= hi[..., 1]) & (hz >= lo[..., 2]) & (hz <= hi[..., 2])
    return ok, t.astype(F32), u.astype(F32), v.astype(F32)


def frozen_hit(o, d, tmin, tmax, v0, e1, e2, lo, hi):
    """the any-hit form (ray_hits_triangle): whether, not where"""
    return frozen_hit_tuv(o, d, tmin, tmax, v0, e1, e2, lo, hi)[0]


def segment_boxes(o, d, tmin, tmax):
    """the box every point o + t * d (mul, then add) of t in [tmin, tmax] lies in"""
    a = o + F32(tmin) * d
    b = o + F32(tmax) * d
    return np.minimum(a, b), np.maximum(a, b)


def brute_force_any_hit(o, d, tmin, tmax, rec, chunk=512):
    """any-hit of every ray against every triangle.  A triangle whose widened box misses the ray's segment box is skipped:
    by the test's own definition it cannot be hit (its hit point lies in both boxes), so this is the exact answer."""
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    out = np.zeros(len(o), dtype=bool)
    lo, hi = rec["lo"], rec["hi"]
    for s in range(0, len(o), chunk):
        so, sd = o[s:s + chunk], d[s:s + chunk]
        slo, shi = segment_boxes(so, sd, tmin, tmax)
        cand = np.ones((len(so), len(lo)), dtype=bool)
        for k in range(3):
            cand &= (slo[:, None, k] <= hi[None, :, k]) & (shi[:, None, k] >= lo[None, :, k])
        ri, ti = np.nonzero(cand)
        if len(ri) == 0:
            continue
        hit = frozen_hit(so[ri], sd[ri], tmin, tmax, rec["v0"][ti], rec["e1"][ti], rec["e2"][ti], lo[ti], hi[ti])
        out[s + np.unique(ri[hit])] = True
    return out


# ---- GTAO's random directions (gtao.cpp:415-443), reproduced from the definitions of the standard library ---------------
def minstd_rand0(seed=1):
    x = seed
    while True:
        x = (16807 * x) % 2147483647
        yield x


def uniform01_float(engine):
    """uniform_real_distribution<float>(0, 1) under libstdc++: generate_canonical<float, 24> with one engine call
    (log2 of the engine's range is 30 >= 24): float(x - min) / float(range), range = 2147483646 -> 2^31 as a float"""
    x = next(engine)
    r = F32(x - 1) / F32(2147483646.0)
    return r if r < F32(1.0) else np.nextafter(F32(1.0), F32(0.0))


def random_directions(count=64):
    eng = minstd_rand0()
    out = []
    while len(out) < count:
        x = F32(float(uniform01_float(eng)) * 2.0 - 1.0)
        y = F32(float(uniform01_float(eng)) * 2.0 - 1.0)
        z = uniform01_float(eng)
        length = np.sqrt((x * x + y * y) + z * z)
        if float(length) <= 0.00001 or length > F32(1.0):
            continue
        out.append([x / length, y / length, z / length, F32(0.0)])
    return np.array(out, dtype=F32)


# ---- the pass ------------------------------------------------------------------------------------------------------------
def rotation_table(rotation):
    """(cos, sin) of 2 PI (rotation + k / 16), k = 0..15, as the C-ABI evaluates them on the host"""
    pi = F32(3.1415926535897932384626433832795)
    out = np.zeros((16, 2), F32)
    for k in range(16):
        angle = (F32(2.0) * pi) * (F32(rotation) + F32(1.0 / 16.0) * F32(k))
        out[k] = (_LIBM.cosf(float(angle)), _LIBM.sinf(float(angle)))
    return out


def pixel_setup(ar, depth_bits, normal_codes, camera_to_world, fovy, aspect, znear, zfar, rotation, out_w, out_h):
    """steps 1-4 for every pixel of an out_w x out_h `raw`: returns (sky mask, world position, normal, tangent, bitangent),
    each [out_h, out_w, ...].  depth_bits: raw D24 texels of the depth view (image mip 1); normal_codes: raw RG16_UNORM
    texels of the full-resolution normal; camera_to_world: 4x4 maths-convention float32."""
    gy, gx = np.mgrid[0:out_h, 0:out_w]
    uvx = ((gx.astype(F32) + F32(0.5)) / F32(out_w)).astype(F32)
    uvy = ((gy.astype(F32) + F32(0.5)) / F32(out_h)).astype(F32)
    depth = d24_to_float(depth_bits.reshape(depth_bits.shape[0], depth_bits.shape[1], 1))
    d = sample(ar, depth, uvx, uvy, 1)[..., 0]
    sky = d >= F32(1.0)
    tg = F32(_LIBM.tanf(float(F32(fovy) / F32(2.0))))
    n_, f_ = F32(znear), F32(zfar)
    z = (n_ * f_) / ar.cfma(d, f_ - n_, -f_)
    xd = ar.cfma(F32(2.0), uvx, F32(-1.0))
    yd = ar.cfma(F32(2.0), uvy, F32(-1.0))
    vx = -xd * ((z * F32(aspect)) * tg)
    vy = -yd * (z * tg)
    M = np.asarray(camera_to_world, F32)
    world = np.stack([ar.cfma(M[r, 3], F32(1.0), ar.cfma(M[r, 2], z, ar.cfma(M[r, 1], vy, M[r, 0] * vx))) for r in range(3)], axis=-1)
    enc = unorm16_to_float(normal_codes)
    normal = decode_normal(ar, sample(ar, enc, uvx, uvy, 2))
    world = ar.madd(world, F32(1e-6), normal)
    max_xy = np.maximum(np.abs(normal[..., 0]), np.abs(normal[..., 1]))
    small = (max_xy < F32(0.00001))[..., None]
    t0 = np.where(small, np.array([1, 0, 0], F32), np.stack([normal[..., 1], -normal[..., 0], np.zeros_like(normal[..., 0])], axis=-1))
    tangent = ar.normalize(t0.astype(F32))
    bitangent = ar.normalize(ar.cross(normal, tangent))
    tangent = ar.normalize(ar.cross(bitangent, normal))
    cs = rotation_table(rotation)
    slot = (((gx + gy) & 3) << 2) + (gx & 3)
    c, s = cs[slot, 0], cs[slot, 1]
    tangent = ar.normalize(ar.madd(tangent * c[..., None], s, bitangent))
    bitangent = ar.normalize(ar.cross(normal, tangent))
    tangent = ar.normalize(ar.cross(bitangent, normal))
    return sky, world.astype(F32), normal, tangent, bitangent


def ray_dirs(ar, directions, normal, tangent, bitangent):
    """step 5: [P, 64, 3] unit directions and the [P, 64] cosines for P pixels"""
    r = ar.normalize(np.asarray(directions, F32)[:, :3])  # [64, 3]
    n, t, b = normal[:, None, :], tangent[:, None, :], bitangent[:, None, :]
    shape = (normal.shape[0], 64, 3)
    w = ar.cfma(np.broadcast_to(r[None, :, 0:1], shape), np.broadcast_to(t, shape), np.broadcast_to(n, shape) * r[None, :, 2:3])
    w = ar.cfma(np.broadcast_to(r[None, :, 1:2], shape), np.broadcast_to(b, shape), w)
    dirs = ar.normalize(w)
    cosv = np.maximum(ar.dot(dirs, np.broadcast_to(n, shape)), F32(0.0))
    return dirs, cosv


def butterfly_sum(v):
    """the wave's sum over 64 lanes (xor shuffles 32, 16, ..., 1)"""
    v = np.asarray(v, F32)
    k = 32
    while k >= 1:
        v = v[:, :k] + v[:, k:2 * k]
        k //= 2
    return v[:, 0]


def gtao_rt(ar, depth_bits, normal_codes, params, rotation, directions, tris, out_w, out_h, pixel_chunk=256):
    """the whole pass: float16 [out_h, out_w, 4] as gtao_rt_main writes `raw`.  params: (camera_to_world 4x4, fovy,
    aspect, znear, zfar)."""
    cam, fovy, aspect, znear, zfar = params
    sky, world, normal, tangent, bitangent = pixel_setup(ar, depth_bits, normal_codes, cam, fovy, aspect, znear, zfar, rotation, out_w, out_h)
    rec = triangle_records(tris)
    P = out_w * out_h
    world, normal, tangent, bitangent = (a.reshape(P, 3) for a in (world, normal, tangent, bitangent))
    live = ~sky.reshape(P)
    occ = np.zeros(P, F32)
    idx_live = np.nonzero(live)[0]
    reach = F32(0.21)  # every segment (o, o + 0.2 dir) lies in [o - 0.21, o + 0.21]
    for s in range(0, len(idx_live), pixel_chunk):
        px = idx_live[s:s + pixel_chunk]
        o = world[px]
        dirs, cosv = ray_dirs(ar, directions, normal[px], tangent[px], bitangent[px])
        scaled = dirs * F32(0.2)
        hit = np.zeros((len(px), 64), dtype=bool)
        if len(rec["lo"]):
            cand = np.ones((len(px), len(rec["lo"])), dtype=bool)
            for k in range(3):
                cand &= (o[:, None, k] - reach <= rec["hi"][None, :, k]) & (o[:, None, k] + reach >= rec["lo"][None, :, k])
            pi, ti = np.nonzero(cand)
            if len(pi):
                oo = np.repeat(o[pi][:, None, :], 64, axis=1)
                h = frozen_hit(oo, scaled[pi], 1e-12, 1.0, *(np.repeat(rec[f][ti][:, None, :], 64, axis=1) for f in ("v0", "e1", "e2", "lo", "hi")))
                np.logical_or.at(hit, pi, h)
        contrib = np.where(hit, F32(0.0), cosv).astype(F32)
        occ[px] = F32(2.0) * (butterfly_sum(contrib) / F32(64.0))
    out = np.zeros((P, 4), np.float16)
    out[:, 0] = occ.astype(np.float16)
    out[:, 1] = np.float16(1.0)
    out[~live, 0] = np.float16(0.0)
    return out.reshape(out_h, out_w, 4)
