"""Constructed inputs of the shadow-mask accumulation tests (tests/test_shadow_mask_accumulate.py,
tests/test_shadow_mask_accumulate_gpu.py).  The pass only reads images: no scene and no ray is needed.  Test infrastructure: the
product package never imports it.

A case is a dict of the arrays and parameters of tests/shadow_mask_accumulate_reference.py's shadow_mask_accumulate:
  mixed       two planes facing the camera with a step edge between them and sky texels in either frame, one camera for both
              frames; per pixel a velocity, a count and a history out of palettes that hold every boundary the rule has
  bound       one plane; the previous frame's depth lies off the pixel's tangent plane by factors of the tolerance on both sides
  two_cameras a floor plane seen by two cameras (the previous one translated and pitched), velocities from the real reprojection
"""
import functools

import numpy as np

from vk_renderer_amd.camera import FrameSetup

from shadow_mask_filter_cases import _oct_codes

F32 = np.float32
F16 = np.float16
SKY = 0xFFFFFF
PLANE_TOLERANCE = 0.01
EXTENTS = [(1, 1), (1, 7), (5, 1), (67, 35), (130, 70)]  # (w, h); 67 x 35 is ragged against any block, 130 x 70 more than one block a side
PARAMS = [(32, 0), (2, 0), (255, 0), (1, 0), (32, 1)]    # (max_count, reset) of the mixed cases
H_PALETTE = (0, 1, 65534, 65535)


def depth_code(view_distance, znear, zfar):
    """the D24 code of a point view_distance in front of the camera (view z = -view_distance)"""
    n, f = float(znear), float(zfar)
    d = (f - n * f / np.asarray(view_distance, np.float64)) / (f - n)
    return np.clip(np.rint(d * 16777215), 0, SKY - 1).astype(np.uint32)


def _f(size_1d, g, vel):
    """f of the rule along one axis, in fp32 as the rule rounds it"""
    s = F32(size_1d)
    uv = ((np.asarray(g).astype(F32) + F32(0.5)) / s).astype(F32)
    with np.errstate(all="ignore"):
        return ((uv + np.asarray(vel, F16).astype(F32)).astype(F32) * s).astype(F32)


def velocity_onto(size_1d, g, target):
    """the fp16 velocity that puts f of pixel g exactly on the integer `target`, if one of the fp16 values around
    (target - g - 0.5) / size does; otherwise the nearest fp16"""
    base = F16((target - (g + 0.5)) / size_1d)
    bits = int(base.view(np.uint16))
    for step in sorted(range(-24, 25), key=abs):
        cand = np.uint16((bits + step) & 0xFFFF).view(F16)
        if np.isfinite(cand) and float(_f(size_1d, g, cand)) == float(target):
            return cand
    return base


def _base(size, setup, seed):
    w, h = size
    rng = np.random.default_rng([0xACC0, seed, w, h])
    axis = np.asarray(setup.inv_view, np.float64)[:3, :3] @ np.array([0.0, 0.0, 1.0])
    codes = np.broadcast_to(_oct_codes(axis / np.linalg.norm(axis)), (h, w, 2)).copy()
    mask = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    flat = mask.reshape(-1)
    flat[: min(flat.size, 256)] = np.arange(min(flat.size, 256), dtype=np.uint8)  # every byte where the extent has room for it
    return rng, codes, mask


def _finish(name, size, setup, prev_inverse_camera, words, prev_words, codes, velocity, mask, history, count, max_count, reset,
            plane_tolerance=PLANE_TOLERANCE):
    return dict(name=name, size=size, depth=words, prev_depth=prev_words, normal=codes, velocity=np.asarray(velocity, F16), mask=mask,
                history=np.asarray(history, np.uint16), count=np.asarray(count, np.uint8), inverse_camera=np.asarray(setup.inv_view),
                prev_inverse_camera=np.asarray(prev_inverse_camera), fazz=tuple(float(v) for v in setup.fazz), max_count=max_count,
                plane_tolerance=plane_tolerance, reset=reset)


def reference_args(c):
    """the arguments of shadow_mask_accumulate after `ar`"""
    return (c["depth"], c["normal"], c["velocity"], c["prev_depth"], c["mask"], c["history"], c["count"], c["inverse_camera"],
            c["prev_inverse_camera"], *c["fazz"], c["max_count"], c["plane_tolerance"], c["reset"])


def mixed(size, max_count, reset, plane_tolerance=PLANE_TOLERANCE):
    w, h = size
    setup = FrameSetup(w, h)
    rng, codes, mask = _base(size, setup, max_count * 2 + reset)
    _, _, zn, zf = setup.fazz
    near, far = depth_code(5.0, zn, zf), depth_code(9.0, zn, zf)
    x = np.arange(w)[None, :].repeat(h, 0)
    y = np.arange(h)[:, None].repeat(w, 1)
    words = np.where(x < (w + 1) // 2, near, far).astype(np.uint32)  # a step edge down the middle
    prev_words = words.copy()
    words[rng.random((h, w)) < 0.08] = SKY       # sky in the current frame only
    prev_words[rng.random((h, w)) < 0.08] = SKY  # sky in the previous frame only
    if w * h == 1:
        words[:] = near; prev_words[:] = near

    # per pixel one velocity of the palette, per axis
    inf, nan, tiny = F16(np.inf), F16(np.nan), np.uint16(1).view(F16)
    pick = rng.integers(0, 18, size=(h, w))
    vel = np.zeros((h, w, 2), F16)
    for (yy, xx), k in np.ndenumerate(pick):
        if k == 0: v = (0.0, 0.0)                                                        # stays
        elif k == 1: v = (F16(3.0 / w), F16(-2.0 / h))                                    # a whole-texel pan
        elif k == 2: v = (velocity_onto(w, xx, xx + 1), velocity_onto(h, yy, yy + 1))     # half a texel: f on the next integer
        elif k == 3: v = (velocity_onto(w, xx, xx), velocity_onto(h, yy, yy))             # half a texel back: f on the pixel's own integer
        elif k == 4: v = (velocity_onto(w, xx, w), 0.0)                                   # f.x on w itself: outside
        elif k == 5: v = (0.0, velocity_onto(h, yy, h))                                   # f.y on h itself: outside
        elif k == 6: v = (velocity_onto(w, xx, 0), velocity_onto(h, yy, 0))               # f on 0: inside
        elif k == 7: v = (F16(-(xx + 1.0) / w), 0.0)                                      # outside, left
        elif k == 8: v = (F16((w - xx + 0.25) / w), 0.0)                                  # outside, right
        elif k == 9: v = (0.0, F16(-(yy + 1.0) / h))                                      # outside, top
        elif k == 10: v = (0.0, F16((h - yy + 0.25) / h))                                 # outside, bottom
        elif k == 11: v = ((inf, -inf, nan, 0.0)[(xx + yy) % 4], (0.0, nan, inf, -inf)[(xx + 2 * yy) % 4])
        elif k == 12: v = (tiny if xx % 2 else -tiny, np.uint16(0x03FF).view(F16))        # fp16 denormals
        elif k == 13: v = (F16(0.3 / w), F16(0.7 / h))                                    # fractions on either side of a half
        elif k == 14: v = (F16(-1.0 / w), F16(1.0 / h))
        elif k == 15: v = (F16(((w - 1) // 2 - xx) / w), 0.0)                             # onto the column left of the step edge
        # Half and a quarter of the frame, exact in fp16: (g + 0.5 + n / 2) / n * n is the integer g + (n + 1) / 2 for an odd n, and a
        # quarter of 70 or 130 is 17.5 or 32.5: f lies exactly on an interior integer, which half a texel ((g + 0.5 +- 0.5) / n
        # through an fp16) reaches at none of these extents but on 0 and on n itself
        elif k == 16: v = (F16(0.5 if 2 * xx < w else -0.5), F16(0.5 if 2 * yy < h else -0.5))
        else: v = (F16(0.25 if 2 * xx < w else -0.25), F16(0.25 if 2 * yy < h else -0.25))
        vel[yy, xx] = v
    counts = np.array(sorted({0, 1, max(max_count - 1, 0), max_count, min(max_count + 1, 255), 255}), np.uint8)
    count = counts[rng.integers(0, len(counts), size=(h, w))]
    history = rng.integers(0, 65536, size=(h, w, 4), dtype=np.uint16)
    special = rng.random((h, w, 4)) < 0.4
    history[special] = np.array(H_PALETTE, np.uint16)[rng.integers(0, 4, size=int(special.sum()))]
    name = f"mixed-{w}x{h}-max{max_count}-reset{reset}" + ("" if plane_tolerance == PLANE_TOLERANCE else f"-tol{plane_tolerance:g}")
    return _finish(name, size, setup, setup.inv_view, words, prev_words, codes, vel, mask, history, count, max_count, reset, plane_tolerance)


# plane distance over the bound; 40: another surface; 1.005 and -0.995: the side changes with the bound taken from the previous depth
BOUND_FACTORS = (0.0, 0.5, -0.5, 0.9, -0.9, 1.1, -1.1, 2.0, -2.0, 40.0, 1.005, -0.995)


def bound(size, max_count=32):
    """zero velocity, one camera: the previous depth of pixel g lies BOUND_FACTORS[k] * tolerance * |z| off the plane"""
    w, h = size
    setup = FrameSetup(w, h)
    rng, codes, mask = _base(size, setup, 77)
    _, _, zn, zf = setup.fazz
    z = 5.0
    k = rng.integers(0, len(BOUND_FACTORS), size=(h, w))
    words = np.full((h, w), depth_code(z, zn, zf), np.uint32)
    prev_words = depth_code(z * (1.0 + np.array(BOUND_FACTORS)[k] * PLANE_TOLERANCE), zn, zf)
    count = rng.integers(1, 40, size=(h, w)).astype(np.uint8)
    history = rng.integers(0, 65536, size=(h, w, 4), dtype=np.uint16)
    c = _finish(f"bound-{w}x{h}", size, setup, setup.inv_view, words, prev_words, codes, np.zeros((h, w, 2), F16), mask, history, count, max_count, 0)
    c["factor"] = np.array(BOUND_FACTORS)[k]
    return c


def floor_gbuffer(size, view, inv_view, fazz, floor_y):
    """the plane y = floor_y seen through `view` (4x4 float64): -> (depth words [h, w], world [h, w, 3] float64, hit [h, w] bool)"""
    w, h = size
    fovy, aspect, zn, zf = [float(v) for v in fazz]
    tg = np.tan(fovy / 2)
    gy, gx = np.mgrid[0:h, 0:w]
    xd, yd = 2 * (gx + 0.5) / w - 1, 2 * (gy + 0.5) / h - 1
    dirs = np.stack([-xd * aspect * tg, -yd * tg, np.ones_like(xd)], -1)  # the view vector per unit of view z
    R, t = np.asarray(inv_view, np.float64)[:3, :3], np.asarray(inv_view, np.float64)[:3, 3]
    wd = dirs @ R.T
    with np.errstate(all="ignore"):
        z = (floor_y - t[1]) / wd[..., 1]
    hit = np.isfinite(z) & (z < -2 * zn) & (z > -0.5 * zf)
    z = np.where(hit, z, -1.0)
    words = np.where(hit, depth_code(-z, zn, zf), SKY).astype(np.uint32)
    return words, wd * z[..., None] + t, hit


def two_cameras(size, max_count=8, prev_delta=(0.05, 0.03, 0.02), prev_pitch_delta=0.6, floor_y=None, seed=5, setup=None):
    """a floor plane under a camera that looks down at it, and the same plane from the previous frame's camera, translated and
    pitched; velocity = prev_uv - uv of the floor point, as a G-buffer pass writes it.  setup: the two cameras (a FrameSetup that
    looks at the plane y = floor_y) instead of the default pair."""
    w, h = size
    setups = [setup] if setup is not None else [FrameSetup(w, h, pitch=s * 35.0, prev_delta=prev_delta, prev_pitch_delta=prev_pitch_delta) for s in (1.0, -1.0)]
    best = None
    for setup in setups:  # the floor lies where the camera looks, whichever way this world's y runs
        forward = -np.asarray(setup.inv_view, np.float64)[:3, 2]
        fy = np.asarray(setup.inv_view, np.float64)[1, 3] + (2.0 if forward[1] > 0 else -2.0) if floor_y is None else floor_y
        words, world, hit = floor_gbuffer(size, setup.view, setup.inv_view, setup.fazz, fy)
        if best is None or hit.sum() > best[3].sum():
            best = (setup, words, world, hit, fy)
    setup, words, world, hit, fy = best
    prev_words, _, _ = floor_gbuffer(size, setup.prev_view, setup.prev_inv_view, setup.fazz, fy)
    fovy, aspect, zn, zf = [float(v) for v in setup.fazz]
    tg = np.tan(fovy / 2)
    pv = np.concatenate([world, np.ones((h, w, 1))], -1) @ np.asarray(setup.prev_view, np.float64).T
    with np.errstate(all="ignore"):
        pu = 0.5 - 0.5 * pv[..., 0] / (pv[..., 2] * aspect * tg)
        pw = 0.5 - 0.5 * pv[..., 1] / (pv[..., 2] * tg)
    gy, gx = np.mgrid[0:h, 0:w]
    vel = np.stack([pu - (gx + 0.5) / w, pw - (gy + 0.5) / h], -1)
    vel = np.where(hit[..., None], vel, 0.0).astype(F16)
    rng, _, rmask = _base(size, setup, seed)
    codes = np.broadcast_to(_oct_codes(np.array([0.0, 1.0, 0.0])), (h, w, 2)).copy()
    history = rng.integers(0, 65536, size=(h, w, 4), dtype=np.uint16)
    count = rng.integers(0, 12, size=(h, w)).astype(np.uint8)
    return _finish(f"two_cameras-{w}x{h}", size, setup, setup.prev_inv_view, words, prev_words, codes, vel, rmask, history, count, max_count, 0)


@functools.lru_cache(maxsize=None)
def all_cases():
    out = [mixed(size, mc, reset) for size in EXTENTS for mc, reset in PARAMS]
    out += [mixed((67, 35), 32, 0, plane_tolerance=1e6)]  # every surface passes the plane test: only the sky tests reject
    out += [bound((67, 35)), bound((130, 70)), two_cameras((67, 35)), two_cameras((130, 70))]
    return tuple(out)


def case_ids():
    return [c["name"] for c in all_cases()]
