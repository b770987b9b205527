"""Constructed inputs of the shadow-mask filter tests (tests/test_shadow_mask_filter.py, tests/test_shadow_mask_filter_gpu.py):
the all-accepted plane, the residue-class mask and the masks of one value but for one texel.  Test infrastructure: the product
package never imports it."""
import numpy as np

F32 = np.float32
NORMAL_MIN_DOT, PLANE_TOLERANCE = 0.9, 0.01  # the thresholds the issue of the filter fixes for the constructed cases
PLANE_DEPTH = 5.0  # view units in front of the camera


def _oct_codes(v):
    """the RG16_UNORM code of the unit vector v (octahedral, as decode_normal reads it); float64, rounded to the nearest code"""
    v = np.asarray(v, np.float64)
    p = v / np.abs(v).sum()
    x, y = p[0], p[1]
    if p[2] < 0:
        x, y = (1 - abs(p[1])) * (1 if p[0] >= 0 else -1), (1 - abs(p[0])) * (1 if p[1] >= 0 else -1)
    return np.array([round((x * 0.5 + 0.5) * 65535), round((y * 0.5 + 0.5) * 65535)], np.uint16)


def plane_gbuffer(size, setup):
    """one plane facing the camera: a constant depth code (PLANE_DEPTH view units away) and the one normal code nearest to the
    camera's axis in world space -> (depth words [h, w] uint32, normal codes [h, w, 2] uint16)"""
    w, h = size
    _, _, n, f = [float(v) for v in setup.fazz]
    d = (f - n * f / PLANE_DEPTH) / (f - n)
    words = np.full((h, w), int(round(d * 16777215)), np.uint32)
    axis = np.asarray(setup.inv_view, np.float64)[:3, :3] @ np.array([0.0, 0.0, 1.0])
    codes = np.broadcast_to(_oct_codes(axis / np.linalg.norm(axis)), (h, w, 2)).copy()
    return words, codes


def residue_values(reach):
    """one RGBA8 value per class (x mod R, y mod R): [R, R, 4], every channel another spread of codes"""
    rng = np.random.default_rng([0xF117, reach])
    return rng.integers(0, 256, size=(reach, reach, 4), dtype=np.uint8)


def residue_mask(size, reach):
    w, h = size
    y, x = np.mgrid[0:h, 0:w]
    return residue_values(reach)[y % reach, x % reach]


def residue_mean(reach):
    """what the filter makes of residue_mask at a pixel that accepts every tap of its window: the tent gives every class the
    weight R * R of A = R^4, so the value is the mean of the R * R class values, rounded half up"""
    v = residue_values(reach).reshape(-1, 4).astype(np.uint64)
    n = np.uint64(reach * reach)
    return ((np.uint64(2) * v.sum(axis=0) + n) // (np.uint64(2) * n)).astype(np.uint8)


def interior(size, reach):
    """[h, w] bool: the pixels at least R - 1 from every border"""
    w, h = size
    y, x = np.mgrid[0:h, 0:w]
    b = reach - 1
    return (x >= b) & (x < w - b) & (y >= b) & (y < h - b)


# the one value of a flat mask (r, g, b, a) and the alpha of the texel that differs.  0 against 255: the smallest weight of a tap is
# 1 of A = R^4 <= 256, and 255 / 256 + 1 / 2 still rounds to 1: the odd texel shows in every pixel whose taps reach it
BASE, ODD = (200, 150, 100, 0), 255


def single_texel_mask(size, at):
    """BASE everywhere but at texel `at` = (x, y), which differs in its alpha channel only"""
    w, h = size
    m = np.empty((h, w, 4), np.uint8)
    m[:] = BASE
    m[at[1], at[0], 3] = ODD
    return m


def single_texel_cases(size, reach):
    """(name, at, tile, changes): the texel at (x, y) next to the 8 x 8 tile of a wave with origin `tile`, at distance R - 1 (a tap of the
    tile's nearest pixel: the tile's output must change) and at distance R (no tap of the tile reaches it) along x, along y and diagonally.  Only positions inside the image."""
    w, h = size
    out = []
    for tx, ty in ((8, 8), (16, 0), (0, 8), (24, 8), (8, 0)):
        if tx + 8 > w or ty + 8 > h:
            continue
        for dist, changes in ((reach - 1, True), (reach, False)):
            for name, at in (("x+", (tx + 7 + dist, ty + 3)), ("x-", (tx - dist, ty + 4)), ("y+", (tx + 3, ty + 7 + dist)), ("y-", (tx + 4, ty - dist)),
                             ("diag", (tx + 7 + dist, ty + 7 + dist)), ("diag-", (tx - dist, ty - dist))):
                if 0 <= at[0] < w and 0 <= at[1] < h:
                    out.append((f"tile{tx},{ty}-{name}-d{dist}", at, (tx, ty), changes))
    return out
