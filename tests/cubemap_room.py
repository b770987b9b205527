"""The box-room known answer of the cube-face bake, shared by tests/test_cubemap_probe.py (restatement against analytic geometry,
no GPU) and tests/test_cubemap_probe_gpu.py (the kernel against the same assertions).

The room is the box [-14, 14] x [0, 7] x [-6, 14], 12 triangles, every wall with its own constant-colour opaque texture.  From a
point inside, the distance along a direction d to the wall first hit is min over the axes of (bound - pos) / d; the direction of a
face texel comes from probe_reference._face_dir, the cube convention vkr_cube2oct samples with, so an agreement pins the
orientation of all six baked faces against what the next program of the chain expects.
"""
import numpy as np

import probe_reference as ref
from vk_renderer_amd import scene as scn

ROOM_LO = np.array([-14.0, 0.0, -6.0])
ROOM_HI = np.array([14.0, 7.0, 14.0])
GRID_MIN, GRID_MAX, GRID = (-6.0, 1.0, 0.0), (6.0, 1.0, 12.0), 4
# wall w = 2 * axis + (1 for the low side): +X, -X, +Y, -Y, +Z, -Z.  Codes chosen so that decode -> encode gives the code back
WALL_CODES = np.array([[200, 60, 50, 255], [60, 200, 80, 255], [230, 220, 200, 255], [90, 90, 100, 255], [70, 90, 220, 255],
                       [220, 180, 40, 255]], np.uint8)
COLOR_BAND = 0.05       # colour is asserted where nearest and second-nearest wall distances differ by more than this
COLOR_BAND_SHARE = 0.05  # and the excluded texels may be at most this share


def grid_positions():
    step = (np.array(GRID_MAX) - np.array(GRID_MIN)) / (GRID - 1)
    return [np.array(GRID_MIN) + step * np.array([x, 0, y]) for y in range(GRID) for x in range(GRID)]


def room_scene():
    sc = scn.Scene()
    lo, hi = ROOM_LO, ROOM_HI
    tr = sc.add_transform(np.eye(4, dtype=np.float32))
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    for wall in range(6):
        axis, low = wall // 2, wall % 2
        a, b = [k for k in range(3) if k != axis]
        corners = np.zeros((4, 3), np.float32)
        corners[:, axis] = lo[axis] if low else hi[axis]
        corners[:, a] = [lo[a], hi[a], hi[a], lo[a]]
        corners[:, b] = [lo[b], lo[b], hi[b], hi[b]]
        normal = np.zeros((4, 3), np.float32)
        normal[:, axis] = 1.0 if low else -1.0
        mesh = sc.add_mesh(corners, normal, uv, np.array([0, 1, 2, 0, 2, 3], np.uint32))
        tex = sc.add_texture(np.tile(WALL_CODES[wall], (4, 4, 1)))
        sc.add_draw(tr, mesh, tex)
    return sc


def analytic(pos, n):
    """per face texel: (fp16 distance to the wall hit first, that wall, texels outside the colour band)"""
    j, i = np.mgrid[0:n, 0:n]
    s, t = (2 * i + 1 - n) / n, (2 * j + 1 - n) / n
    dist = np.zeros((6, n, n), np.float64)
    wall = np.zeros((6, n, n), np.int64)
    clear = np.zeros((6, n, n), bool)
    for f in range(6):
        x, y, z = ref._face_dir(np.full(s.shape, f), s, t, 1.0)
        d = np.stack([x, y, z], -1).astype(np.float64)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        with np.errstate(divide="ignore"):
            tt = np.where(d > 0, (ROOM_HI - pos) / d, np.where(d < 0, (ROOM_LO - pos) / d, np.inf))
        axis = np.argmin(tt, axis=-1)
        srt = np.sort(tt, axis=-1)
        dist[f] = srt[..., 0]
        wall[f] = 2 * axis + (np.take_along_axis(d, axis[..., None], -1)[..., 0] < 0)
        clear[f] = srt[..., 1] > srt[..., 0] * (1.0 + COLOR_BAND)
    return dist, wall, clear


def fp16_ulps(a, b):
    """distance in fp16 codes between two arrays of positive finite fp16 values"""
    return np.abs(a.astype(np.float16).view(np.uint16).astype(np.int64) - b.astype(np.float16).view(np.uint16).astype(np.int64))


def assert_room(color, distance, pos, n):
    """the known-answer assertions on one baked cube (colour codes [6, n, n, 4], fp16 distance [6, n, n]); returns the share of
    texels excluded from the colour check"""
    dist, wall, clear = analytic(np.asarray(pos, np.float64), n)
    assert (distance != np.float16(100.0)).all(), f"pos {pos}: {int((distance == np.float16(100.0)).sum())} texels not covered"
    ulps = fp16_ulps(distance, dist.astype(np.float16))
    assert ulps.max() <= 1, f"pos {pos}: distance {int(ulps.max())} fp16 ulps from the analytic one ({int((ulps > 1).sum())} texels)"
    want = WALL_CODES[wall]
    bad = (color != want).any(-1) & clear
    assert not bad.any(), f"pos {pos}: {int(bad.sum())} texels with the wrong wall colour outside the {COLOR_BAND:.0%} band"
    return 1.0 - clear.mean()
