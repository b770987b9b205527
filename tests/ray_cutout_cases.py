"""Constructed cases for alpha cutouts in the ray query, shared by tests/test_ray_cutout.py (known answers of the numpy brute
force, no GPU) and tests/test_ray_cutout_gpu.py (the two ray-level entries against it).

The geometry is a stack of large triangles parallel to the xy plane: triangle k is ((-1, -1, z), (3, -1, z), (-1, 3, z)), so the ray
from (x, y, 0) along +z hits it at t = z, u = (x + 1) / 4, v = (y + 1) / 4, all exact for the dyadic numbers used here, and with the
default attribute uvs ((0, 0), (2, 0), (0, 2)) uv_hit is (2 u, 2 v): rays_at() takes the wanted uv_hit in [0, 1]^2 and aims at half
of it, which keeps u + v <= 1.  A case names, per ray, the index the closest hit must report (MISS: none); `expect` None leaves
the answer to the brute force (the GPU test compares with it either way).
"""
import numpy as np

from vk_renderer_amd import abi
from vk_renderer_amd import scene as scn

F32 = np.float32
MISS = 0xFFFFFFFF


def _rgba(alpha):
    a = np.asarray(alpha, np.uint8)
    out = np.empty(a.shape + (4,), np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = 200, 100, 50
    out[..., 3] = a
    return out


def textures():
    """the texture table of every case: 0: 1 x 1 alpha 0; 1: 1 x 1 alpha 255; 2: a 2 x 2 checker (alpha 0 at (0, 0) and (1, 1));
    3: 8 x 8 with a mip chain, alpha 0 in texels [0, 4) x [0, 4): a hole at levels 0, 1 and 2 that the 1 x 1 level averages away;
    4: 3 x 5 (the non-power-of-two wrap), alpha 0 in column 1 and in rows 3 and 4; 5: 2 x 2, column 0 alpha 0 beside column 1 of alpha
    code 1"""
    big = np.full((8, 8), 255, np.uint8)
    big[0:4, 0:4] = 0
    y, x = np.mgrid[0:5, 0:3]
    odd = np.where((x == 1) | (y >= 3), 0, 255)
    chain = scn.build_mips(_rgba(big))
    assert [lv.shape[0] for lv in chain] == [8, 4, 2, 1] and chain[2][0, 0, 3] == 0 and chain[3][0, 0, 3] > 0
    return [[_rgba([[0]])], [_rgba([[255]])], [_rgba([[0, 255], [255, 0]])], chain, [_rgba(odd)], [_rgba([[0, 1], [0, 1]])]]


HOLE, SOLID, CHECKER, MIPPED, ODD, EDGE = range(6)
TEXTURE_COUNT = 6


def stack(zs):
    return np.array([[[-1, -1, z], [3, -1, z], [-1, 3, z]] for z in zs], F32)


def attributes(albedo, uv0=(0.0, 0.0), scale=2.0):
    """one record per triangle: uvs (uv0, uv0 + (scale, 0), uv0 + (0, scale)) and the albedo index"""
    a = np.zeros(len(albedo), abi.hit_attrib_dtype())
    a["uv"][:, 0] = uv0
    a["uv"][:, 1] = (uv0[0] + scale, uv0[1])
    a["uv"][:, 2] = (uv0[0], uv0[1] + scale)
    a["albedo_index"] = np.asarray(albedo, np.int64).astype(np.uint32)
    return a


def rays_at(uvs):
    """rays from (x, y, 0) along +z that hit every triangle of a stack at (u, v) = uvs / 2"""
    uv = np.asarray(uvs, F32).reshape(-1, 2) * F32(0.5)
    o = np.zeros((len(uv), 3), F32)
    o[:, 0], o[:, 1] = uv[:, 0] * F32(4) - F32(1), uv[:, 1] * F32(4) - F32(1)
    d = np.tile(np.array([0, 0, 1], F32), (len(uv), 1))
    return o, d


CENTRE = [(0.25, 0.25)]


def _case(zs, albedo, expect, uvs=CENTRE, tmin=0.0, tmax=100.0, lod=0, mask=0, count=TEXTURE_COUNT, **attr):
    o, d = rays_at(uvs)
    return dict(tris=stack(zs), attribs=attributes(albedo, **attr), o=o, d=d, tmin=tmin, tmax=tmax, lod=lod, mask=mask, texture_count=count,
                expect=None if expect is None else np.asarray(expect, np.int64).astype(np.uint32))


def cases():
    c = {}
    # (a) nearest candidate transparent, a farther one opaque: the farther index
    c["a_nearest_transparent"] = _case([1, 2], [HOLE, SOLID], [1])
    c["a_three_deep"] = _case([1, 2, 3, 4], [HOLE, HOLE, SOLID, SOLID], [2])
    # (b) two coincident triangles, equal t
    c["b_lower_transparent"] = _case([1, 1], [HOLE, SOLID], [1])
    c["b_both_opaque"] = _case([1, 1], [SOLID, SOLID], [0])
    c["b_both_transparent"] = _case([1, 1], [HOLE, HOLE], [MISS])
    c["b_higher_transparent"] = _case([1, 1], [SOLID, HOLE], [0])
    # (c) any hit: the first triangle of a leaf transparent, a later one opaque (two triangles are one leaf in input order); and
    # transparent below the root's first child, opaque below its second (the layouts are asserted in tests/test_ray_cutout.py)
    c["c_same_leaf"] = _case([1, 1.25], [HOLE, SOLID], [1])
    c["c_second_subtree"] = _case([1, 1.5, 10, 10.5], [HOLE, HOLE, SOLID, SOLID], [2])
    # (d) everything transparent: (0, 0, 0, MISS)
    c["d_all_transparent"] = _case([1, 2, 3], [HOLE, HOLE, CHECKER], [MISS])
    # (e) uv_hit on texel centres, on the boundary between alpha 0 and alpha code 1 (tiny alpha: opaque), deep inside a hole
    c["e_checker_centres"] = _case([1], [CHECKER], [MISS, 0, 0, MISS], uvs=[(0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)])
    c["e_edge"] = _case([1], [EDGE], [MISS, 0, 0, MISS], uvs=[(0.25, 0.25), (0.5, 0.25), (0.375, 0.75), (0.25, 0.75)])
    c["e_deep_inside"] = _case([1, 2], [MIPPED, SOLID], [1, 1, 0], uvs=[(0.25, 0.25), (0.1875, 0.3125), (0.75, 0.75)])
    # (f) attribute uv outside [0, 1) and negative, |uv| <= 64: REPEAT
    c["f_negative"] = _case([1, 2], [CHECKER, SOLID], [1, 0, 0, 1], uvs=[(0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)], uv0=(-7.0, -3.0))
    c["f_far"] = _case([1, 2], [CHECKER, SOLID], [1, 0], uvs=[(0.25, 0.25), (0.75, 0.25)], uv0=(-64.0, 63.0))
    c["f_odd_scaled"] = _case([1, 2], [ODD, SOLID], None, uvs=[(x / 16.0, y / 16.0) for x in range(1, 12, 2) for y in range(1, 12, 3)], uv0=(-9.5, 4.25), scale=5.0)
    c["f_mipped_scaled"] = _case([1, 2], [MIPPED, SOLID], None, uvs=[(x / 32.0, y / 32.0) for x in range(1, 24, 3) for y in range(1, 24, 5)], uv0=(-1.25, 0.5),
                                 scale=-3.0)
    # (g) alpha_lod 0, a level where the hole has vanished, a level beyond the chain (clamped to the last: vanished too)
    for lod, want in ((0, 1), (1, 1), (2, 1), (3, 0), (9, 0), (0xFFFFFFFF, 0)):
        c[f"g_lod_{lod}"] = _case([1, 2], [MIPPED, SOLID], [want], lod=lod)
    # (h) no texture at all, and an index beyond the table: opaque
    c["h_untextured"] = _case([1, 2], [MISS, SOLID], [0])
    c["h_beyond_table"] = _case([1, 2], [TEXTURE_COUNT, SOLID], [0])
    c["h_beyond_short_table"] = _case([1, 2], [CHECKER, HOLE], [0], count=1)  # only texture 0 is bound: index 2 is beyond it
    c["h_no_textures"] = _case([1, 2], [HOLE, SOLID], [0], count=0)
    # (i) the mask bit: on a texture without holes the same answers as clear, on a holed one the opaque answers
    c["i_mask_on_solid"] = _case([1, 2], [HOLE, SOLID], [1], mask=1 << SOLID)
    c["i_mask_on_hole"] = _case([1, 2], [HOLE, SOLID], [0], mask=1 << HOLE)
    c["i_mask_all"] = _case([1, 2], [CHECKER, SOLID], [0, 0], uvs=[(0.25, 0.25), (0.75, 0.25)], mask=0xFFFFFFFF)
    c["i_mask_other_bits"] = _case([1, 2], [CHECKER, SOLID], [1, 0], uvs=[(0.25, 0.25), (0.75, 0.25)], mask=0xFFFFFFFF & ~(1 << CHECKER))
    # (j) tmin == tmax at the t of a transparent candidate, and at the t of an opaque one
    c["j_at_transparent"] = _case([1, 2], [HOLE, SOLID], [MISS], tmin=1.0, tmax=1.0)
    c["j_at_opaque"] = _case([1, 2], [HOLE, SOLID], [1], tmin=2.0, tmax=2.0)
    return c


def forty():
    """the scene of the random-ray properties: 40 triangles in [-2, 2]^3 with uvs up to +-64 and every kind of albedo index ->
    (tris, attribs)"""
    rng = np.random.default_rng(0xC0705)
    centre = rng.uniform(-2, 2, size=(40, 1, 3))
    tris = (centre + rng.uniform(-1.2, 1.2, size=(40, 3, 3))).astype(F32)
    a = np.zeros(40, abi.hit_attrib_dtype())
    a["uv"] = rng.uniform(-64, 64, size=(40, 3, 2)).astype(F32)
    a["uv"][::3] = rng.uniform(-2, 2, size=(len(a["uv"][::3]), 3, 2)).astype(F32)  # some with few repeats: large holes
    kinds = np.array([HOLE, SOLID, CHECKER, MIPPED, ODD, EDGE, MISS, TEXTURE_COUNT + 1], np.int64)
    a["albedo_index"] = kinds[rng.integers(0, len(kinds), 40)].astype(np.uint32)
    return tris, a


def random_rays(n, seed=7):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-4, 4, size=(n, 3)).astype(F32)
    target = rng.uniform(-2, 2, size=(n, 3)).astype(F32)
    return o, ((target - o) * F32(2.0)).astype(F32)
