"""Shared helper of the shadow-map tests: the three light set-ups, the oracle's expectation and the unprojection of a map.

default.vert is mvp * model * vec4(pos, 1) — opaque_taa.vert:39 with zero jitter — and default.frag is empty.  So the expected
shadow map is the depth attachment of the ORACLE's G-buffer rasteriser run with view_projection = the light's matrix, zero
jitter, a square target and every draw's texture indices set to "none" (no alpha discard can fire: a cutout casts a solid
shadow).  Nothing under oracle/ is changed for it."""
import copy

import numpy as np

from vk_renderer_amd import camera
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PostFxChain

# eye -> center; every light is perspective(90 deg, 1, 0.05, 80) * lookAt(eye, center, (0, -1, 0))
LIGHTS = {
    "A": ((-1.85867, 5.81832, -0.247114), (0.0, 2.0, 1.0)),  # main.cpp:295
    "B": ((0.3, 0.4, 4.0), (0.0, 1.0, 8.0)),                 # inside the scene, between the spheres: the near plane cuts geometry
    "C": ((-3.0, 2.5, 9.0), (1.0, 0.5, 3.0)),                # from the far side, looking back
}
D24_MAX = 0x00FFFFFF


def mvp(name):
    eye, center = LIGHTS[name]
    return camera.shadow_mvp(eye=eye, center=center)


def eye(name):
    return np.asarray(LIGHTS[name][0], dtype=np.float32)


def strip(scene):
    """a copy of `scene` whose draws carry no texture indices"""
    out = copy.copy(scene)
    out.draws = [dict(d, albedo=scn.INVALID, mr=scn.INVALID) for d in scene.draws]
    for key in ("_scene_host", "_scene_dev"):  # PostFxChain.raster caches its upload on the scene object
        if hasattr(out, key):
            delattr(out, key)
    return out


def oracle_depth(scene, m, n):
    """depth attachment (uint32 [n, n], low 24 bits) of the oracle's G-buffer rasteriser on `scene` as it is, seen through m"""
    setup = FrameSetup(n, n)
    setup.mvp = setup.prev_mvp = np.asarray(m, dtype=np.float32).astype(np.float64)
    chain = PostFxChain(n, n, backend="oracle", setup=setup)
    chain.raster(scene)
    return chain.depth.raw(0)[..., 0].astype(np.uint32) & D24_MAX


def expected(scene, m, n):
    """the shadow map the pass must produce: uint32 [n, n], 24 bits"""
    return oracle_depth(strip(scene), m, n)


def add_backdrop(scene, m, z=0.999, reach=1.5):
    """Adds to `scene` an untextured quad (two triangles, identity model) that fills the target seen through m behind everything
    else: the corners (+-reach, +-reach, z) of NDC unprojected.  The bounding box of each triangle is the whole target, so both
    go to a rasteriser's large list whatever the extent.  Returns the scene."""
    ndc = np.array([[-reach, -reach, z, 1.0], [reach, -reach, z, 1.0], [reach, reach, z, 1.0], [-reach, reach, z, 1.0]])
    w = ndc @ np.linalg.inv(np.asarray(m, dtype=np.float64)).T
    pos = (w[:, :3] / w[:, 3:4]).astype(np.float32)
    mesh = scene.add_mesh(pos, np.array([[0, 0, 1]] * 4, np.float32), np.zeros((4, 2), np.float32), np.array([0, 1, 2, 0, 2, 3], np.uint32))
    scene.add_draw(scene.add_transform(np.eye(4, dtype=np.float32)), mesh)
    return scene


def unproject(texels, depth, m):
    """world positions (float64 [k, 3]) of the centres of texels [k, 2] (x, y) of an n x n map with D24 words depth[n, n]"""
    n = depth.shape[0]
    t = np.asarray(texels, dtype=np.int64)
    ndc = np.empty((len(t), 4), dtype=np.float64)
    ndc[:, 0] = (t[:, 0] + 0.5) / n * 2.0 - 1.0
    ndc[:, 1] = (t[:, 1] + 0.5) / n * 2.0 - 1.0
    ndc[:, 2] = depth[t[:, 1], t[:, 0]].astype(np.float64) / float(D24_MAX)
    ndc[:, 3] = 1.0
    w = ndc @ np.linalg.inv(np.asarray(m, dtype=np.float64)).T
    return w[:, :3] / w[:, 3:4]


def sample_grid(depth, step):
    """the covered texels of the grid [step // 2 :: step]^2 as [k, 2] (x, y)"""
    n = depth.shape[0]
    ys, xs = np.meshgrid(np.arange(step // 2, n, step), np.arange(step // 2, n, step), indexing="ij")
    pts = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1)
    return pts[depth[pts[:, 1], pts[:, 0]] != D24_MAX]


def rays(name, texels, depth, m):
    """(origins, directions) float32 [k, 3]: from the light's eye to the unprojected centre of every texel (t = 1 there)"""
    p = unproject(texels, depth, m)
    o = np.broadcast_to(eye(name), p.shape).astype(np.float32)
    return o, (p - o.astype(np.float64)).astype(np.float32)


def near_plane_counts(scene, m):
    """(triangles crossing the near plane z_clip = 0, triangles wholly behind it) of `scene` seen through m"""
    from vk_renderer_amd import abi

    tris = abi.scene_triangles(scene).astype(np.float64)  # [t, 3, 3] world
    h = np.concatenate([tris, np.ones(tris.shape[:2] + (1,))], axis=2) @ np.asarray(m, dtype=np.float64).T
    behind = (h[..., 2] < 0.0).sum(axis=1)
    return int(((behind > 0) & (behind < 3)).sum()), int((behind == 3).sum())
