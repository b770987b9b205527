"""CPU tests of the shadow-map pass (no GPU): the refusals of the C-ABI entry, the program table, the frame's gates, the light
matrix, and the expectation itself — the oracle's depth under the light's matrix (tests/shadow_light.py) pinned against rays
through the scene's triangles, so that the GPU tests compare the kernel with something that is known to be a shadow map.

Measured with the oracle on procedural_scene(cutout=True), lights A, B, C: coverage 0.9444 / 1.0000 / 0.5941 at both sizes;
texels where the textured raster differs from the stripped one 1728 / 100403 / 4863 at 1024^2 and 0 / 4813 / 0 at 360^2;
triangles crossing the near plane 4 / 136 / 4, wholly behind it 0 / 3952 / 0; rays 8553 to 16384 per case, none disagreeing
(none at 3e-4 either)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from vk_renderer_amd import abi, camera, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.images import ArrayImageBuf, ImageBuf

import gtao_rt_reference as rt
import shadow_light as sl

ERR_NULL, ERR_FORMAT, ERR_EXTENT, ERR_MIPS, ERR_LAYOUT = 1001, 1002, 1003, 1004, 1005
HOST_DIR = os.path.join(abi.ROOT, "vk-renderer_amd", "host")
RAY_EPS = 1e-3  # of the distance eye -> surface; the cap on disagreeing rays is 0


@pytest.fixture(scope="module")
def lib():
    return abi.product()


@pytest.fixture(scope="module")
def cutout_scene():
    return scn.procedural_scene(cutout=True)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_exported_and_typed(lib):
    assert hasattr(lib, "vkr_default_shadow") and hasattr(lib, "vkr_default_shadow_scratch_bytes")
    assert lib.vkr_default_shadow_scratch_bytes.restype is C.c_uint64 and lib.vkr_default_shadow.restype is C.c_int
    assert len(lib.vkr_default_shadow.argtypes) == 7
    txt = open(os.path.join(abi.ROOT, "include", "vkr_postfx.h")).read()
    assert "vkr_default_shadow(" in txt and "vkr_default_shadow_scratch_bytes(" in txt
    one, four = abi.default_shadow_scratch_bytes(1024, 1, 1000), abi.default_shadow_scratch_bytes(1024, 4, 1000)
    assert four > one > 2 * 1000 * 48, "two 48-byte records per triangle and layer"
    assert abi.default_shadow_scratch_bytes(1024, 1, 2000) > one
    # no visibility buffer: the scratch does not grow with the map (8 B per texel would be 8 MiB here)
    assert abi.default_shadow_scratch_bytes(2048, 1, 1000) - one < 1024 * 1024


def _tris(sc):
    return sum(d["index_count"] // 3 for d in sc.draws)


def test_refusals_without_a_device(lib):
    """every refusal returns its code with a message that names the argument, before anything touches a device"""
    sc = scn.procedural_scene(detail=6)
    s, keep = sc.upload(None)
    n = 64
    layers = ArrayImageBuf(abi.FMT_D24_UNORM_S8, n, n, 4)
    need = abi.default_shadow_scratch_bytes(n, 4, _tris(sc))
    fake = np.zeros(64, np.uint8)  # never dereferenced: a refusal comes first
    mats = (abi.Mat4 * 8)(*[abi.Mat4.from_np(sl.mvp("A"))] * 8)

    def call(scene=s, mvps=mats, descs=None, count=1, scratch=fake.ctypes.data, nbytes=need):
        descs = layers.descs() if descs is None else descs
        return lib.vkr_default_shadow(C.byref(scene) if scene is not None else None, mvps, descs, count, scratch, nbytes, None)

    def err():
        return (lib.vkr_last_error() or b"").decode()

    # NULL arguments
    assert call(scene=None) == ERR_NULL and "scene" in err()
    assert call(mvps=None) == ERR_NULL and "mvps" in err()
    assert lib.vkr_default_shadow(C.byref(s), mats, None, 1, fake.ctypes.data, need, None) == ERR_NULL and "layers" in err()
    assert call(scratch=None) == ERR_NULL and "scratch" in err()
    # layer_count
    assert call(count=0) == ERR_EXTENT and "layer_count" in err()
    assert call(count=9) == ERR_EXTENT and "layer_count" in err()
    # a layer without memory, a wrong format
    hole = layers.descs()
    hole[1].base = None
    assert call(descs=hole, count=2) == ERR_NULL and "layers" in err()
    color = ArrayImageBuf(abi.FMT_RGBA8_UNORM, n, n, 1)
    assert call(descs=color.descs()) == ERR_FORMAT and "layers" in err()
    # non-square, unequal
    wide = ArrayImageBuf(abi.FMT_D24_UNORM_S8, n + 8, n, 1)
    assert call(descs=wide.descs()) == ERR_EXTENT and "square" in err()
    mixed = layers.descs()
    small = ArrayImageBuf(abi.FMT_D24_UNORM_S8, n // 2, n // 2, 1)
    mixed[1] = small.desc(0)
    assert call(descs=mixed, count=2) == ERR_EXTENT and "one extent" in err()
    # a window of a larger frame
    win = ImageBuf(abi.FMT_D24_UNORM_S8, n, n, full=(n, 2 * n), origin=(0, n))
    assert call(descs=(abi.VkrImg * 1)(win.desc())) == ERR_EXTENT and "windows are not supported (single-GPU pass)" in err()
    # scratch
    assert call(count=4, nbytes=need - 1) == ERR_EXTENT and "scratch too small" in err()
    # draws that point outside the scene
    for field, value, word in (("transform_index", len(sc.transforms), "transform_index"), ("index_count", len(sc.indices) + 3, "indices"),
                               ("index_offset", 0xFFFFFFF0, "indices")):
        bad, keep_bad = sc.upload(None)
        draws = C.cast(bad.draws, C.POINTER(abi.RasterDraw))
        setattr(draws[1], field, value)
        assert call(scene=bad, nbytes=1 << 40) == ERR_EXTENT and word in err() and "draw 1" in err(), err()
    # textures are not read: NULL with a count of 0 passes validation (the next refusal is the scratch)
    bare, keep_bare = sc.upload(None)
    bare.textures, bare.texture_count = None, 0
    draws = C.cast(bare.draws, C.POINTER(abi.RasterDraw))
    for i in range(bare.draw_count):
        draws[i].albedo_index, draws[i].mr_index = 12345, 67890  # ignored, even out of range
    assert call(scene=bare, nbytes=16) == ERR_EXTENT and "scratch too small" in err()
    with pytest.raises(RuntimeError, match="2 matrices for 1 layers"):
        abi.default_shadow(s, [sl.mvp("A"), sl.mvp("B")], [layers.desc(0)], 1, 1)


# ---- host mirror ---------------------------------------------------------------------------------------------------------------
def test_program_table_knows_default_shadow():
    assert host.lib().vkrh_has_program(b"default_shadow") == 1


def _malloc_allocator(l):
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    alloc = host._ALLOC(lambda n, u: libc.malloc(n))
    free = host._FREE(lambda p, u: libc.free(p))
    l.vkrh_set_allocator(alloc, free, None)
    return alloc, free


def test_frame_gates_and_default_light():
    """A fresh frame has one light, bit-equal to camera.shadow_mvp(); vkrh_set_shadow_lights replaces it and refuses bad
    arguments; VKRH_STAGE_SHADOW is refused, before anything is recorded, without a scene and on a tiled frame; the image
    "shadows" does not exist before the stage.  No GPU: the frame's images come from malloc."""
    l = host.lib()
    assert hasattr(l, "vkrh_set_shadow_lights") and hasattr(l, "vkrh_shadow_lights")
    frame_h = open(os.path.join(HOST_DIR, "frame.hpp")).read()
    assert "VKRH_STAGE_SHADOW             = 1u << 23" in frame_h and host.STAGE_SHADOW == 1 << 23
    keep = _malloc_allocator(l)
    try:
        cam = host.HostCamera()
        for i in (0, 5, 10, 15):
            cam.view[i] = cam.prev_view[i] = cam.projection[i] = 1.0

        def err():
            return (l.vkrh_last_error() or b"").decode()

        def lights(h):
            out, n = (C.c_float * 64)(), C.c_uint32(0)
            assert l.vkrh_shadow_lights(h, out, C.byref(n)) == 0, err()
            return [np.array(out[16 * i: 16 * i + 16], dtype=np.float32).reshape(4, 4).T for i in range(n.value)]

        cfg = host.HostConfig(64, 64, 0, 0, 64, 64, 0, None)
        h = l.vkrh_create(C.byref(cfg))
        assert h, err()
        try:
            got = lights(h)
            want = camera.shadow_mvp()
            assert len(got) == 1 and np.array_equal(got[0].view(np.uint32), want.view(np.uint32)), (got, want)
            assert l.vkrh_set_camera(h, C.byref(cam)) == 0
            assert l.vkrh_run(h, host.STAGE_SHADOW) != 0 and "without a loaded scene" in err()
            assert l.vkrh_run(h, host.STAGE_RASTER | host.STAGE_SHADOW) != 0 and "VKRH_STAGE_SHADOW without a loaded scene" in err()
            assert b"ShadowPass" not in (l.vkrh_last_tasks(h) or b"")
            d = abi.VkrImg()
            assert l.vkrh_image_layer(h, b"shadows", 0, C.byref(d)) != 0 and "only exists after" in err()
            two = (C.c_float * 32)(*(list(host._mat16(sl.mvp("B"))) + list(host._mat16(sl.mvp("C")))))
            assert l.vkrh_set_shadow_lights(h, two, 2, 360) == 0, err()
            got = lights(h)
            assert len(got) == 2 and np.array_equal(got[0], sl.mvp("B")) and np.array_equal(got[1], sl.mvp("C"))
            assert l.vkrh_set_shadow_lights(h, two, 0, 0) != 0 and "count" in err()
            assert l.vkrh_set_shadow_lights(h, two, 5, 0) != 0 and "count" in err()
            assert l.vkrh_set_shadow_lights(h, None, 1, 0) != 0 and "NULL" in err()
            assert l.vkrh_set_shadow_lights(h, two, 1, 1 << 20) != 0 and "size" in err()
            assert len(lights(h)) == 2, "a refused call changes nothing"
            assert l.vkrh_shadow_lights(h, None, None) != 0
        finally:
            l.vkrh_destroy(h)
        tiled = host.HostConfig(64, 128, 0, 0, 64, 64, 1, None)
        h = l.vkrh_create(C.byref(tiled))
        assert h, err()
        try:
            assert l.vkrh_set_camera(h, C.byref(cam)) == 0
            assert l.vkrh_run(h, host.STAGE_SHADOW) != 0 and "tiled frame" in err()
        finally:
            l.vkrh_destroy(h)
    finally:
        l.vkrh_set_allocator(host._ALLOC(0), host._FREE(0), None)
    del keep


def test_shadow_mvp_is_the_light_of_the_shading_pass():
    """main.cpp:295: the eye is LIGHT_POS of the shading pass; the matrix maps it to w = 0 and the point it looks at to the
    centre of the map"""
    assert tuple(np.float32(camera.LIGHT_POS)) == (np.float32(-1.85867), np.float32(5.81832), np.float32(-0.247114))
    assert "-1.85867f, 5.81832f, -0.247114f" in open(os.path.join(abi.ROOT, "vk-renderer_amd", "csrc", "shading.hip")).read()
    m = camera.shadow_mvp().astype(np.float64)
    assert camera.shadow_mvp().dtype == np.float32
    e = m @ np.array(list(camera.LIGHT_POS) + [1.0])
    assert abs(e[3]) < 1e-5 and abs(e[0]) < 1e-5 and abs(e[1]) < 1e-5
    c = m @ np.array([0.0, 2.0, 1.0, 1.0])
    assert abs(c[0] / c[3]) < 1e-6 and abs(c[1] / c[3]) < 1e-6 and 0.0 < c[2] / c[3] < 1.0
    v = camera.look_at(camera.LIGHT_POS, (0.0, 2.0, 1.0), (0.0, -1.0, 0.0)).astype(np.float64)
    assert np.allclose(v[:3, :3] @ v[:3, :3].T, np.eye(3), atol=1e-6) and np.allclose(v, camera.look_at_rh(camera.LIGHT_POS, (0, 2, 1), (0, -1, 0)), atol=1e-6)


MIRROR_TU = r"""
#include "scene_renderer.hpp"

void bind(rendergraph::RenderGraph &graph, SceneRenderer &scene_renderer, rendergraph::ImageResourceId shadows_tex) {
  const glm::mat4 shadow_mvp = glm::perspective(glm::radians(90.f), 1.f, 0.05f, 80.f) * glm::lookAt(glm::vec3{-1.85867f, 5.81832f, -0.247114f}, glm::vec3{0.f, 2.f, 1.f}, glm::vec3{0.f, -1.f, 0.f});
  scene_renderer.render_shadow(graph, shadow_mvp, shadows_tex, 0);  // main.cpp:346
  gpu::VertexInput vinput = scene::get_vertex_input_shadow();
  (void)vinput;
}
"""


def test_mirror_header_compiles(tmp_path):
    src = tmp_path / "bind_render_shadow.cpp"
    src.write_text(MIRROR_TU)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST_DIR, str(src)]

    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


# ---- the expectation itself, oracle only -----------------------------------------------------------------------------------------
def test_inputs_are_not_vacuous(cutout_scene):
    """B exercises the near-plane clip and the rejection hard; at 1024^2, A and B show that ignoring alpha matters"""
    crossing = {k: sl.near_plane_counts(cutout_scene, sl.mvp(k)) for k in "ABC"}
    print(f"[shadow inputs] (crossing, wholly behind) the near plane: {crossing}")
    for k in "ABC":
        assert crossing[k][0] > 0, f"light {k}: no triangle crosses the near plane"
    assert crossing["B"][1] > 0, "light B: no triangle lies wholly behind the near plane"
    for k in "AB":
        m = sl.mvp(k)
        differ = int((sl.expected(cutout_scene, m, 1024) != sl.oracle_depth(cutout_scene, m, 1024)).sum())
        print(f"[shadow inputs] light {k} 1024: the textured raster differs from the stripped one on {differ} texels")
        assert differ > 0


@pytest.mark.parametrize("n,step", [(1024, 8), (360, 3)])
@pytest.mark.parametrize("light", ["A", "B", "C"])
def test_expectation_is_a_shadow_map(cutout_scene, light, n, step):
    """A ray from the light's eye to the unprojected centre of a covered texel of the EXPECTED map reports no hit on
    t in [0, 1 - 1e-3] and a hit on [0, 1 + 1e-3] (brute force over the scene's world triangles), for every texel of the grid
    [step // 2 :: step]^2.  Cap on disagreeing texels: 0."""
    rec = rt.triangle_records(abi.scene_triangles(cutout_scene))
    m = sl.mvp(light)
    want = sl.expected(cutout_scene, m, n)
    pts = sl.sample_grid(want, step)
    o, d = sl.rays(light, pts, want, m)
    early = int(rt.brute_force_any_hit(o, d, 0.0, 1.0 - RAY_EPS, rec).sum())
    missed = int((~rt.brute_force_any_hit(o, d, 0.0, 1.0 + RAY_EPS, rec)).sum())
    print(f"[shadow expectation] {n} light {light}: coverage {float((want != sl.D24_MAX).mean()):.4f}, {len(pts)} rays, {early} hit before the "
          f"surface, {missed} miss it")
    assert len(pts) > 1000
    assert early == 0 and missed == 0
