"""Alpha cutouts in the ray query without a GPU: the C-ABI record and symbols, every refusal of vkr_accel_occluded_cutout,
vkr_accel_closest_cutout, vkr_shadow_mask_rt_cutout and vkr_reflections_rt_cutout with its text (validation never reaches a launch),
abi.scene_opaque_texture_mask, the frame's setting and its refusal on a tiled frame, and known answers of the numpy brute force
(tests/ray_cutout_reference.py) on the constructed cases of tests/ray_cutout_cases.py: the nearest candidate transparent and a
farther one opaque reports the farther index, coincident triangles report the lowest opaque index, everything transparent is the
miss record, a tiny non-zero alpha is opaque, a masked or absent texture is opaque, and the layouts the any-hit cases rely on."""
import ctypes as C
import functools

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn

import closest_hit_reference as closest
import ray_cutout_cases as cs
import ray_cutout_reference as ref
from test_abi_errors import ERR_EXTENT, ERR_FORMAT, ERR_LAYOUT, ERR_NULL, FAKE, img
from test_shadow_mask_rt import _HostMemoryFrame

F32 = np.float32
D24, RG16, RGBA16, RGBA8 = abi.FMT_D24_UNORM_S8, abi.FMT_RG16_UNORM, abi.FMT_RGBA16_UNORM, abi.FMT_RGBA8_UNORM
W, H = 64, 32
ENTRIES = ("vkr_accel_cutout_scratch_bytes", "vkr_accel_occluded_cutout", "vkr_accel_closest_cutout", "vkr_shadow_mask_rt_cutout",
           "vkr_reflections_rt_cutout")


# ---- the record and the symbols -------------------------------------------------------------------------------------------------
def test_record_layout_and_symbols():
    assert C.sizeof(abi.RayCutout) == 8
    assert abi.RayCutout.alpha_lod.offset == 0 and abi.RayCutout.opaque_texture_mask.offset == 4
    c = abi.ray_cutout(3, 0x1FFFFFFFF)
    assert (c.alpha_lod, c.opaque_texture_mask) == (3, 0xFFFFFFFF)
    txt = open(abi.ROOT + "/include/vkr_postfx.h").read()
    lib = abi.product()
    for name in ENTRIES:
        assert name + "(" in txt and hasattr(lib, name), name
    assert "typedef struct vkr_ray_cutout { uint32_t alpha_lod; uint32_t opaque_texture_mask; } vkr_ray_cutout;" in txt
    for n in (0, 1, 7, 32):
        assert abi.accel_cutout_scratch_bytes(n) == abi.reflections_rt_scratch_bytes(n) > 0
    assert hasattr(host.lib(), "vkrh_set_ray_cutouts")
    assert host.lib().vkrh_has_program(b"shadow_mask_rt_cutout") == 1 and host.lib().vkrh_has_program(b"reflections_rt_cutout") == 1


def test_scene_opaque_texture_mask():
    sc = scn.procedural_scene(detail=3, cutout=True)
    assert len(sc.textures) == 4
    assert abi.scene_opaque_texture_mask(sc) == 0b0111, "the three checkers have no alpha-0 texel, the fence's texture has"
    assert abi.scene_opaque_texture_mask(scn.procedural_scene(detail=3)) == 0b111
    assert abi.scene_opaque_texture_mask(scn.Scene()) == 0
    table = scn.Scene()
    table.textures = cs.textures()
    assert abi.scene_opaque_texture_mask(table) == (1 << cs.SOLID), "of the cases' table only the 1 x 1 of alpha 255 cannot make a hole"


# ---- the refusals of the two ray-level entries -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _empty_accel():
    return abi.Accel(np.zeros((0, 3, 3), F32))  # no triangles: nothing is allocated on a device


def _texture_array(fmt=abi.FMT_RGBA8_SRGB, **kw):
    t = (abi.VkrImg * 1)()
    t[0] = img(fmt, 8, 8, **kw)
    return t


CUT = abi.ray_cutout()


def _ray_entry(entry, accel="ok", org=FAKE, dirs=FAKE, n=4, attribs=None, attrib_count=0, textures=None, texture_count=0, cutout=CUT, out=FAKE,
               scratch=FAKE, scratch_bytes=None):
    lib = abi.product()
    a = _empty_accel().handle if accel == "ok" else accel
    nbytes = abi.accel_cutout_scratch_bytes(texture_count) if scratch_bytes is None else scratch_bytes
    rc = getattr(lib, "vkr_" + entry)(a, org, dirs, 0.0, 1.0, n, attribs, attrib_count, textures, texture_count,
                                      None if cutout is None else C.byref(cutout), out, scratch, nbytes, None)
    return rc, (lib.vkr_last_error() or b"").decode()


RAY_REFUSALS = {
    "accel NULL": (dict(accel=None), ERR_NULL, "NULL acceleration structure"),
    "origins NULL": (dict(org=None), ERR_NULL, "NULL rays or output"),
    "dirs NULL": (dict(dirs=None), ERR_NULL, "NULL rays or output"),
    "out NULL": (dict(out=None), ERR_NULL, "NULL rays or output"),
    "too many rays": (dict(n=(1 << 30) + 1), ERR_EXTENT, "at most 2^30"),
    "cutout NULL": (dict(cutout=None), ERR_NULL, "cutout is NULL"),
    "scratch NULL": (dict(scratch=None), ERR_NULL, "scratch is NULL"),
    "textures NULL with a count": (dict(texture_count=2), ERR_NULL, "2 textures but a NULL texture array"),
    "too many textures": (dict(textures=_texture_array(), texture_count=33), ERR_EXTENT, "33 textures, at most 32"),
    "attrib_count": (dict(attribs=FAKE, attrib_count=3), ERR_EXTENT, "3 attribute records for a structure of 0 triangles"),
    "texture format": (dict(textures=_texture_array(RGBA8), texture_count=1), ERR_FORMAT, ".texture: format"),
    "texture without memory": (dict(textures=_texture_array(base=None), texture_count=1), ERR_NULL, ".texture: NULL image"),
    "windowed texture": (dict(textures=_texture_array(full=(8, 16)), texture_count=1), ERR_EXTENT, "texture: a texture is sampled with REPEAT"),
    "scratch too small": (dict(textures=_texture_array(), texture_count=1, scratch_bytes=abi.accel_cutout_scratch_bytes(1) - 1), ERR_EXTENT,
                          "scratch too small"),
}


@pytest.mark.parametrize("entry", ["accel_occluded_cutout", "accel_closest_cutout"])
@pytest.mark.parametrize("name", sorted(RAY_REFUSALS))
def test_ray_entry_refusals(entry, name):
    kwargs, code, message = RAY_REFUSALS[name]
    rc, msg = _ray_entry(entry, **kwargs)
    assert rc == code, (name, rc, msg)
    assert msg.startswith(entry + ": ") or msg.startswith(entry + "."), msg
    assert message in msg, (name, msg)


@pytest.mark.parametrize("entry", ["accel_occluded_cutout", "accel_closest_cutout"])
def test_no_rays_is_not_an_error(entry):
    assert _ray_entry(entry, org=None, dirs=None, out=None, n=0, cutout=None, scratch=None, scratch_bytes=0)[0] == 0


def test_closest_cutout_wants_aligned_records():
    rc, msg = _ray_entry("accel_closest_cutout", out=FAKE + 8)
    assert rc == ERR_LAYOUT and "accel_closest_cutout: out_hits must be 16-byte aligned" in msg


# ---- the refusals of the two passes ----------------------------------------------------------------------------------------------
def _byref(v):
    return None if v is None else C.byref(v)


def _shadow_params(**over):
    p = abi.shadow_rt_params(np.eye(4), over.pop("lights", [(0, 5, 0, 1)]), 1.0, 2.0, 0.05, 80.0, tmin=over.pop("tmin", 0.0))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _shadow(depth="ok", normal="ok", accel="ok", attribs=None, attrib_count=0, textures=None, texture_count=0, params="ok", cutout=CUT, out="ok",
            scratch=FAKE, scratch_bytes=None):
    lib = abi.product()
    d = img(D24, W, H) if depth == "ok" else depth
    n = img(RG16, W, H) if normal == "ok" else normal
    o = img(RGBA8, W, H) if out == "ok" else out
    p = _shadow_params() if params == "ok" else params
    a = _empty_accel().handle if accel == "ok" else accel
    nbytes = abi.accel_cutout_scratch_bytes(texture_count) if scratch_bytes is None else scratch_bytes
    rc = lib.vkr_shadow_mask_rt_cutout(_byref(d), _byref(n), a, attribs, attrib_count, textures, texture_count, _byref(p), _byref(cutout), _byref(o),
                                       scratch, nbytes, None)
    return rc, (lib.vkr_last_error() or b"").decode()


WINDOW = dict(full=(W, 2 * H), origin=(0, 2))
WHOLE = "windows are not supported (the rays reach anywhere: a single-GPU pass)"
TABLE_REFUSALS = {k: RAY_REFUSALS[k] for k in ("cutout NULL", "scratch NULL", "textures NULL with a count", "too many textures", "attrib_count",
                                                "texture format", "texture without memory", "windowed texture", "scratch too small")}
SHADOW_REFUSALS = dict(TABLE_REFUSALS, **{
    "depth NULL": (dict(depth=None), ERR_NULL, "depth is NULL"),
    "normal NULL": (dict(normal=None), ERR_NULL, "normal is NULL"),
    "accel NULL": (dict(accel=None), ERR_NULL, "NULL acceleration structure"),
    "params NULL": (dict(params=None), ERR_NULL, "params is NULL"),
    "out NULL": (dict(out=None), ERR_NULL, "out_mask is NULL"),
    "depth without memory": (dict(depth=img(D24, W, H, base=None)), ERR_NULL, "shadow_mask_rt_cutout.depth: NULL image"),
    "depth format": (dict(depth=img(abi.FMT_R32_SFLOAT, W, H)), ERR_FORMAT, "shadow_mask_rt_cutout.depth: format"),
    "normal format": (dict(normal=img(abi.FMT_RG16_SFLOAT, W, H)), ERR_FORMAT, "shadow_mask_rt_cutout.normal: format"),
    "out format": (dict(out=img(abi.FMT_RGBA8_SRGB, W, H)), ERR_FORMAT, "shadow_mask_rt_cutout.out_mask: format"),
    "out extent": (dict(out=img(RGBA8, W, H + 1)), ERR_EXTENT, "one extent expected"),
    "normal extent": (dict(normal=img(RG16, W // 2, H // 2)), ERR_EXTENT, "one extent expected"),
    "extent above 65535": (dict(depth=img(D24, 65536, 1), normal=img(RG16, 65536, 1), out=img(RGBA8, 65536, 1)), ERR_EXTENT, "at most 65535 texels a side"),
    "windowed depth": (dict(depth=img(D24, W, H, **WINDOW)), ERR_EXTENT, "depth: " + WHOLE),
    "windowed normal": (dict(normal=img(RG16, W, H, **WINDOW)), ERR_EXTENT, "normal: " + WHOLE),
    "windowed out": (dict(out=img(RGBA8, W, H, full=(W, 2 * H), origin=(0, 0))), ERR_EXTENT, "out_mask: " + WHOLE),
    "no lights": (dict(params=_shadow_params(light_count=0)), ERR_EXTENT, "light_count 0, expected 1..4"),
    "five lights": (dict(params=_shadow_params(light_count=5)), ERR_EXTENT, "light_count 5, expected 1..4"),
    "light w": (dict(params=_shadow_params(lights=[(0, 5, 0, 0.5)])), ERR_EXTENT, "light 0 has w = 0.5"),
    "reserved": (dict(params=_shadow_params(reserved=7)), ERR_EXTENT, "reserved is 7, must be 0"),
    "tmin NaN": (dict(params=_shadow_params(tmin=float("nan"))), ERR_EXTENT, "tmin is NaN"),
})


@pytest.mark.parametrize("name", sorted(SHADOW_REFUSALS))
def test_shadow_mask_rt_cutout_refusals(name):
    kwargs, code, message = SHADOW_REFUSALS[name]
    rc, msg = _shadow(**kwargs)
    assert rc == code, (name, rc, msg)
    assert msg.startswith("shadow_mask_rt_cutout"), msg
    assert message in msg, (name, msg)


def _reflect_params(**over):
    p = abi.reflect_rt_params(np.eye(4), 1.0, 2.0, 0.05, 80.0, fill_misses=over.pop("fill", False), tmin=over.pop("tmin", 0.0),
                              max_distance=over.pop("max_distance", None))
    for k, v in over.items():
        if k == "reserved":
            p.reserved[1] = v
        else:
            setattr(p, k, v)
    return p


def _reflect(depth="ok", normal="ok", rays=None, accel="ok", attribs=None, attrib_count=0, textures=None, texture_count=0, params="ok", cutout=CUT,
             out="ok", scratch=FAKE, scratch_bytes=None):
    lib = abi.product()
    d = img(D24, W, H) if depth == "ok" else depth
    n = img(RG16, W, H) if normal == "ok" else normal
    o = img(RGBA8, W, H) if out == "ok" else out
    p = _reflect_params() if params == "ok" else params
    a = _empty_accel().handle if accel == "ok" else accel
    nbytes = abi.reflections_rt_scratch_bytes(texture_count) if scratch_bytes is None else scratch_bytes
    rc = lib.vkr_reflections_rt_cutout(_byref(d), _byref(n), _byref(rays), a, attribs, attrib_count, textures, texture_count, _byref(p), _byref(cutout),
                                       _byref(o), scratch, nbytes, None)
    return rc, (lib.vkr_last_error() or b"").decode()


REFLECT_REFUSALS = dict(TABLE_REFUSALS, **{
    "depth NULL": (dict(depth=None), ERR_NULL, "depth is NULL"),
    "normal NULL": (dict(normal=None), ERR_NULL, "normal is NULL"),
    "accel NULL": (dict(accel=None), ERR_NULL, "NULL acceleration structure"),
    "params NULL": (dict(params=None), ERR_NULL, "params is NULL"),
    "out NULL": (dict(out=None), ERR_NULL, "out_reflections is NULL"),
    "rays NULL with the flag": (dict(params=_reflect_params(fill=True)), ERR_NULL, "rays is NULL with VKR_REFLECT_RT_FILL_MISSES"),
    "depth without memory": (dict(depth=img(D24, W, H, base=None)), ERR_NULL, "reflections_rt_cutout.depth: NULL image"),
    "depth format": (dict(depth=img(abi.FMT_R32_SFLOAT, W, H)), ERR_FORMAT, "reflections_rt_cutout.depth: format"),
    "normal format": (dict(normal=img(abi.FMT_RG16_SFLOAT, W, H)), ERR_FORMAT, "reflections_rt_cutout.normal: format"),
    "out format": (dict(out=img(abi.FMT_RGBA8_SRGB, W, H)), ERR_FORMAT, "reflections_rt_cutout.out_reflections: format"),
    "rays format": (dict(rays=img(abi.FMT_RGBA16_SFLOAT, W, H), params=_reflect_params(fill=True)), ERR_FORMAT, "reflections_rt_cutout.rays: format"),
    "out extent": (dict(out=img(RGBA8, W, H + 1)), ERR_EXTENT, "one extent expected"),
    "normal extent": (dict(normal=img(RG16, W // 2, H // 2)), ERR_EXTENT, "one extent expected"),
    "rays extent": (dict(rays=img(RGBA16, W, H - 1), params=_reflect_params(fill=True)), ERR_EXTENT, "one extent expected"),
    "extent above 65535": (dict(depth=img(D24, 65536, 1), normal=img(RG16, 65536, 1), out=img(RGBA8, 65536, 1)), ERR_EXTENT, "at most 65535 texels a side"),
    "windowed depth": (dict(depth=img(D24, W, H, **WINDOW)), ERR_EXTENT, "depth: " + WHOLE),
    "windowed normal": (dict(normal=img(RG16, W, H, **WINDOW)), ERR_EXTENT, "normal: " + WHOLE),
    "windowed rays": (dict(rays=img(RGBA16, W, H, **WINDOW), params=_reflect_params(fill=True)), ERR_EXTENT, "rays: " + WHOLE),
    "windowed out": (dict(out=img(RGBA8, W, H, full=(W, 2 * H), origin=(0, 0))), ERR_EXTENT, "out_reflections: " + WHOLE),
    "unknown flag": (dict(params=_reflect_params(flags=2)), ERR_EXTENT, "unknown flag bits 0x2"),
    "reserved": (dict(params=_reflect_params(reserved=7)), ERR_EXTENT, "reserved must be 0"),
    "tmin NaN": (dict(params=_reflect_params(tmin=float("nan"))), ERR_EXTENT, "tmin is NaN"),
    "max_distance NaN": (dict(params=_reflect_params(max_distance=float("nan"))), ERR_EXTENT, "max_distance is NaN"),
})


@pytest.mark.parametrize("name", sorted(REFLECT_REFUSALS))
def test_reflections_rt_cutout_refusals(name):
    kwargs, code, message = REFLECT_REFUSALS[name]
    rc, msg = _reflect(**kwargs)
    assert rc == code, (name, rc, msg)
    assert msg.startswith("reflections_rt_cutout"), msg
    assert message in msg, (name, msg)


# ---- the frame's setting -----------------------------------------------------------------------------------------------------------
def test_frame_setting_and_its_refusal_on_a_tiled_frame():
    l = host.lib()
    frame = _HostMemoryFrame(tiled=False)
    try:
        assert l.vkrh_set_ray_cutouts(frame.h, 1, 0) == 0 and l.vkrh_set_ray_cutouts(frame.h, 0, 5) == 0
        assert l.vkrh_set_ray_cutouts(frame.h, 1, 3) == 0
        # the stages still refuse what they refused, before anything is recorded
        rc, msg = frame.run(host.STAGE_SHADOW_MASK_RT)
        assert rc != 0 and "VKRH_STAGE_SHADOW_MASK_RT without a loaded scene" in msg
        rc, msg = frame.run(host.STAGE_REFLECTIONS_RT)
        assert rc != 0 and "VKRH_STAGE_REFLECTIONS_RT without a loaded scene" in msg
    finally:
        frame.close()
    frame = _HostMemoryFrame(tiled=True)
    try:
        assert l.vkrh_set_ray_cutouts(frame.h, 1, 0) != 0 and "vkrh_set_ray_cutouts: on a tiled frame" in l.vkrh_last_error().decode()
        assert l.vkrh_set_ray_cutouts(frame.h, 0, 0) != 0
    finally:
        frame.close()


# ---- known answers of the brute force ----------------------------------------------------------------------------------------------
CASES = cs.cases()
AR = ref.Arith(2)


def _answers(c, contract=2):
    ar = ref.Arith(contract)
    args = (c["o"], c["d"], c["tmin"], c["tmax"], ref.triangle_records(c["tris"]), c["attribs"], cs.textures()[:c["texture_count"]], c["lod"], c["mask"])
    return ref.brute_force_closest_cutout(ar, *args), ref.brute_force_any_hit_cutout(ar, *args)


@pytest.mark.parametrize("contract", [1, 2])
@pytest.mark.parametrize("name", sorted(k for k, c in CASES.items() if c["expect"] is not None))
def test_known_answers(name, contract):
    c = CASES[name]
    hits, any_hit = _answers(c, contract)
    assert (hits["index"] == c["expect"]).all(), (name, hits["index"], c["expect"])
    assert (any_hit == (c["expect"] != cs.MISS)).all()
    for h in hits:
        if h["index"] == cs.MISS:
            assert (h["t"], h["u"], h["v"]) == (0.0, 0.0, 0.0), "a miss is (0, 0, 0, 0xFFFFFFFF)"
        else:
            assert h["t"] == c["tris"][h["index"]][0, 2], "t is the z of the reported triangle"


def test_nearest_transparent_farther_opaque_returns_the_farther_index():
    c = CASES["a_nearest_transparent"]
    hits, _ = _answers(c)
    opaque = closest.brute_force_closest(c["o"], c["d"], c["tmin"], c["tmax"], ref.triangle_records(c["tris"]))
    assert opaque["index"][0] == 0 and opaque["t"][0] == 1.0, "the opaque query stops at the hole"
    assert hits["index"][0] == 1 and hits["t"][0] == 2.0 and (hits["u"][0], hits["v"][0]) == (F32(0.125), F32(0.125))


def test_a_tiny_alpha_is_opaque_and_a_hole_needs_every_tap():
    """between the alpha-0 column and the column of alpha code 1 the sample is a positive number below 1 / 255: opaque"""
    tex = cs.textures()[cs.EDGE][0]
    for u, want in ((0.25, 0.0), (0.5, 0.5 / 255.0), (0.375, 0.25 / 255.0)):
        alpha = ref._sample_level(AR, tex, np.array([u], F32), np.array([0.25], F32))[0, 3]
        assert abs(float(alpha) - want) < 1e-9 and (alpha == 0) == (want == 0.0)


def test_layouts_the_any_hit_cases_rely_on():
    nodes = abi.accel_layout(CASES["c_same_leaf"]["tris"])[0].view(np.uint32).reshape(-1, 8)
    recs = abi.accel_layout(CASES["c_same_leaf"]["tris"])[1].view(np.uint32).reshape(-1, 16)
    assert len(nodes) == 1 and nodes[0, 7] == 2 and recs[:, 3].tolist() == [0, 1], "one leaf: the transparent triangle first, the opaque one after it"
    nodes, recs = abi.accel_layout(CASES["c_second_subtree"]["tris"])
    nodes, order = nodes.view(np.uint32).reshape(-1, 8), recs.view(np.uint32).reshape(-1, 16)[:, 3]
    assert nodes[0, 7] == 0, "the root is interior"
    first, second = nodes[nodes[0, 3]], nodes[nodes[0, 3] + 1]
    assert sorted(order[first[3]:first[3] + first[7]].tolist()) == [0, 1], "the transparent triangles lie below the root's first child"
    assert sorted(order[second[3]:second[3] + second[7]].tolist()) == [2, 3], "the opaque ones below its second"


def test_masked_equals_opaque_and_monotonic_on_random_rays():
    """on the 40-triangle scene: with every texture masked, and without textures, the brute force is the opaque one; a cutout hit
    is never nearer than the opaque hit of its ray"""
    tris, attribs = cs.forty()
    o, d = cs.random_rays(128)
    rec = ref.triangle_records(tris)
    opaque = closest.brute_force_closest(o, d, 0.0, 1.0, rec)
    for textures, mask in ((cs.textures(), 0xFFFFFFFF), ([], 0)):
        same = ref.brute_force_closest_cutout(AR, o, d, 0.0, 1.0, rec, attribs, textures, 0, mask)
        assert same.tobytes() == opaque.tobytes()
    cut = ref.brute_force_closest_cutout(AR, o, d, 0.0, 1.0, rec, attribs, cs.textures(), 0, 0)
    hit = cut["index"] != cs.MISS
    assert (cut["index"] != opaque["index"]).any() and (opaque["index"][hit] != cs.MISS).all() and (cut["t"][hit] >= opaque["t"][hit]).all()
