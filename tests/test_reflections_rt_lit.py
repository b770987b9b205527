"""Lit ray-traced reflections without a GPU: the C-ABI records and symbols, abi.scene_triangle_normals on the procedural scene,
every refusal of vkr_reflections_rt_lit, vkr_reflections_rt_lit_cutout and vkr_scene_triangle_normals with its text (validation
never reaches a launch), and the numpy restatement (tests/reflections_rt_lit_reference.py) held to three things: with no light and
ambient 1 it is tests/reflections_rt_reference.py's image; on the procedural scene at 64 x 36 it covers what the rule can do; and
every mutant of the rule changes that image.

Coverage at raster 64 x 36 (the procedural scene at detail 8, the frozen camera, the frame's ray offsets, max_distance = zfar,
shadow_offset 0.001, shadow_tmin 0, the four lights below), measured on the restatement under contract 2: 851 hits, on all five draws
165 / 338 / 129 / 88 / 131; 338 of them with a flipped normal; facing away / shadowed / lit per light: L0 148 / 42 / 661,
L1 171 / 36 / 644, L2 196 / 162 / 493, L3 605 / 101 / 145.  The test asserts at least half of each.  With COLOURS and AMBIENT, 783 of
the 851 hits are lit by at least one light, and 776 of those store no channel at 255 and differ from their ambient-only value.

Three mutants need an input of their own, because on ordinary lights they are the rule up to the byte that is stored:
  * "reverse_order": the order of four sums of like magnitude shows in the last bits of a float, not in 8 bits.  L3 becomes a second
    copy of L1 with the colour -2^26 against L1's +2^26 (four distinct colours): in index order L0's term is absorbed by the large
    one before that is taken away again, in reverse order it is added last and survives;
  * "ndl_unclamped": behind facing > 0 the cosine dot(N, normalize(dvec)) can only be <= 0 or NaN when the normalisation of dvec
    degenerates, so L3 is scaled by 2^-100 (dot(dvec, dvec) underflows to 0, the direction becomes inf / NaN, and the rule's "0 unless
    ndl > 0" is what keeps the ambient term);
  * "facing_ge": facing == 0 means a cosine of 0, which adds nothing whether or not the light is taken, unless 0 meets an infinite
    colour (legal: only a NaN is refused).  L3 becomes the horizontal (1, 0, 0) with an infinite colour: the ground's normal is
    (0, 1, 0) exactly, the rule skips the light there, the mutant adds 0 * inf = NaN and stores 0."""
import ctypes as C

import numpy as np
import pytest

from vk_renderer_amd import abi
from vk_renderer_amd import scene as scn

import reflections_rt_lit_reference as lit
import reflections_rt_reference as unlit
import test_ray_cutout as cut
import test_reflections_rt_gpu as base  # its scene, G-buffer kit and expectations (the module's gpu mark stays its own)
from test_abi_errors import ERR_EXTENT, ERR_LAYOUT, ERR_NULL, FAKE, img

F32 = np.float32
SIZE = (64, 36)
LIGHTS = [(-1.85867, 5.81832, -0.247114, 1.0), (3.0, 4.0, -2.0, 0.0), (0.0, 0.25, 4.0, 1.0), (-6.0, 1.0, 3.0, 0.0)]
COLOURS = [(3.0, 2.5, 2.0), (0.30, 0.27, 0.22), (0.25, 0.35, 0.45), (0.12, 0.2, 0.16)]  # four distinct ones
AMBIENT = (0.1, 0.12, 0.14)
SHADOW_OFFSET, SHADOW_TMIN = 0.001, 0.0
AR = lit.Arith(2)


# ---- the records and the symbols --------------------------------------------------------------------------------------------------------
def test_record_layouts_and_symbols():
    assert C.sizeof(abi.HitNormal) == 48 and abi.hit_normal_dtype().itemsize == 48
    assert C.sizeof(abi.ReflectLights) == 176
    assert (abi.ReflectLights.colour.offset, abi.ReflectLights.ambient.offset, abi.ReflectLights.light_count.offset) == (64, 128, 144)
    assert (abi.ReflectLights.shadow_offset.offset, abi.ReflectLights.shadow_tmin.offset, abi.ReflectLights.reserved.offset) == (148, 152, 156)
    txt = open(abi.ROOT + "/include/vkr_postfx.h").read()
    lib = abi.product()
    for name in ("reflections_rt_lit", "reflections_rt_lit_cutout", "scene_triangle_normals"):
        assert name in abi.ENTRY_ARGS and "vkr_" + name + "(" in txt and hasattr(lib, "vkr_" + name), name
    p = abi.reflect_lights(LIGHTS[:2], COLOURS[:2], AMBIENT, 0.5, 0.25)
    assert p.light_count == 2 and (p.shadow_offset, p.shadow_tmin) == (0.5, 0.25) and list(p.reserved) == [0] * 5
    assert [list(v) for v in p.lights[:2]] == [[F32(x) for x in l] for l in LIGHTS[:2]]
    assert list(p.colour[1]) == [F32(0.30), F32(0.27), F32(0.22), 0.0] and list(p.ambient) == [F32(0.1), F32(0.12), F32(0.14), 0.0]
    with pytest.raises(RuntimeError, match="at most 4"):
        abi.reflect_lights(LIGHTS + LIGHTS[:1], COLOURS + COLOURS[:1])


# ---- abi.scene_triangle_normals ------------------------------------------------------------------------------------------------------------
def test_scene_triangle_normals_on_the_procedural_scene():
    """one record per triangle of scene_triangles, .w 0, every normal the draw's normal matrix times the vertex normal in fp32; on
    the procedural scene the ground's and the wall's have unit length up to rounding, the scaled spheres' have not (the table is
    not normalised), and the flat ground's point straight up"""
    sc, tris, att, draw_of = base._scene()
    nr = abi.scene_triangle_normals(sc)
    assert nr.dtype == abi.hit_normal_dtype() and len(nr) == len(tris) == len(att)
    assert (nr["n"][..., 3] == 0).all()
    lengths = np.linalg.norm(nr["n"][..., :3].astype(np.float64), axis=-1)
    assert lengths.min() > 0.3 and lengths.max() < 3.0
    assert np.abs(lengths[draw_of <= 1] - 1.0).max() < 1e-5 and (np.abs(lengths - 1.0) > 0.1).any(), "scaled draws: the table is not normalised"
    assert np.allclose(nr["n"][draw_of == 0][..., :3], [0.0, 1.0, 0.0], atol=1e-6), "draw 0 is the ground"
    # the rule, restated for one draw with a transform that is no rotation: a non-uniform scale and a shear
    one = scn.Scene()
    model = np.array([[2, 0.5, 0, 1], [0, 0.25, 0, 2], [0, 0, -3, 3], [0, 0, 0, 1]], F32)
    t = one.add_transform(model)
    normal = one.transforms[t][1]
    v = np.array([[0, 0, 0, 0.3, -0.4, 0.5, 0, 0], [1, 0, 0, 1, 2, 3, 1, 0], [0, 1, 0, -7, 0.125, 0, 0, 1]], F32)
    one.vertices, one.indices = v, np.array([0, 1, 2], np.uint32)
    one.draws = [dict(index_offset=0, index_count=3, vertex_offset=0, transform=t, albedo=scn.INVALID)]
    got = abi.scene_triangle_normals(one)["n"][0]
    for k in range(3):
        x, y, z = v[k, 3:6]
        for r in range(3):
            assert got[k, r] == (normal[r, 0] * x + normal[r, 1] * y) + normal[r, 2] * z
    assert len(abi.scene_triangle_normals(scn.Scene())) == 0


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------------
W, H = cut.W, cut.H


def _lights(**over):
    p = abi.reflect_lights(over.pop("lights", LIGHTS[:1]), over.pop("colours", COLOURS[:1]), over.pop("ambient", AMBIENT),
                           over.pop("shadow_offset", SHADOW_OFFSET), over.pop("shadow_tmin", SHADOW_TMIN))
    for k, v in over.items():
        if k == "reserved":
            p.reserved[3] = v
        elif k == "colour_w":
            p.colour[v][3] = 1.0
        elif k == "ambient_w":
            p.ambient[3] = v
        else:
            setattr(p, k, v)
    return p


class _FakeAccel:
    """the bytes of a structure of three triangles that no launch ever sees: the gates read its counts and nothing else (the
    record of accel_traverse.hpp: two device pointers, two counts, the refit schedule's pointer and vector)"""

    def __init__(self, tri_count=3):
        self.buf = (C.c_uint64 * 8)()
        self.buf[0] = self.buf[1] = FAKE
        self.buf[2] = (tri_count << 32) | 1  # node_count 1, tri_count
        self.handle = C.cast(self.buf, C.c_void_p)


FAKE_ACCEL = _FakeAccel()


def _entry(entry, depth="ok", normal="ok", rays=None, accel="ok", attribs=None, attrib_count=0, normals=None, normal_count=0, textures=None,
           texture_count=0, params="ok", lights="ok", cutout=cut.CUT, out="ok", scratch=FAKE, scratch_bytes=None):
    lib = abi.product()
    d = img(cut.D24, W, H) if depth == "ok" else depth
    n = img(cut.RG16, W, H) if normal == "ok" else normal
    o = img(cut.RGBA8, W, H) if out == "ok" else out
    p = cut._reflect_params() if params == "ok" else params
    li = _lights() if lights == "ok" else lights
    a = cut._empty_accel().handle if accel == "ok" else accel
    nbytes = abi.reflections_rt_scratch_bytes(texture_count) if scratch_bytes is None else scratch_bytes
    head = (cut._byref(d), cut._byref(n), cut._byref(rays), a, attribs, attrib_count, normals, normal_count, textures, texture_count, cut._byref(p),
            cut._byref(li))
    tail = (cut._byref(o), scratch, nbytes, None)
    if entry == "reflections_rt_lit":
        rc = lib.vkr_reflections_rt_lit(*head, *tail)
    else:
        rc = lib.vkr_reflections_rt_lit_cutout(*head, cut._byref(cutout), *tail)
    return rc, (lib.vkr_last_error() or b"").decode()


NAN = float("nan")
THREE = dict(accel=FAKE_ACCEL.handle, attribs=FAKE, attrib_count=3)
LIT_REFUSALS = {
    "lights NULL": (dict(lights=None), ERR_NULL, "lights is NULL"),
    "normals NULL with triangles": (dict(THREE, normals=None, normal_count=3), ERR_NULL, "normals is NULL"),
    "normals unaligned": (dict(THREE, normals=FAKE + 8, normal_count=3), ERR_LAYOUT, "normals must be 16-byte aligned"),
    "normal_count": (dict(normals=FAKE, normal_count=3), ERR_EXTENT, "3 normal records for a structure of 0 triangles"),
    "normal_count of a structure with triangles": (dict(THREE, normals=FAKE, normal_count=2), ERR_EXTENT, "2 normal records for a structure of 3 triangles"),
    "five lights": (dict(lights=_lights(light_count=5)), ERR_EXTENT, "light_count 5, expected 0..4"),
    "light w": (dict(lights=_lights(lights=[(0, 5, 0, 0.5)])), ERR_EXTENT, "light 0 has w = 0.5"),
    "second light w": (dict(lights=_lights(lights=[LIGHTS[0], (0, 5, 0, NAN)], colours=COLOURS[:2])), ERR_EXTENT, "light 1 has w = nan"),
    "colour w": (dict(lights=_lights(colour_w=2)), ERR_EXTENT, "colour 2 has w = 1, must be 0"),
    "ambient w": (dict(lights=_lights(ambient_w=0.5)), ERR_EXTENT, "ambient has w = 0.5, must be 0"),
    "lights reserved": (dict(lights=_lights(reserved=7)), ERR_EXTENT, "lights: reserved must be 0"),
    "shadow_offset NaN": (dict(lights=_lights(shadow_offset=NAN)), ERR_EXTENT, "shadow_offset is NaN"),
    "shadow_tmin NaN": (dict(lights=_lights(shadow_tmin=NAN)), ERR_EXTENT, "shadow_tmin is NaN"),
    "ambient NaN": (dict(lights=_lights(ambient=(0.1, NAN, 0.1))), ERR_EXTENT, "ambient is NaN"),
    "colour NaN": (dict(lights=_lights(colours=[(1.0, 1.0, NAN)])), ERR_EXTENT, "colour 0 is NaN"),
}
# all of the unlit sibling's, under this program's prefix; the entry without a cutout has no cutout to refuse
SIBLING = {k: (kw, code, text.replace("reflections_rt_cutout", "{program}")) for k, (kw, code, text) in cut.REFLECT_REFUSALS.items()}


REFUSALS = [(entry, name) for entry in ("reflections_rt_lit", "reflections_rt_lit_cutout") for name in sorted(LIT_REFUSALS) + sorted(SIBLING)
            if not (name == "cutout NULL" and entry == "reflections_rt_lit")]


@pytest.mark.parametrize("entry,name", REFUSALS)
def test_entry_refusals(entry, name):
    kwargs, code, message = LIT_REFUSALS[name] if name in LIT_REFUSALS else SIBLING[name]
    rc, msg = _entry(entry, **kwargs)
    assert rc == code, (name, rc, msg)
    assert msg.startswith(entry + ": ") or msg.startswith(entry + "."), msg
    assert message.replace("{program}", entry) in msg, (name, msg)


def test_what_the_gates_let_through():
    """a NaN colour of a light that is not in use, an infinite colour, zero lights and a NULL table for an empty structure are no
    refusals: with the empty structure the call gets as far as the launch, which this machine cannot make or makes for nothing"""
    li = _lights(lights=[], colours=[])
    li.colour[2][0] = NAN
    li.colour[0][1] = float("inf")
    rc, msg = _entry("reflections_rt_lit", lights=li, out=None)
    assert rc == ERR_NULL and "out_reflections is NULL" in msg, "the sibling's gates come first"
    # behind the sibling's gates the first of this entry's refusals still fires: the lights above pass, a sixth word does not
    li.reserved[0] = 1
    rc, msg = _entry("reflections_rt_lit", lights=li)
    assert rc == ERR_EXTENT and "reserved must be 0" in msg


def test_scene_triangle_normals_refusals():
    lib = abi.product()

    def call(scene, out=FAKE, capacity=10, scratch=FAKE, nbytes=None):
        nbytes = abi.scene_triangles_scratch_bytes(scene.draw_count if scene is not None else 0) if nbytes is None else nbytes
        rc = lib.vkr_scene_triangle_normals(None if scene is None else C.byref(scene), out, capacity, scratch, nbytes, None)
        return rc, (lib.vkr_last_error() or b"").decode()

    rc, msg = call(None)
    assert rc == ERR_NULL and msg == "scene_triangle_normals: NULL scene"
    sc = scn.procedural_scene(detail=3)
    rs, keep = sc.upload()  # host memory: no launch is reached
    total = sum(d["index_count"] // 3 for d in sc.draws)
    for kwargs, code, text in ((dict(out=None), ERR_NULL, "NULL output or scratch"), (dict(scratch=None), ERR_NULL, "NULL output or scratch"),
                               (dict(out=FAKE + 4), ERR_LAYOUT, "out must be 16-byte aligned"),
                               (dict(capacity=total - 1), ERR_EXTENT, f"{total} triangles do not fit into {total - 1}"),
                               (dict(capacity=total, nbytes=8), ERR_EXTENT, "scratch too small")):
        rc, msg = call(rs, **dict(dict(capacity=total), **kwargs))
        assert rc == code and msg.startswith("scene_triangle_normals: ") and text in msg, (kwargs, rc, msg)
    keep[-2][0].transform_index = 99  # the draw array
    rc, msg = call(rs, capacity=total)
    assert rc == ERR_EXTENT and "scene_triangle_normals: scene: draw 0: transform_index 99" in msg
    empty = abi.RasterScene()
    assert call(empty, out=None, scratch=None, nbytes=0)[0] == 0, "no triangles is not an error"
    del keep


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def _restate(lights=LIGHTS, colours=COLOURS, ambient=AMBIENT, mutant=None, cutout=None, scene=None, size=SIZE, name="raster"):
    words, codes, setup, _, _ = base._inputs(name, size)
    sc, tris, att, _ = base._scene() if scene is None else scene
    before = np.zeros(words.shape + (4,), np.uint8)
    return lit.reflections_rt_lit(AR, words, codes, None, setup.inv_view, *setup.fazz, base.OFFSET, base.TMIN, float(setup.fazz[3]), 0, 0, tris, att,
                                  abi.scene_triangle_normals(sc), sc.textures, before, lights, colours, ambient, SHADOW_OFFSET, SHADOW_TMIN,
                                  cutout=cutout, mutant=mutant)


@pytest.fixture(scope="module")
def stock():
    return _restate()


@pytest.mark.parametrize("name", ["raster", "normal_noise", "checker_px"])
def test_no_light_and_ambient_one_is_the_unlit_pass(name):
    words, codes, setup, _, _ = base._inputs(name, SIZE)
    sc, tris, att, _ = base._scene()
    before = np.full(words.shape + (4,), 0xA5, np.uint8)
    for fill in (None, "px"):
        args = (AR, words, codes, base._rays_w(SIZE, fill) if fill else None, setup.inv_view, *setup.fazz, base.OFFSET, base.TMIN, float(setup.fazz[3]), 1,
                unlit.FILL_MISSES if fill else 0, tris, att)
        want, traced, index = unlit.reflections_rt(*args, sc.textures, before)
        got, traced2, index2, _ = lit.reflections_rt_lit(*args, abi.scene_triangle_normals(sc), sc.textures, before, [], [], (1.0, 1.0, 1.0),
                                                         SHADOW_OFFSET, SHADOW_TMIN)
        assert np.array_equal(got, want) and np.array_equal(traced, traced2) and np.array_equal(index, index2)
        assert (index != unlit.MISS).sum() > 100 or name != "raster"


def test_the_restatement_covers_what_the_rule_can_do(stock):
    image, traced, index, info = stock
    sc, _, _, draw_of = base._scene()
    hit = index != unlit.MISS
    per_draw = np.bincount(draw_of[index[hit]], minlength=len(sc.draws)).tolist()
    flipped = int(info["flipped"].sum())
    per_light = [tuple(int(m.sum()) for m in s) for s in info["lights"]]
    print(f"[reflections rt lit] raster 64x36: {int(hit.sum())} hits, per draw {per_draw}, {flipped} flipped, away / shadowed / lit per light {per_light}")
    assert int(hit.sum()) >= 851 // 2 and len(info["hits"]) == int(hit.sum())
    for got, measured in zip(per_draw, (165, 338, 129, 88, 131)):
        assert got >= measured // 2 + measured % 2, (per_draw, "hits on all five draws")
    assert flipped >= 338 // 2
    for got, measured in zip(per_light, ((148, 42, 661), (171, 36, 644), (196, 162, 493), (605, 101, 145))):
        assert all(g >= (m + 1) // 2 for g, m in zip(got, measured)), (per_light, measured)
    # the colours: most lit hits neither saturate nor stay at their ambient-only value
    ambient_only = _restate(lights=[], colours=[])[0]
    lit_any = np.zeros(len(info["hits"]), bool)
    for _, _, l in info["lights"]:
        lit_any |= l
    texels, dark = image.reshape(-1, 4)[info["hits"]], ambient_only.reshape(-1, 4)[info["hits"]]
    good = lit_any & (texels[:, :3] != 255).all(axis=1) & (texels != dark).any(axis=1)
    print(f"[reflections rt lit] {int(lit_any.sum())} hits lit by a light, {int(good.sum())} of them unsaturated and other than ambient-only")
    assert 2 * int(good.sum()) >= int(lit_any.sum()) > 400
    assert (image[..., 3] == 0).all() and (image[~hit] == 0).all()


@pytest.mark.parametrize("mutant", lit.MUTANTS)
def test_every_mutant_changes_the_image(stock, mutant):
    lights, colours = list(LIGHTS), list(COLOURS)
    want = stock[0]
    if mutant == "ndl_unclamped":  # see the module's text
        lights[3] = tuple(F32(v) * F32(2.0 ** -100) for v in LIGHTS[3][:3]) + (0.0,)
    if mutant == "facing_ge":
        lights[3], colours[3] = (1.0, 0.0, 0.0, 0.0), (np.inf, np.inf, np.inf)
    if mutant == "reverse_order":
        lights[3], colours[1], colours[3] = LIGHTS[1], (2.0 ** 26,) * 3, (-2.0 ** 26,) * 3
    if mutant in ("ndl_unclamped", "facing_ge", "reverse_order"):
        want = _restate(lights=lights, colours=colours)[0]
    got = _restate(lights=lights, colours=colours, mutant=mutant)[0]
    differing = int((got != want).any(axis=-1).sum())
    print(f"[reflections rt lit] mutant {mutant}: {differing} of {got.shape[0] * got.shape[1]} texels differ")
    assert differing > 0, f"the inputs cannot tell the rule from the mutant {mutant}"


# ---- the frame's setting -----------------------------------------------------------------------------------------------------------------------
def test_frame_setting_and_its_refusal_on_a_tiled_frame():
    from vk_renderer_amd import host
    from test_shadow_mask_rt import _HostMemoryFrame

    l = host.lib()
    assert hasattr(l, "vkrh_set_reflection_lights") and hasattr(l, "vkrh_scene_hit_normals")
    fl = (C.c_float * 4)(*LIGHTS[0])
    fc = (C.c_float * 3)(*COLOURS[0])
    fa = (C.c_float * 3)(*AMBIENT)
    frame = _HostMemoryFrame(tiled=False)
    try:
        assert l.vkrh_set_reflection_lights(frame.h, 1, None, None, None, 1e-3, 0.0) == 0, "the default light"
        assert l.vkrh_set_reflection_lights(frame.h, 1, fl, fc, fa, 1e-3, 0.0) == 0
        assert l.vkrh_set_reflection_lights(frame.h, 0, None, None, fa, 1e-3, 0.0) == 0, "ambient alone"
        for args, text in (((5, fl, fc, fa, 1e-3, 0.0), "5 lights, at most 4"), ((1, None, fc, fa, 1e-3, 0.0), "NULL argument"),
                           ((1, fl, fc, None, 1e-3, 0.0), "NULL argument"), ((1, fl, fc, fa, NAN, 0.0), "shadow_offset is NaN"),
                           ((1, fl, fc, fa, 1e-3, NAN), "shadow_tmin is NaN")):
            assert l.vkrh_set_reflection_lights(frame.h, *args) != 0 and "vkrh_set_reflection_lights: " + text in l.vkrh_last_error().decode(), args
        # the stage still refuses what it refused, before anything is recorded
        rc, msg = frame.run(host.STAGE_REFLECTIONS_RT)
        assert rc != 0 and "VKRH_STAGE_REFLECTIONS_RT without a loaded scene" in msg
        n = C.c_uint32(7)
        assert l.vkrh_scene_hit_normals(frame.h, None, 0, C.byref(n)) != 0 and "without a loaded scene" in l.vkrh_last_error().decode()
    finally:
        frame.close()
    frame = _HostMemoryFrame(tiled=True)
    try:
        assert l.vkrh_set_reflection_lights(frame.h, 1, None, None, None, 1e-3, 0.0) != 0
        assert "vkrh_set_reflection_lights: on a tiled frame" in l.vkrh_last_error().decode()
    finally:
        frame.close()
