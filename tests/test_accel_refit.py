"""Refit of the ray-query structure, without a GPU: vkr_accel_refit_layout (the rule of vkr_accel_refit as a pure host function, sharing
make_record with the builder) against the numpy restatement tests/accel_refit_reference.py, byte for byte with NaN equal to NaN, for
every scene x motion of that module; the invariants of ray_scene_cases.check_layout on the refitted arrays; the refusals; the
mutants of the restatement, each caught by a named case; the numpy twin of vkr_scene_triangles against abi.scene_triangles; the
bindings and sizes.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from vk_renderer_amd import abi
from vk_renderer_amd import scene as scn

import accel_refit_reference as ref
import ray_scene_cases as cs

F32 = np.float32
SCENES, MOTIONS = sorted(ref.SCENES), sorted(ref.MOTIONS)


def _refit_host(name, motion):
    """vkr_accel_refit_layout applied pose after pose -> [(nodes, recs)]"""
    nodes, recs = ref.built(name)
    out = []
    for p in ref.poses(name, motion):
        nodes, recs = ref.view(*abi.accel_refit_layout(nodes, recs, p))
        out.append((nodes, recs))
    return out


def test_the_small_scenes_are_what_they_are_for():
    """tri1, tri2: a root leaf (two triangles are never split); tri3: the first legal split; tri9: the first forced split; deep has a
    leaf of 14; detail24 has a level wider than the others can hold in one workgroup"""
    assert [len(ref.built(n)[0]) for n in ("tri1", "tri2")] == [1, 1]
    assert len(ref.built("tri3")[0]) == 3 and len(ref.built("tri9")[0]) >= 3
    assert int(ref.built("deep")[0]["count"].max()) == 14 and int(ref.heights(ref.built("deep")[0]).max()) == 48
    assert 4000 < len(ref.scene("detail24")) < 10000
    sizes = np.bincount(ref.heights(ref.built("detail24")[0]))
    assert sizes[0] > 256 and (np.diff(sizes) <= 0).all(), "level sizes never grow with the height"


@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("name", SCENES)
def test_refit_layout_equals_the_restatement(name, motion):
    built_nodes, built_recs = ref.built(name)
    for step, ((nodes, recs), (want_nodes, want_recs)) in enumerate(zip(_refit_host(name, motion), ref.expected(name, motion))):
        assert ref.same_bytes(recs, want_recs), f"{name} x {motion}, pose {step}: records"
        assert ref.same_bytes(nodes, want_nodes), f"{name} x {motion}, pose {step}: nodes"
        # the topology words
        assert np.array_equal(nodes["first"], built_nodes["first"]) and np.array_equal(nodes["count"], built_nodes["count"])
        assert np.array_equal(recs["index"], built_recs["index"])
        assert not np.isnan(nodes["lo"]).any() and not np.isnan(nodes["hi"]).any(), "a node box holds a NaN"


@pytest.mark.parametrize("name", SCENES)
def test_identity_reproduces_the_layout_and_heal_the_identity(name):
    nodes, recs = ref.built(name)
    got_nodes, got_recs = _refit_host(name, "identity")[0]
    assert got_nodes.tobytes() == nodes.tobytes() and got_recs.tobytes() == recs.tobytes()
    poisoned, healed = _refit_host(name, "poison_heal")
    assert healed[0].tobytes() == nodes.tobytes() and healed[1].tobytes() == recs.tobytes()
    assert poisoned[1].tobytes() != recs.tobytes()


def _check_refitted(nodes, recs, tris):
    """ray_scene_cases.check_layout's invariants on refitted arrays: every node the exact union of what lies below it, no NaN in a
    node, every finite vertex inside its leaf, every record in exactly one leaf"""
    want = cs.host_records(tris)
    idx = recs["index"].astype(np.int64)
    assert sorted(idx.tolist()) == list(range(len(tris)))
    for f in ("v0", "e1", "e2", "lo", "hi"):
        got, exp = recs[f], want[f][idx]
        assert ((got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))).all(), f
    covered = np.zeros(len(recs), np.int64)
    seen = np.zeros(len(nodes), np.int64)
    stack = [0]
    while stack:
        i = stack.pop()
        seen[i] += 1
        nd = nodes[i]
        first, count = int(nd["first"]), int(nd["count"])
        if count == 0:
            ch = nodes[[first, first + 1]]
            ulo, uhi = cs._union(ch["lo"], ch["hi"])
            assert np.all(ch["lo"] >= nd["lo"]) and np.all(ch["hi"] <= nd["hi"]), f"a child leaves node {i}"
            stack += [first, first + 1]
        else:
            r = recs[first:first + count]
            covered[first:first + count] += 1
            ulo, uhi = cs._union(r["lo"], r["hi"])
            assert np.all((r["lo"] >= nd["lo"]) | np.isnan(r["lo"])) and np.all((r["hi"] <= nd["hi"]) | np.isnan(r["hi"]))
            with np.errstate(all="ignore"):
                v = np.stack([r["v0"], r["v0"] + r["e1"], r["v0"] + r["e2"]], 1)
            fin = np.isfinite(v) & np.isfinite(tris[r["index"]])
            assert np.all((v >= nd["lo"][None, None]) | ~fin) and np.all((v <= nd["hi"][None, None]) | ~fin), f"a finite vertex leaves leaf {i}"
        assert np.array_equal(ulo.view(np.uint32), nd["lo"].view(np.uint32)) and np.array_equal(uhi.view(np.uint32), nd["hi"].view(np.uint32)), \
            f"node {i} is not the union of what lies below it"
    assert not np.isnan(nodes["lo"]).any() and not np.isnan(nodes["hi"]).any()
    assert np.all(seen == 1) and np.all(covered == 1)


@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("name", [n for n in SCENES if n != "detail24"])
def test_layout_invariants_hold_after_a_refit(name, motion):
    for (nodes, recs), pose in zip(_refit_host(name, motion), ref.poses(name, motion)):
        _check_refitted(nodes, recs, pose)


def test_layout_invariants_hold_on_the_large_scene():
    for motion in ("cluster_swap", "poison_heal"):
        for (nodes, recs), pose in zip(_refit_host("detail24", motion), ref.poses("detail24", motion)):
            _check_refitted(nodes, recs, pose)


def test_the_built_layouts_pass_the_same_check():
    """_check_refitted is check_layout's hierarchy walk: what the builder made passes it too"""
    for name in ("procedural", "deep", "area_overflow"):
        _check_refitted(*ref.built(name), ref.scene(name))
        cs.check_layout(ref.scene(name))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_a_malformed_topology_is_refused():
    tris = ref.scene("procedural")
    nodes, recs = ref.built("procedural")
    interior = int(np.nonzero(nodes["count"] == 0)[0][-1])
    leaf = int(np.nonzero(nodes["count"] > 0)[0][0])
    for what, (kind, i, field, value) in {
        "a child before its parent": ("n", interior, "first", interior - 1),
        "a child that is the node itself": ("n", interior, "first", interior),
        "a second child past the array": ("n", interior, "first", len(nodes) - 1),
        "a child far outside": ("n", interior, "first", 0xFFFFFFFF),
        "a leaf range past the records": ("n", leaf, "first", len(recs) - int(nodes["count"][leaf]) + 1),
        "a leaf count that wraps": ("n", leaf, "count", 0xFFFFFFFF),
        "a record index outside the input": ("t", 5, "index", len(recs)),
    }.items():
        n, r = nodes.copy(), recs.copy()
        (n if kind == "n" else r)[field][i] = value
        before = n.tobytes() + r.tobytes()
        with pytest.raises(RuntimeError) as e:
            abi.accel_refit_layout(n, r, tris)
        assert "vkr_accel_refit_layout" in str(e.value), what
        assert n.tobytes() + r.tobytes() == before
    # the error code is VKR_ERR_EXTENT, the one vkr_accel_layout gives for too little room
    lib = abi.product()
    cap_nodes = (abi.AccelNode * 1)()
    count = C.c_uint32(0)
    t = np.ascontiguousarray(tris).reshape(-1, 9)
    rc_room = lib.vkr_accel_layout(t.ctypes.data, len(t), cap_nodes, 1, (abi.AccelTri * len(t))(), C.byref(count))
    n = nodes.copy()
    n["first"][interior] = interior
    r = recs.copy()
    rc = lib.vkr_accel_refit_layout(n.ctypes.data, len(n), r.ctypes.data, len(r), t.ctypes.data)
    assert rc != 0 and rc == rc_room


def test_host_error_paths():
    lib = abi.product()
    nodes, recs = ref.built("box")
    n, r = nodes.copy(), recs.copy()
    t = np.ascontiguousarray(ref.scene("box")).reshape(-1, 9)
    null_rc = lib.vkr_accel_info(None, None, None)  # VKR_ERR_NULL
    assert null_rc != 0
    assert lib.vkr_accel_refit_layout(n.ctypes.data, len(n), r.ctypes.data, len(r), None) == null_rc
    assert b"NULL triangles" in lib.vkr_last_error()
    assert lib.vkr_accel_refit_layout(None, len(n), r.ctypes.data, len(r), t.ctypes.data) == null_rc
    assert lib.vkr_accel_refit_layout(n.ctypes.data, len(n), None, len(r), t.ctypes.data) == null_rc
    assert lib.vkr_accel_refit_layout(None, 0, None, 0, None) == 0, "an empty structure is a no-op"
    assert n.tobytes() == nodes.tobytes() and r.tobytes() == recs.tobytes()
    # the device entries refuse a NULL handle before they touch a device
    assert lib.vkr_accel_refit(None, None, None) == null_rc and b"vkr_accel_refit" in lib.vkr_last_error()
    assert lib.vkr_accel_download(None, None, 0, None, 0, None) == null_rc
    assert lib.vkr_accel_refit_schedule(None, None, 0, None, None) == null_rc
    assert lib.vkr_scene_triangles(None, None, 0, None, 0, None) == null_rc
    # vkr_scene_triangles: check_scene is the gate, and runs before the device is needed
    sc = scn.procedural_scene(detail=3)
    rs, keep = sc.upload(device=None)
    draws = C.cast(rs.draws, C.POINTER(abi.RasterDraw))
    draws[2].index_count = 0xFFFFFFF0
    rc = lib.vkr_scene_triangles(C.byref(rs), None, 0, None, 0, None)
    assert rc != 0 and rc != null_rc and b"scene_triangles: scene: draw 2" in lib.vkr_last_error()
    rs2, keep2 = sc.upload(device=None)
    C.cast(rs2.draws, C.POINTER(abi.RasterDraw))[0].transform_index = 99
    assert lib.vkr_scene_triangles(C.byref(rs2), None, 0, None, 0, None) == rc
    rs3, keep3 = sc.upload(device=None)
    rs3.vertices = None
    assert lib.vkr_scene_triangles(C.byref(rs3), None, 0, None, 0, None) == null_rc
    rs4, keep4 = sc.upload(device=None)
    assert lib.vkr_scene_triangles(C.byref(rs4), None, 0, None, 0, None) == null_rc and b"NULL output or scratch" in lib.vkr_last_error()
    rs4.draw_count = 0
    assert lib.vkr_scene_triangles(C.byref(rs4), None, 0, None, 0, None) == 0, "a scene without draws has no triangles"


def test_sizes_and_bindings():
    lib = abi.product()
    for name in ("accel_refit", "accel_refit_layout", "accel_download", "accel_refit_schedule", "scene_triangles", "scene_triangles_scratch_bytes"):
        assert getattr(lib, "vkr_" + name).argtypes is not None, name
    assert C.sizeof(abi.AccelNode) == 32 == cs.NODE.itemsize and C.sizeof(abi.AccelTri) == 64 == cs.TRI.itemsize
    assert abi.scene_triangles_scratch_bytes(0) == 256 and abi.scene_triangles_scratch_bytes(4) == 256
    assert abi.scene_triangles_scratch_bytes(5) == 512 and abi.scene_triangles_scratch_bytes(1024) == 64 * 1024
    for method in ("refit", "download", "refit_schedule"):
        assert callable(getattr(abi.Accel, method))
    assert callable(abi.scene_world_triangles)
    hdr = open(abi.ROOT + "/include/vkr_postfx.h").read()
    for name in ("vkr_accel_refit(", "vkr_accel_refit_layout(", "vkr_accel_download(", "vkr_scene_triangles(", "vkr_scene_triangles_scratch_bytes("):
        assert name in hdr, name


def test_the_frame_entry_and_its_refusals_without_a_device():
    from vk_renderer_amd import host
    from test_shadow_mask_rt import _HostMemoryFrame

    l = host.lib()
    assert hasattr(l, "vkrh_set_draw_transforms") and callable(host.HostFrame.set_draw_transforms)
    m = (C.c_float * 16)(*np.eye(4, dtype=F32).reshape(-1))
    frame = _HostMemoryFrame(tiled=False)
    try:
        assert l.vkrh_set_draw_transforms(frame.h, m, 1) != 0
        assert l.vkrh_last_error().decode() == "vkrh_set_draw_transforms: without a loaded scene (vkrh_load_scene)"
    finally:
        frame.close()
    frame = _HostMemoryFrame(tiled=True)
    try:
        assert l.vkrh_set_draw_transforms(frame.h, m, 1) != 0
        assert l.vkrh_last_error().decode() == "vkrh_set_draw_transforms: on a tiled frame (the ray-traced stages run on one GPU)"
    finally:
        frame.close()
    assert l.vkrh_set_draw_transforms(None, m, 1) != 0


# ---- mutants ----------------------------------------------------------------------------------------------------------------------
# mutant -> the (scene, motion) that catches it
CAUGHT_BY = {
    "grow": ("procedural", "scale_2m40"),          # every box shrinks: a grown one keeps the old extent
    "skip_level": ("procedural", "translation"),   # the nodes of height 1 stay where the scene was
    "drop_last": ("procedural", "cluster_swap"),   # the last record of a leaf now lies in the other half of the scene
    "nan_min": ("procedural", "poison_heal"),      # the poisoned pose has NaN record bounds, which must not enter a node
    "old_margin": ("procedural", "translation"),   # the margin grows from about 2^-8 to 2: the old one is too small
}


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_of_the_restatement_is_caught(mutant):
    name, motion = CAUGHT_BY[mutant]
    nodes, recs = ref.built(name)
    old = ref.scene(name)
    caught = False
    for pose, (want_nodes, want_recs), (got_nodes, got_recs) in zip(ref.poses(name, motion), ref.expected(name, motion), _refit_host(name, motion)):
        m_nodes, m_recs = ref.refit(nodes, recs, pose, mutant=mutant, old_tris=old)
        assert ref.same_bytes(got_nodes, want_nodes) and ref.same_bytes(got_recs, want_recs)
        caught = caught or not (ref.same_bytes(m_nodes, got_nodes) and ref.same_bytes(m_recs, got_recs))
        nodes, recs, old = m_nodes, m_recs, pose
    assert caught, f"{mutant} passes {name} x {motion}"


def test_the_identity_catches_no_mutant_but_the_others_do():
    """the motions matter: on the identity every mutant but drop_last gives the right bytes"""
    nodes, recs = ref.built("procedural")
    for mutant in ("grow", "skip_level", "nan_min", "old_margin"):
        m_nodes, m_recs = ref.refit(nodes, recs, ref.scene("procedural"), mutant=mutant, old_tris=ref.scene("procedural"))
        assert ref.same_bytes(m_nodes, nodes) and ref.same_bytes(m_recs, recs), mutant


# ---- vkr_scene_triangles' rule ----------------------------------------------------------------------------------------------------
def _twin_of(sc):
    draws = [dict(transform=d["transform"], index_offset=d["index_offset"], index_count=d["index_count"], vertex_offset=d["vertex_offset"]) for d in sc.draws]
    return ref.scene_triangles_twin(sc.vertices, sc.indices, [m for m, _ in sc.transforms], draws)


@pytest.mark.parametrize("detail", [3, 24])
def test_the_twin_of_scene_triangles_equals_abi_scene_triangles(detail):
    sc = scn.procedural_scene(detail=detail, cutout=True)
    want = np.asarray(abi.scene_triangles(sc), F32)
    got = _twin_of(sc)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


def test_the_twin_marks_a_triangle_with_an_index_outside_the_vertex_buffer():
    sc = scn.procedural_scene(detail=3)
    want = np.asarray(abi.scene_triangles(sc), F32)
    bad = 7
    d = sc.draws[2]
    sc.indices = sc.indices.copy()
    sc.indices[d["index_offset"] + 3 * bad + 1] = len(sc.vertices)  # vertex_offset is added on top: outside
    got = _twin_of(sc)
    # the three spheres share the mesh: the triangle is bad in each of their draws
    base = np.cumsum([0] + [x["index_count"] // 3 for x in sc.draws])
    at = [int(base[k]) + bad for k, x in enumerate(sc.draws) if x["index_offset"] == d["index_offset"]]
    assert len(at) == 3 and np.isnan(got[at]).all()
    keep = ~np.isin(np.arange(len(want)), at)
    assert not np.isnan(got[keep]).any()
    assert got[keep].tobytes() == want[keep].tobytes()
