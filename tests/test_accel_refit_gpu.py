"""Refit of the ray-query structure on the GPU (csrc/accel_refit.hip): vkr_accel_refit then vkr_accel_download against
vkr_accel_refit_layout for every scene x motion of tests/accel_refit_reference.py; the ordering contract (two refits queued back to
back with a query between them and nothing synchronised); every ray-level entry on a refitted structure against the brute force of
the MOVED triangles and against a structure freshly created from them, bit for bit; vkr_scene_triangles against
abi.scene_triangles.

Every comparison is of bytes.  One exception is stated where it applies: a NaN is equal to a NaN (the host's and the device's
invalid operations give quiet NaNs of different sign; no entry reads a NaN's payload)."""
import functools

import numpy as np
import pytest

from vk_renderer_amd import abi
from vk_renderer_amd import scene as scn

import accel_refit_reference as ref
import closest_hit_reference as closest
import gtao_rt_reference as gref
import ray_cutout_cases as cut
import ray_cutout_reference as cutref
import ray_scene_cases as cs
from test_accel_closest_gpu import _compare as _compare_closest
from test_accel_closest_gpu import _last_subtree_rays, _run
from test_accel_occluded_gpu import _both, _rays
from test_accel_occluded_gpu import _compare as _compare_any
from test_ray_cutout_gpu import _arith, _same_bits, _textures
from test_ray_cutout_gpu import _run as _run_cutout

pytestmark = pytest.mark.gpu

F32 = np.float32
MISS = closest.MISS
SCENES, MOTIONS = sorted(ref.SCENES), sorted(ref.MOTIONS)


def _dev(tris):
    import torch

    return torch.from_numpy(np.array(tris, dtype=F32, order="C")).to("cuda")


@pytest.fixture(scope="module")
def accels():
    """name -> abi.Accel of the scene as built, made on first use, closed with the module; a refit is from scratch, so whatever
    pose an earlier test left behind does not matter to the next"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = abi.Accel(ref.scene(name))
        return made[name]

    yield get
    for a in made.values():
        a.close()


def _host(nodes, recs, pose):
    return ref.view(*abi.accel_refit_layout(nodes, recs, pose))


# ---- the bytes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("name", SCENES)
def test_refit_then_download_equals_refit_layout(name, motion, accels):
    accel = accels(name)
    nodes, recs = ref.built(name)
    for step, pose in enumerate(ref.poses(name, motion)):
        verts = _dev(pose)
        accel.refit(verts)
        got_nodes, got_recs = ref.view(*accel.download())
        nodes, recs = _host(nodes, recs, pose)
        assert ref.same_bytes(got_recs, recs), f"{name} x {motion}, pose {step}: records"
        assert ref.same_bytes(got_nodes, nodes), f"{name} x {motion}, pose {step}: nodes"
        assert np.array_equal(got_nodes["first"], nodes["first"]) and np.array_equal(got_nodes["count"], nodes["count"])
        assert np.array_equal(got_recs["index"], recs["index"])
        assert not np.isnan(got_nodes["lo"]).any() and not np.isnan(got_nodes["hi"]).any(), "a node box holds a NaN"
        if not (np.isnan(recs["lo"]).any() or np.isnan(recs["e1"]).any() or np.isnan(recs["e2"]).any() or np.isnan(recs["v0"]).any()):
            assert got_nodes.tobytes() == nodes.tobytes() and got_recs.tobytes() == recs.tobytes(), "without a NaN the bytes are the same"


@pytest.mark.parametrize("name", ["tri1", "procedural", "deep", "detail24"])
def test_identity_and_heal_give_the_built_bytes(name, accels):
    accel = accels(name)
    nodes, recs = ref.built(name)
    for pose in ref.poses(name, "poison_heal") + ref.poses(name, "identity"):
        accel.refit(_dev(pose))
    got_nodes, got_recs = ref.view(*accel.download())
    assert got_nodes.tobytes() == nodes.tobytes() and got_recs.tobytes() == recs.tobytes()


def test_the_schedule_of_the_large_scene_has_level_launches_and_a_tail(accels):
    sizes, tail = accels("detail24").refit_schedule()
    want = np.bincount(ref.heights(ref.built("detail24")[0])).tolist()
    assert sizes == want and tail == 256
    launched = [s for s in sizes if s > tail]
    assert len(launched) >= 1 and len(launched) < len(sizes), "at least one per-level launch and the tail"
    assert sizes[:len(launched)] == launched, "the levels with a launch of their own are the first ones"
    small, tail = accels("procedural").refit_schedule()
    assert small == np.bincount(ref.heights(ref.built("procedural")[0])).tolist() and max(small) <= tail, "procedural runs in the tail alone"
    deep, _ = accels("deep").refit_schedule()
    assert len(deep) == 49 and deep[-1] == 1
    assert abi.Accel(np.zeros((0, 3, 3), F32)).refit_schedule()[0] == []


def test_an_empty_structure_is_a_no_op_and_null_vertices_are_refused():
    empty = abi.Accel(np.zeros((0, 3, 3), F32))
    empty.refit(None)
    assert [len(x) for x in empty.download()] == [0, 0]
    lib = abi.product()
    one = abi.Accel(ref.scene("tri1"))
    assert lib.vkr_accel_refit(one.handle, None, None) == lib.vkr_accel_info(None, None, None) != 0
    nodes, recs = one.download()
    assert nodes.tobytes() == ref.built("tri1")[0].tobytes() and recs.tobytes() == ref.built("tri1")[1].tobytes()
    assert lib.vkr_accel_download(one.handle, nodes.ctypes.data, 0, recs.ctypes.data, 1, None) != 0, "too little room is refused"


# ---- rays ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _moved_case(name, motion):
    """the pose of a motion (the first: for poison_heal the poisoned one) with the ray classes of ray_scene_cases.case rebuilt
    around it; a poisoned pose gets the rays of the unpoisoned scene, as nonfinite_vertices does"""
    tris = ref.poses(name, motion)[0]
    geometry = ref.scene(name) if motion == "poison_heal" else tris
    rng = np.random.default_rng([97, SCENES.index(name), MOTIONS.index(motion)])
    with np.errstate(all="ignore"):
        o, d, tag = _rays(np.array(geometry), rng)
        fo, fd, ftag, _ = cs.far_rays(np.array(geometry), rng)
        o, d, tag = np.concatenate([o, fo]), np.concatenate([d, fd]), np.concatenate([tag, ftag])
        last = _last_subtree_rays(np.array(geometry), rng)
    if last is not None:
        o, d, tag = np.concatenate([o, last[0]]), np.concatenate([d, last[1]]), np.concatenate([tag, np.array(["last_subtree"] * len(last[0]))])
    return tris, np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32), tag, cs.host_records(tris)


MOVED = [("procedural", "jitter"), ("procedural", "cluster_swap"), ("procedural", "translation"), ("procedural", "poison_heal"),
         ("deep", "cluster_swap"), ("deep", "jitter")]


def _attributes(n):
    kinds = np.array([cut.CHECKER, cut.SOLID, cut.HOLE, cut.MIPPED, cut.ODD, cut.EDGE, cut.MISS, cut.TEXTURE_COUNT + 1], np.int64)
    return cut.attributes(kinds[np.arange(n) % len(kinds)])


@pytest.mark.parametrize("name,motion", MOVED)
def test_entries_on_a_refitted_structure_equal_the_brute_force_of_the_moved_triangles(name, motion, accels):
    tris, o, d, tag, rec = _moved_case(name, motion)
    accel = accels(name)
    accel.refit(_dev(tris))
    fresh = abi.Accel(tris)
    attribs = _attributes(len(tris))
    textures = _textures()[0]
    for tmin, tmax in ((0.0, 1.0), (0.25, 0.75)):
        what = f"{name} x {motion}, t in [{tmin}, {tmax}]"
        with np.errstate(all="ignore"):
            want = closest.brute_force_closest(o, d, tmin, tmax, rec)
            want_any = gref.brute_force_any_hit(o, d, tmin, tmax, rec)
        hits = want["index"] != MISS
        assert np.array_equal(hits, want_any), "the two brute forces disagree"
        print(f"[accel refit gpu] {what}: {len(o)} rays, {int(hits.sum())} hits")
        assert hits.sum() > 100 and (~hits).sum() > 100
        got_any, query = _both(accel, o, d, tmin, tmax)
        _compare_any(name, what, got_any, query, want_any, tag)
        got, occluded = _run(accel, o, d, tmin, tmax)
        _compare_closest(name, what, got, occluded, want, tag)
        fresh_any, fresh_query = _both(fresh, o, d, tmin, tmax)
        fresh_got, _ = _run(fresh, o, d, tmin, tmax)
        assert np.array_equal(fresh_any, got_any) and np.array_equal(fresh_query, query) and fresh_got.tobytes() == got.tobytes(), \
            "a structure created from the moved triangles answers differently"
        if tmin != 0.0:
            continue
        want_cut = cutref.brute_force_closest_cutout(_arith(), o, d, tmin, tmax, rec, attribs, textures, 0, 0)
        want_cut_any = cutref.brute_force_any_hit_cutout(_arith(), o, d, tmin, tmax, rec, attribs, textures, 0, 0)
        got_cut, got_cut_any = _run_cutout(tris, attribs, o, d, tmin, tmax, 0, 0, accel=accel)
        _same_bits(got_cut, want_cut, what + ", cutouts")
        assert np.array_equal(got_cut_any, want_cut_any)
        fresh_cut, fresh_cut_any = _run_cutout(tris, attribs, o, d, tmin, tmax, 0, 0, accel=fresh)
        assert fresh_cut.tobytes() == got_cut.tobytes() and np.array_equal(fresh_cut_any, got_cut_any)
    fresh.close()


def test_two_refits_back_to_back_with_a_query_between_them(accels):
    """refit to pose A, query, refit to pose B, nothing synchronised in between: the answers are pose A's, the bytes pose B's"""
    import torch

    accel = accels("procedural")
    a_tris, o, d, tag, rec = _moved_case("procedural", "jitter")
    b_tris = ref.poses("procedural", "cluster_swap")[0]
    n = len(o)
    stream = torch.cuda.current_stream().cuda_stream
    va, vb = _dev(a_tris), _dev(b_tris)
    to, td = _dev(o), _dev(d)
    out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    occ = torch.zeros((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    accel.refit(va, stream)
    accel.closest(to, td, 0.0, 1.0, out, stream)
    accel.occluded(to, td, 0.0, 1.0, occ, stream)
    accel.refit(vb, stream)
    got_nodes, got_recs = ref.view(*accel.download(stream))
    with np.errstate(all="ignore"):
        want = closest.brute_force_closest(o, d, 0.0, 1.0, rec)
    got = out.cpu().numpy().view(np.uint32).view(closest.HIT_DTYPE).reshape(n)
    _same_bits(got, want, "between the refits: pose A")
    assert np.array_equal(occ.cpu().numpy().astype(bool), want["index"] != MISS)
    with np.errstate(all="ignore"):
        other = closest.brute_force_closest(o, d, 0.0, 1.0, cs.host_records(b_tris))
    assert (other.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)).any(axis=1).sum() > 100, "the two poses answer differently"
    nodes, recs = _host(*ref.built("procedural"), b_tris)
    assert got_nodes.tobytes() == nodes.tobytes() and got_recs.tobytes() == recs.tobytes()


# ---- vkr_scene_triangles ------------------------------------------------------------------------------------------------------------
def _device_triangles(sc):
    rs, keep = sc.upload(device="cuda")
    n = sum(d["index_count"] // 3 for d in sc.draws)
    return abi.scene_world_triangles(rs, n).cpu().numpy()


@pytest.mark.parametrize("cutout", [False, True])
def test_scene_triangles_equals_abi_scene_triangles(cutout):
    sc = scn.procedural_scene(detail=3, cutout=cutout)
    want = np.asarray(abi.scene_triangles(sc), F32)
    got = _device_triangles(sc)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


def test_scene_triangles_with_an_index_outside_the_vertex_buffer():
    sc = scn.procedural_scene(detail=3)
    want = np.asarray(abi.scene_triangles(sc), F32)
    bad, d = 7, sc.draws[2]
    sc.indices = sc.indices.copy()
    sc.indices[d["index_offset"] + 3 * bad + 1] = len(sc.vertices)  # with vertex_offset on top: outside the buffer
    got = _device_triangles(sc)
    base = np.cumsum([0] + [x["index_count"] // 3 for x in sc.draws])
    at = [int(base[k]) + bad for k, x in enumerate(sc.draws) if x["index_offset"] == d["index_offset"]]  # the spheres share the mesh
    assert len(at) == 3 and np.isnan(got[at]).all()
    keep = ~np.isin(np.arange(len(want)), at)
    assert got[keep].tobytes() == want[keep].tobytes()
    draws = [dict(transform=x["transform"], index_offset=x["index_offset"], index_count=x["index_count"], vertex_offset=x["vertex_offset"]) for x in sc.draws]
    twin = ref.scene_triangles_twin(sc.vertices, sc.indices, [m for m, _ in sc.transforms], draws)
    assert np.array_equal(np.isnan(got), np.isnan(twin)) and np.array_equal(got[~np.isnan(got)].view(np.uint32), twin[~np.isnan(twin)].view(np.uint32))
    # a structure refitted to it: the bad triangle is hit by nothing, every other one as before
    accel = abi.Accel(want)
    accel.refit(_dev(got))
    nodes, recs = ref.view(*accel.download())
    host_nodes, host_recs = _host(*ref.view(*abi.accel_layout(want)), got)
    assert ref.same_bytes(nodes, host_nodes) and ref.same_bytes(recs, host_recs)
    accel.close()


def test_scene_triangles_of_a_scene_of_many_draws():
    """more draws than one chunk of the draw table holds (32), some of them empty"""
    sc = scn.procedural_scene(detail=3)
    base = list(sc.draws)
    rng = np.random.default_rng(5)
    for k in range(70):
        d = dict(base[int(rng.integers(0, len(base)))])
        if k % 9 == 4:
            d["index_count"] = 2  # no whole triangle
        sc.draws.append(d)
    want = np.asarray(abi.scene_triangles(sc), F32)
    got = _device_triangles(sc)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


# ---- the frame ----------------------------------------------------------------------------------------------------------------------
FW, FH = 64, 48
FRAME_LIGHTS = [(0.5, 2.5, 8.0, 1.0), (-1.85867, 5.81832, -0.247114, 1.0), (0.2, 1.5, 4.0, 0.0)]
FRAME_RADII = [0.5, 0.25, 0.0]


def _models(sc):
    return [np.array(sc.transforms[d["transform"]][0], F32) for d in sc.draws]


def _pose2(sc):
    """the model matrix of every draw with the three spheres (draws 2, 3, 4) moved; one also rotated, one also scaled"""
    models = _models(sc)

    def trs(t, s=1.0, rot_y=0.0):
        c, sn = np.cos(rot_y), np.sin(rot_y)
        return np.array([[c * s, 0, sn * s, t[0]], [0, s, 0, t[1]], [-sn * s, 0, c * s, t[2]], [0, 0, 0, 1]], np.float64)

    models[2] = (trs((0.9, 0.4, -0.6), rot_y=1.2) @ models[2].astype(np.float64)).astype(F32)
    models[3] = (trs((-0.8, 0.5, 1.1), s=1.5) @ models[3].astype(np.float64)).astype(F32)
    models[4] = (trs((-1.1, -0.3, -1.4)) @ models[4].astype(np.float64)).astype(F32)
    return models


def _scene_at(models):
    """procedural_scene(detail=3, cutout=True) with one transform per draw"""
    sc = scn.procedural_scene(detail=3, cutout=True)
    sc.transforms = []
    for d, m in zip(sc.draws, models):
        d["transform"] = sc.add_transform(m)
    return sc


def _render(sc, move_to=None):
    """one frame at FW x FH: loads sc, optionally moves its draws, runs raster + shadow map + the traced stages -> {image: bytes}"""
    import torch
    from vk_renderer_amd import host
    from vk_renderer_amd.camera import FrameSetup

    frame = host.HostFrame(FrameSetup(FW, FH), device="cuda")
    out = {}
    try:
        frame.load_scene(sc)
        if move_to is not None:
            frame.set_draw_transforms(move_to)
        frame.run(host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH)
        frame.set_shadow_rays(FRAME_LIGHTS)
        frame.set_ray_cutouts(True, alpha_lod=0)
        frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE | host.STAGE_SHADOW)
        torch.cuda.synchronize()
        for name in ("depth", "normal", "albedo", "material", "velocity"):
            out[name] = frame.download(name).host.tobytes()
        out["shadows"] = frame.download("shadows", 0).host.tobytes()
        frame.run(host.STAGE_SHADOW_MASK_RT)
        torch.cuda.synchronize()
        assert frame.last_tasks() == ["ShadowMaskRT"], frame.last_tasks()
        out["shadow_mask hard"] = frame.download("shadow_mask").host.tobytes()
        frame.set_shadow_area_lights(FRAME_RADII, 16, 4)
        frame.run(host.STAGE_SHADOW_MASK_RT)
        torch.cuda.synchronize()
        assert frame.last_tasks() == ["ShadowMaskRTSoft"], frame.last_tasks()
        out["shadow_mask soft"] = frame.download("shadow_mask").host.tobytes()
        frame.run(host.STAGE_REFLECTIONS_RT)
        torch.cuda.synchronize()
        out["reflections"], out["blurred"] = frame.download("reflections").host.tobytes(), frame.download("blurred").host.tobytes()
        frame.run(host.STAGE_GTAO_RT)
        torch.cuda.synchronize()
        for name in ("raw", "acc_ao"):
            out[name] = frame.download(name).host.tobytes()
    finally:
        frame.close()
    return out


def test_a_moved_frame_equals_a_frame_loaded_in_that_pose():
    sc = scn.procedural_scene(detail=3, cutout=True)
    pose2 = _pose2(sc)
    moved = _render(sc, move_to=pose2)       # frame A: loaded at pose 1, moved to pose 2, the structure refitted
    loaded = _render(_scene_at(pose2))       # frame B: loaded at pose 2, the structure built there
    assert sorted(moved) == sorted(loaded)
    differing = [name for name in moved if moved[name] != loaded[name]]
    assert not differing, f"images differ between the moved and the loaded frame: {differing}"
    # the move is seen: pose 1 renders differently, in the raster and in every traced image
    still = _render(_scene_at(_models(sc)))
    assert still == _render(sc, move_to=_models(sc)), "moving to the pose it is in changes a frame"
    for name in ("depth", "albedo", "shadows", "shadow_mask hard", "shadow_mask soft", "reflections", "raw"):
        assert still[name] != moved[name], f"{name} does not see the move"


def test_set_draw_transforms_refusals():
    from vk_renderer_amd import host
    from vk_renderer_amd.camera import FrameSetup

    sc = scn.procedural_scene(detail=3)
    frame = host.HostFrame(FrameSetup(FW, FH), device="cuda")
    try:
        with pytest.raises(RuntimeError, match=r"vkrh_set_draw_transforms: without a loaded scene \(vkrh_load_scene\)"):
            frame.set_draw_transforms(_models(sc))
        frame.load_scene(sc)
        with pytest.raises(RuntimeError, match=r"vkrh_set_draw_transforms: 4 transforms for the 5 draws of vkrh_load_scene"):
            frame.set_draw_transforms(_models(sc)[:4])
        with pytest.raises(RuntimeError, match="vkrh_set_draw_transforms: 0 transforms"):
            frame.set_draw_transforms([])
        frame.set_draw_transforms(_models(sc))
    finally:
        frame.close()
    tiled = host.HostFrame(FrameSetup(FW, FH), device="cuda", tiled=True)
    try:
        with pytest.raises(RuntimeError, match=r"vkrh_set_draw_transforms: on a tiled frame \(the ray-traced stages run on one GPU\)"):
            tiled.set_draw_transforms(_models(sc))
    finally:
        tiled.close()
