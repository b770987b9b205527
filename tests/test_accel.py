"""The scene's acceleration structure and the ray-query AO pass without a GPU: vkr_accel_layout's hierarchy (every triangle
in exactly one leaf, boxes nested, records as DESIGN_NUMERICS.md defines them, the same bytes on every build), GTAO's 64
random directions against an independent reproduction, the host mirror's ray-query gate, and the new ABI entries."""
import ctypes as C
import os

import numpy as np
import pytest

from vk_renderer_amd import abi
from vk_renderer_amd import scene as scn

import gtao_rt_reference as ref

NODE = np.dtype([("lo", "<f4", 3), ("first", "<u4"), ("hi", "<f4", 3), ("count", "<u4")])
TRI = np.dtype([("v0", "<f4", 3), ("index", "<u4"), ("e1", "<f4", 3), ("e2", "<f4", 3), ("lo", "<f4", 3), ("hi", "<f4", 3)])


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(abi.PRODUCT_LIB):
        pytest.skip("HIP library not built yet (run __graft_entry__.build())")
    return abi.product()


def _planes():
    """axis-aligned planes: 2 x 200 triangles in z = 0, 100 in x = 3 (zero thickness before the margin), stacked copies"""
    rng = np.random.default_rng(5)
    out = []
    for axis, c, n in ((2, 0.0, 200), (2, 0.0, 200), (0, 3.0, 100)):
        p = rng.uniform(-4, 4, size=(n, 3, 3)).astype(np.float32)
        p[:, :, axis] = c
        out.append(p)
    return np.concatenate(out)


def _degenerate():
    """zero-area triangles: repeated vertices, collinear vertices, a point, mixed with ordinary ones"""
    rng = np.random.default_rng(9)
    a = rng.uniform(-1, 1, size=(40, 3)).astype(np.float32)
    b = rng.uniform(-1, 1, size=(40, 3)).astype(np.float32)
    tris = [np.stack([a, a, b], 1), np.stack([a, b, (a + b) * np.float32(0.5)], 1), np.stack([a, a, a], 1),
            rng.uniform(-1, 1, size=(40, 3, 3)).astype(np.float32)]
    return np.concatenate(tris)


CASES = {
    "procedural": lambda: abi.scene_triangles(scn.procedural_scene(detail=12)),
    "degenerate": _degenerate,
    "planes": _planes,
    "single": lambda: np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32),
}


def _layout(tris):
    nodes, recs = abi.accel_layout(tris)
    return nodes.view(NODE).reshape(-1), recs.view(TRI).reshape(-1)


@pytest.mark.parametrize("case", sorted(CASES))
def test_layout_hierarchy(lib, case):
    tris = CASES[case]()
    n = len(tris)
    nodes, recs = _layout(tris)
    assert 1 <= len(nodes) <= max(1, 2 * n - 1)
    assert len(recs) == n
    # records: what the frozen test reads, computed as DESIGN_NUMERICS.md states it
    want = ref.triangle_records(tris)
    idx = recs["index"].astype(np.int64)
    assert sorted(idx.tolist()) == list(range(n)), "every input triangle has exactly one record"
    for f in ("v0", "e1", "e2", "lo", "hi"):
        assert np.array_equal(recs[f].view(np.uint32), want[f][idx].view(np.uint32)), f
    # walk from the root: every node reached once, every record in exactly one leaf, boxes nested
    covered = np.zeros(n, dtype=np.int64)
    seen = np.zeros(len(nodes), dtype=np.int64)
    stack = [(0, 0)]
    max_depth = 0
    while stack:
        i, depth = stack.pop()
        seen[i] += 1
        max_depth = max(max_depth, depth)
        nd = nodes[i]
        if nd["count"] == 0:
            for c in (nd["first"], nd["first"] + 1):
                ch = nodes[c]
                assert np.all(ch["lo"] >= nd["lo"]) and np.all(ch["hi"] <= nd["hi"]), f"child {c} leaves parent {i}"
                stack.append((int(c), depth + 1))
        else:
            r = recs[nd["first"]:nd["first"] + nd["count"]]
            assert len(r) == nd["count"]
            covered[nd["first"]:nd["first"] + nd["count"]] += 1
            assert np.all(r["lo"] >= nd["lo"]) and np.all(r["hi"] <= nd["hi"]), f"leaf {i} does not contain its triangles"
            v = np.stack([r["v0"], r["v0"] + r["e1"], r["v0"] + r["e2"]], 1)
            assert np.all(v >= nd["lo"][None, None]) and np.all(v <= nd["hi"][None, None])
    assert np.all(seen == 1), "a node is unreachable or shared"
    assert np.all(covered == 1), "a triangle is in no leaf or in two"
    assert max_depth <= 48
    # the same input gives the same bytes
    nodes2, recs2 = _layout(tris)
    assert nodes.tobytes() == nodes2.tobytes() and recs.tobytes() == recs2.tobytes()


def test_layout_of_nothing(lib):
    nodes, recs = abi.accel_layout(np.zeros((0, 3, 3), np.float32))
    assert len(nodes) == 0 and len(recs) == 0


def test_layout_rejects_small_arrays(lib):
    tris = CASES["procedural"]()
    n = len(tris)
    nodes = (abi.AccelNode * 1)()
    recs = (abi.AccelTri * n)()
    count = C.c_uint32(0)
    rc = lib.vkr_accel_layout(np.ascontiguousarray(tris).ctypes.data, n, nodes, 1, recs, C.byref(count))
    assert rc != 0 and b"do not fit" in lib.vkr_last_error()


def test_random_directions_match_an_independent_reproduction():
    from vk_renderer_amd import host

    if not os.path.exists(abi.HOST_LIB):
        pytest.skip("host library not built yet")
    got = np.zeros((64, 4), np.float32)
    assert host.lib().vkrh_gtao_directions(got.ctypes.data, 64) == 0
    want = ref.random_directions(64)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(want[:, 2] >= 0) and np.allclose(np.linalg.norm(want[:, :3], axis=1), 1.0, atol=1e-6)


def test_host_mirror_ray_query_gate():
    """GTAO(..., use_ray_query = true) constructs on a graph whose device has ray query and keeps refusing on a default graph;
    add_main_rt_pass names what is missing.  Runs on the CPU with a malloc-backed allocator, like test_host_mirror.py."""
    from vk_renderer_amd import host

    if not os.path.exists(abi.HOST_LIB):
        pytest.skip("host library not built yet")
    l = host.lib()
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    alloc = host._ALLOC(lambda n, u: libc.malloc(n))
    free = host._FREE(lambda p, u: libc.free(p))
    l.vkrh_set_allocator(alloc, free, None)
    try:
        buf = C.create_string_buffer(8192)
        assert l.vkrh_selftest_ray_query(buf, 8192) == 0
    finally:
        l.vkrh_set_allocator(host._ALLOC(0), host._FREE(0), None)
    report = dict(line.split(": ", 1) for line in buf.value.decode().splitlines())
    assert "ray-query" in report["default_graph"]
    assert report["ray_query_graph"] == "no error"
    assert report["device_config"] == "no error"
    assert "null acceleration structure" in report["null_tlas"]
    assert "without use_ray_query" in report["rt_pass_without_ray_query"]
    assert "null acceleration structure" in report["null_accel_binding"]


def test_abi_structs_and_exports(lib):
    assert C.sizeof(abi.AccelNode) == 32
    assert C.sizeof(abi.AccelTri) == 64
    assert C.sizeof(abi.GtaoRtParams) == 80
    assert C.sizeof(abi.GtaoRtPush) == 4
    for sym in ("vkr_accel_layout", "vkr_accel_create", "vkr_accel_destroy", "vkr_accel_info", "vkr_accel_query", "vkr_gtao_rt_main"):
        assert hasattr(lib, sym)
    txt = open(os.path.join(abi.ROOT, "include", "vkr_postfx.h")).read()
    for sym in ("vkr_accel_layout", "vkr_accel_query", "vkr_gtao_rt_main"):
        assert sym + "(" in txt
    frame_h = open(os.path.join(abi.ROOT, "vk-renderer_amd", "host", "frame.hpp")).read()
    from vk_renderer_amd import host

    assert "VKRH_STAGE_GTAO_RT            = 1u << 21" in frame_h and host.STAGE_GTAO_RT == 1 << 21


def test_program_table_knows_gtao_rt_main():
    from vk_renderer_amd import host

    if not os.path.exists(abi.HOST_LIB):
        pytest.skip("host library not built yet")
    assert host.lib().vkrh_has_program(b"gtao_rt_main") == 1


def test_entry_argument_checks(lib):
    """null handles and arguments are refused with a message before anything is launched"""
    rc = lib.vkr_accel_query(None, None, None, 0.0, 1.0, 16, None, None)
    assert rc != 0 and b"NULL acceleration structure" in lib.vkr_last_error()
    p, push = abi.GtaoRtParams(), abi.GtaoRtPush()
    rc = lib.vkr_gtao_rt_main(C.byref(p), None, None, None, None, None, C.byref(push), None)
    assert rc != 0 and b"acceleration structure" in lib.vkr_last_error()
    rc = lib.vkr_accel_info(None, None, None)
    assert rc != 0
