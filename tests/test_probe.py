"""CPU checks of the octahedral probe programs (no GPU): the C-ABI declarations, struct size and new format, the octahedral
helpers of tests/probe_reference.py and the frozen seamless cube rules (the resource guard of csrc/probe.hip is
tests/test_kernel_resources_probe.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from vk_renderer_amd import abi

import probe_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ENTRIES = ("vkr_cube2oct", "vkr_probe_downsample", "vkr_trace_probe")


def test_header_declares_probe_entries_and_format():
    txt = open(os.path.join(ROOT, "include", "vkr_postfx.h")).read()
    for name in ENTRIES:
        assert name + "(" in txt
    assert "VKR_FMT_R16_UNORM      = 12" in txt
    assert abi.FMT_R16_UNORM == 12 and abi.FORMAT_BYTES[12] == 2


def test_constants_struct_is_116_bytes():
    assert C.sizeof(abi.ProbeTraceConsts) == 116
    assert abi.ProbeTraceConsts.grid_size.offset == 64 + 32


def test_library_exports_probe_entries():
    if not os.path.exists(abi.PRODUCT_LIB):
        pytest.fail("HIP library not built (run __graft_entry__.build())")
    lib = abi.product()
    for name in ENTRIES:
        assert hasattr(lib, name)
    assert lib.vkr_format_bytes(abi.FMT_R16_UNORM) == 2


def test_refusals_before_any_launch():
    """argument checks run on the host and fail before anything is launched"""
    lib = abi.product()
    c = abi.ProbeTraceConsts()
    c.grid_size = 1
    img = abi.VkrImg()
    assert lib.vkr_trace_probe(C.byref(img), C.byref(img), C.byref(img), C.byref(img), 16, C.byref(c), C.byref(img), None) != 0
    assert b"grid_size" in lib.vkr_last_error()
    c.grid_size = 4
    assert lib.vkr_trace_probe(C.byref(img), C.byref(img), C.byref(img), C.byref(img), 15, C.byref(c), C.byref(img), None) != 0
    assert b"layers" in lib.vkr_last_error()
    assert lib.vkr_probe_downsample(None, None) != 0
    assert lib.vkr_cube2oct(None, None, None, None, None) != 0


def test_octahedral_round_trip():
    ar = ref.Arith(2)
    rng = np.random.default_rng(3)
    v = rng.normal(size=(20000, 3)).astype(F32)
    v = ref.normalize(ar, v)
    u, w = ref.oct_encode(ar, v)
    assert ((u >= 0) & (u <= 1) & (w >= 0) & (w <= 1)).all()
    back = ref.oct_decode(ar, u, w)
    assert np.abs(back - v).max() < 1e-5
    # oct_center is one of the 26 normalised sign vectors, and points into the same octant
    c = ref.oct_center(ar, u, w)
    assert np.allclose(np.linalg.norm(c, axis=-1), 1, atol=1e-6)
    assert ((np.sign(c) == np.sign(v)) | (np.sign(c) == 0)).all()


def test_oct_depth_round_trip():
    ar = ref.Arith(2)
    z = np.linspace(0.05, 80, 1001).astype(F32)
    d = ref.encode_oct_depth(z)
    assert abs(float(d[0])) < 1e-6 and abs(float(d[-1]) - 1) < 1e-6
    assert np.allclose(ref.decode_oct_depth(ar, d), z, rtol=2e-4)  # encode takes -z: decode returns the distance


def test_across_edge_is_consistent():
    """every texel just past an edge maps to an edge texel of another face, whose own neighbour across that edge is back
    on the first face (the seams are symmetric), for every face, edge and position"""
    n = 8
    for f in range(6):
        for k in range(n):
            for i, j in ((-1, k), (n, k), (k, -1), (k, n)):
                g, gi, gj = (int(x) for x in ref.across_edge(np.array(f), np.array(i), np.array(j), n))
                assert g != f and (gi in (0, n - 1) or gj in (0, n - 1))
                # step off the neighbour's texel across the same edge: direction away from face g's centre
                cands = [(gi - 1, gj), (gi + 1, gj), (gi, gj - 1), (gi, gj + 1)]
                back = {tuple(int(x) for x in ref.across_edge(np.array(g), np.array(a), np.array(b), n))
                        for a, b in cands if a in (-1, n) or b in (-1, n)}
                assert (f, min(max(i, 0), n - 1), min(max(j, 0), n - 1)) in back


def test_face_table_matches_calc_matrix():
    """cube2oct reads face f at the texel the reference renders it to: calc_matrix (probe_renderer.cpp:65-78) looks along
    fwd with up; with Vulkan's y-down framebuffer, screen right is cross(fwd, up) and screen down is up."""
    fwd_up = [((1, 0, 0), (0, -1, 0)), ((-1, 0, 0), (0, -1, 0)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (0, 0, -1)),
              ((0, 0, 1), (0, -1, 0)), ((0, 0, -1), (0, -1, 0))]
    for f, (fwd, up) in enumerate(fwd_up):
        right = np.cross(fwd, up)
        x, y, z = ref._face_dir(np.array(f), np.array(1), np.array(0), 1)
        assert np.array_equal([x, y, z], np.array(fwd) + right)  # sc = +1: screen right
        x, y, z = ref._face_dir(np.array(f), np.array(0), np.array(1), 1)
        assert np.array_equal([x, y, z], np.array(fwd) + np.array(up))  # tc = +1: screen down


def test_probe_downsample_restatement_reads_zero_past_the_edge():
    m0 = np.full((5, 5), 65535, np.uint16)
    mips = ref.probe_downsample(m0, 3)
    assert mips[1].shape == (2, 2) and mips[2].shape == (1, 1)
    assert (mips[1] == 65535).all()
