"""The SSAO pass without a GPU: the C-ABI block, the program table, what the host mirror records and how its two packings reach
the entry (vkrh_selftest_ssao), a known answer for the numpy restatement (tests/ssao_reference.py), and the properties of the
restatement's result on the synthetic depth that keep the GPU parity test (tests/test_ssao_gpu.py) from being vacuous."""
import ctypes as C

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PostFxChain

import ssao_reference as ref

F32 = np.float32


def test_block_layout():
    assert C.sizeof(abi.SsaoParams) == 336
    assert abi.SsaoParams.samples.offset == 80
    txt = open(abi.ROOT + "/include/vkr_postfx.h").read()
    assert "int vkr_ssao(" in txt and "vkr_ssao_params" in txt
    assert hasattr(abi.product(), "vkr_ssao")


def test_program_is_registered():
    assert host.lib().vkrh_has_program(b"ssao") == 1
    assert host.STAGE_SSAO == 1 << 25


def _malloc_allocator(l):
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    alloc = host._ALLOC(lambda n, u: libc.malloc(n))
    free = host._FREE(lambda p, u: libc.free(p))
    l.vkrh_set_allocator(alloc, free, None)
    return alloc, free


@pytest.fixture(scope="module")
def selftest():
    """(task lines, {block bytes: 84 floats})"""
    l = host.lib()
    keep = _malloc_allocator(l)
    try:
        buf = C.create_string_buffer(8192)
        assert l.vkrh_selftest_ssao(buf, 8192) == 0, l.vkrh_last_error().decode()
    finally:
        l.vkrh_set_allocator(host._ALLOC(0), host._FREE(0), None)
    del keep
    tasks, blocks = [], {}
    for line in buf.value.decode().splitlines():
        if line.startswith("packing "):
            head, nums = line.split(":")
            blocks[int(head.split()[1])] = np.array([float(v) for v in nums.split()], F32)
        else:
            tasks.append(line)
    return tasks, blocks


def test_mirror_records_the_references_task(selftest):
    """ssao.cpp:60-64: task "SSAO" samples depth mip 0 (image 0) and renders into the target (image 1); nothing else"""
    assert selftest[0] == ["SSAO: R0.0 W1.0"], selftest[0]


def test_reference_packing_reaches_the_entry_as_the_shader_reads_it(selftest):
    """pinned s[k] = (3k, 3k + 1, 3k + 2): the flat array is 0..47, so the shader's sample i is (4i, 4i + 1, 4i + 2) for
    i <= 11 with the next float in .w, and bytes the host never wrote are 0"""
    blocks = selftest[1]
    assert sorted(blocks) == [272, 336]
    b = blocks[272]
    assert b.shape == (84,)
    assert np.array_equal(b[:16].reshape(4, 4), np.eye(4, dtype=F32))
    assert np.array_equal(b[16:20], np.array([1.0, 1.5, 0.05, 80.0], F32))
    s = b[20:].reshape(16, 4)
    for i in range(12):
        assert tuple(s[i, :3]) == (4 * i, 4 * i + 1, 4 * i + 2), (i, s[i])
    for i in range(11):
        assert s[i, 3] == 4 * i + 3
    assert s[11, 3] == 47
    assert not s[12:].any()
    assert np.array_equal(s, ref.quirk_packed(np.arange(48, dtype=F32).reshape(16, 3)))


def test_std140_packing_gives_every_sample_its_slot(selftest):
    b = selftest[1][336]
    assert np.array_equal(b[:20], selftest[1][272][:20])
    s = b[20:].reshape(16, 4)
    assert np.array_equal(s[:, :3], np.arange(48, dtype=F32).reshape(16, 3))
    assert not s[:, 3].any()


def _contract():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


def constant_depth_case(w=64, h=36):
    """-> (depth words [h, w], setup, samples, expected code): a wall at view z = -2.  d(z) = f / (f - n) + f n / (z (f - n));
    a sample 0.05 v moves it by 0.05 |v.z| dd/dz = 0.05 * 0.05 * f n / (z^2 (f - n)) >= 3e-5 for |v.z| >= 0.05, far above the
    1e-7 of the compare, and clamp-to-edge makes every off-screen tap read the same constant: k = #{v.z > 0} everywhere."""
    setup = FrameSetup(w, h)
    n, f, z = 0.05, 80.0, -2.0
    d = f / (f - n) + f * n / (z * (f - n))
    code = int(np.rint(d * 16777215.0))
    samples = ref.fixed_samples(min_abs_z=0.05)
    k = int((samples[:, 2] > 0).sum())
    return np.full((h, w), code, np.uint32), setup, samples, ref.CODES[k]


def test_unorm8_tie_rounds_to_even():
    assert ref.CODES[8] == 128 and ref.CODES[0] == 0 and ref.CODES[16] == 255 and len(set(ref.CODES.tolist())) == 17


def test_known_answer_constant_depth():
    depth, setup, samples, want = constant_depth_case()
    codes, counts = ref.ssao(_contract(), depth, setup.proj, *setup.fazz, samples, 64, 36)
    assert 0 < want < 255
    assert (codes == want).all(), (want, np.unique(codes))


def test_restatement_on_the_synthetic_depth_is_not_trivial():
    W, H = 256, 144
    chain = PostFxChain(W, H, backend="oracle")
    chain.synth()
    depth = chain.depth.raw(0)[..., 0]
    stats = {}
    codes, counts = ref.ssao(_contract(), depth, chain.setup.proj, *chain.setup.fazz, ref.fixed_samples(), W, H, stats)
    ks, share = np.unique(counts, return_counts=True)
    figures = f"distinct k {len(ks)} ({ks.tolist()}), largest share {share.max() / counts.size:.3f}, off-screen taps {stats['offscreen_taps']} of {stats['taps']}"
    print("[ssao]", figures)
    assert np.isin(codes, ref.CODES).all(), figures
    assert np.array_equal(codes, ref.CODES[counts]), figures
    assert len(ks) >= 10, figures
    assert share.max() <= counts.size // 2, figures
    assert stats["offscreen_taps"] * 1000 >= stats["taps"], figures
