"""The backbuffer texdraw pass without a GPU: the C-ABI push block and enum, the refusals of vkr_texdraw (all of them return
before any launch), the program table and the stage value, what the host mirror records (vkrh_selftest_texdraw), and the numpy
restatement (tests/texdraw_reference.py): the flag precedence on a hand-made image, an up-scale worked out by hand, the
non-zero fractions at equal extents, and the estimate behind the kernel's sRGB encode (float_to_srgb8_fast of vkr_device.hpp)."""
import ctypes as C
import re

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd.images import ImageBuf

import texdraw_reference as ref
import transfer_reference as tr

F32 = np.float32


def test_push_layout_enum_and_entry():
    assert C.sizeof(abi.TexdrawPush) == 4 and abi.TexdrawPush.flags.offset == 0
    assert (abi.TEXDRAW_SHOW_ALL, abi.TEXDRAW_SHOW_R, abi.TEXDRAW_SHOW_G, abi.TEXDRAW_SHOW_B, abi.TEXDRAW_SHOW_A) == (0, 1, 2, 4, 8)
    assert (ref.SHOW_ALL, ref.SHOW_R, ref.SHOW_G, ref.SHOW_B, ref.SHOW_A) == (0, 1, 2, 4, 8)
    txt = open(abi.ROOT + "/include/vkr_postfx.h").read()
    assert "int vkr_texdraw(const vkr_img* target_tex, const vkr_img* backbuffer, const vkr_texdraw_push* push, void* stream);" in txt
    assert "typedef struct vkr_texdraw_push { uint32_t flags; } vkr_texdraw_push;" in txt
    enum = re.search(r"enum \{ VKR_TEXDRAW_SHOW_ALL = (\d+), VKR_TEXDRAW_SHOW_R = (\d+), VKR_TEXDRAW_SHOW_G = (\d+), VKR_TEXDRAW_SHOW_B = (\d+), "
                     r"VKR_TEXDRAW_SHOW_A = (\d+) \};", txt)
    assert enum and [int(v) for v in enum.groups()] == [0, 1, 2, 4, 8]
    assert "int vkr_selftest_srgb_encode(uint32_t* device_counter, void* stream);" in txt
    assert hasattr(abi.product(), "vkr_texdraw") and hasattr(abi.product(), "vkr_selftest_srgb_encode")
    gpu_cpp = open(abi.ROOT + "/vk-renderer_amd/host/gpu/gpu.cpp").read()
    assert "static_assert(sizeof(vkr_texdraw_push) == 4" in gpu_cpp


def test_program_and_stage_are_registered():
    assert host.lib().vkrh_has_program(b"texdraw") == 1
    assert host.STAGE_BACKBUFFER == 1 << 27
    assert not host.STAGE_CHAIN & host.STAGE_BACKBUFFER
    hpp = open(abi.ROOT + "/vk-renderer_amd/host/frame.hpp").read()
    assert re.search(r"VKRH_STAGE_BACKBUFFER\s*= 1u << 27,", hpp)
    assert "int vkrh_set_backbuffer(void* frame, const char* source_image, uint32_t flags, uint32_t width, uint32_t height);" in hpp


# ---- refusals: host memory stands in for device memory, because every case returns before any launch ---------------------------
def _edited(img, **fields):
    d = img.desc()
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def test_refusals_return_before_any_launch():
    lib = abi.product()
    W, H = 16, 8
    src = ImageBuf(abi.FMT_RGBA16_SFLOAT, W, H)
    dst = ImageBuf(abi.FMT_RGBA8_SRGB, W, H, fill=0xA5)
    depth = ImageBuf(abi.FMT_D24_UNORM_S8, W, H)
    wrong_dst = ImageBuf(abi.FMT_RGBA16_SFLOAT, W, H)
    r8_dst = ImageBuf(abi.FMT_R8_UNORM, W, H)
    window_src = ImageBuf(abi.FMT_RGBA16_SFLOAT, W, H // 2, full=(W, H), origin=(0, 2))
    window_dst = ImageBuf(abi.FMT_RGBA8_SRGB, W, H // 2, full=(W, H), origin=(0, 0))
    same = ImageBuf(abi.FMT_RGBA8_UNORM, W, H)
    push = abi.texdraw_push(abi.TEXDRAW_SHOW_ALL)
    good_s, good_d = src.desc(), dst.desc()
    cases = {
        "target_tex NULL": (None, good_d, push, "target_tex is NULL"),
        "backbuffer NULL": (good_s, None, push, "backbuffer is NULL"),
        "push NULL": (good_s, good_d, None, "push is NULL"),
        "source without memory": (_edited(src, base=None), good_d, push, "texdraw.target_tex: NULL image"),
        "backbuffer without memory": (good_s, _edited(dst, base=None), push, "texdraw.backbuffer: NULL image"),
        "depth source": (depth.desc(), good_d, push, "D24_UNORM_S8 is not a colour format"),
        "unknown source format": (_edited(src, format=13), good_d, push, "unknown format 13"),
        "undefined source format": (_edited(src, format=0), good_d, push, "unknown format 0"),
        "fp16 backbuffer": (good_s, wrong_dst.desc(), push, "texdraw.backbuffer: format 7, expected RGBA8_SRGB"),
        "r8 backbuffer": (good_s, r8_dst.desc(), push, "texdraw.backbuffer: format 10, expected RGBA8_SRGB"),
        "depth backbuffer": (good_s, depth.desc(), push, "texdraw.backbuffer: format 1, expected RGBA8_SRGB"),
        "zero source extent": (_edited(src, width=0, full_width=0), good_d, push, "texdraw.target_tex: zero extent"),
        "zero backbuffer extent": (good_s, _edited(dst, height=0, full_height=0), push, "texdraw.backbuffer: zero extent"),
        "backbuffer too wide": (good_s, _edited(dst, width=65536, full_width=65536, pitch_bytes=(C.c_uint32 * 16)(*([65536 * 4] * 16))), push,
                                "at most 65535 texels a side"),
        "windowed source": (window_src.desc(), good_d, push, "target_tex: windows are not supported"),
        "windowed backbuffer": (good_s, window_dst.desc(), push, "backbuffer: windows are not supported"),
        "the same image": (same.desc(), same.desc(), push, "target_tex and backbuffer are the same memory"),
    }
    for name, (s, d, p, message) in cases.items():
        rc = lib.vkr_texdraw(C.byref(s) if s is not None else None, C.byref(d) if d is not None else None, C.byref(p) if p is not None else None, None)
        assert rc != 0, name
        assert message in lib.vkr_last_error().decode(), (name, lib.vkr_last_error().decode())
        with pytest.raises(RuntimeError, match=re.escape(message)):
            abi.check(rc, lib)
    assert (dst.to_host() == 0xA5).all() and not same.to_host().any()  # nothing ran


# ---- the host mirror --------------------------------------------------------------------------------------------------------
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
    """{first word of the line: rest of the line}"""
    l = host.lib()
    keep = _malloc_allocator(l)
    try:
        buf = C.create_string_buffer(8192)
        assert l.vkrh_selftest_texdraw(buf, 8192) == 0, l.vkrh_last_error().decode()
    finally:
        l.vkrh_set_allocator(host._ALLOC(0), host._FREE(0), None)
    del keep
    return dict(line.split(":", 1) for line in buf.value.decode().splitlines())


def test_mirror_records_the_references_tasks(selftest):
    """backbuffer_subpass2.cpp:22-29: task "BackbufSubpass" samples mip 0 of the source (one level of its three) and renders into
    the backbuffer; :95-104: task "presentPrepare" follows and only hands the backbuffer over.  The backbuffer is the graph's
    RGBA8_SRGB image (VK_FORMAT_R8G8B8A8_SRGB = 43) at the extent the graph was given."""
    words = selftest["images"].split()
    source, backbuffer = int(words[1]), int(words[3])
    assert source != backbuffer
    assert selftest["BackbufSubpass"].split() == [f"W{backbuffer}.0", f"R{source}.0"], selftest  # declared in the reference's order
    assert selftest["presentPrepare"].split() == [f"R{backbuffer}.0"], selftest
    assert list(selftest) == ["images", "backbuffer", "BackbufSubpass", "presentPrepare", "program", "push 4"], selftest
    assert selftest["backbuffer"].split() == ["64x36", "format", "43"]
    assert selftest["program"].split() == ["texdraw", "1"]


def test_push_constants_are_the_flags(selftest):
    assert selftest["push 4"].split() == [str(abi.TEXDRAW_SHOW_R)]


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def _contract():
    return int(abi.product().vkr_numeric_contract())


# four texels whose channels are all different codes, so that a wrong channel or a wrong texel shows
HAND_2X2 = np.array([[[10, 60, 110, 160], [20, 70, 120, 170]], [[30, 80, 130, 180], [40, 90, 140, 190]]], np.uint8)


@pytest.mark.parametrize("flags", [0, 1, 2, 4, 8, 3, 6, 12, 15, 16])
def test_flag_precedence(flags):
    """2 x 2 -> 2 x 2 RGBA8_UNORM: uv = 0.25, 0.75, texel coordinates 0 and 1 exactly, fractions 0: the image itself, all four
    channels or the shown one in all four.  The last set bit wins: 3 shows G, 6 B, 12 and 15 A; 16 is no bit of the shader's."""
    assert ref.nonzero_fractions(2, 2, 2, 2, _contract())[0] == 0
    out = ref.texdraw(HAND_2X2, tr.FMT_RGBA8_UNORM, 2, 2, tr.FMT_RGBA8_UNORM, flags, _contract())
    shown = {0: None, 1: 0, 2: 1, 4: 2, 8: 3, 3: 1, 6: 2, 12: 3, 15: 3, 16: None}[flags]
    assert ref.shown_channel(flags) == shown
    want = HAND_2X2 if shown is None else np.repeat(HAND_2X2[..., shown:shown + 1], 4, axis=-1)
    assert np.array_equal(out, want), (flags, out, want)


def test_upscale_of_a_two_texel_row_by_hand():
    """R32_SFLOAT (0, 1) -> 4 x 1 RGBA8_UNORM.  uv = 1/8, 3/8, 5/8, 7/8; x = 2 uv - 1/2 = -1/4, 1/4, 3/4, 5/4 (all exact); floors
    -1, 0, 0, 1, fractions 3/4, 1/4, 3/4, 1/4; taps (0, 0), (0, 1), (0, 1), (1, 1): r = 0, 1/4, 3/4, 1 -> rint(255 r) = 0, 64
    (63.75), 191 (191.25), 255.  g = b = 0, alpha 1 -> 255.  One row: y = -0 + ... = 0, fraction 0, both rows the same."""
    src = np.array([[[0.0], [1.0]]], F32)
    out = ref.texdraw(src, tr.FMT_R32_SFLOAT, 4, 1, tr.FMT_RGBA8_UNORM, 0, _contract())
    assert out.tolist() == [[[0, 0, 0, 255], [64, 0, 0, 255], [191, 0, 0, 255], [255, 0, 0, 255]]]
    # into sRGB: the codes of 1/4 and 3/4 by the threshold rule are 137 and 225 (255 * OETF = 137.0, 224.9), alpha stays linear
    srgb = ref.texdraw(src, tr.FMT_R32_SFLOAT, 4, 1, tr.FMT_RGBA8_SRGB, 0, _contract())
    assert srgb[0, :, 0].tolist() == [0, 137, 225, 255] and (srgb[0, :, 3] == 255).all()
    # ShowR puts r into alpha as well, stored linearly
    shown = ref.texdraw(src, tr.FMT_R32_SFLOAT, 4, 1, tr.FMT_RGBA8_SRGB, ref.SHOW_R, _contract())
    assert shown[0].tolist() == [[0, 0, 0, 0], [137, 137, 137, 64], [225, 225, 225, 191], [255, 255, 255, 255]]


def test_equal_extents_are_no_identity_of_coordinates():
    """cfma((g + 0.5) / W, W, -0.5) is not g for every g and W: 3910 of the 35 500 pixel centres of 250 x 142 have a non-zero
    fraction on an axis (a coordinate just below g floors to g - 1 with a fraction just below 1), so no single-tap shortcut
    exists at equal extents.  The counts are those DESIGN.md 7.6 records."""
    report = ref.fraction_report(_contract())
    print("\n".join("[texdraw] " + line for line in report))
    if _contract() >= 2:
        assert ref.nonzero_fractions(250, 142, 250, 142, 2) == (3910, 7, 12)
        assert ref.nonzero_fractions(64, 36, 64, 36, 2) == (64, 0, 1)
        assert ref.nonzero_fractions(3840, 2160, 3840, 2160, 2)[0] == 543862
    n, nx, ny = ref.nonzero_fractions(250, 142, 250, 142, _contract())
    assert n > 0
    # and such a pixel still resolves to its own texel within the fraction's distance from 1: the image is not shifted
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (142, 250, 4), dtype=np.uint8)
    out = ref.texdraw(src, tr.FMT_RGBA8_UNORM, 250, 142, tr.FMT_RGBA8_UNORM, 0, _contract())
    assert np.abs(out.astype(int) - src.astype(int)).max() <= 1


def test_fast_encode_estimate_stays_inside_its_margin():
    """float_to_srgb8_fast needs |est - 255 * OETF(x)| < 0.5 (minus the < 1e-5 a threshold moves when it is rounded to fp32) to
    be the code or one less.  The formula in fp32 with numpy's log2 / exp2 (within an ulp, like v_log_f32 / v_exp_f32) on every
    threshold, its two neighbours and 2 000 000 points spread over the exponents of [2^-20, 2] stays within 0.01, fifty times
    inside; and floor(clamp(est, 0, 254)) + (thresh[e + 1] <= x) is the threshold rule's code on all of them.  The proof over
    all 2^32 bit patterns runs on the device (vkr_selftest_srgb_encode, tests/test_texdraw_gpu.py)."""
    thr = tr.SRGB_THRESH[1:]
    rng = np.random.default_rng(11)
    spread = (rng.uniform(1.0, 2.0, 2_000_000) * np.exp2(rng.integers(-20, 1, 2_000_000))).astype(F32)
    special = np.array([0.0, -0.0, -1.0, 1.0, 2.0, 1e30, np.inf, -np.inf, 1e-40, 0.0031308, 0.00313080495], F32)
    x = np.concatenate([thr, np.nextafter(thr, F32(-np.inf)), np.nextafter(thr, F32(np.inf)), spread, special]).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        curve = np.exp2(tr.fma32(np.log2(x), F32(1.0 / 2.4), F32(np.log2(269.025)))).astype(F32) - F32(14.025)
        est = np.where(x < F32(0.0031308), x * F32(3294.6), curve).astype(F32)
    xd = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        true = 255.0 * np.where(xd <= 0.0031308, 12.92 * xd, 1.055 * np.power(np.maximum(xd, 0.0), 1.0 / 2.4) - 0.055)
    inside = (x > 0) & (x <= 1)
    worst = np.abs(est[inside].astype(np.float64) - true[inside]).max()
    print(f"[texdraw] estimate of 255 * OETF: worst error {worst:.3g} of a code over {int(inside.sum())} points")
    assert worst < 0.01
    e = np.minimum(np.maximum(np.where(np.isnan(est), F32(0), est), F32(0)), F32(254)).astype(np.uint32)
    code = e + (tr.SRGB_THRESH[e + 1] <= x)
    assert np.array_equal(code, tr.float_to_srgb8(x))
