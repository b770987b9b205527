"""Area lights in the traced shadow mask without a GPU: the C-ABI block and the program table, every refusal that
vkr_shadow_mask_rt_soft, vkr_shadow_mask_rt_soft_cutout and vkrh_set_shadow_area_lights add to those of the hard pass (validation
never reaches a launch), the table of vkr_shadow_disk_samples against its formula, and the numpy restatement
(tests/shadow_mask_rt_soft_reference.py) alone: radius 0 and an all-zero table are the hard reference, the order of the samples
does not matter, the quantisation, and that the inputs of the GPU parity test have a penumbra under every light.

Measured here (oracle rasteriser, procedural scene at detail 8, the four lights of test_shadow_mask_rt_gpu.LIGHT_SETS[4], radius
0.5, S = 16, P = 4): at 64 x 36, 2024 geometry pixels, 39 / 55 / 86 / 45 of them strictly between 0 and 255 under lights 0-3, with
15 / 16 / 17 / 16 distinct codes; at 8 x 8, 3 / 5 / 5 / 1 strictly between.  The table of vkr_shadow_disk_samples equals numpy's after
rounding to fp32 for every (S, P) tried (no 1-ulp case occurred with this C library)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import LIGHT_POS, FrameSetup
from vk_renderer_amd.chain import PostFxChain

import shadow_mask_rt_reference as hard
import shadow_mask_rt_soft_reference as ref
from test_abi_errors import ERR_EXTENT, ERR_NULL, img
from test_shadow_mask_rt import _HostMemoryFrame

F32 = np.float32
D24 = abi.FMT_D24_UNORM_S8
RG16 = abi.FMT_RG16_UNORM
RGBA8 = abi.FMT_RGBA8_UNORM
SKY = 0xFFFFFF
# the lights of tests/test_shadow_mask_rt_gpu.py::LIGHT_SETS[4] (that module is a GPU suite; the values are restated)
LIGHTS4 = [tuple(LIGHT_POS) + (1.0,), (1.5, 4.5, -1.5, 0.0), (3.0, 4.0, 2.0, 1.0), (-6.0, 9.0, 3.0, 0.0)]
OFFSET, TMIN = abi.SHADOW_RT_NORMAL_OFFSET, abi.SHADOW_RT_TMIN


# ---- declarations -------------------------------------------------------------------------------------------------------------------
def test_block_layout_and_symbols():
    txt = open(abi.ROOT + "/include/vkr_postfx.h").read()
    body = re.search(r"typedef struct vkr_shadow_rt_soft \{(.*?)\} vkr_shadow_rt_soft;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert fields == ["float radius[4]", "uint32_t sample_count", "uint32_t pattern_side", "const float* samples", "uint32_t reserved[2]"]
    assert C.sizeof(abi.ShadowRtSoft) == 16 + 4 + 4 + 8 + 8 == 40
    offsets = {"radius": 0, "sample_count": 16, "pattern_side": 20, "samples": 24, "reserved": 32}
    for name, off in offsets.items():
        assert getattr(abi.ShadowRtSoft, name).offset == off, name
    lib = abi.product()
    for name in ("vkr_shadow_mask_rt_soft", "vkr_shadow_mask_rt_soft_cutout", "vkr_shadow_disk_samples"):
        assert re.search(r"\b(int|void)\s+" + name + r"\(", txt), name
        assert hasattr(lib, name), name
    assert "int vkrh_set_shadow_area_lights(void* frame, const float* radii, uint32_t count, uint32_t sample_count, uint32_t pattern_side);" in \
        open(abi.ROOT + "/vk-renderer_amd/host/frame.hpp").read()


def test_programs_and_setter_are_registered():
    for program in (b"shadow_mask_rt_soft", b"shadow_mask_rt_soft_cutout"):
        assert host.lib().vkrh_has_program(program) == 1, program
    assert hasattr(host.lib(), "vkrh_set_shadow_area_lights")
    assert hasattr(host.HostFrame, "set_shadow_area_lights")
    assert host.STAGE_SHADOW_MASK_RT == 1 << 29  # no new stage bit


# ---- the entries' new gates -----------------------------------------------------------------------------------------------------------
W, H = 64, 32
_TABLE = np.zeros(2 * 64 * 16, F32)  # host memory: a refusal never reads it


@functools.lru_cache(maxsize=None)
def _empty_accel():
    return abi.Accel(np.zeros((0, 3, 3), F32))


def _params(lights=((0.0, 4.0, 4.0, 1.0), (1.0, 2.0, 0.0, 0.0))):
    return abi.shadow_rt_params(np.eye(4), list(lights), 1.0, 2.0, 0.05, 80.0, normal_offset=1e-3, tmin=0.0)


def _soft(radii=(0.5, 0.0), S=16, P=4, samples="ok", reserved=(0, 0)):
    s = abi.shadow_rt_soft(radii, S, P)
    s.samples = _TABLE.ctypes.data if samples == "ok" else samples
    s.reserved[0], s.reserved[1] = reserved
    return s


def _call(entry, soft="ok", params="ok"):
    lib = abi.product()
    d, n, o = img(D24, W, H), img(RG16, W, H), img(RGBA8, W, H)
    p = _params() if params == "ok" else params
    s = _soft() if soft == "ok" else soft
    byref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    if entry == "shadow_mask_rt_soft":
        rc = lib.vkr_shadow_mask_rt_soft(byref(d), byref(n), _empty_accel().handle, byref(p), byref(s), byref(o), None)
    else:
        cut = abi.ray_cutout(0, 0)
        scratch = np.zeros(int(abi.accel_cutout_scratch_bytes(0)) + 64, np.uint8)
        rc = lib.vkr_shadow_mask_rt_soft_cutout(byref(d), byref(n), _empty_accel().handle, None, 0, None, 0, byref(p), byref(cut), byref(s), byref(o),
                                                scratch.ctypes.data, scratch.nbytes, None)
    return rc, (lib.vkr_last_error() or b"").decode()


NAN, INF = float("nan"), float("inf")
REFUSALS = {
    "soft NULL": (dict(soft=None), ERR_NULL, "soft is NULL"),
    "samples NULL": (dict(soft=_soft(samples=None)), ERR_NULL, "samples is NULL"),
    "S 0": (dict(soft=_soft(S=0)), ERR_EXTENT, "sample_count 0, expected 1..64"),
    "S 65": (dict(soft=_soft(S=65)), ERR_EXTENT, "sample_count 65, expected 1..64"),
    "P 0": (dict(soft=_soft(P=0)), ERR_EXTENT, "pattern_side 0, expected 1, 2 or 4"),
    "P 3": (dict(soft=_soft(P=3)), ERR_EXTENT, "pattern_side 3, expected 1, 2 or 4"),
    "P 8": (dict(soft=_soft(P=8)), ERR_EXTENT, "pattern_side 8, expected 1, 2 or 4"),
    "radius negative": (dict(soft=_soft(radii=(0.5, -1.0))), ERR_EXTENT, "light 1 has radius -1"),
    "radius NaN": (dict(soft=_soft(radii=(NAN, 0.5))), ERR_EXTENT, "light 0 has radius nan"),
    "radius inf": (dict(soft=_soft(radii=(0.0, INF))), ERR_EXTENT, "light 1 has radius inf"),
    "reserved 0": (dict(soft=_soft(reserved=(3, 0))), ERR_EXTENT, "soft reserved is 3, 0"),
    "reserved 1": (dict(soft=_soft(reserved=(0, 9))), ERR_EXTENT, "soft reserved is 0, 9"),
    # the gates of the hard entry come first, under the new entry's prefix
    "params NULL": (dict(params=None), ERR_NULL, "params is NULL"),
    "light_count 5": (dict(params=(lambda p: (setattr(p, "light_count", 5), p)[1])(_params())), ERR_EXTENT, "light_count 5"),
}


@pytest.mark.parametrize("entry", ["shadow_mask_rt_soft", "shadow_mask_rt_soft_cutout"])
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_entry_refusals(name, entry):
    kwargs, code, message = REFUSALS[name]
    rc, msg = _call(entry, **kwargs)
    assert rc == code, (name, rc, msg)
    assert message in msg and msg.startswith(entry + ":"), (name, msg)


def test_the_last_entry_gate_is_the_cutout_binding():
    """every soft gate passes, the next refusal is bind_cutout's: the soft gates lie before anything is recorded"""
    lib = abi.product()
    d, n, o, p, s = img(D24, W, H), img(RG16, W, H), img(RGBA8, W, H), _params(), _soft()
    rc = lib.vkr_shadow_mask_rt_soft_cutout(C.byref(d), C.byref(n), _empty_accel().handle, None, 0, None, 0, C.byref(p), None, C.byref(s), C.byref(o),
                                            None, 0, None)
    assert rc == ERR_NULL and "shadow_mask_rt_soft_cutout: cutout is NULL" in lib.vkr_last_error().decode()


# ---- the frame setter's refusals --------------------------------------------------------------------------------------------------------
def _set_area(frame, radii, S=16, P=4, count=None):
    l = host.lib()
    flat = (C.c_float * max(1, len(radii)))(*[float(r) for r in radii])
    rc = l.vkrh_set_shadow_area_lights(frame.h, flat, len(radii) if count is None else count, S, P)
    return rc, l.vkrh_last_error().decode()


def test_frame_setter_refusals():
    frame = _HostMemoryFrame(tiled=False)
    try:
        assert host.lib().vkrh_set_shadow_area_lights(frame.h, None, 1, 16, 4) != 0
        # one light is set by default
        for kwargs, text in ((dict(radii=[0.5, 0.5]), "count 2, but 1 lights are set"), (dict(radii=[0.5], count=0), "count 0, but 1 lights are set"),
                             (dict(radii=[0.5], S=0), "sample_count 0, needs 1..64"), (dict(radii=[0.5], S=65), "sample_count 65, needs 1..64"),
                             (dict(radii=[0.5], P=3), "pattern_side 3, needs 1, 2 or 4"), (dict(radii=[0.5], P=0), "pattern_side 0, needs 1, 2 or 4"),
                             (dict(radii=[-0.5]), "light 0: the radius must be finite and >= 0"), (dict(radii=[NAN]), "light 0: the radius must be finite"),
                             (dict(radii=[INF]), "light 0: the radius must be finite")):
            rc, msg = _set_area(frame, **kwargs)
            assert rc != 0 and "vkrh_set_shadow_area_lights: " + text in msg, (kwargs, msg)
        assert _set_area(frame, [0.5])[0] == 0
        assert frame.set_rays([(0, 1, 0, 1), (1, 2, 0, 0), (0, 3, 0, 1)])[0] == 0
        rc, msg = _set_area(frame, [0.5])
        assert rc != 0 and "count 1, but 3 lights are set" in msg
        assert _set_area(frame, [0.5, 0.0, 1.0], S=64, P=1)[0] == 0
        # the stage's own refusals are untouched by the setter
        rc, msg = frame.run(host.STAGE_SHADOW_MASK_RT)
        assert rc != 0 and "VKRH_STAGE_SHADOW_MASK_RT without a loaded scene" in msg
    finally:
        frame.close()


def test_frame_setter_is_refused_on_a_tiled_frame():
    frame = _HostMemoryFrame(tiled=True)
    try:
        rc, msg = _set_area(frame, [0.5])
        assert rc != 0 and "vkrh_set_shadow_area_lights: on a tiled frame" in msg
    finally:
        frame.close()


# ---- the table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,P", [(1, 1), (3, 2), (4, 2), (16, 4), (64, 4), (64, 1), (7, 4)])
def test_disk_samples_table(S, P):
    """allowed difference: equal after rounding to fp32, or 1 ulp where libm's cos / sin differ from numpy's"""
    got = abi.shadow_disk_samples(S, P)
    want = ref.disk_samples(S, P)
    assert got.shape == want.shape == (P * P, S, 2) and got.dtype == np.float32
    equal = np.array_equal(got, want)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print(f"[shadow mask rt soft] table S {S} P {P}: {'equal after rounding to fp32' if equal else f'{int((ulps != 0).sum())} values differ, at most {int(ulps.max())} ulp'}")
    assert equal or ulps.max() <= 1
    assert (np.hypot(got[..., 0].astype(np.float64), got[..., 1].astype(np.float64)) <= 1.0).all()
    for p in range(P * P):
        assert len({(float(u), float(v)) for u, v in got[p]}) == S, "two samples of a pattern coincide"
    for p in range(P * P):
        for q in range(p):
            assert not np.array_equal(got[p], got[q]), f"patterns {p} and {q} are equal"


def test_disk_samples_refuses_in_python_what_the_library_ignores():
    for S, P in ((0, 1), (65, 1), (4, 3)):
        with pytest.raises(RuntimeError, match="shadow_disk_samples"):
            abi.shadow_disk_samples(S, P)
    out = np.full(8, 7.0, F32)
    abi.product().vkr_shadow_disk_samples(4, 3, out.ctypes.data)
    assert (out == 7.0).all()


# ---- the reference alone ----------------------------------------------------------------------------------------------------------------
def _arith():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


@functools.lru_cache(maxsize=None)
def _scene():
    sc = scn.procedural_scene(detail=8)
    return sc, abi.scene_triangles(sc)


@functools.lru_cache(maxsize=None)
def _raster(size):
    w, h = size
    setup = FrameSetup(w, h)
    chain = PostFxChain(w, h, backend="oracle", setup=setup)
    chain.raster(_scene()[0])
    return chain.depth.raw(0)[..., 0].astype(np.uint32), chain.normal.raw(0).copy(), setup


def _soft_mask(size, lights, radii, samples):
    words, codes, setup = _raster(size)
    return ref.shadow_mask_rt_soft(_arith(), words, codes, setup.inv_view, *setup.fazz, list(lights), OFFSET, TMIN, _scene()[1], radii, samples)


@functools.lru_cache(maxsize=None)
def _hard_mask(size):
    words, codes, setup = _raster(size)
    return hard.shadow_mask_rt(_arith(), words, codes, setup.inv_view, *setup.fazz, LIGHTS4, OFFSET, TMIN, _scene()[1])


def test_radius_zero_is_the_hard_reference():
    size = (16, 10)
    got = _soft_mask(size, LIGHTS4, (0.0, 0.0, 0.0, 0.0), ref.disk_samples(16, 4))
    assert np.array_equal(got, _hard_mask(size))
    assert (got == 0).any() and (got == 255).any()


def test_an_all_zero_table_is_the_hard_reference():
    size = (16, 10)
    got = _soft_mask(size, LIGHTS4, (0.5, 0.5, 0.5, 0.5), np.zeros((16, 5, 2), F32))
    assert np.array_equal(got, _hard_mask(size))


def test_the_order_of_the_samples_does_not_matter():
    size = (16, 10)
    table = ref.disk_samples(16, 4)
    rng = np.random.default_rng(0x50F7)
    permuted = np.stack([table[p][rng.permutation(16)] for p in range(16)])
    assert not np.array_equal(permuted, table)
    a = _soft_mask(size, LIGHTS4, (0.5, 0.5, 1.0, 0.5), table)
    assert np.array_equal(a, _soft_mask(size, LIGHTS4, (0.5, 0.5, 1.0, 0.5), permuted))
    assert not np.array_equal(a, _hard_mask(size))


@pytest.mark.parametrize("S", [1, 3, 16, 64])
def test_quantisation(S):
    V = np.arange(S + 1)
    codes = ref.quantise(V, S)
    assert codes[0] == 0 and codes[S] == 255 and (np.diff(codes.astype(int)) > 0).all()
    for v in V:
        # 255 v / S rounded half up, in exact integers: floor((2 * 255 v + S) / (2 S))
        q, r = divmod(255 * int(v), S)
        assert int(codes[v]) == q + (1 if 2 * r >= S else 0), (v, S)
    assert len(ref.code_set(S)) == S + 1


def test_reference_inputs_have_a_penumbra():
    """what keeps the GPU parity test from passing on masks without a penumbra: at 64 x 36 every channel has geometry pixels at 0, at
    255 and strictly between, and at least 8 distinct codes; at 8 x 8 every channel has a pixel strictly between"""
    radii = (0.5, 0.5, 0.5, 0.5)
    table = ref.disk_samples(16, 4)
    words, _, _ = _raster((64, 36))
    geometry = (words & SKY) != SKY
    mask = _soft_mask((64, 36), LIGHTS4, radii, table)
    between = [int(((mask[..., l] > 0) & (mask[..., l] < 255) & geometry).sum()) for l in range(4)]
    distinct = [len(np.unique(mask[..., l][geometry])) for l in range(4)]
    print(f"[shadow mask rt soft] 64x36 S 16 P 4 radius 0.5: {int(geometry.sum())} geometry pixels, strictly between per light {between}, distinct codes {distinct}")
    for l in range(4):
        ch = mask[..., l][geometry]
        assert (ch == 0).any() and (ch == 255).any() and between[l] >= 1 and distinct[l] >= 8, (l, between, distinct)
        assert set(np.unique(ch).tolist()) <= ref.code_set(16)
    assert (mask[~geometry] == 255).all()
    words8, _, _ = _raster((8, 8))
    geometry8 = (words8 & SKY) != SKY
    mask8 = _soft_mask((8, 8), LIGHTS4, radii, table)
    between8 = [int(((mask8[..., l] > 0) & (mask8[..., l] < 255) & geometry8).sum()) for l in range(4)]
    print(f"[shadow mask rt soft] 8x8: strictly between per light {between8}")
    assert all(b >= 1 for b in between8), between8
