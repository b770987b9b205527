"""The temporal accumulation of the shadow mask without a GPU: the C-ABI block (header, library and abi.py agree), every refusal of
vkr_shadow_mask_accumulate and of vkrh_set_shadow_mask_accumulate with its own message (validation never reaches a launch), the
host-only table vkr_shadow_disk_samples_frame against numpy, and the numpy restatement
(tests/shadow_mask_accumulate_reference.py) alone on the constructed cases of tests/shadow_mask_accumulate_cases.py: the
consequences of the rule, every branch of the validity decision reached, and every mutant of the rule observed.

Measured here over the case set (test_every_branch_is_reached prints it): 31987 pixels with a valid history, 11458 / 3855 / 16968 /
6842 / 1698 / 9717 whose first failing condition is 1 .. 6; the clamp changes 3393 counts, the rounding term 55136 history values;
the ten mutants change between 485 (`<= w`) and 440770 (256 for 257) values."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd.chain import PostFxChain

import shadow_mask_accumulate_cases as cases
import shadow_mask_accumulate_reference as ref
from test_abi_errors import ERR_EXTENT, ERR_FORMAT, ERR_LAYOUT, ERR_NULL, FAKE, img
from test_shadow_mask_rt import _HostMemoryFrame

F32 = np.float32
D24 = abi.FMT_D24_UNORM_S8
RG16 = abi.FMT_RG16_UNORM
RG16F = abi.FMT_RG16_SFLOAT
RGBA8 = abi.FMT_RGBA8_UNORM
RGBA16 = abi.FMT_RGBA16_UNORM
R8 = abi.FMT_R8_UNORM
NAN = float("nan")


# ---- declarations -------------------------------------------------------------------------------------------------------------------
def test_block_layout_and_symbols():
    txt = open(abi.ROOT + "/include/vkr_postfx.h").read()
    body = re.search(r"typedef struct vkr_shadow_accum_params \{(.*?)\} vkr_shadow_accum_params;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert fields == ["vkr_mat4 inverse_camera", "vkr_mat4 prev_inverse_camera", "float fovy, aspect, znear, zfar", "uint32_t max_count",
                      "float plane_tolerance", "uint32_t reset", "uint32_t reserved"]
    assert C.sizeof(abi.ShadowAccumParams) == 64 + 64 + 16 + 16 == 160
    offsets = {"inverse_camera": 0, "prev_inverse_camera": 64, "fovy": 128, "aspect": 132, "znear": 136, "zfar": 140, "max_count": 144,
               "plane_tolerance": 148, "reset": 152, "reserved": 156}
    for name, off in offsets.items():
        assert getattr(abi.ShadowAccumParams, name).offset == off, name
    assert re.search(r"\bint\s+vkr_shadow_mask_accumulate\(const vkr_img\* depth, const vkr_img\* normal, const vkr_img\* velocity, const vkr_img\* prev_depth,\s+"
                     r"const vkr_img\* mask, const vkr_img\* history, const vkr_img\* history_count,\s+const vkr_shadow_accum_params\* params,\s+"
                     r"const vkr_img\* out_history, const vkr_img\* out_count, const vkr_img\* out_mask, void\* stream\);", txt)
    assert "void vkr_shadow_disk_samples_frame(uint32_t sample_count, uint32_t pattern_side, uint32_t frame, uint32_t frame_count, float* out);" in txt
    assert "int vkr_selftest_accum_division(uint32_t* device_counter, void* stream);" in txt
    for name in ("vkr_shadow_mask_accumulate", "vkr_shadow_disk_samples_frame", "vkr_selftest_accum_division"):
        assert hasattr(abi.product(), name), name
    assert "int vkrh_set_shadow_mask_accumulate(void* frame, uint32_t max_count, float plane_tolerance, uint32_t pattern_frames);" in \
        open(abi.ROOT + "/vk-renderer_amd/host/frame.hpp").read()
    p = abi.shadow_accum_params(np.eye(4), 2 * np.eye(4), 1.0, 2.0, 0.05, 80.0, 8, reset=True)
    assert (p.max_count, p.reset, p.reserved) == (8, 1, 0) and p.plane_tolerance == F32(0.01) and p.prev_inverse_camera.m[0] == 2.0


def test_setter_is_exported_and_no_program_is_registered():
    assert hasattr(host.lib(), "vkrh_set_shadow_mask_accumulate") and hasattr(host.HostFrame, "set_shadow_mask_accumulate")
    assert host.lib().vkrh_has_program(b"shadow_mask_accumulate") == 0  # the task calls the entry: the table stays as it is
    assert hasattr(PostFxChain, "shadow_mask_accumulate") and hasattr(PostFxChain, "reset")


# ---- the entry's gates ----------------------------------------------------------------------------------------------------------------
W, H = 64, 32
NAMES = ("depth", "normal", "velocity", "prev_depth", "mask", "history", "history_count", "out_history", "out_count", "out_mask")
FORMATS = dict(zip(NAMES, (D24, RG16, RG16F, D24, RGBA8, RGBA16, R8, RGBA16, R8, RGBA8)))
WRONG = dict(zip(NAMES, (abi.FMT_R32_SFLOAT, RG16F, RG16, abi.FMT_R32_SFLOAT, abi.FMT_RGBA8_SRGB, abi.FMT_RGBA16_SFLOAT, abi.FMT_R16_UNORM,
                         abi.FMT_RGBA16_SFLOAT, abi.FMT_R16_UNORM, abi.FMT_RGBA8_SRGB)))
BASE = {name: FAKE + 0x100000 * i for i, name in enumerate(NAMES)}  # ten images that do not overlap (the largest is 16 KiB)


def _img(name, w=W, h=H, fmt=None, **kw):
    kw.setdefault("base", BASE[name])
    return img(FORMATS[name] if fmt is None else fmt, w, h, **kw)


def _params(max_count=8, plane_tolerance=0.01, reset=0, reserved=0):
    p = abi.shadow_accum_params(np.eye(4), np.eye(4), 1.0, 2.0, 0.05, 80.0, max_count, plane_tolerance, reset)
    p.reserved = reserved
    return p


def _call(**over):
    lib = abi.product()
    a = {name: _img(name) for name in NAMES}
    a["params"] = _params()
    a.update(over)
    byref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    rc = lib.vkr_shadow_mask_accumulate(*[byref(a[n]) for n in NAMES[:7]], byref(a["params"]), *[byref(a[n]) for n in NAMES[7:]], None)
    return rc, (lib.vkr_last_error() or b"").decode()


WINDOW = dict(full=(W, 2 * H), origin=(0, H))
REFUSALS = {"params NULL": (dict(params=None), ERR_NULL, "params is NULL")}
for _n in NAMES:
    REFUSALS[f"{_n} NULL"] = ({_n: None}, ERR_NULL, f"{_n} is NULL")
    REFUSALS[f"{_n} without memory"] = ({_n: _img(_n, base=None)}, ERR_NULL, f"shadow_mask_accumulate.{_n}: NULL image")
    REFUSALS[f"{_n} format"] = ({_n: _img(_n, fmt=WRONG[_n])}, ERR_FORMAT, f"shadow_mask_accumulate.{_n}: format")
    REFUSALS[f"{_n} window"] = ({_n: _img(_n, **WINDOW)}, ERR_EXTENT,
                                f"shadow_mask_accumulate: {_n}: windows are not supported (the reprojection reaches across strips")
    if _n != "out_mask":
        REFUSALS[f"{_n} extent"] = ({_n: _img(_n, W, H + 1)}, ERR_EXTENT, f"{_n} is 64x33, out_mask 64x32: one extent expected")
REFUSALS.update({
    "out_mask extent": (dict(out_mask=_img("out_mask", W, H - 1)), ERR_EXTENT, "depth is 64x32, out_mask 64x31: one extent expected"),
    "extent above 65535": ({n: _img(n, 65536, 1) for n in NAMES}, ERR_EXTENT, "depth is 65536x1, at most 65535 texels a side"),
    "max_count 0": (dict(params=_params(max_count=0)), ERR_EXTENT, "max_count 0, expected 1..255"),
    "max_count 256": (dict(params=_params(max_count=256)), ERR_EXTENT, "max_count 256, expected 1..255"),
    "reset 2": (dict(params=_params(reset=2)), ERR_EXTENT, "reset is 2, must be 0 or 1"),
    "reserved": (dict(params=_params(reserved=7)), ERR_EXTENT, "reserved is 7, must be 0"),
    "plane_tolerance NaN": (dict(params=_params(plane_tolerance=NAN)), ERR_EXTENT, "plane_tolerance is NaN"),
    "history in place": (dict(out_history=_img("out_history", base=BASE["history"])), ERR_LAYOUT, "history and out_history overlap in memory"),
    "history overlap by one row": (dict(out_history=_img("out_history", base=BASE["history"] + (H - 1) * W * 8)), ERR_LAYOUT,
                                   "history and out_history overlap in memory"),
    "count in place": (dict(out_count=_img("out_count", base=BASE["history_count"])), ERR_LAYOUT, "history_count and out_count overlap in memory"),
    "mask shifted by one row": (dict(out_mask=_img("out_mask", base=BASE["mask"] + W * 4)), ERR_LAYOUT, "mask and out_mask overlap in memory"),
    "out_mask over depth": (dict(out_mask=_img("out_mask", base=BASE["depth"])), ERR_LAYOUT, "depth and out_mask overlap in memory"),
    "out_history over mask": (dict(out_history=_img("out_history", base=BASE["mask"])), ERR_LAYOUT, "mask and out_history overlap in memory"),
    "out_count over velocity": (dict(out_count=_img("out_count", base=BASE["velocity"] + 4)), ERR_LAYOUT, "velocity and out_count overlap in memory"),
    "out_count inside out_history": (dict(out_count=_img("out_count", base=BASE["out_history"] + 8)), ERR_LAYOUT, "out_count and out_history overlap in memory"),
})


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_entry_refusals(name):
    kwargs, code, message = REFUSALS[name]
    rc, msg = _call(**kwargs)
    assert rc == code, (name, rc, msg)
    assert message in msg and msg.startswith("shadow_mask_accumulate"), (name, msg)


def test_refusal_messages_are_distinct():
    texts = [_call(**kwargs)[1] for kwargs, _, _ in REFUSALS.values()]
    assert len(set(texts)) == len(texts) - 1  # "in place" and "overlap by one row" of the history share the one overlap message


# ---- the frame setter -------------------------------------------------------------------------------------------------------------------
def _set(frame, max_count, plane_tolerance=0.01, pattern_frames=1):
    l = host.lib()
    rc = l.vkrh_set_shadow_mask_accumulate(frame.h, max_count, plane_tolerance, pattern_frames)
    return rc, l.vkrh_last_error().decode()


def test_frame_setter_refusals():
    frame = _HostMemoryFrame(tiled=False)
    try:
        for args, text in (((256,), "max_count 256, needs 0 (off) or 1..255"), ((8, NAN), "plane_tolerance is NaN"), ((8, 0.01, 0), "pattern_frames 0, needs 1..64"),
                           ((8, 0.01, 65), "pattern_frames 65, needs 1..64")):
            rc, msg = _set(frame, *args)
            assert rc != 0 and "vkrh_set_shadow_mask_accumulate: " + text in msg, (args, msg)
        for max_count, frames in ((0, 1), (1, 1), (8, 8), (255, 64), (0, 1)):
            assert _set(frame, max_count, 0.01, frames)[0] == 0
        # the stages' own refusals are untouched by the setter
        assert _set(frame, 8, 0.01, 4)[0] == 0
        rc, msg = frame.run(host.STAGE_SHADOW_MASK_RT)
        assert rc != 0 and "VKRH_STAGE_SHADOW_MASK_RT without a loaded scene" in msg
        l = host.lib()
        for name in (b"shadow_mask_accumulated", b"shadow_history", b"shadow_history_out", b"shadow_history_count", b"shadow_history_count_out"):
            assert l.vkrh_image(frame.h, name, 0, 1, C.byref(abi.VkrImg())) != 0
            assert f"'{name.decode()}' only exists after a mask stage with vkrh_set_shadow_mask_accumulate on" in l.vkrh_last_error().decode()
    finally:
        frame.close()


def test_frame_setter_is_refused_on_a_tiled_frame():
    frame = _HostMemoryFrame(tiled=True)
    try:
        rc, msg = _set(frame, 8)
        assert rc != 0 and "vkrh_set_shadow_mask_accumulate: on a tiled frame" in msg
    finally:
        frame.close()


# ---- the sample tables of a cycle of frames ---------------------------------------------------------------------------------------------
def _disk_samples_frame(S, P, frame, T):
    k = np.arange(S, dtype=np.float64)[None, :]
    p = np.arange(P * P, dtype=np.int64)[:, None]
    rho = np.sqrt((k + 0.5) / S)
    phi = k * 2.399963229728653 + 2 * np.pi * (((7 * p) % (P * P)) * T + frame % T) / (P * P * T)
    return np.stack([rho * np.cos(phi), rho * np.sin(phi)], -1).astype(F32)


@pytest.mark.parametrize("S,P,T", [(1, 4, 8), (16, 4, 4), (5, 2, 3), (64, 1, 64), (3, 2, 1)])
def test_disk_samples_frame(S, P, T):
    """compared as test_disk_samples_table compares: equal after rounding to fp32, or 1 ulp where libm's cos / sin differ from numpy's"""
    tables = [abi.shadow_disk_samples_frame(S, P, f, T) for f in range(T)]
    for f, got in enumerate(tables):
        want = _disk_samples_frame(S, P, f, T)
        assert got.shape == want.shape == (P * P, S, 2) and got.dtype == np.float32
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert np.array_equal(got, want) or ulps.max() <= 1, (f, int(ulps.max()))
        assert np.array_equal(abi.shadow_disk_samples_frame(S, P, f + T, T), got), "the cycle does not repeat after T frames"
        for g in range(f):
            assert not np.array_equal(got, tables[g]), f"the tables of frames {g} and {f} are equal"
    # the rotations of sample 0 over all tables and patterns: P * P * T evenly spaced angles
    turns = np.sort(np.concatenate([np.arctan2(t[:, 0, 1].astype(np.float64), t[:, 0, 0].astype(np.float64)) % (2 * np.pi) for t in tables]))
    steps = np.diff(np.concatenate([turns, turns[:1] + 2 * np.pi]))
    assert len(turns) == P * P * T and np.allclose(steps, 2 * np.pi / (P * P * T), atol=1e-5), steps


@pytest.mark.parametrize("S,P", [(1, 1), (1, 4), (16, 4), (5, 2), (64, 4)])
def test_disk_samples_frame_of_one_frame_is_the_old_table(S, P):
    for frame in (0, 1, 9):
        assert abi.shadow_disk_samples_frame(S, P, frame, 1).tobytes() == abi.shadow_disk_samples(S, P).tobytes()


def test_disk_samples_frame_writes_nothing_for_what_it_does_not_take():
    for S, P, T in ((0, 1, 1), (65, 1, 1), (4, 3, 1), (4, 2, 0), (4, 2, 65)):
        with pytest.raises(RuntimeError, match="shadow_disk_samples_frame"):
            abi.shadow_disk_samples_frame(S, P, 0, T)
        out = np.full(2 * 64 * 16, 7.0, F32)
        abi.product().vkr_shadow_disk_samples_frame(S, P, 0, T, out.ctypes.data)
        assert (out == 7.0).all()
    abi.product().vkr_shadow_disk_samples_frame(4, 2, 0, 2, None)


# ---- the reference alone ----------------------------------------------------------------------------------------------------------------
def _arith():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


@functools.lru_cache(maxsize=None)
def _reference(index, mutant=None):
    return ref.shadow_mask_accumulate(_arith(), *cases.reference_args(cases.all_cases()[index]), mutant=mutant)


def _run(c, **over):
    c = dict(c, **over)
    return ref.shadow_mask_accumulate(_arith(), *cases.reference_args(c))


def test_the_case_set_holds_what_the_issue_lists():
    cs = cases.all_cases()
    assert {c["size"] for c in cs} == set(cases.EXTENTS)
    assert {(c["max_count"], c["reset"]) for c in cs} >= {(1, 0), (2, 0), (32, 0), (255, 0), (32, 1)}
    big = [c for c in cs if c["name"].startswith("mixed-130x70") and c["reset"] == 0]
    for c in big:
        v = c["velocity"].astype(F32)
        assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
        denormal = (v != 0) & (np.abs(v) < F32(2.0 ** -14))
        assert denormal.any()
        assert set(np.unique(c["mask"])) == set(range(256))
        assert {0, 1, 65534, 65535} <= set(np.unique(c["history"]))
        mc = c["max_count"]
        assert {0, 1, max(mc - 1, 0), mc, min(mc + 1, 255), 255} <= set(np.unique(c["count"]).tolist())
        # f exactly on integers, on 0 and on w and h themselves
        h, w = c["depth"].shape
        gy, gx = np.mgrid[0:h, 0:w]
        fx, fy = cases._f(w, gx, c["velocity"][..., 0]), cases._f(h, gy, c["velocity"][..., 1])
        moved = c["velocity"].astype(F32) != 0
        assert (moved[..., 0] & (fx == np.floor(fx)) & (fx > 0) & (fx < w)).any() and (moved[..., 1] & (fy == np.floor(fy)) & (fy > 0) & (fy < h)).any()
        assert (fx == w).any() and (fy == h).any() and (moved[..., 0] & (fx == 0)).any() and (moved[..., 1] & (fy == 0)).any()
        assert (fx < 0).any() and (fx > w).any() and (fy < 0).any() and (fy > h).any()
        sky, prev_sky = c["depth"] == cases.SKY, c["prev_depth"] == cases.SKY
        assert (sky & ~prev_sky).any() and (prev_sky & ~sky).any()
    assert big
    for c in cs:
        if c["name"].startswith("bound"):
            assert set(np.unique(np.sign(np.abs(c["factor"]) - 1))) == {-1.0, 1.0}


def test_every_branch_is_reached():
    """branch coverage as a condition: every first-failing validity condition and the valid branch occur; the clamp and the rounding
    term each change an output"""
    counts = np.zeros(7, np.int64)
    clamp = rounding = 0
    for i, c in enumerate(cases.all_cases()):
        out_history, out_count, out_mask, failed = _reference(i)
        counts += np.bincount(failed.reshape(-1), minlength=7)
        if c["size"] == (67, 35) and c["max_count"] < 255:  # where the clamp binds, the count differs from that of a cap out of reach
            clamp += int((_run(c, max_count=255)[1] != out_count).sum())
        rounding += int((_reference(i, "no_rounding")[0] != out_history).sum())
    print(f"[shadow mask accumulate] valid {counts[0]}, first failing condition 1..6: {counts[1:].tolist()}; the clamp changes {clamp} counts, "
          f"the rounding term {rounding} history values")
    assert (counts > 0).all(), counts
    assert clamp > 0 and rounding > 0


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_changes_a_byte(mutant):
    changed = 0
    for i in range(len(cases.all_cases())):
        good, bad = _reference(i), _reference(i, mutant)
        changed += sum(int((a != b).sum()) for a, b in zip(good[:3], bad[:3]))
    print(f"[shadow mask accumulate] mutant {mutant}: {changed} values differ")
    assert changed > 0


def _mixed(max_count=32, reset=0):
    return next(c for c in cases.all_cases() if c["name"] == f"mixed-67x35-max{max_count}-reset{reset}")


def test_no_history_copies_the_mask():
    """max_count == 1, reset == 1 or an all-zero count image: out_mask == mask byte for byte and out_history == 257 * mask"""
    base = _mixed()
    for c in (_mixed(1, 0), _mixed(32, 1), dict(base, count=np.zeros_like(base["count"]))):
        out_history, out_count, out_mask, failed = _run(c)
        assert np.array_equal(out_mask, c["mask"]) and np.array_equal(out_history, c["mask"].astype(np.uint16) * 257)
        assert (out_count == 1).all()
    assert (_run(base)[2] != base["mask"]).any()  # not vacuous: with its histories the case does change the mask


def test_a_constant_mask_is_a_fixed_point():
    c = next(c for c in cases.all_cases() if c["name"] == "two_cameras-67x35")
    for value in ((0, 0, 0, 0), (255, 255, 255, 255), (1, 127, 128, 254)):
        mask = np.empty_like(c["mask"])
        mask[:] = value
        history = np.empty_like(c["history"])
        history[:] = np.array(value, np.uint16) * 257
        out_history, out_count, out_mask, failed = _run(c, mask=mask, history=history)
        assert (failed == ref.VALID).any() and (failed != ref.VALID).any()
        assert np.array_equal(out_mask, mask) and np.array_equal(out_history, history), value


def test_a_count_above_max_count_is_clamped():
    c = _mixed(2, 0)
    out_history, out_count, out_mask, failed = _run(c, count=np.full_like(c["count"], 255))
    valid = failed == ref.VALID
    assert valid.any() and (out_count[valid] == 2).all() and (out_count[~valid] == 1).all()
    out255 = _run(_mixed(255, 0), count=np.full_like(c["count"], 255))
    assert (out255[1][out255[3] == ref.VALID] == 255).all()  # min(255, 254) + 1: the count never wraps


def test_two_cameras_reproject_through_the_plane_test():
    """the floor seen by two cameras: nearly every floor pixel whose reprojection stays inside has a valid history (the plane test
    passes through a real reprojection), and a previous camera that is not the one that wrote prev_depth fails it"""
    i = next(i for i, c in enumerate(cases.all_cases()) if c["name"] == "two_cameras-130x70")
    c = cases.all_cases()[i]
    failed = _reference(i)[3]
    floor = c["depth"] != cases.SKY
    reached = floor & np.isin(failed, (ref.VALID, 6))
    print(f"[shadow mask accumulate] two cameras: {int(floor.sum())} floor pixels, {int(reached.sum())} reach the plane test, {int((failed == 6).sum())} fail it")
    assert reached.sum() > 0.8 * floor.sum() and (failed[reached] == ref.VALID).mean() > 0.99
    wrong = _reference(i, "current_camera")[3]
    assert (wrong[reached] == 6).mean() > 0.9
