"""vkr_clear_image, vkr_blit_image, vkr_gen_mipmaps (and vkr_texdraw at 1:1) on the constructed texels, extents and row layouts of
tests/transfer_cases.py, against the numpy restatement (tests/transfer_reference.py, tests/texdraw_reference.py): byte for byte,
except that in an fp16 / fp32 destination a NaN matches any NaN (tc.canonical on both sides; tests/test_transfer_cases.py caps
the NaNs any case expects at 5 %).  Every image is filled with a poison byte and stands between guard bytes: a texel a kernel
did not write, a byte of padding it did, or a byte outside the image shows.  Both mip schedules run on every chain.

The tests named *tight_layout* run the least the C-ABI promises: pitch w * bpp with odd w, mips and base aligned to min(bpp, 4)
only (tc.LAYOUT_TIGHT; the module docstring of transfer_cases.py lists what every access of the kernels needs).
"""
import numpy as np
import pytest

from vk_renderer_amd import abi
from vk_renderer_amd.images import ROW_ALIGN, ImageBuf, mip_extent

import transfer_cases as tc
import transfer_reference as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xCD
SCHEDULES = [("per_level", abi.SWITCH_MIPS_PER_LEVEL), ("fused", abi.SWITCH_MIPS_FUSED)]
FILTERS = {tc.LINEAR: abi.FILTER_LINEAR, tc.NEAREST: abi.FILTER_NEAREST}
TALLY = {"cases": 0, "values": 0}


def _sync():
    import torch

    torch.cuda.synchronize()


def _contract():
    return int(abi.product().vkr_numeric_contract())


@pytest.fixture
def switches():
    lib = abi.product()
    before = lib.vkr_get_switches()
    yield lambda bits: lib.vkr_set_switches((before & ~(abi.SWITCH_MIPS_PER_LEVEL | abi.SWITCH_MIPS_FUSED)) | bits)
    lib.vkr_set_switches(before)


def _image(fmt, w, h, mips=1, level0=None, layout=tc.LAYOUT_ALIGNED):
    """a device image full of POISON between POISON guards, level 0 set"""
    row_align, guard = tc.tight_layout(fmt) if layout == tc.LAYOUT_TIGHT else (ROW_ALIGN, ROW_ALIGN)
    staged = ImageBuf(fmt, w, h, mips, fill=POISON, row_align=row_align)
    if level0 is not None:
        staged.set_raw(level0, 0)
    dev = ImageBuf(fmt, w, h, mips, device=DEV, fill=POISON, row_align=row_align, guard=guard)
    dev.upload(staged.to_host())
    if layout == tc.LAYOUT_TIGHT:
        # the base is min(bpp, 4) past a 64-byte boundary: aligned to what the C-ABI asks for and to nothing more
        assert dev.ptr % 64 == min(dev.bpp, 4) and all(p == mip_extent(w, m) * dev.bpp for m, p in enumerate(dev.pitch))
    return dev


def _levels(img, host_bytes):
    dt, c = tr.RAW_DTYPE[img.format]
    out = []
    for m in range(img.mips):
        w, h = mip_extent(img.width, m), mip_extent(img.height, m)
        rows = host_bytes[img.offset[m]: img.offset[m] + img.pitch[m] * h].reshape(h, img.pitch[m])[:, : w * img.bpp]
        out.append(np.ascontiguousarray(rows).view(dt).reshape(h, w, c))
    return out


def _check(img, want_levels, label, first_level=0):
    """the image's levels from `first_level` on against `want_levels`; padding and guards untouched"""
    host_bytes = img.to_host()
    got = _levels(img, host_bytes)
    mask = np.ones(img.nbytes, bool)
    for m in range(img.mips):
        w, h = mip_extent(img.width, m), mip_extent(img.height, m)
        mask[img.offset[m]: img.offset[m] + img.pitch[m] * h].reshape(h, img.pitch[m])[:, : w * img.bpp] = False
    assert len(want_levels) == img.mips - first_level, label
    for m, want in enumerate(want_levels, start=first_level):
        g, w_ = tc.canonical(img.format, got[m]), tc.canonical(img.format, np.broadcast_to(want, got[m].shape))
        bad = g != w_
        TALLY["values"] += int(bad.size)
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            raise AssertionError(f"{label} level {m}: {int(bad.sum())} of {bad.size} values differ, first at (y, x, c) = {at}: "
                                 f"got {int(g[at]):#x}, expected {int(w_[at]):#x}")
    assert np.all(host_bytes[mask] == POISON), f"{label}: padding written"
    assert np.all(img.guards() == POISON), f"{label}: bytes outside the image written"
    TALLY["cases"] += 1


def _run_blit(key, layout=tc.LAYOUT_ALIGNED):
    _, cls, sfmt, (sw, sh), dfmt, (dw, dh), filt, seed = key
    src = _image(sfmt, sw, sh, 1, tc.source(cls, sfmt, sw, sh, seed), layout)
    dst = _image(dfmt, dw, dh, 1, None, layout)
    abi.blit_image(src.desc(), dst.desc(), FILTERS[filt])
    _sync()
    _check(dst, tc.expected(key, _contract()), f"{layout} {key}")
    assert np.all(src.guards() == POISON)


def _run_mips(key, switches, layout=tc.LAYOUT_ALIGNED):
    _, cls, fmt, (w, h), seed = key
    want = tc.expected(key)
    outs = []
    for name, bit in SCHEDULES:
        switches(bit)
        img = _image(fmt, w, h, len(want), tc.source(cls, fmt, w, h, seed), layout)
        abi.gen_mipmaps(img.desc())
        _sync()
        _check(img, want, f"{layout} {name} {key}")
        outs.append(img.to_host())
    assert np.array_equal(outs[0], outs[1]), f"{key}: the two schedules leave different bytes"


def _run_clear(fmt, w, h, mips, color, depth, stencil, want, layout, label):
    img = _image(fmt, w, h, mips, None, layout)
    abi.clear_image(img.desc(), color, depth, stencil)
    _sync()
    _check(img, [want] * mips, f"{layout} clear {label}")


def _report(name):
    print(f"[transfer cases gpu] {name}: 0 differing values; so far {TALLY['cases']} images, {TALLY['values']} values compared")


# ---- tight layouts (sent to the GPU before the rest) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", range(len(tc.TIGHT_PAIRS)))
def test_tight_layout_blits(pair):
    sfmt, dfmt = tc.TIGHT_PAIRS[pair]
    for key in tc.TIGHT_BLITS:
        if (key[2], key[4]) == (sfmt, dfmt):
            _run_blit(key, tc.LAYOUT_TIGHT)
    _report(f"tight blits {sfmt} -> {dfmt}")


def test_tight_layout_depth_copy():
    w, h = 37, 21
    words = tr.random_texels(tr.FMT_D24_UNORM_S8, w, h, 3)
    src = _image(tr.FMT_D24_UNORM_S8, w, h, 1, words, tc.LAYOUT_TIGHT)
    dst = _image(tr.FMT_D24_UNORM_S8, w, h, 1, None, tc.LAYOUT_TIGHT)
    abi.blit_image(src.desc(), dst.desc(), abi.FILTER_NEAREST)
    _sync()
    _check(dst, [words], "tight D24 copy")


@pytest.mark.parametrize("fmt", tr.MIP_FORMATS)
def test_tight_layout_mips(switches, fmt):
    for key in tc.TIGHT_MIPS:
        if key[2] == fmt:
            _run_mips(key, switches, tc.LAYOUT_TIGHT)
    _report(f"tight mips format {fmt}")


@pytest.mark.parametrize("fmt", sorted(tr.RAW_DTYPE))
def test_tight_layout_clears(fmt):
    color, depth, stencil = tc.OLD_CLEAR
    want = tr.clear_texel(fmt, color, depth, stencil)
    for w, h in tc.TIGHT_EXTENTS:
        _run_clear(fmt, w, h, tr.mip_count(w, h), color, depth, stencil, want, tc.LAYOUT_TIGHT, f"format {fmt} {w}x{h}")
    _report(f"tight clears format {fmt}")


# ---- texels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfmt", tc.CODE_FORMATS)
def test_all_codes_nearest_to_every_destination(sfmt):
    """decode x store, exhaustively, through the real kernel"""
    keys = [k for k in tc.ALL_CODES_BLITS if k[2] == sfmt]
    assert len(keys) == len(tr.COLOR_FORMATS)
    for key in keys:
        _run_blit(key)
    _report(f"all_codes format {sfmt} -> {len(keys)} destinations")


def test_all_codes_linear():
    for key in tc.ALL_CODES_LINEAR:
        _run_blit(key)
    _report("all_codes LINEAR")


@pytest.mark.parametrize("sfmt", tc.F32_FORMATS)
def test_store_ties_nearest_to_every_destination(sfmt):
    keys = [k for k in tc.STORE_TIES_BLITS if k[2] == sfmt]
    assert len(keys) == len(tr.COLOR_FORMATS)
    for key in keys:
        _run_blit(key)
    _report(f"store_ties format {sfmt} -> {len(keys)} destinations")


@pytest.mark.parametrize("group", tc.CONTENT_GROUPS, ids=lambda g: f"{g[0]}_{g[1]}_to_{g[2]}_{'linear' if g[3] == tc.LINEAR else 'nearest'}")
def test_content_classes_blit(group):
    for key in tc.content_blit_group(*group):
        _run_blit(key)
    _report(f"content blit {group}")


@pytest.mark.parametrize("group", tc.CONTENT_MIP_GROUPS, ids=lambda g: f"{g[0]}_{g[1]}")
def test_content_classes_mips(switches, group):
    for key in tc.CONTENT_MIPS:
        if key[1:3] == group:
            _run_mips(key, switches)
    _report(f"content mips {group}")


# ---- extents -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", range(len(tc.GEOMETRIES)), ids=lambda i: "{0[0]}x{0[1]}_to_{1[0]}x{1[1]}".format(*tc.GEOMETRIES[i]))
def test_blit_geometries(geometry):
    src, dst = tc.GEOMETRIES[geometry]
    keys = [k for k in tc.GEOMETRY_BLITS if (k[3], k[5]) == (src, dst)]
    assert len(keys) == 4
    for key in keys:
        _run_blit(key)
    _report(f"geometry {src} -> {dst}")


@pytest.mark.parametrize("extent", tc.ONE_WIDE_EXTENTS + tc.OTHER_MIP_EXTENTS, ids=lambda e: f"{e[0]}x{e[1]}")
def test_mip_extents(switches, extent):
    keys = [k for k in tc.EXTENT_MIPS if k[3] == extent]
    assert len(keys) == (len(tr.MIP_FORMATS) if extent in tc.ONE_WIDE_EXTENTS else len(tc.OTHER_MIP_FORMATS))
    for key in keys:
        _run_mips(key, switches)
    _report(f"mips {extent}")


# ---- clears ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", tr.COLOR_FORMATS)
def test_clear_special_colours(fmt):
    w, h = tc.CLEAR_EXTENT
    for key in tc.COLOUR_CLEARS:
        if key[1] == fmt:
            color, depth, stencil = tc.clear_want(key)
            _run_clear(fmt, w, h, tc.CLEAR_MIPS, color, depth, stencil, tc.expected(key)[0], tc.LAYOUT_ALIGNED, f"{key} {color}")
    _report(f"clear colours format {fmt}")


def test_clear_special_depths():
    w, h = tc.CLEAR_EXTENT
    for key in tc.DEPTH_CLEARS:
        color, depth, stencil = tc.clear_want(key)
        _run_clear(tr.FMT_D24_UNORM_S8, w, h, tc.CLEAR_MIPS, color, depth, stencil, tc.expected(key)[0], tc.LAYOUT_ALIGNED, f"{key} depth {depth!r}")
    _report("clear depths")


@pytest.mark.parametrize("layout", [tc.LAYOUT_ALIGNED, tc.LAYOUT_TIGHT])
def test_clear_rows_around_one_block_and_one_thread_tight_layout_too(layout):
    color = (0.3, 0.0, 0.0, 0.0)
    for fmt, w in tc.CLEAR_ROWS:
        _run_clear(fmt, w, 5, 1, color, 1.0, 0, tr.clear_texel(fmt, color), layout, f"format {fmt} row of {w} texels")
    _report(f"clear rows {layout}")


# ---- texdraw -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", tc.TEXDRAWS, ids=lambda k: f"{k[1]}_{k[2]}_onto_{k[3]}")
def test_texdraw_of_every_code_and_tie(key):
    import torch

    _, cls, sfmt, dfmt = key
    w, h = tc.class_extent(cls, sfmt)
    src = _image(sfmt, w, h, 1, tc.source(cls, sfmt, w, h, 1))
    out = _image(dfmt, w, h)
    abi.texdraw(src.desc(), out.desc(), abi.texdraw_push(0), torch.cuda.current_stream().cuda_stream)
    _sync()
    _check(out, tc.expected(key, _contract()), f"{key}")
    _report(f"texdraw {key}")
