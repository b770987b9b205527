"""Constructed texels, extents and row layouts for the image transfers (csrc/transfer.hip: vkr_clear_image, vkr_blit_image,
vkr_gen_mipmaps), shared by tests/test_transfer_cases.py (CPU: the classes contain what they claim, the restatement equals
independent definitions, mutants of the frozen rules change expected bytes) and tests/test_transfer_cases_gpu.py (the kernels).

Everything is seeded and small: no image exceeds 256 x 256 or 16384 x 1.  A case is a hashable key; `source()` gives its texels,
`expected()` what tests/transfer_reference.py says the kernel leaves (a list of arrays: the blit's destination, the levels of a
chain, the texel of a clear).  Both are cached; `expected.__wrapped__` computes afresh (the mutant test).

Texel classes (`source(cls, fmt, w, h, seed)`):
  random          tr.random_texels: what tests/test_transfer_gpu.py runs on
  all_codes       every code of an 8-/16-bit channel in every channel, channel c rolled by another odd offset (extent fixed by
                  the format: 256 x 256 or 16 x 16); for fp16 that is every denormal, +-0, +-inf, every NaN, 65504
  store_ties      fp32 values on and next to the ties of every store rule (STORE_TIE_GROUPS), 128 texels wide
  non_finite      random, with 1 % each of the largest finite value, -0 and a denormal and 0.25 % each of +inf, -inf and NaN; an
                  inf planted at (0, 0) and (w - 1, h - 1), a NaN at (w / 2, h / 2), a -inf at (w / 3, 2 h / 3)
  denormal_steps  fp16 codes 0..7 with random sign
  fp32_denormals  fp32 words with a zero exponent field
  overflow        +-FLT_MAX and +-0.75 FLT_MAX: the left half positive, the right half negative, one texel in ten flipped

The three NaN makers of non_finite stand at 0.25 %, not 1 %: the GPU compare lets a NaN match any NaN, so no (class, format,
filter) case may expect more than 5 % NaNs (NAN_CAP, asserted per case by the CPU test), and under LINEAR at 1:1 a NaN reaches
four and an infinity three destination texels (0 * inf): 1 % each gives 10 %.  On a 3 x 3 source one planted NaN is 11 % by
itself, so the cap is taken over the pooled values of a case's three geometries (64 x 64, 3 x 3 -> 7 x 7, 7 x 7 -> 3 x 3) and
over all levels of the chains of a mip case.

Row layouts.  LAYOUT_ALIGNED is ImageBuf's (rows and mips at multiples of 256).  LAYOUT_TIGHT is the least the C-ABI promises
(make_tex, csrc/vkr_host.hpp): pitch exactly w * bpp with odd w, mips packed at multiples of min(bpp, 4), and the base only
min(bpp, 4)-aligned (TIGHT_GUARD leading guard bytes: 64 + min(bpp, 4)), 64 poison bytes or more on both sides.

What every global access reachable from the three entries needs, read in csrc/transfer.hip and csrc/vkr_device.hpp:
  clear   store_u32x4 (one 16-byte store) only where `n == 16 && (p & 3) == 0`: dword alignment; everything else byte stores.
  blit    load_rgba -> load_raw<bpp>: uint8 (1), uint16 (2-aligned: base and pitch are multiples of 2), uint32 (4), U32x2 (one
          8-byte load, 4-aligned), U32x4 (one 16-byte load, 4-aligned); store_texel -> store_raw<bpp>, the same widths; the
          D24 copy a uint32 load and store (4).  The sRGB tables are the library's own arrays.
  mips    mip_load = load_raw<bpp>; mip_load_pair: two loads for 1- and 2-byte texels, load_raw_pair<4> one U32x2 (8 bytes at a
          4-aligned address) and load_raw_pair<8> one U32x4 (16 bytes at a 4-aligned address: 8 * x0 + a 4-aligned row), taken
          only where x0 + 1 < w; mip_store = store_raw<bpp>.  The LDS levels are arrays of uint32 / uint2, naturally aligned.
So under LAYOUT_TIGHT every access is aligned to min(bpp, 4) and in bounds (a pair load never crosses the row's last texel; the
clear writes `n` bytes of the row and no more).  The 8- and 16-byte accesses go through U32x2 / U32x4, declared
`packed, aligned(4)`: the compiler may only emit global_load/store_dwordx2/x4 for them because the target allows multi-dword
global accesses at dword alignment (LLVM's SITargetLowering::allowsMisalignedMemoryAccessesImpl: "Alignment >= 4" suffices
outside LDS; the CDNA ISA guide, "Memory alignment": in every SH_MEM_CONFIG.alignment_mode but STRICT a multi-dword global access
needs dword alignment at most), which is what the comment above load_u32x2 in vkr_device.hpp states, and what the pair
footprints of TAA and texdraw (pair_rows: xs any texel, so 8-byte loads at 4- and 16-byte loads at 8-byte alignment) already do
under GPU test.
"""
import functools

import numpy as np

import texdraw_reference as texdraw_ref
import transfer_reference as tr

F32 = np.float32
FLT_MAX = np.finfo(F32).max
NEAREST, LINEAR = tr.NEAREST, tr.LINEAR
NAN_CAP = 0.05

HALF_FORMATS = [tr.FMT_RG16_SFLOAT, tr.FMT_RGBA16_SFLOAT, tr.FMT_R16_SFLOAT]
F32_FORMATS = [tr.FMT_R32_SFLOAT, tr.FMT_RGBA32_SFLOAT]
FLOAT_FORMATS = HALF_FORMATS + F32_FORMATS
CODE_FORMATS = [f for f in tr.COLOR_FORMATS if f not in F32_FORMATS]   # 8 or 16 bits a channel
ROLL = {8: (1, 77, 131, 201), 16: (1, 77, 4099, 30011)}               # odd, different per channel
NAN_BITS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFBFFFFF], np.uint32)  # quiet NaNs of both signs, then signalling ones


def bpp(fmt):
    dt, c = tr.RAW_DTYPE[fmt]
    return np.dtype(dt).itemsize * c


# ---- texel classes ----------------------------------------------------------------------------------------------------------------
def all_codes(fmt):
    dt, c = tr.RAW_DTYPE[fmt]
    bits = 8 * np.dtype(dt).itemsize
    assert bits in (8, 16), fmt
    side = 1 << (bits // 2)
    codes = np.arange(1 << bits, dtype=np.uint32)
    img = np.stack([np.roll(codes, ROLL[bits][ch]) for ch in range(c)], axis=-1).reshape(side, side, c)
    return img.astype(np.uint8) if bits == 8 else img.astype(np.uint16).view(dt)


def _with_neighbours(v):
    v = np.asarray(v, F32)
    return np.stack([np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))], axis=1).reshape(-1)


def half_value(code):
    """the value of the positive fp16 code, 0x7C00 continued as 65536 (the step 65504 -> 65536 whose midpoint is 65520)"""
    code = np.asarray(code, np.int64)
    e, m = code >> 10, code & 0x3FF
    return np.where(e == 0, m * 2.0 ** -24, (1024 + m) * 2.0 ** (e - 25.0))


UNORM16_TIE_K = np.unique(np.concatenate([[0, 1, 65534], np.random.default_rng(2024).choice(np.arange(2, 65534), 4093, replace=False)]))
HALF_NORMAL_STEPS = np.array(sorted(set(range(1024, 0x7BFF, 211)) | {1024, 0x7BFE, 0x7BFF}))


@functools.lru_cache(maxsize=None)
def store_tie_groups():
    """name -> fp32 values; every entry of the first five groups stands between its two fp32 neighbours"""
    k8, k16 = np.arange(256), UNORM16_TIE_K
    den = (half_value(np.arange(1023)) + half_value(np.arange(1, 1024))) * 0.5      # exact in fp32: (k + 0.5) * 2^-24
    nrm = (half_value(HALF_NORMAL_STEPS) + half_value(HALF_NORMAL_STEPS + 1)) * 0.5
    specials = np.concatenate([np.array([-0.0, -1e-45, np.nextafter(F32(1), F32(0)), 1.0, np.nextafter(F32(1), F32(2)), FLT_MAX, -FLT_MAX,
                                         np.inf, -np.inf, 0.0, 65504.0, -65504.0, 1e-45], F32), NAN_BITS.view(F32)])
    return {
        "unorm8": _with_neighbours((k8 + 0.5) / 255.0),
        "unorm16": _with_neighbours((k16 + 0.5) / 65535.0),
        "half_denormal": _with_neighbours(np.concatenate([den, -den])),
        "half_normal": _with_neighbours(np.concatenate([nrm, -nrm])),
        "srgb": _with_neighbours(tr.SRGB_THRESH[1:]),
        "specials": specials,
    }


def store_tie_values():
    g = store_tie_groups()
    return np.concatenate([g[k] for k in ("unorm8", "unorm16", "half_denormal", "half_normal", "srgb", "specials")]).astype(F32)


# the scalars a clear is given as colour components: the specials, and the named ties with their neighbours
def clear_scalars():
    g = store_tie_groups()
    ties = _with_neighbours(np.array([0.5 / 255, 1.5 / 255, 254.5 / 255, 0.5 / 65535, 65534.5 / 65535, 65520.0, 2.0 ** -25, 1.5 * 2.0 ** -24,
                                      float(tr.SRGB_THRESH[1]), float(tr.SRGB_THRESH[128]), float(tr.SRGB_THRESH[255])], np.float64).astype(F32))
    return np.concatenate([g["specials"], ties]).astype(F32)


def _store_ties(fmt):
    c = tr.RAW_DTYPE[fmt][1]
    v = store_tie_values()
    w = 128
    h = -(-v.size // w)
    v = np.concatenate([v, np.full(w * h - v.size, 0.25, F32)])
    return np.stack([np.roll(v, ROLL[16][ch] if ch else 0) for ch in range(c)], axis=-1).reshape(h, w, c)


STORE_TIES_EXTENT = (128, -(-store_tie_values().size // 128))


def _plant(img, value, x, y):
    img[min(y, img.shape[0] - 1), min(x, img.shape[1] - 1)] = value


def _non_finite(fmt, w, h, seed):
    dt, c = tr.RAW_DTYPE[fmt]
    img = tr.random_texels(fmt, w, h, seed)
    pick = np.random.default_rng(seed + 7919).random(img.shape)
    big, den = (65504.0, 6e-8) if dt == np.float16 else (FLT_MAX, 1e-40)
    lo = 0.0
    for rate, value in ((0.01, big), (0.01, -0.0), (0.01, den), (0.0025, np.inf), (0.0025, -np.inf), (0.0025, np.nan)):
        img[(pick >= lo) & (pick < lo + rate)] = value
        lo += rate
    _plant(img, np.nan, w // 2, h // 2)
    _plant(img, -np.inf, w // 3, 2 * h // 3)
    _plant(img, np.inf, 0, 0)
    _plant(img, np.inf, w - 1, h - 1)
    return img


def _denormal_steps(fmt, w, h, seed):
    dt, c = tr.RAW_DTYPE[fmt]
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 8, size=(h, w, c)) | (rng.integers(0, 2, size=(h, w, c)) << 15)
    return codes.astype(np.uint16).view(np.float16)


def _fp32_denormals(fmt, w, h, seed):
    c = tr.RAW_DTYPE[fmt][1]
    rng = np.random.default_rng(seed)
    words = rng.integers(1, 1 << 23, size=(h, w, c), dtype=np.int64) | (rng.integers(0, 2, size=(h, w, c), dtype=np.int64) << 31)
    return words.astype(np.uint32).view(F32)


def _overflow(fmt, w, h, seed):
    c = tr.RAW_DTYPE[fmt][1]
    rng = np.random.default_rng(seed)
    mag = np.where(rng.random((h, w, c)) < 0.5, FLT_MAX, F32(0.75) * FLT_MAX).astype(F32)
    sign = np.where(np.arange(w)[None, :, None] < (w + 1) // 2, 1.0, -1.0) * np.where(rng.random((h, w, c)) < 0.1, -1.0, 1.0)
    return (mag * sign.astype(F32)).astype(F32)


CLASS_FORMATS = {"non_finite": FLOAT_FORMATS, "denormal_steps": HALF_FORMATS, "fp32_denormals": [tr.FMT_R32_SFLOAT], "overflow": F32_FORMATS}
_MAKERS = {"non_finite": _non_finite, "denormal_steps": _denormal_steps, "fp32_denormals": _fp32_denormals, "overflow": _overflow}


@functools.lru_cache(maxsize=None)
def source(cls, fmt, w, h, seed):
    """texels [h, w, c] of the storage type; read-only"""
    if cls == "random":
        img = tr.random_texels(fmt, w, h, seed)
    elif cls == "all_codes":
        img = all_codes(fmt)
    elif cls == "store_ties":
        img = _store_ties(fmt)
    else:
        assert fmt in CLASS_FORMATS[cls], (cls, fmt)
        img = _MAKERS[cls](fmt, w, h, seed)
    assert img.shape[:2] == (h, w) and img.dtype == tr.RAW_DTYPE[fmt][0], (cls, fmt, img.shape, img.dtype)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


def class_extent(cls, fmt):
    if cls == "all_codes":
        return (256, 256) if np.dtype(tr.RAW_DTYPE[fmt][0]).itemsize == 2 else (16, 16)
    assert cls == "store_ties"
    return STORE_TIES_EXTENT


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# ("blit", class, source format, (sw, sh), destination format, (dw, dh), filter, seed)
def _blit(cls, sfmt, src, dfmt, dst, filt, seed=1):
    return ("blit", cls, sfmt, tuple(src), dfmt, tuple(dst), filt, seed)


def _one_to_one(cls, sfmt, dfmt, filt):
    e = class_extent(cls, sfmt)
    return _blit(cls, sfmt, e, dfmt, e, filt)


ALL_CODES_BLITS = [_one_to_one("all_codes", s, d, NEAREST) for s in CODE_FORMATS for d in tr.COLOR_FORMATS]
ALL_CODES_LINEAR = [_one_to_one("all_codes", tr.FMT_RGBA16_SFLOAT, tr.FMT_RGBA32_SFLOAT, LINEAR)]
STORE_TIES_BLITS = [_one_to_one("store_ties", s, d, NEAREST) for s in F32_FORMATS for d in tr.COLOR_FORMATS]

GEOMETRIES = [((1, 1), (65, 5)), ((65, 5), (1, 1)), ((1, 300), (7, 300)), ((300, 1), (300, 7)), ((3, 3), (1000, 2)), ((1000, 2), (997, 3)),
              ((2049, 3), (3, 2049)), ((16384, 1), (16383, 1)), ((16383, 1), (16384, 1)), ((64, 4), (64, 4)), ((65, 5), (65, 5)), ((7, 7), (3, 3)),
              ((3, 3), (7, 7))]
GEOMETRY_PAIRS = [(tr.FMT_RGBA32_SFLOAT, tr.FMT_RGBA32_SFLOAT), (tr.FMT_RGBA16_SFLOAT, tr.FMT_RGBA8_SRGB)]
GEOMETRY_BLITS = [_blit("random", s, src, d, dst, filt, seed=3 + i) for i, (src, dst) in enumerate(GEOMETRIES) for s, d in GEOMETRY_PAIRS
                  for filt in (LINEAR, NEAREST)]

CONTENT_CLASSES = ["non_finite", "denormal_steps", "fp32_denormals", "overflow"]
CONTENT_GEOMETRIES = [((64, 64), (64, 64)), ((3, 3), (7, 7)), ((7, 7), (3, 3))]
CONTENT_MIP_EXTENTS = [(64, 64), (33, 65)]


def content_destinations(cls, fmt):
    """the class's own format (nothing hides a value) and, for the non-finite texels, a UNORM16 destination"""
    return [fmt, tr.FMT_RGBA16_UNORM] if cls == "non_finite" else [fmt]


def content_blit_group(cls, fmt, dfmt, filt):
    """one GPU case: the three geometries of a (class, format, destination, filter)"""
    return [_blit(cls, fmt, src, dfmt, dst, filt, seed=11) for src, dst in CONTENT_GEOMETRIES]


CONTENT_GROUPS = [(cls, fmt, dfmt, filt) for cls in CONTENT_CLASSES for fmt in CLASS_FORMATS[cls] for dfmt in content_destinations(cls, fmt)
                  for filt in (LINEAR, NEAREST)]
CONTENT_BLITS = [k for g in CONTENT_GROUPS for k in content_blit_group(*g)]

# ("mips", class, format, (w, h), seed)
ONE_WIDE_EXTENTS = [(1, 300), (2, 300), (3, 1000), (300, 1), (300, 2)]
OTHER_MIP_EXTENTS = [(100, 700), (700, 100), (63, 63), (64, 64), (65, 65), (127, 33)]
OTHER_MIP_FORMATS = [tr.FMT_RGBA8_SRGB, tr.FMT_RGBA16_SFLOAT, tr.FMT_R32_SFLOAT]
EXTENT_MIPS = ([("mips", "random", f, e, 5) for e in ONE_WIDE_EXTENTS for f in tr.MIP_FORMATS]
               + [("mips", "random", f, e, 5) for e in OTHER_MIP_EXTENTS for f in OTHER_MIP_FORMATS])
CONTENT_MIP_GROUPS = [(cls, fmt) for cls in CONTENT_CLASSES for fmt in CLASS_FORMATS[cls] if fmt in tr.MIP_FORMATS]
CONTENT_MIPS = [("mips", cls, fmt, e, 11) for cls, fmt in CONTENT_MIP_GROUPS for e in CONTENT_MIP_EXTENTS]

# ("clear", format, colour, depth, stencil) on CLEAR_EXTENT with CLEAR_MIPS levels
CLEAR_EXTENT, CLEAR_MIPS = (5, 3), 3
_scalars = clear_scalars()
_scalars = np.concatenate([_scalars, np.full(-_scalars.size % 4, 0.5, F32)])
CLEAR_COLOURS = [tuple(float(v) for v in _scalars[i: i + 4]) for i in range(0, _scalars.size, 4)]
# NaN colour components compare equal as keys only by identity, so the colours are named by their index
CLEAR_DEPTHS = [float(F32((k + 0.5) / 16777215.0)) for k in (0, 1, 2, 4097, 8388606)] + [0.0, 1.0, -0.5, 1.5, float("inf"), float("-inf"),
                                                                                             float(np.nextafter(F32(1), F32(0))), float("nan")]
COLOUR_CLEARS = [("clear", f, i, None, 0) for f in tr.COLOR_FORMATS for i in range(len(CLEAR_COLOURS))]
DEPTH_CLEARS = [("clear", tr.FMT_D24_UNORM_S8, None, i, 0x5A + i) for i in range(len(CLEAR_DEPTHS))]
# rows around the 1024 bytes of one block and the 16 bytes of one thread (R16 rows hold an even number of bytes: 14, 16, 18)
CLEAR_ROWS = [(tr.FMT_R8_UNORM, 1023), (tr.FMT_R8_UNORM, 1024), (tr.FMT_R8_UNORM, 1025), (tr.FMT_R8_UNORM, 15), (tr.FMT_R8_UNORM, 16),
              (tr.FMT_R8_UNORM, 17), (tr.FMT_R16_UNORM, 7), (tr.FMT_R16_UNORM, 8), (tr.FMT_R16_UNORM, 9)]

# ("texdraw", class, source format, backbuffer format): 1:1 onto both surface formats
TEXDRAWS = ([("texdraw", "all_codes", s, d) for s in (tr.FMT_RGBA16_SFLOAT, tr.FMT_RGBA16_UNORM) for d in (tr.FMT_RGBA8_SRGB, tr.FMT_RGBA8_UNORM)]
            + [("texdraw", "store_ties", tr.FMT_RGBA32_SFLOAT, d) for d in (tr.FMT_RGBA8_SRGB, tr.FMT_RGBA8_UNORM)])

# ---- tight layouts ------------------------------------------------------------------------------------------------------------------
LAYOUT_ALIGNED, LAYOUT_TIGHT = "aligned", "tight"
TIGHT_EXTENTS = [(5, 3), (37, 21), (75, 9)]
# every texel size once as the source and once as the destination
TIGHT_PAIRS = [(tr.FMT_R8_UNORM, tr.FMT_R16_SFLOAT), (tr.FMT_R16_UNORM, tr.FMT_R8_UNORM), (tr.FMT_RGBA8_SRGB, tr.FMT_RGBA16_SFLOAT),
               (tr.FMT_RGBA16_SFLOAT, tr.FMT_RGBA32_SFLOAT), (tr.FMT_RGBA32_SFLOAT, tr.FMT_RGBA8_UNORM), (tr.FMT_RG16_UNORM, tr.FMT_RGBA16_UNORM),
               (tr.FMT_R32_SFLOAT, tr.FMT_RG16_SFLOAT)]
TIGHT_BLITS = [_blit("random", s, e, d, dst, filt, seed=17) for s, d in TIGHT_PAIRS for i, e in enumerate(TIGHT_EXTENTS)
               for dst in (e, TIGHT_EXTENTS[(i + 1) % 3]) for filt in (LINEAR, NEAREST)]
TIGHT_MIP_EXTENTS = TIGHT_EXTENTS + [(1, 37), (37, 1)]
TIGHT_MIPS = [("mips", "random", f, e, 19) for f in tr.MIP_FORMATS for e in TIGHT_MIP_EXTENTS]


def tight_layout(fmt):
    """-> (row_align, guard) for ImageBuf: rows and mips at multiples of min(bpp, 4), the base min(bpp, 4) past a 64-byte guard"""
    a = min(bpp(fmt), 4)
    return a, 64 + a


def clear_want(key):
    _, fmt, ci, di, stencil = key
    color = CLEAR_COLOURS[ci] if ci is not None else (0.0, 0.0, 0.0, 0.0)
    depth = CLEAR_DEPTHS[di] if di is not None else 1.0
    return color, depth, stencil


# ---- what the restatement says ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(key, contract=2):
    """-> list of arrays: [the destination] of a blit or texdraw, the levels of a chain, [the texel] of a clear"""
    kind = key[0]
    if kind == "blit":
        _, cls, sfmt, (sw, sh), dfmt, (dw, dh), filt, seed = key
        return [tr.blit(source(cls, sfmt, sw, sh, seed), sfmt, dw, dh, dfmt, filt, contract)]
    if kind == "mips":
        _, cls, fmt, (w, h), seed = key
        return tr.mip_chain(fmt, source(cls, fmt, w, h, seed))
    if kind == "clear":
        color, depth, stencil = clear_want(key)
        return [tr.clear_texel(key[1], color, depth, stencil)]
    if kind == "clear_old":
        return [tr.clear_texel(key[1], *OLD_CLEAR)]
    if kind == "texdraw":
        _, cls, sfmt, dfmt = key
        w, h = class_extent(cls, sfmt)
        return [texdraw_ref.texdraw(source(cls, sfmt, w, h, 1), sfmt, w, h, dfmt, 0, contract)]
    raise ValueError(key)


def canonical(fmt, raw):
    """the stored texels as unsigned words with every NaN code of an fp16 / fp32 format mapped to one code: sign and payload of
    a NaN are not frozen.  Everything else (+-0, +-inf, every UNORM / sRGB byte) stays as it is."""
    raw = np.ascontiguousarray(raw)
    dt = tr.RAW_DTYPE[fmt][0]
    if dt == np.float16:
        bits = raw.view(np.uint16).copy()
        bits[(bits & 0x7FFF) > 0x7C00] = 0x7E00
        return bits
    if dt == np.float32:
        bits = raw.view(np.uint32).copy()
        bits[(bits & 0x7FFFFFFF) > 0x7F800000] = 0x7FC00000
        return bits
    return raw.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[np.dtype(dt).itemsize])


def destination_format(key):
    return key[{"blit": 4, "mips": 2, "clear": 1, "clear_old": 1, "texdraw": 3}[key[0]]]


# ---- the cases tests/test_transfer_gpu.py had before this module: its sizes on tr.random_texels -----------------------------------------
# (the RGBA8_SRGB chains of 2048 x 2048 and 4096 x 1024 are left out: random bytes at more texels.  No byte content holds a
# NaN, a denormal or an overflow, and one_wide_levels() covers their extents, so they kill nothing the smaller chains let through)
OLD_CLEAR = ((0.25, 1.5, -1.0, 0.6), 0.4, 0x5A)
OLD_GEOMETRY = [((640, 360), (640, 360)), ((256, 128), (128, 64)), ((300, 201), (200, 134)), ((64, 48), (128, 96)), ((257, 129), (100, 77))]
OLD_SRGB_CHAIN_SIZES = [(256, 256), (300, 200), (257, 129), (5, 1), (1, 1), (2048, 2048), (4096, 1024)]
OLD_OTHER_CHAIN_SIZES = [(300, 200), (257, 129), (5, 1), (1, 1), (1024, 512)]
OLD_CHAIN_SIZES = sorted(set(OLD_SRGB_CHAIN_SIZES + OLD_OTHER_CHAIN_SIZES))
OLD_CASES = (
    [("mips", "random", tr.FMT_RGBA8_SRGB, e, 11 * e[0] + e[1]) for e in OLD_SRGB_CHAIN_SIZES if e[0] * e[1] <= 256 * 256]
    + [("mips", "random", f, e, 100 * f + e[0]) for f in tr.MIP_FORMATS if f != tr.FMT_RGBA8_SRGB for e in OLD_OTHER_CHAIN_SIZES]
    + [_blit("random", tr.FMT_RGBA16_SFLOAT, s, tr.FMT_RGBA8_SRGB, d, filt) for s, d in OLD_GEOMETRY for filt in (LINEAR, NEAREST)]
    + [_blit("random", tr.COLOR_FORMATS[i], (93, 41), tr.COLOR_FORMATS[(i + 4) % 11], (50, 67), filt, seed=i) for i in range(11)
       for filt in (LINEAR, NEAREST)]
    + [_blit("random", tr.FMT_RGBA8_SRGB, s, tr.FMT_RGBA8_SRGB, d, filt) for s, d in (((300, 200), (150, 100)), ((64, 64), (64, 64)))
       for filt in (LINEAR, NEAREST)]
    + [("clear_old", f) for f in sorted(tr.RAW_DTYPE)])


def nan_counts(keys):
    """-> (NaN values, values) expected over the cases `keys`"""
    nans = total = 0
    for k in keys:
        for a in expected(k):
            total += a.size
            if a.dtype.kind == "f":
                nans += int(np.isnan(a).sum())
    return nans, total


# ---- counters -------------------------------------------------------------------------------------------------------------------------
def fused_coordinate_differences(dst_n, src_n):
    """destination positions of one axis whose tap or fraction changes when u - 0.5 is fused with the multiply"""
    from gtao_rt_reference import fma32

    scale = F32(src_n) / F32(dst_n)
    x = tr.linear_coords(dst_n, src_n)
    xf = fma32(np.arange(dst_n).astype(F32) + F32(0.5), scale, F32(-0.5))
    return int(((np.floor(x) != np.floor(xf)) | ((x - np.floor(x)) != (xf - np.floor(xf)))).sum())


def one_wide_levels(w, h):
    """-> (levels of the chain that are read as a source and are one texel wide, ... one texel high)"""
    n = tr.mip_count(w, h)
    ws, hs = [max(1, w >> m) for m in range(n - 1)], [max(1, h >> m) for m in range(n - 1)]
    return sum(1 for v in ws if v == 1), sum(1 for v in hs if v == 1)
