"""The constructed cases of tests/transfer_cases.py on the CPU: the numpy restatement of the image transfers alone.  Three things
are proven here, so that tests/test_transfer_cases_gpu.py may rely on them: the classes contain what they claim (counters), the
restatement's codecs equal independent definitions in exact rational arithmetic (and the oracle's C conversions), and every
wrong rule of MUTANTS changes at least one expected byte of at least one new case.

SURVIVE_OLD is why the module exists: the mutants that change no byte of any case tests/test_transfer_gpu.py had before (its
sizes on tr.random_texels; test_the_old_cases_let_these_mutants_through asserts the list).  Seven of the nineteen survive there:
both fp32 denormal flushes (mixf, avg4), the fp16 overflow that saturates at 65504, NaN storing the maximum UNORM code, the D24
clear of NaN storing all ones, the skipped zero-weight tap, and the one-wide source that reads the next row.  The other twelve
are killed by the old cases too, some barely: the fp16 denormal flushes by 1 and 2 values of a 256 x 256 chain, the strict sRGB
compare by 2 values of one blit, the fused coordinate by 15 values of 93 x 41 -> 50 x 67 (one column); the round-half-up and
double-product UNORM stores die on the mip chains of the 8-bit formats, whose averages of four codes are ties by construction,
not on any blit.  Every mutant is killed by a new case; EXEMPT is empty.

Measured (`-s` prints every figure; 32 tests, about 15 s):
store_ties: 257 of 768 UNORM8 values and 4097 of 12 288 UNORM16 values are exact fp32 ties of the store, 129 / 2009 of them to an
even code (round half up differs), 129 / 2053 values store another code when the product is formed in double; 2046 + 2 x
len(HALF_NORMAL_STEPS) exact fp16 ties between their neighbours, 65520 and 2^-25 among them; the 255 sRGB thresholds.
denormal_steps 64 x 64 R16_SFLOAT: 807 of 1024 level-1 values are non-zero denormals, 261 exact ties of the denormal step.
fp32_denormals: 1024 of 1024 level-1 values are non-zero denormals.  overflow: 977 of 1024 level-1 values are infinite with a
finite exact mean, 20 are NaN.  non_finite 64 x 64: 10 .. 51 of each infinity and NaN, 35 .. 202 of the other three.
Fused coordinate: 0, 0, 1 positions of an axis change in the old 257 -> 100, 300 -> 200, 93 -> 50; 301 of 1000 in 3 -> 1000, 619
of 2049 in 3 -> 2049, 37 of 65 in 1 -> 65.  NaN cap: the most NaNs any case expects is 3.9 % (all_codes LINEAR).
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import transfer_cases as tc
import transfer_reference as tr
from gtao_rt_reference import fma32

F32 = np.float32


# ---- independent definitions: exact rationals, one rounding ---------------------------------------------------------------------------
def round_fraction(q, p, emin, emax):
    """the rational q rounded to nearest even in a binary format of p significant bits, least normal exponent emin, greatest
    emax, denormals kept -> (exact Fraction | +-inf as float)"""
    if q == 0:
        return Fraction(0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (max(e, emin) - (p - 1))
    r = round(a / ulp) * ulp          # round() of a Fraction rounds half to even
    if r >= Fraction(2) ** (emax + 1):
        return float("inf") if q > 0 else float("-inf")
    return r if q > 0 else -r


def f32_of(q):
    r = round_fraction(q, 24, -126, 127)
    return F32(r) if isinstance(r, float) else F32(r.numerator / r.denominator)   # exact: r is an fp32 value, the quotient a double


def half_code_of(x):
    """fp32 -> fp16 code by the definition: nearest even, denormals kept, 65520 and above to infinity; None for a NaN"""
    x = float(x)
    if np.isnan(x):
        return None
    sign = 0x8000 if np.signbit(x) else 0
    if np.isinf(x):
        return sign | 0x7C00
    r = round_fraction(Fraction(x), 11, -14, 15)
    if isinstance(r, float):
        return sign | 0x7C00
    a = abs(r)
    if a < Fraction(2) ** -14:
        return sign | int(a / Fraction(2) ** -24)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    return sign | ((e + 15) << 10) | (int(a / Fraction(2) ** (e - 10)) - 1024)


def half_value_of(code):
    """fp16 code -> value by the bit fields; None for a NaN"""
    s, e, m = code >> 15, (code >> 10) & 31, code & 1023
    if e == 31:
        return None if m else (float("-inf") if s else float("inf"))
    v = m * 2.0 ** -24 if e == 0 else (1024 + m) * 2.0 ** (e - 25)
    return -v if s else v


def unorm_code_of(x, bits):
    """rint(clamp(x, 0, 1) * (2^bits - 1)), the product rounded to fp32 once, ties to even, NaN -> 0"""
    x = float(x)
    if np.isnan(x):
        return 0
    c = Fraction(min(max(x, 0.0), 1.0))
    return round(Fraction(float(f32_of(c * (2 ** bits - 1)))))


def srgb_code_of(x):
    return 0 if np.isnan(x) else int((tr.SRGB_THRESH[1:] <= x).sum())


def test_decode_equals_the_definitions():
    k16 = np.arange(65536, dtype=np.uint16)
    got = tr.unorm_to_float(k16, 16)
    want = np.array([f32_of(Fraction(int(k), 65535)) for k in k16], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got = tr.unorm_to_float(np.arange(256, dtype=np.uint8), 8)
    want = np.array([f32_of(Fraction(k, 255)) for k in range(256)], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got = tr.decode(tr.FMT_R16_SFLOAT, k16.view(np.float16).reshape(256, 256, 1))[..., 0].reshape(-1)
    nans = 0
    for code in range(65536):
        v = half_value_of(code)
        if v is None:
            nans += 1
            assert np.isnan(got[code]), hex(code)
        else:
            assert got[code] == F32(v) and np.signbit(got[code]) == bool(code >> 15), hex(code)
    assert nans == 2046
    # decode() of whole texels: every channel of every code format against the per-channel rule, absent channels 0, 0, 0, 1
    for fmt in tc.CODE_FORMATS:
        raw = tc.source("all_codes", fmt, *tc.class_extent("all_codes", fmt), 1)
        rgba = tr.decode(fmt, raw)
        c = raw.shape[2]
        assert (rgba[..., c:3] == 0).all() and (c == 4 or (rgba[..., 3] == 1).all()), fmt
        assert len(np.unique(raw[..., 0].view(np.uint8 if raw.dtype == np.uint8 else np.uint16))) == (256 if raw.dtype == np.uint8 else 65536)


def _oracle_half(lib):
    lib.vkr_ref_half_to_float.restype, lib.vkr_ref_half_to_float.argtypes = C.c_float, [C.c_uint16]
    lib.vkr_ref_float_to_half.restype, lib.vkr_ref_float_to_half.argtypes = C.c_uint16, [C.c_float]
    return lib


def test_encode_of_the_store_ties_equals_the_definitions(oracle_lib):
    lib = _oracle_half(oracle_lib)
    v = tc.store_tie_values()
    u8 = np.array([unorm_code_of(x, 8) for x in v])
    u16 = np.array([unorm_code_of(x, 16) for x in v])
    srgb = np.array([srgb_code_of(x) for x in v])
    half = [half_code_of(x) for x in v]
    # the oracle's C conversions on the same values
    for x, h in zip(v, half):
        got = lib.vkr_ref_float_to_half(float(x))
        if h is None:
            assert (got & 0x7FFF) > 0x7C00, x
        else:
            assert got == h, (x, hex(got), hex(h))
            back = lib.vkr_ref_half_to_float(h)
            assert back == F32(half_value_of(h)) and np.signbit(back) == bool(h >> 15), hex(h)
    for code in range(0, 0x0400):  # every denormal, both signs
        for c in (code, code | 0x8000):
            assert lib.vkr_ref_half_to_float(c) == F32(half_value_of(c))
    half_bits = np.array([0x7E00 if h is None else h for h in half], np.uint16)
    rgba = np.stack([np.roll(v, s) for s in (0, 1, 2, 3)], axis=-1).reshape(1, -1, 4)
    per_channel = {8: u8, 16: u16, "srgb": srgb, "half": half_bits}
    for fmt in tr.COLOR_FORMATS:
        got = tr.encode(fmt, rgba)[0]
        dt, c = tr.RAW_DTYPE[fmt]
        for ch in range(c):
            if dt == np.float32:
                want = np.roll(v, ch).view(np.uint32)
                assert np.array_equal(got[:, ch].view(np.uint32), want), fmt
                continue
            rule = "half" if dt == np.float16 else "srgb" if (fmt == tr.FMT_RGBA8_SRGB and ch < 3) else 8 * np.dtype(dt).itemsize
            want = np.roll(per_channel[rule], ch)
            g = tc.canonical(fmt, got[:, ch]) if dt == np.float16 else got[:, ch]
            bad = np.flatnonzero(g != want)
            assert bad.size == 0, f"format {fmt} channel {ch}: {bad.size} differ, first value {np.roll(v, ch)[bad[0]]!r}: {g[bad[0]]} != {want[bad[0]]}"
    # the named edges
    assert half_code_of(65520.0) == 0x7C00 and half_code_of(np.nextafter(F32(65520), F32(0))) == 0x7BFF
    assert half_code_of(2.0 ** -25) == 0 and half_code_of(np.nextafter(F32(2.0 ** -25), F32(1))) == 1
    assert unorm_code_of(F32(0.5 / 255), 8) in (0, 1) and unorm_code_of(-0.0, 8) == 0 and unorm_code_of(np.inf, 16) == 65535


def test_clear_of_a_nan_depth_stores_zero():
    assert tr.clear_texel(tr.FMT_D24_UNORM_S8, depth=float("nan"), stencil=0x1A5)[0] == 0xA5000000
    assert tr.clear_texel(tr.FMT_D24_UNORM_S8, depth=float("inf"), stencil=0)[0] == 0x00FFFFFF
    assert tr.clear_texel(tr.FMT_D24_UNORM_S8, depth=-1.0, stencil=0)[0] == 0
    for i, d in enumerate(tc.CLEAR_DEPTHS):
        want = unorm_code_of(d, 24) | ((0x5A + i) & 0xFF) << 24
        assert tc.expected(tc.DEPTH_CLEARS[i])[0][0] == want, d
    assert tr.clear_texel(tr.FMT_RGBA16_UNORM, (float("nan"), 2.0, -1.0, 0.5))[0] == 0


# ---- counters: the classes contain what they claim ------------------------------------------------------------------------------------
def test_store_ties_hold_the_ties():
    g = tc.store_tie_groups()
    figures = {}
    for name, bits in (("unorm8", 8), ("unorm16", 16)):
        v = g[name]
        p32 = (v * F32(2 ** bits - 1)).astype(np.float64)
        tie = (p32 - np.floor(p32)) == 0.5
        even_tie = tie & (np.floor(p32) % 2 == 0)                                   # round half up stores one more there
        p64 = v.astype(np.float64) * (2 ** bits - 1)
        double_differs = np.rint(p64) != np.rint(p32)                                # the product in double stores another code
        figures[name] = (int(tie.sum()), int(even_tie.sum()), int(double_differs.sum()), v.size)
        assert tie.sum() >= v.size // 6 and even_tie.sum() >= v.size // 12 and double_differs.sum() > 0, figures[name]
    print(f"[transfer cases] store ties (exact fp32 ties, of them to an even code, codes a double product changes, values): {figures}")
    den, nrm = g["half_denormal"], g["half_normal"]
    assert den.size == 3 * 2 * 1023 and nrm.size == 3 * 2 * len(tc.HALF_NORMAL_STEPS)
    for v in (den, nrm):  # the middle of each triple is an exact tie: its neighbours store the two adjacent codes
        lo, mid, hi = (tr.float_to_half(v[i::3]).view(np.uint16).astype(np.int64) for i in range(3))
        assert (np.abs(hi - lo) == 1).all() and ((mid == lo) | (mid == hi)).all() and (mid % 2 == 0).all()
    assert F32(65520.0) in nrm and F32(2.0 ** -25) in den
    assert np.array_equal(g["srgb"][1::3], tr.SRGB_THRESH[1:])
    sp = g["specials"]
    assert np.isnan(sp).sum() == 4 and np.signbit(sp[np.isnan(sp)]).tolist() == [False, True, False, True] and np.isinf(sp).sum() == 2
    assert (sp.view(np.uint32) == 0x80000000).any() and (sp.view(np.uint32) == 0x80000001).any() and (np.abs(sp) == tc.FLT_MAX).sum() == 2
    src = tc.source("store_ties", tr.FMT_RGBA32_SFLOAT, *tc.STORE_TIES_EXTENT, 1)
    for ch in range(4):
        assert np.array_equal(np.sort(src[..., ch].reshape(-1).view(np.uint32)), np.sort(src[..., 0].reshape(-1).view(np.uint32)))
    assert set(tc.store_tie_values().view(np.uint32).tolist()) <= set(src[..., 0].reshape(-1).view(np.uint32).tolist())


def test_all_codes_hold_every_code_in_every_channel():
    for fmt in tc.CODE_FORMATS:
        raw = tc.source("all_codes", fmt, *tc.class_extent("all_codes", fmt), 1)
        bits = raw.view(np.uint8 if raw.dtype == np.uint8 else np.uint16)
        n = 256 if raw.dtype == np.uint8 else 65536
        for ch in range(raw.shape[2]):
            assert np.array_equal(np.sort(bits[..., ch].reshape(-1)), np.arange(n)), (fmt, ch)
        if raw.shape[2] > 1:
            assert len({int(bits[0, 0, ch]) for ch in range(raw.shape[2])}) == raw.shape[2]
        if raw.dtype == np.float16:
            f = raw[..., 0].reshape(-1)
            den = ((bits[..., 0] & 0x7C00) == 0) & ((bits[..., 0] & 0x3FF) != 0)
            assert np.isnan(f).sum() == 2046 and np.isinf(f).sum() == 2 and den.sum() == 2046 and (f == 65504).sum() == 1


def test_denormal_classes_stay_denormal():
    src = tc.source("denormal_steps", tr.FMT_R16_SFLOAT, 64, 64, 11)
    assert set(np.unique(src.view(np.uint16) & 0x7FFF).tolist()) == set(range(8)) and len(np.unique(src.view(np.uint16) >> 15)) == 2
    level1 = tc.expected(("mips", "denormal_steps", tr.FMT_R16_SFLOAT, (64, 64), 11))[1]
    b = level1.view(np.uint16)
    nonzero_denormal = ((b & 0x7C00) == 0) & ((b & 0x3FF) != 0)
    a, bb, c, d = tr.mip_taps(tr.decode(tr.FMT_R16_SFLOAT, src))
    exact = (a.astype(np.float64) + bb + c + d)[..., 0] * 0.25 / 2.0 ** -24        # in units of the denormal step
    ties = np.abs(exact - np.floor(exact)) == 0.5
    print(f"[transfer cases] denormal_steps 64 x 64 R16_SFLOAT: level 1 has {int(nonzero_denormal.sum())} non-zero denormals of {b.size}, {int(ties.sum())} exact ties of the step")
    assert nonzero_denormal.sum() > b.size // 2 and ties.sum() > b.size // 8
    flushed = np.where(nonzero_denormal, b & 0x8000, b)
    assert (flushed != b).sum() == nonzero_denormal.sum()
    src = tc.source("fp32_denormals", tr.FMT_R32_SFLOAT, 64, 64, 11)
    assert ((src.view(np.uint32) & 0x7F800000) == 0).all() and (src != 0).all()
    chain = tc.expected(("mips", "fp32_denormals", tr.FMT_R32_SFLOAT, (64, 64), 11))
    l1 = chain[1].view(np.uint32)
    assert ((l1 & 0x7F800000) == 0).all() and ((l1 & 0x7FFFFF) != 0).sum() > l1.size * 0.99
    print(f"[transfer cases] fp32_denormals 64 x 64: level 1 has {int(((l1 & 0x7FFFFF) != 0).sum())} non-zero denormals of {l1.size}")


def test_overflow_and_non_finite_hold_what_they_claim():
    src = tc.source("overflow", tr.FMT_R32_SFLOAT, 64, 64, 11)
    a, b, c, d = (t.astype(np.float64)[..., 0] for t in tr.mip_taps(tr.decode(tr.FMT_R32_SFLOAT, src)))
    level1 = tc.expected(("mips", "overflow", tr.FMT_R32_SFLOAT, (64, 64), 11))[1][..., 0]
    mean_finite = np.abs((a + b + c + d) * 0.25) <= tc.FLT_MAX
    inf_but_finite_mean, nan = int((np.isinf(level1) & mean_finite).sum()), int(np.isnan(level1).sum())
    print(f"[transfer cases] overflow 64 x 64: level 1 has {inf_but_finite_mean} infinities whose exact mean is finite, {nan} NaN (inf - inf) of {level1.size}")
    assert inf_but_finite_mean > level1.size // 2 and nan > 0
    lin = tc.expected(tc._blit("overflow", tr.FMT_R32_SFLOAT, (3, 3), tr.FMT_R32_SFLOAT, (7, 7), tc.LINEAR, seed=11))[0]
    assert np.isfinite(lin).any()
    for fmt in tc.FLOAT_FORMATS:
        src = tc.source("non_finite", fmt, 64, 64, 11)
        big, den = (65504.0, 6e-8) if src.dtype == np.float16 else (tc.FLT_MAX, 1e-40)
        counts = {"+inf": int((src == np.inf).sum()), "-inf": int((src == -np.inf).sum()), "nan": int(np.isnan(src).sum()),
                  "largest": int((src == src.dtype.type(big)).sum()), "-0": int(((src == 0) & np.signbit(src)).sum()),
                  "denormal": int((src == src.dtype.type(den)).sum())}
        print(f"[transfer cases] non_finite 64 x 64 format {fmt}: {counts} of {src.size}")
        assert all(n >= 3 for n in counts.values()), counts
        assert np.isinf(src[0, 0]).all() and np.isinf(src[63, 63]).all() and np.isnan(src[32, 32]).all() and (src[42, 21] == -np.inf).all()
    # LINEAR at equal extents is not the identity next to an infinity: one inf at (3, 3) of an 8 x 8 image
    img = np.full((8, 8, 1), 0.5, F32)
    img[3, 3] = np.inf
    out = tr.blit(img, tr.FMT_R32_SFLOAT, 8, 8, tr.FMT_R32_SFLOAT, tr.LINEAR)[..., 0]
    assert sorted(map(tuple, np.argwhere(np.isnan(out)).tolist())) == [(2, 2), (2, 3), (3, 2)] and np.isinf(out[3, 3])
    img[3, 3], img[7, 7] = 0.5, np.inf
    out = tr.blit(img, tr.FMT_R32_SFLOAT, 8, 8, tr.FMT_R32_SFLOAT, tr.LINEAR)[..., 0]
    assert np.isnan(out[7, 7]) and np.isnan(out).sum() == 4
    assert np.array_equal(tr.blit(img, tr.FMT_R32_SFLOAT, 8, 8, tr.FMT_R32_SFLOAT, tr.NEAREST), img)


def test_no_case_expects_more_than_the_cap_of_nans():
    worst = (0.0, None)
    groups = [[k] for k in tc.ALL_CODES_BLITS + tc.ALL_CODES_LINEAR + tc.STORE_TIES_BLITS + tc.GEOMETRY_BLITS + tc.EXTENT_MIPS + tc.TIGHT_BLITS
              + tc.TIGHT_MIPS + tc.TEXDRAWS]
    groups += [tc.content_blit_group(*g) for g in tc.CONTENT_GROUPS]
    groups += [[("mips", cls, fmt, e, 11) for e in tc.CONTENT_MIP_EXTENTS] for cls, fmt in tc.CONTENT_MIP_GROUPS]
    total_nans = 0
    for keys in groups:
        nans, total = tc.nan_counts(keys)
        total_nans += nans
        if nans / total > worst[0]:
            worst = (nans / total, keys[0])
        assert nans <= tc.NAN_CAP * total, f"{keys[0]}: {nans} of {total} expected values are NaN"
    n, t = tc.nan_counts(tc.ALL_CODES_LINEAR)
    print(f"[transfer cases] {len(groups)} cases, {total_nans} expected NaN values; most in {worst[1]}: {worst[0]:.2%}; all_codes LINEAR {n} of {t}")
    assert total_nans > 1000 and worst[0] > 0.03, "the cap is approached, not avoided"


def test_the_extents_reach_the_one_wide_branches():
    for e in tc.ONE_WIDE_EXTENTS[:3]:
        assert tc.one_wide_levels(*e)[0] >= 1, e
    assert tc.one_wide_levels(1, 300) == (8, 0) and tc.one_wide_levels(300, 1) == (0, 8)
    assert tc.one_wide_levels(2, 300)[0] == 7 and tc.one_wide_levels(3, 1000)[0] == 8
    # level 6 of 100 x 700 is 1 x 10: the source of the second fused launch (six levels a launch) is one texel wide
    assert (max(1, 100 >> 6), max(1, 700 >> 6)) == (1, 10) and tc.one_wide_levels(100, 700)[0] == 3 and tc.one_wide_levels(700, 100)[1] == 3
    # inside the LDS levels of one launch: 3 x 1000 has its levels 1..5 one texel wide
    assert [max(1, 3 >> m) for m in range(1, 6)] == [1] * 5
    # no chain of the old cases has a source level one texel wide (only one texel high)
    for e in tc.OLD_CHAIN_SIZES:
        assert tc.one_wide_levels(*e)[0] == 0, e
    assert tc.one_wide_levels(5, 1)[1] == 2 and tc.one_wide_levels(4096, 1024)[1] == 2


def test_the_geometries_see_the_unfused_coordinate():
    old = {(d, s): tc.fused_coordinate_differences(d, s) for d, s in ((100, 257), (200, 300), (50, 93), (128, 256), (128, 64), (640, 640))}
    new = {(d, s): tc.fused_coordinate_differences(d, s) for d, s in ((1000, 3), (65, 1), (2049, 3), (7, 3), (997, 1000), (16384, 16383))}
    print(f"[transfer cases] positions of an axis that change when u - 0.5 is fused, (dst, src): old {old}, new {new}")
    assert sum(old.values()) <= 1 and new[(1000, 3)] > 100 and new[(2049, 3)] > 100 and new[(65, 1)] > 10


# ---- mutants: the classes can tell a wrong kernel from a right one -----------------------------------------------------------------------
def _clamped(f):
    f = np.asarray(f, F32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(f), F32(0.0), np.minimum(np.maximum(f, F32(0.0)), F32(1.0))).astype(F32)


def _unorm_half_up(f, bits):
    return np.floor((_clamped(f) * F32(2 ** bits - 1)).astype(np.float64) + 0.5).astype(np.uint32)


def _unorm_product_in_double(f, bits):
    return np.rint(_clamped(f).astype(np.float64) * (2 ** bits - 1)).astype(np.uint32)


def _unorm_nan_is_max(f, bits, original=tr.float_to_unorm):
    return np.where(np.isnan(np.asarray(f, F32)), np.uint32(2 ** bits - 1), original(f, bits)).astype(np.uint32)


def _half_is_denormal(bits):
    return ((bits & 0x7C00) == 0) & ((bits & 0x3FF) != 0)


def _half_store_flushes(x, original=tr.float_to_half):
    b = original(x).view(np.uint16)
    return np.where(_half_is_denormal(b), b & 0x8000, b).astype(np.uint16).view(np.float16)


def _half_decode_flushes(h, original=tr.half_to_float):
    b = np.asarray(h, np.float16).view(np.uint16)
    return original(np.where(_half_is_denormal(b), b & 0x8000, b).astype(np.uint16).view(np.float16))


def _half_store_truncates(x, original=tr.float_to_half):
    x = np.asarray(x, F32)
    h = original(x)
    with np.errstate(invalid="ignore"):
        beyond = np.abs(h.astype(np.float64)) > np.abs(x.astype(np.float64))
    return np.where(beyond, h.view(np.uint16) - 1, h.view(np.uint16)).astype(np.uint16).view(np.float16)


def _half_store_saturates(x, original=tr.float_to_half):
    x = np.asarray(x, F32)
    h = original(x)
    return np.where(np.isinf(h) & np.isfinite(x), np.copysign(np.float16(65504), h), h).astype(np.float16)


def _srgb_strictly_less(x):
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        code = np.searchsorted(tr.SRGB_THRESH[1:], x, side="left")
    return np.where(np.isnan(x), 0, code).astype(np.uint32)


def _mix_skips_zero_weights(ar, a, b, t, original=tr.mix):
    return np.where(t == 0, a, original(ar, a, b, t)).astype(F32)


def _flush32(v):
    v = np.asarray(v, F32)
    return np.where((v.view(np.uint32) & 0x7F800000) == 0, np.copysign(F32(0), v), v).astype(F32)


def _mix_flushes_denormals(ar, a, b, t, original=tr.mix):
    return _flush32(original(ar, _flush32(a), _flush32(b), t))


def _avg4_flushes_denormals(a, b, c, d):
    with np.errstate(over="ignore", invalid="ignore"):
        return _flush32(_flush32(_flush32(_flush32(a) + _flush32(b)) + _flush32(_flush32(c) + _flush32(d))) * F32(0.25))


def _avg4_columns_first(a, b, c, d):
    with np.errstate(over="ignore", invalid="ignore"):
        return ((a + c) + (b + d)) * F32(0.25)


def _linear_coords_fused(dst_n, src_n):
    return fma32(np.arange(dst_n).astype(F32) + F32(0.5), F32(src_n) / F32(dst_n), F32(-0.5))


def _bilinear_columns_first(ar, t00, t10, t01, t11, wx, wy):
    return tr.mix(ar, tr.mix(ar, t00, t01, wy), tr.mix(ar, t10, t11, wy), wx)


def _mip_chain_unquantised(fmt, level0, levels=None):
    out = [np.ascontiguousarray(level0)]
    h, w = out[0].shape[:2]
    lin = tr.decode(fmt, out[0])
    for _ in range(1, tr.mip_count(w, h) if levels is None else levels):
        lin = tr.avg4(*tr.mip_taps(lin))
        out.append(tr.encode(fmt, lin))
    return out


def _mip_taps_alias_the_next_row(lin, original=tr.mip_taps):
    """below a source one texel wide the tap x + 1 is read where it would lie in memory: texel 0 of the next row"""
    a, b, c, d = original(lin)
    sh, sw = lin.shape[:2]
    if sw == 1:
        dh = max(1, sh // 2)
        y0, y1 = np.minimum(2 * np.arange(dh), sh - 1), np.minimum(2 * np.arange(dh) + 1, sh - 1)
        b, d = lin[np.minimum(y0 + 1, sh - 1)][:, [0]], lin[np.minimum(y1 + 1, sh - 1)][:, [0]]
    return a, b, c, d


def _d24_nan_is_all_ones(depth, original=tr.depth_to_d24):
    return 0xFFFFFF if np.isnan(depth) else original(depth)


# mutant -> (attribute of transfer_reference, replacement, the cases tried first)
MUTANTS = {
    "unorm_store_rounds_half_up": ("float_to_unorm", _unorm_half_up, "store_ties"),
    "unorm_product_in_double": ("float_to_unorm", _unorm_product_in_double, "store_ties"),
    "nan_stores_the_maximum_code": ("float_to_unorm", _unorm_nan_is_max, "store_ties"),
    "half_store_flushes_denormals": ("float_to_half", _half_store_flushes, "denormal_steps"),
    "half_decode_flushes_denormals": ("half_to_float", _half_decode_flushes, "denormal_steps"),
    "half_store_truncates": ("float_to_half", _half_store_truncates, "store_ties"),
    "half_overflow_saturates": ("float_to_half", _half_store_saturates, "store_ties"),
    "srgb_threshold_strictly_less": ("float_to_srgb8", _srgb_strictly_less, "store_ties"),
    "absent_alpha_is_zero": ("ABSENT_ALPHA", F32(0.0), "all_codes"),
    "zero_weight_taps_skipped": ("mix", _mix_skips_zero_weights, "non_finite"),
    "linear_coordinate_fused": ("linear_coords", _linear_coords_fused, "random"),
    "floor_is_truncation": ("floor", np.trunc, "random"),
    "columns_mixed_before_rows": ("bilinear", _bilinear_columns_first, "random"),
    "mix_flushes_fp32_denormals": ("mix", _mix_flushes_denormals, "fp32_denormals"),
    "avg4_flushes_fp32_denormals": ("avg4", _avg4_flushes_denormals, "fp32_denormals"),
    "mip_level_from_the_unquantised_level": ("mip_chain", _mip_chain_unquantised, "random"),
    "avg4_adds_columns_first": ("avg4", _avg4_columns_first, "random"),
    "one_wide_source_reads_the_next_row": ("mip_taps", _mip_taps_alias_the_next_row, "random"),
    "d24_clear_of_nan_is_all_ones": ("depth_to_d24", _d24_nan_is_all_ones, "clear"),
}
# mutants no new case distinguishes (at most two), each with its reason
EXEMPT = {}
# the mutants that change no byte of the cases tests/test_transfer_gpu.py had before this module
SURVIVE_OLD = ["avg4_flushes_fp32_denormals", "d24_clear_of_nan_is_all_ones", "half_overflow_saturates", "mix_flushes_fp32_denormals",
               "nan_stores_the_maximum_code", "one_wide_source_reads_the_next_row", "zero_weight_taps_skipped"]

NEW_CASES = (tc.STORE_TIES_BLITS + tc.CONTENT_BLITS + tc.CONTENT_MIPS + tc.DEPTH_CLEARS + tc.COLOUR_CLEARS + tc.GEOMETRY_BLITS + tc.EXTENT_MIPS
             + tc.ALL_CODES_LINEAR + tc.ALL_CODES_BLITS)


def _same(key, got, want):
    fmt = tc.destination_format(key)
    return len(got) == len(want) and all(np.array_equal(tc.canonical(fmt, g), tc.canonical(fmt, w)) for g, w in zip(got, want))


def _killer(mutant, cases, monkeypatch):
    """-> (key, differing values) of the first case whose expected bytes the mutant changes, or None"""
    attr, replacement, first = MUTANTS[mutant]
    ordered = [k for k in cases if first in (k[0], k[1])] + [k for k in cases if first not in (k[0], k[1])]
    baseline = [tc.expected(k) for k in ordered]
    monkeypatch.setattr(tr, attr, replacement)
    try:
        for key, want in zip(ordered, baseline):
            got = tc.expected.__wrapped__(key)
            if not _same(key, got, want):
                fmt = tc.destination_format(key)
                return key, sum(int((tc.canonical(fmt, g) != tc.canonical(fmt, w)).sum()) for g, w in zip(got, want))
    finally:
        monkeypatch.undo()
    return None


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_wrong_rule_changes_an_expected_byte_of_a_new_case(mutant, monkeypatch):
    killed_by = _killer(mutant, NEW_CASES, monkeypatch)
    if mutant in EXEMPT:
        print(f"[transfer mutant] {mutant}: survives, exempt: {EXEMPT[mutant]}")
        assert killed_by is None, f"{mutant} is listed as indistinguishable but {killed_by[0]} tells it apart"
        return
    print(f"[transfer mutant] {mutant}: " + (f"killed by {killed_by[0]} ({killed_by[1]} values differ)" if killed_by else "SURVIVES"))
    assert killed_by is not None, f"{mutant}: no new case changes a single byte"


def test_the_old_cases_let_these_mutants_through(monkeypatch):
    survivors = []
    for mutant in sorted(MUTANTS):
        killed_by = _killer(mutant, tc.OLD_CASES, monkeypatch)
        print(f"[transfer mutant, old cases] {mutant}: " + (f"killed by {killed_by[0]} ({killed_by[1]} values differ)" if killed_by else "survives"))
        if killed_by is None:
            survivors.append(mutant)
    assert survivors, "the old cases kill every mutant: the new classes add nothing"
    assert survivors == sorted(SURVIVE_OLD), survivors


def test_at_most_two_exempt_mutants():
    assert len(EXEMPT) <= 2 and set(EXEMPT) <= set(MUTANTS)
