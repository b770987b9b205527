"""The adversarial content of tests/side_pass_content.py on the CPU: the numpy restatements of ssao, tile_regression,
gtao_rt_main and trace_probe alone.  Two things are proven here, so that tests/test_side_pass_content_gpu.py may rely on them:
the classes reach what they are meant to reach (counters below), and they can tell a wrong kernel from a right one (mutants).

Measured (`-s` prints every figure per case; 23 tests, about 30 s in all, no restatement call above 0.6 s, so no size was reduced):

ssao, 10 depth classes x 3 extents x 2 sample sets.  near_all under the eye_plane samples has non-finite sample coordinates
with depth code 0 as it is (view z = -znear exactly, sample 0 = (0, 0, 1) puts pos.z = 0 and clip.w = 0): 2660 of 42 560 taps at
70 x 38, 777 of 12 432 at 35 x 19 -> 37 x 21, 15 of 240 at 1 x 19 -> 5 x 3, one per pixel; 0 under the fixed samples and in every
other class of the issue.  near_codes (codes 0 .. 3, added here) mixes them with huge finite coordinates, clip.w being one or
two float steps of 0.05 away from 0: 653 / 150 / 0 non-finite taps.

tile_regression, 9 classes x 3 views x 2 cameras, 486 tiles: 480 finite planes, 6 with a NaN, 6 with a residual of exactly 1e10.
Every NaN plane lies in the 33 x 9 view under the frame's camera (raster, stencil_noise, checker_tile, depth_stripes one tile
each, depth_noise two): no D24 content reaches the NaN branch at these extents except through a rank-deficient partial tile, so
that view is what holds the branch.  All sky, all near plane and the checkers give finite planes in every tile.

gtao_rt_main, 11 classes x 2 extents x 2 rotations x 2 scenes; the scene is procedural_scene(detail=16), 3076 triangles, one
restatement call at 35 x 19 takes 0.6 s at most.  Partly occluded live pixels over the four (extent, rotation) cases: raster 339,
depth_noise 4, normal_noise 1189, normal_poles 1171, checker_px 163, checker_tile 181, checker_tile8 154, depth_stripes 102;
near_all and sky_all 0; the empty structure occludes nothing.

trace_probe, 18 (G-buffer, probe) cases x 2 extents x 3 grids, restatement 0.26 s at most at 70 x 38 (that size is kept).  Over
the set: 72 122 HIT, 8 455 MISS, 34 392 UNKNOWN, 47 997 pixels with more than one probe traced.  short_chain fetches past its
last mip in every case (10 193 lanes on raster at 70 x 38, grid 4; 28 986 under depth_noise); the 6-mip room is climbed past as
well (408).  Uniform 16-bit noise in the probe depth ended every march at its first step and made noise_pyramid and
independent_mips the same image, so their codes are drawn where the rays are (side_pass_content._probe_noise).

Mutants: every one of the issue's list is killed or exempt, one exemption per pass at most.  Two findings about the classes:
short_chain on the raster G-buffer alone does not tell "past the last mip reads the last mip's texel" from "reads 0" (the rays
that differ end as MISS or UNKNOWN either way and store 0), so short_chain carries noise colour and also runs under near_all,
depth_noise and depth_stripes, each of which changes 1 .. 4 texels; and the NaN-propagating min / max is killed through the
segment sort and its clamps (a NaN tmin handed on by the probe before) - taken site by site, the march's t_min and the
start-probe clamp never see a NaN operand from legal texels (the march's operands are finite unless the whole ray is NaN, and
then `surface_z > position.z` is false and t_min is not used; the world position of a live pixel is finite).  Exempt:
ssao / f2i_nan_saturates and trace_probe / f2i_index_nan_saturates, for the reasons in EXEMPT.
"""
import time

import numpy as np
import pytest

import gtao_rt_reference as gtao_ref
import probe_reference as probe_ref
import side_pass_content as sp
import ssao_reference as ssao_ref
import tile_regression_reference as tile_ref

F32 = np.float32
SKY = sp.SKY


# ---- the classes reach what they are meant to reach -------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sp.SSAO_SAMPLE_SETS)
@pytest.mark.parametrize("sizes", sp.SSAO_SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}_out_{s[1][0]}x{s[1][1]}")
def test_ssao_classes(sizes, which):
    """near_all under the eye_plane samples puts a sample on the eye plane: depth code 0 is view z = -znear = -0.05 exactly and
    sample 0 = (0, 0, 1) adds 0.05, so clip.w = -pos.z = 0 and the division gives infinities and NaNs (depth code 0 does it as it
    is: no other code had to be searched for)"""
    depth_size, out_size = sizes
    for name in sp.SSAO_CLASSES:
        t0 = time.perf_counter()
        codes, counts, stats = sp.ssao_expected(name, depth_size, out_size, which)
        print(f"[side ssao] {name} depth {depth_size} out {out_size} {which}: non-finite sample_uv {stats['nonfinite_sample_uv']}, offscreen "
              f"{stats['offscreen_taps']} of {stats['taps']} taps, counts {np.unique(counts).tolist()}, {time.perf_counter() - t0:.2f} s")
        assert codes.shape == (out_size[1], out_size[0])
        if name == "near_all":
            assert (stats["nonfinite_sample_uv"] > 0) == (which == "eye_plane"), "near_all reaches the eye plane under the eye_plane samples only"
    assert np.array_equal(sp.ssao_expected("stencil_noise", depth_size, out_size, which)[0], sp.ssao_expected("raster", depth_size, out_size, which)[0])
    words = sp.inputs("ssao", "stencil_noise", depth_size)[0]
    assert len(np.unique(words >> 24)) > min(words.size, 256) // 3, "the stencil bytes vary"


def test_tile_regression_classes():
    """over the class set: tiles with finite planes, tiles with a NaN in the plane, tiles with a residual of exactly 1e10"""
    total = np.zeros(3, np.int64)
    nan_outside_33x9 = 0
    for size in sp.TILE_SIZES:
        for cam in sp.TILE_CAMERAS:
            for name in sp.DEPTH_CLASSES:
                want = sp.tile_expected(name, size, cam)
                c = sp.tile_counts(want)
                print(f"[side tile_regression] {name} view {size} {cam}: finite {c[0]}, NaN {c[1]}, residual 1e10 {c[2]} of {want.shape[0] * want.shape[1]} tiles")
                total += c
                if size != (33, 9):
                    nan_outside_33x9 += c[1]
            a, b = sp.tile_expected("stencil_noise", size, cam), sp.tile_expected("raster", size, cam)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    print(f"[side tile_regression] over the class set: finite {total[0]}, NaN {total[1]}, residual 1e10 {total[2]}; NaN planes outside the 33 x 9 view {nan_outside_33x9}")
    assert (total > 0).all(), total


def _ao_partly(want):
    """live pixels that are neither 0 nor the open-hemisphere value (a float16 step below it or less counts as open)"""
    occ = want[..., 0].astype(F32)
    live = want[..., 1] == 1
    return live & (occ > 0) & (occ < F32(sp.ao_open_hemisphere()) * F32(0.995))


def test_traced_ao_classes():
    partly = {n: 0 for n in sp.CLASSES}
    for size in sp.AO_SIZES:
        for rotation in sp.AO_ROTATIONS:
            for name in sp.CLASSES:
                t0 = time.perf_counter()
                want = sp.ao_expected(name, size, rotation, "scene")
                words, codes = sp.inputs("gtao_rt", name, size, 1)[:2]
                sky = np.all(want == np.array([0, 1, 0, 0], np.float16), axis=-1)
                n = int(_ao_partly(want).sum())
                partly[name] += n
                print(f"[side gtao_rt] {name} {size} rotation {rotation}: partly occluded {n}, black {int((want[..., 0] == 0).sum() - sky.sum())}, "
                      f"sky {int(((words & SKY) == SKY).sum())} of {want.shape[0] * want.shape[1]} pixels, {time.perf_counter() - t0:.2f} s")
                if name == "sky_all":
                    assert sky.all()
                assert not _ao_partly(sp.ao_expected(name, size, rotation, "empty")).any(), "nothing occludes in the empty structure"
            assert np.array_equal(sp.ao_expected("stencil_noise", size, rotation, "scene"), sp.ao_expected("raster", size, rotation, "scene"))
    print(f"[side gtao_rt] {len(sp.ao_triangles('scene'))} triangles; partly occluded pixels per class: {partly}")
    for name in ("raster", "depth_noise", "normal_noise"):
        assert partly[name] > 0, name
    # normal_poles: every one of the six codes occurs in the footprint of a live pixel (the normal has twice the extent; a pixel
    # centre falls between four texels)
    size = sp.AO_SIZES[0]
    words, codes = sp.inputs("gtao_rt", "normal_poles", size, 1)[:2]
    live = (words & SKY) != SKY
    seen = set()
    for oy in (0, 1):
        for ox in (0, 1):
            seen |= set(np.unique(codes[oy::2, ox::2][live]).tolist())
    assert seen == {0, 1, 32767, 32768, 65534, 65535}, seen
    # checker_px: retired and walking waves alternate pixel by pixel, so every block of four holds both
    words = sp.inputs("gtao_rt", "checker_px", size, 1)[0].reshape(-1)
    blocks = ((words[: words.size // 4 * 4] & SKY) == SKY).reshape(-1, 4)
    assert (blocks.any(axis=1) & ~blocks.all(axis=1)).mean() > 0.9


def test_probe_trace_classes():
    seen = {"HIT": 0, "MISS": 0, "UNKNOWN": 0, "traced>1": 0}
    for size in sp.PROBE_SIZES:
        for grid, layers in sp.GRIDS:
            for gname, pname in sp.PROBE_CASES:
                t0 = time.perf_counter()
                out, result, traced, past = sp.probe_expected(gname, size, pname, grid, layers)
                c = {"HIT": int((result == probe_ref.HIT).sum()), "MISS": int((result == probe_ref.MISS).sum()),
                     "UNKNOWN": int((result == probe_ref.UNKNOWN).sum()), "traced>1": int((traced > 1).sum())}
                print(f"[side trace_probe] {gname} / {pname} {size} grid {grid} ({layers} layers): {c}, sky {int((result == -1).sum())}, "
                      f"fetches past the last mip {past}, {time.perf_counter() - t0:.2f} s")
                for k in seen:
                    seen[k] += c[k]
                if pname == "short_chain":
                    assert past > 0, "no lane climbs past the last of the 3 mips"
                if gname == "sky_all":
                    assert (out == 0).all() and (result == -1).all()
                if pname == "colour_noise":  # the bilinear filter of noise: a hit's texel is (almost) never one stored code
                    assert len(np.unique(out.reshape(-1, 4), axis=0)) > (result == probe_ref.HIT).sum() // 2
            a, b = sp.probe_expected("stencil_noise", size, "room", grid, layers), sp.probe_expected("raster", size, "room", grid, layers)
            assert np.array_equal(a[0], b[0])
    print(f"[side trace_probe] over the class set: {seen}")
    assert all(v > 0 for v in seen.values()), seen
    # independent_mips is no min-pyramid, and it sends the march somewhere else than the min-pyramid of the same noise would
    grid, layers = sp.GRIDS[0]
    assert not np.array_equal(sp.probe_expected("raster", sp.PROBE_SIZES[0], "independent_mips", grid, layers)[0],
                              sp.probe_expected("raster", sp.PROBE_SIZES[0], "noise_pyramid", grid, layers)[0])


# ---- the classes can tell a wrong kernel from a right one -------------------------------------------------------------------------
def _d24_with_stencil(bits):
    """d24_to_float without the mask: the top byte is part of the number"""
    x = np.asarray(bits).astype(np.uint32).astype(F32) * F32(2.0 ** -24)
    return gtao_ref.fma32(x, np.array([0x33800001], np.uint32).view(F32)[0], x)


def _f2i_nan_saturates(x):
    lim = 1073741824.0
    with np.errstate(invalid="ignore"):
        c = np.clip(np.nan_to_num(np.asarray(x, F32).astype(np.float64), nan=lim, posinf=lim, neginf=-lim), -lim, lim)
    return np.trunc(c).astype(np.int64)


def _f2i_index_nan_saturates(x):
    with np.errstate(invalid="ignore"):
        t = np.where(np.isnan(x), F32(np.inf), np.trunc(x)).astype(np.float64)
    return np.clip(t, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


class _StrictGe(np.ndarray):
    """a depth that answers `d >= 1.0` with `d > 1.0`: the sky test of a kernel that lets d == 1.0 through.  The restatements
    write the test inline, so the mutant hands them their sampled depth as this type; every other use of it goes through
    np.asarray and sees the plain numbers."""

    def __ge__(self, other):
        return np.asarray(self) > other


def _sample_strict_sky(ar, img, uv_x, uv_y, lerp_channels, original=gtao_ref.sample):
    out = original(ar, img, uv_x, uv_y, lerp_channels)
    return out.view(_StrictGe) if lerp_channels == 1 else out


class _NanPropagatingNp:
    """numpy with minimum / maximum where the restatement asks for fmin / fmax"""

    fmin, fmax = staticmethod(np.minimum), staticmethod(np.maximum)

    def __getattr__(self, name):
        return getattr(np, name)


def _fetch_last_mip(self, px, py, layer, mip, original=probe_ref.ProbeArrays.fetch):
    """a fetch past the last mip returns the last mip's texel instead of 0"""
    return original(self, px, py, layer, np.minimum(mip, self.mips - 1))


def _sequential_sum(v):
    """the 64 lanes added one after another instead of by the tree"""
    s = np.asarray(v)
    acc = s[:, 0].copy()
    for i in range(1, s.shape[1]):
        acc = acc + s[:, i]
    return acc


def _sample_depth_nan_visible(ar, depth, uv_x, uv_y, original=ssao_ref.sample_depth):
    """the compare `ndc.z < sample + 1e-7` written so that a NaN sample passes it (e.g. as !(ndc.z >= ...))"""
    out = original(ar, depth, uv_x, uv_y)
    return np.where(np.isnan(out), F32(np.inf), out).astype(F32)


# pass -> mutant -> (module, attribute, replacement)
MUTANTS = {
    "ssao": {
        "stencil_not_masked": (ssao_ref, "d24_to_float", _d24_with_stencil),
        "f2i_nan_saturates": (ssao_ref, "f2i", _f2i_nan_saturates),
        "nan_sample_counts_as_visible": (ssao_ref, "sample_depth", _sample_depth_nan_visible),
    },
    "tile_regression": {
        "stencil_not_masked": (tile_ref, "d24_to_float", _d24_with_stencil),
        "nan_residual_not_applied": (tile_ref, "NAN_RESIDUAL", np.nan),
        "sums_in_lane_order": (tile_ref, "tree_sum", _sequential_sum),
    },
    "gtao_rt": {
        "stencil_not_masked": (gtao_ref, "d24_to_float", _d24_with_stencil),
        "sky_test_greater_than": (gtao_ref, "sample", _sample_strict_sky),
    },
    "trace_probe": {
        "stencil_not_masked": (probe_ref, "d24_to_float", _d24_with_stencil),
        "sky_test_greater_than": (probe_ref, "sample", _sample_strict_sky),
        "f2i_index_nan_saturates": (probe_ref, "f2i_index", _f2i_index_nan_saturates),
        "min_max_propagate_nan": (probe_ref, "np", _NanPropagatingNp()),
        "fetch_past_last_mip_reads_last_mip": (probe_ref.ProbeArrays, "fetch", _fetch_last_mip),
    },
}
# mutants no legal input distinguishes, at most one per pass, each with its reason
EXEMPT = {
    ("ssao", "f2i_nan_saturates"): "f2i only sees floor(x) of a texel coordinate x; where that is NaN (or x infinite) the weight x - floor(x) is NaN "
                                   "too, every D24 texel decodes to a finite number, so the sample is NaN whichever texels the index picks and "
                                   "the compare is false.",
    ("trace_probe", "f2i_index_nan_saturates"): "a NaN coordinate reaches the fetches only in a ray that is NaN as a whole (a NaN tmin handed on by the "
                                                "probe before): its march position is NaN, `surface_z > position.z` is false whatever was fetched, and "
                                                "the bilinear depth has a NaN weight; the stop is NaN, no compare holds, the result is MISS.",
}


def _same(a, b):
    if a.dtype.kind == "f":
        bits = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
        return bool(((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))).all())
    return np.array_equal(a, b)


def _cases(pass_name):
    """-> [(label, cached expectation, the same computed afresh)] of every case of the pass, the likeliest killers first"""
    out = []
    if pass_name == "ssao":
        order = ["near_all", "stencil_noise"] + [n for n in sp.SSAO_CLASSES if n not in ("near_all", "stencil_noise")]
        for which in reversed(sp.SSAO_SAMPLE_SETS):
            for name in order:
                for ds, os_ in sp.SSAO_SIZES:
                    a = (name, ds, os_, which)
                    out.append((a, lambda a=a: sp.ssao_expected(*a)[0], lambda a=a: sp.ssao_expected.__wrapped__(*a)[0]))
    elif pass_name == "tile_regression":
        for size in reversed(sp.TILE_SIZES):
            for name in ["stencil_noise"] + [n for n in sp.DEPTH_CLASSES if n != "stencil_noise"]:
                for cam in sp.TILE_CAMERAS:
                    a = (name, size, cam)
                    out.append((a, lambda a=a: sp.tile_expected(*a), lambda a=a: sp.tile_expected.__wrapped__(*a)))
    elif pass_name == "gtao_rt":
        for name in ["stencil_noise", "sky_all", "checker_px"] + [n for n in sp.CLASSES if n not in ("stencil_noise", "sky_all", "checker_px")]:
            for size in reversed(sp.AO_SIZES):
                a = (name, size, 0.3, "scene")
                out.append((a, lambda a=a: sp.ao_expected(*a), lambda a=a: sp.ao_expected.__wrapped__(*a)))
    else:
        first = [("stencil_noise", "room"), ("sky_all", "room"), ("depth_stripes", "short_chain"), ("depth_noise", "room")]
        for gname, pname in first + [c for c in sp.PROBE_CASES if c not in first]:
            for size in reversed(sp.PROBE_SIZES):
                for grid, layers in sp.GRIDS:
                    a = (gname, size, pname, grid, layers)
                    out.append((a, lambda a=a: sp.probe_expected(*a)[0], lambda a=a: sp.probe_expected.__wrapped__(*a)[0]))
    return out


@pytest.mark.parametrize("pass_name,mutant", [(p, m) for p in MUTANTS for m in MUTANTS[p]])
def test_a_wrong_rule_changes_the_expected_image(pass_name, mutant, monkeypatch):
    """one helper of the restatement replaced by a plausibly wrong rule: some texel of some class must change"""
    owner, attr, replacement = MUTANTS[pass_name][mutant]
    cases = _cases(pass_name)
    baseline = [(label, cached()) for label, cached, _ in cases]
    monkeypatch.setattr(owner, attr, replacement)
    killed_by = None
    for (label, want), (_, _, fresh) in zip(baseline, cases):
        got = fresh()
        if not _same(np.asarray(got), np.asarray(want)):
            killed_by = (label, int((np.asarray(got) != np.asarray(want)).sum()))
            break
    monkeypatch.undo()
    if (pass_name, mutant) in EXEMPT:
        print(f"[side mutant] {pass_name} / {mutant}: survives, exempt: {EXEMPT[(pass_name, mutant)]}")
        assert killed_by is None, f"{pass_name} / {mutant} is listed as indistinguishable but {killed_by[0]} tells it apart"
        return
    print(f"[side mutant] {pass_name} / {mutant}: " + (f"killed by {killed_by[0]} ({killed_by[1]} values differ)" if killed_by else "SURVIVES"))
    assert killed_by is not None, f"{pass_name} / {mutant}: no class of the set changes a single texel"


def test_at_most_one_exempt_mutant_per_pass():
    for p in MUTANTS:
        assert sum(1 for (q, _) in EXEMPT if q == p) <= 1, p
