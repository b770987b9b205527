"""The degenerate extents of tests/degenerate_extents.py on the CPU oracle alone: conditions on the reference that keep
tests/test_degenerate_extents_gpu.py from passing vacuously.  Under stage_noise every non-integer stage output holds many
different texels; what the floored 8 x 4 dispatches (gtao_main, gtao_filter and the variants built on the same dispatch)
leave unwritten is on record, so the GPU test has a stated expectation; the SSAO restatement on a depth one texel wide or
high still produces many different sample counts."""
import functools

import numpy as np
import pytest

from vk_renderer_amd import abi

import degenerate_extents as de
import ssao_reference as ssao_ref

SIZE_IDS = [f"{w}x{h}" for w, h in de.SIZES]


@functools.lru_cache(maxsize=None)
def _case(name, size):
    return de.Case(name, size)


def test_sizes_are_what_they_claim():
    """the table of the helper: which sizes have a zero floor-dispatch extent, one group, the smallest ragged dispatch"""
    half = {s: (s[0] // 2, s[1] // 2) for s in de.SIZES}
    assert [s for s in de.SIZES if de.zero_dispatch(s)] == [(2, 2), (2, 130), (130, 2), (4, 4), (6, 10), (14, 34), (34, 6)]
    assert de.floor_extent(*half[(14, 34)]) == (0, 16) and de.floor_extent(*half[(34, 6)]) == (16, 0) and de.floor_extent(*half[(6, 10)]) == (0, 4)
    assert de.floor_extent(*half[(16, 8)]) == half[(16, 8)] == (8, 4)
    assert de.floor_extent(*half[(18, 10)]) == (8, 4) and half[(18, 10)] == (9, 5)
    assert all(w % 2 == 0 and h % 2 == 0 and w * h <= 476 for w, h in de.SIZES)  # HostFrame and the chain take even extents


@pytest.mark.parametrize("size", de.SIZES, ids=SIZE_IDS)
def test_stage_noise_is_not_vacuous(size, oracle_lib):
    """Among the texels a stage writes, at least a third hold pairwise distinct values whenever there are 8 or more.
    Measured with this seeding: reflections 44/45 .. 118/119, blurred 49/51 .. all, acc_ao and taa_target all, rays all,
    raw 60/65 .. all, filtered 24/32 at 16 x 8 and 22/32 at 18 x 10.  A third leaves room for another seed."""
    c = _case("stage_noise", size)
    for stage, outs in de.STAGES:
        for o in outs:
            if o in de.EXACT:
                continue
            img = getattr(c.ref, o)
            sel = de.texels(img, 0, c.post[stage][o])[de.written(stage, img.width, img.height)]
            distinct = len(np.unique(sel, axis=0)) if len(sel) else 0
            print(f"[degenerate] stage_noise {size} {stage}:{o}: {distinct} distinct of {len(sel)} written texels")
            if len(sel) >= 8:
                assert 3 * distinct >= len(sel), f"{stage}: `{o}` holds {distinct} distinct texels of {len(sel)}"


@pytest.mark.parametrize("name,size", de.CASES, ids=de.IDS)
def test_floor_dispatch_leaves_the_rest_unwritten(name, size, oracle_lib):
    """gtao_main and gtao_filter leave every byte outside their floor-dispatch extent as it was: all of `raw` and `filtered`
    at the sizes with a zero extent, column 8 and row 4 at 18 x 10, nothing at 16 x 8.  Every other stage may write anywhere."""
    c = _case(name, size)
    for stage, out in (("gtao_main", "raw"), ("gtao_filter", "filtered")):
        img = getattr(c.ref, out)
        before, after = c.pre[stage][out], c.post[stage][out]
        keep = ~de.written(stage, img.width, img.height)
        if de.zero_dispatch(size):
            assert keep.all() and np.array_equal(before, after), f"{stage} wrote `{out}` on a zero dispatch extent"
        assert np.array_equal(de.texels(img, 0, before)[keep], de.texels(img, 0, after)[keep]), f"{stage}: texels outside the dispatch extent changed"
        if size == (18, 10):
            assert keep[:, 8].all() and keep[4, :].all() and int(keep.sum()) == 13
        if size == (16, 8):
            assert not keep.any()


def _fill(img):
    img.host[:] = 0x5A


def _unwritten(img):
    return (de.texels(img, 0, img.host) == 0x5A).all(axis=-1)


@pytest.mark.parametrize("size", de.SIZES, ids=SIZE_IDS)
def test_variants_on_the_floor_dispatch(size, oracle_lib):
    """gtao_reproject, gtao_main_deinterleaved (half-res) and the screen-trace filter and accumulate (full-res) run the same
    floored 8 x 4 dispatch: with the output pre-filled, exactly the texels outside it keep the fill — the whole image on a
    zero extent.  (The fill is no value these passes store for these inputs: a written texel always changes.)"""
    c = de.prepare("stage_noise", size)
    c.downsample()
    w2, h2 = c.raw.width, c.raw.height
    # reprojection
    c.gtao_main()
    c.gtao_filter()
    de.seed_stage(c, "gtao_accumulate", size)  # `filtered` as noise: every texel a number
    c._half_img(abi.FMT_R16_SFLOAT, "ao_prev_frame")
    _fill(c._half_img(abi.FMT_R16_SFLOAT, "ao_output"))
    c.gtao_reproject()
    fw, fh = de.floor_extent(w2, h2)
    want = np.ones((h2, w2), dtype=bool)
    want[:fh, :fw] = False
    assert np.array_equal(_unwritten(c.ao_output), want), "gtao_reproject"
    # deinterleaved main pass, pattern 2 x 2 (layers of half the half-res extent, so only where that is not empty)
    if w2 >= 2 and h2 >= 2:
        c._layer_descs(1)
        c.deinterleave_depth(1)
        _fill(c.raw)
        c.gtao_main_deinterleaved(layer=2, pattern_n=1)  # offset (0, 1)
        want = np.ones((h2, w2), dtype=bool)
        for iy in range(fh):
            for ix in range(fw):
                if 2 * ix < w2 and 2 * iy + 1 < h2:
                    want[2 * iy + 1, 2 * ix] = False
        assert np.array_equal(_unwritten(c.raw), want), "gtao_main_deinterleaved"
        if fw == 0 or fh == 0:
            assert want.all()
    # ScreenSpaceTrace: the filter and the accumulation, at full resolution
    W, H = size
    FW, FH = de.floor_extent(W, H)
    want = np.ones((H, W), dtype=bool)
    want[:FH, :FW] = False
    rng = np.random.default_rng([0x57A6E, 99, W, H])
    raw = c._full_img("st_raw")
    raw.set_raw(rng.random((H, W, 4), dtype=np.float32).astype(np.float16))
    _fill(c._full_img("st_filtered"))
    c.screen_trace_filter()
    assert np.array_equal(_unwritten(c.st_filtered), want), "screen_trace_filter"
    c.st_filtered.set_raw(rng.random((H, W, 4), dtype=np.float32).astype(np.float16))
    _fill(c._full_img("st_accumulated"))
    c.screen_trace_accumulate()
    assert np.array_equal(_unwritten(c.st_accumulated), want), "screen_trace_accumulate"


@pytest.mark.parametrize("extent", [(1, 37), (37, 1)], ids=["1x37", "37x1"])
def test_ssao_restatement_on_a_one_texel_wide_depth(extent):
    """the numpy restatement of the SSAO on a depth one texel wide / high (codes 0xFFFFFF - U[0, 2^16)): at least 8
    distinct sample counts (measured: see the printed figure), so the bit-for-bit GPU comparison compares something"""
    w, h = extent
    depth, setup, samples = de.ssao_case(w, h)
    ar = ssao_ref.Arith(int(abi.product().vkr_numeric_contract()))
    codes, counts = ssao_ref.ssao(ar, depth, setup.proj, *setup.fazz, samples, w, h)
    ks = np.unique(counts)
    print(f"[degenerate] ssao {w}x{h}: distinct counts {len(ks)} ({ks.tolist()})")
    assert np.array_equal(codes, ssao_ref.CODES[counts])
    assert len(ks) >= 8
