"""The content classes of tests/gbuffer_content.py on the CPU oracle alone: the generators are frozen, the oracle is
deterministic on them whatever its thread count, no class is silently empty, and which texels every pass leaves
unwritten on a frame of only sky is on record (tests/test_content_gpu.py holds the kernels to the same)."""
import functools
import hashlib

import numpy as np
import pytest

import gbuffer_content as gc

STAGES = [("downsample", ("depth", "dn", "dv")), ("ssr_trace", ("rays", "raw")), ("ssr_filter", ("reflections",)), ("ssr_blur", ("blurred",)),
          ("gtao_main", ("raw",)), ("gtao_filter", ("filtered",)), ("gtao_accumulate", ("acc_ao",)), ("taa", ("taa_target",))]

# Measured on the oracle, one frame() on the prepared chain: share of `reflections` texels with a non-zero colour, share
# of `raw` texels whose AO channel is below 1 (a sky texel stores 0 there under MIS), number of distinct `filtered`
# codes, number of output texels holding a non-finite value (summed over the fp16 outputs).  The inputs are frozen, so
# the floors asserted below are half of these: they only guard against a class silently becoming empty.
MEASURED = {
    ("sky_all", (70, 38)): (0.0, 1.0, 46, 0),                  ("sky_all", (206, 226)): (0.0, 1.0, 196, 0),
    ("near_all", (70, 38)): (0.0, 0.7955, 454, 0),             ("near_all", (206, 226)): (0.0, 0.7726, 2005, 0),
    ("checker_px", (70, 38)): (0.0406, 0.7278, 402, 0),        ("checker_px", (206, 226)): (0.1984, 0.6523, 1328, 0),
    ("checker_tile", (70, 38)): (0.0211, 0.8436, 382, 0),      ("checker_tile", (206, 226)): (0.0430, 0.7773, 2694, 0),
    ("checker_block", (70, 38)): (0.0271, 0.8150, 330, 0),     ("checker_block", (206, 226)): (0.0367, 0.7931, 2216, 0),
    ("depth_noise", (70, 38)): (0.0195, 0.9489, 462, 0),       ("depth_noise", (206, 226)): (0.0152, 0.9822, 3034, 0),
    ("depth_stripes", (70, 38)): (0.0060, 0.8000, 419, 0),     ("depth_stripes", (206, 226)): (0.0394, 0.7594, 2351, 0),
    ("normal_noise", (70, 38)): (0.0, 0.7398, 408, 0),         ("normal_noise", (206, 226)): (0.0126, 0.7911, 1488, 0),
    ("normal_poles", (70, 38)): (0.0090, 0.7519, 400, 0),      ("normal_poles", (206, 226)): (0.0549, 0.7799, 1590, 0),
    ("material_extremes", (70, 38)): (0.1579, 0.7053, 391, 1), ("material_extremes", (206, 226)): (0.3448, 0.6592, 1357, 1),
    ("velocity_wild", (70, 38)): (0.0271, 0.7293, 401, 281),   ("velocity_wild", (206, 226)): (0.1924, 0.6519, 1322, 4734),
    ("history_nonfinite", (70, 38)): (0.0271, 0.7293, 401, 2955), ("history_nonfinite", (206, 226)): (0.1924, 0.6519, 1322, 52863),
    ("all_noise", (70, 38)): (0.0015, 0.8767, 463, 158),       ("all_noise", (206, 226)): (0.0017, 0.8769, 3540, 2688),
}

ids = [f"{n}-{s[0]}x{s[1]}" for n, s in gc.CASES]


def _output_bytes(c):
    return {n: getattr(c, n).to_host().tobytes() for n in c.OUTPUTS}


@functools.lru_cache(maxsize=None)
def _frame(name, size, threads=None):
    """One oracle frame on the class: the outputs' bytes and the non-vacuity quantities.  threads None: the oracle's default
    count, or 4 where the default is fewer (a machine with one CPU), so that it is never the single thread it is held against."""
    from oracle import binding

    lib = binding.install(build_if_missing=True)
    default = lib.vkr_ref_threads()
    if threads is None:
        threads = max(4, default)
    c = gc.prepare(name, size)
    inputs = hashlib.sha256(gc.input_bytes(c)).hexdigest()
    try:
        lib.vkr_ref_set_threads(threads)
        c.frame()
    finally:
        lib.vkr_ref_set_threads(default)
    refl = float((c.reflections.raw(0)[..., :3] != 0).any(axis=-1).mean())
    ao = float((c.raw.decode(0)[..., 0] < 1).mean())
    distinct = len(np.unique(c.filtered.raw(0).view(np.uint16)))
    nonfinite = 0
    for n in c.OUTPUTS:
        r = getattr(c, n).raw(0)
        if r.dtype == np.float16:
            nonfinite += int((~np.isfinite(r.astype(np.float32))).any(axis=-1).sum())
    return dict(threads=threads, inputs=inputs, outputs=_output_bytes(c), refl=refl, ao=ao, distinct=distinct, nonfinite=nonfinite)


def test_every_case_has_a_measurement():
    assert set(MEASURED) == set(gc.CASES)
    assert len(gc.FINITE) == 10 and len(gc.NONFINITE) == 3 and set(gc.SKIP_EXACT) <= set(gc.CLASSES)
    # 1.0 -> 254 | 255, 0.7 -> 217 | 218, 0.5 -> 187 | 188, 0.35 -> 159 | 160 (sRGB EOTF), each with its outer neighbour
    t = gc._srgb_table()
    for thr, below in ((0.7, 217), (0.5, 187), (0.35, 159)):
        assert t[below] < thr <= t[below + 1] and {below, below + 1} <= set(gc.threshold_codes())
    assert {254, 255} <= set(gc.threshold_codes())


@pytest.mark.parametrize("name,size", gc.CASES, ids=ids)
def test_generator_is_deterministic(name, size, oracle_lib):
    again = gc.prepare(name, size)
    assert hashlib.sha256(gc.input_bytes(again)).hexdigest() == _frame(name, size)["inputs"]
    if name in gc.FINITE:
        for n in ("velocity", "acc_hist", "acc_ao", "taa_hist"):
            assert np.isfinite(getattr(again, n).raw(0).astype(np.float32)).all(), f"{name}: {n} holds a non-finite value"


@pytest.mark.parametrize("name,size", gc.CASES, ids=ids)
def test_oracle_is_thread_count_independent(name, size, oracle_lib):
    one, many = _frame(name, size, 1), _frame(name, size)
    assert many["threads"] >= 4
    for n in one["outputs"]:
        assert one["outputs"][n] == many["outputs"][n], f"{name} {size}: `{n}` differs between 1 thread and {many['threads']} threads"


@pytest.mark.parametrize("name,size", gc.CASES, ids=ids)
def test_class_is_not_vacuous(name, size, oracle_lib):
    got = _frame(name, size)
    refl, ao, distinct, nonfinite = MEASURED[(name, size)]
    print(f"[content] {name} {size}: reflections {got['refl']:.4f} ao<1 {got['ao']:.4f} distinct filtered {got['distinct']} non-finite {got['nonfinite']}")
    if name in ("sky_all", "near_all"):
        assert got["refl"] == 0.0, "no ray can start on sky, none can hit behind the near plane"
    else:
        assert got["refl"] >= 0.5 * refl  # (inert for normal_noise at 70x38, which measures 0: its 206x226 case carries the floor)
    assert got["ao"] >= 0.5 * ao
    assert got["distinct"] >= 0.5 * distinct
    if name in gc.NONFINITE:
        assert got["nonfinite"] >= 0.5 * nonfinite
    elif name == "material_extremes":
        # roughness code 0 under a grazing normal (alpha2 * rcp(0) in the trace's PDF): one `raw` texel at either size, measured.
        # The inputs are frozen; twice the measured count bounds it from above as half of it bounds the other classes from below.
        assert 1 <= got["nonfinite"] <= 2 * nonfinite
    else:
        assert got["nonfinite"] == 0, "non-finite values may come out only where non-finite values went in"


def _unwritten(img, mip):
    r = img.raw(mip)
    return (r.view(np.uint8).reshape(r.shape[0], r.shape[1], -1) == 0x5A).all(axis=-1)


def _padding_untouched(img, mip):
    h = max(1, img.height >> mip)
    rows = img.host[img.offset[mip]: img.offset[mip] + img.pitch[mip] * h].reshape(h, img.pitch[mip])
    return bool((rows[:, max(1, img.width >> mip) * img.bpp:] == 0x5A).all())


@pytest.mark.parametrize("size", gc.SIZES)
def test_sky_is_left_alone(size, oracle_lib):
    """On a frame of only sky, with the outputs pre-filled with 0x5A: what a pass does not write keeps its bytes.  On
    record here: every pass of the chain writes its sky texels (zeros, AO (0, 1), the history-free resolve), over its
    whole image — except gtao_main and gtao_filter, whose floor-divided dispatch (8 x 4 groups) never reaches the ragged
    right and bottom edge; those texels must still hold 0x5A, and so must the row padding of every image."""
    c = gc.prepare("sky_all", size)
    for stage, outs in STAGES:
        for o in outs:
            img = getattr(c, o)
            img.host[img.offset[1] if o == "depth" else 0:] = 0x5A  # depth: mip 0 is the pass's input
        getattr(c, stage)()
        for o in outs:
            img = getattr(c, o)
            for mip in range(1 if o == "depth" else 0, img.mips):
                w, h = max(1, img.width >> mip), max(1, img.height >> mip)
                want = np.zeros((h, w), dtype=bool)
                if stage in ("gtao_main", "gtao_filter"):
                    want[(h // 4) * 4:, :] = True
                    want[:, (w // 8) * 8:] = True
                assert np.array_equal(_unwritten(img, mip), want), f"{stage}: `{o}` mip {mip} leaves other texels unwritten than recorded"
                assert _padding_untouched(img, mip), f"{stage}: `{o}` mip {mip}: row padding overwritten"
