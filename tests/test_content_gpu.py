"""The hot path on adversarial G-buffer content (tests/gbuffer_content.py): every pass fed the oracle's bytes of a frame
of only sky, of sky and geometry alternating per pixel / tile / trace block, of incoherent depth, of normals on the
octahedral seams, of material codes either side of every threshold, of velocities that leave the frame or are not
finite, of histories holding Inf / NaN / 65504 — and compared with the oracle under the rule of tests/parity.py, with
the cap of tests/test_fuzz_gpu.py.  Four views per (class, size): the chain stage by stage (and the empty-tile skips
against no skips), the trace's launch schedules, the blur's and the TAA's alternative paths, the rows either side of
the hot path.  The pre-stage bytes the product is given are the oracle's, outputs included, so a texel the oracle leaves
unwritten must be left unwritten."""
import numpy as np
import pytest

from vk_renderer_amd import abi
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PDF_LUT_SIZE, PostFxChain
from vk_renderer_amd.images import ImageBuf

import gbuffer_content as gc
from parity import ROWS, record, report
from test_parity_gpu import ALL_IMAGES, EXACT, STAGES

pytestmark = pytest.mark.gpu

SNAP = tuple(n for n in ALL_IMAGES if n != "pdf")  # the LUT never changes: uploaded once


def _cap(texels):
    # tests/test_fuzz_gpu.py: a texel may flip a hit / break decision through libm-vs-ocml ulps in the smooth part
    return max(1, int(2e-4 * texels))


def _snapshot(c):
    return {n: getattr(c, n).to_host().copy() for n in SNAP}


class Case:
    """One oracle run of the class, stage by stage: what every image held before each stage and after the last"""

    def __init__(self, name, size):
        self.name, self.size = name, size
        ref = gc.prepare(name, size)
        self.pdf = ref.pdf.to_host().copy()
        self.pre, self.post = {}, {}
        for stage, outs in STAGES:
            self.pre[stage] = _snapshot(ref)
            getattr(ref, stage)()
            self.post[stage] = {o: getattr(ref, o).to_host().copy() for o in outs}
        self.final = _snapshot(ref)
        # half-res texels holding a roughness code 0 or a depth code 0: where a filter / blur weight can be infinite or NaN
        bad = (ref.material.raw(0)[..., 1] == 0) | ((ref.depth.raw(0)[..., 0] & 0xFFFFFF) == 0)
        h2, w2 = ref.rays.height, ref.rays.width
        self.nonfinite_weight = bad[:2 * h2, :2 * w2].reshape(h2, 2, w2, 2).any(axis=(1, 3))

    def product(self):
        import torch

        assert torch.cuda.is_available()
        gpu = PostFxChain(*self.size, backend="product", device="cuda", setup=FrameSetup(*self.size))
        gpu.pdf.upload(self.pdf)
        return gpu

    def oracle(self):
        """a fresh oracle chain in the state after the last stage (the shared record itself is never run on)"""
        ref = PostFxChain(*self.size, backend="oracle", setup=FrameSetup(*self.size))
        ref.pdf.upload(self.pdf)
        load(ref, self.final)
        return ref


def load(chain, snap):
    for n in SNAP:
        getattr(chain, n).upload(snap[n])


@pytest.fixture(scope="module", params=gc.CASES, ids=[f"{n}-{s[0]}x{s[1]}" for n, s in gc.CASES])
def case(request, oracle_lib):
    return Case(*request.param)


def _bits(img, mip, host):
    r = img.raw(mip, host)
    return r.view(np.uint16) if r.dtype == np.float16 else r


def _report(what, fmt, got, ref):
    """parity.report, and more where the oracle's value is not finite: there the rule of tests/parity.py cannot tell (its
    relative bound and the fp16 storage step of an infinity are infinite, so any number passes), and the product must store
    the same thing — an infinity of the same sign for an infinity, a NaN for a NaN — as it must not store either where the
    oracle stores a number."""
    nbad, bad = report(what, fmt, got, ref)
    g, r = got.astype(np.float64), ref.astype(np.float64)
    strict = ((np.isinf(r) | np.isinf(g)) & (g != r)) | (np.isnan(r) != np.isnan(g))
    bad = bad | strict.any(axis=-1)
    if int(bad.sum()) != nbad:
        print(f"[content] {what}: {int(bad.sum()) - nbad} more texels differ in a non-finite channel")
        ROWS[-1]["outside_tolerance"] = int(bad.sum())
    return int(bad.sum()), bad


def _check_outputs(case, what, gpu, want, outs):
    """`outs` of the product against the oracle's bytes `want`: integer outputs bit for bit, the others under the cap"""
    gpu.sync()
    total = 0
    for name in outs:
        g = getattr(gpu, name)
        hg = g.to_host()
        for mip in range(g.mips):
            if name in EXACT:
                a, b = _bits(g, mip, hg), _bits(g, mip, want[name])
                if name == "depth":
                    a, b = a & 0xFFFFFF, b & 0xFFFFFF
                nbad = int((a != b).any(axis=-1).sum())
                record(f"{what}:{name}.{mip}", a.shape[0] * a.shape[1], a.shape[0] * a.shape[1] - nbad, nbad, 0.0, "bit-exact")
                assert nbad == 0, f"{case.name} {case.size} {what} {name} mip {mip}: {nbad} texels differ (integer path must be bit-exact)"
            else:
                nbad, bad = _report(f"{what}:{name}.{mip}", g.format, g.decode(mip, hg), g.decode(mip, want[name]))
                total += nbad
                where = [(int(x), int(y)) for y, x in zip(*np.nonzero(bad))][:4]
                assert nbad <= _cap(g.width * g.height), f"{case.name} {case.size} {what} {name}: {nbad} texels outside tolerance, first at (x, y) {where}"
    return total


def _near(mask, r):
    """texels within r (Chebyshev) of a set texel of `mask`"""
    h, w = mask.shape
    s = np.zeros((h + 2 * r + 1, w + 2 * r + 1), dtype=np.int64)
    s[r + 1: r + 1 + h, r + 1: r + 1 + w] = mask
    s = s.cumsum(axis=0).cumsum(axis=1)
    n = 2 * r + 1
    return (s[n:, n:] - s[:-n, n:] - s[n:, :-n] + s[:-n, :-n])[:h, :w] > 0


NO_SKIP = abi.SWITCH_FILTER_NO_SKIP | abi.SWITCH_BLUR_NO_SKIP


def test_stagewise(case, parity_table):
    """Every stage on the oracle's pre-stage bytes.  The filter and the blur restate the shaders exactly only without their
    empty-tile skips (their comments: every weight finite), so those two are held to the oracle with the skips off, and
    the skips to the no-skip run: no difference at all where no weight can be infinite or NaN, otherwise only within
    a blur radius + the filter's cross (13 half-res pixels) of a texel with roughness code 0 or depth code 0."""
    lib = abi.product()
    before = lib.vkr_get_switches()
    gpu = case.product()
    total = 0
    try:
        for stage, outs in STAGES:
            load(gpu, case.pre[stage])
            skipping = stage in ("ssr_filter", "ssr_blur")
            if skipping:
                lib.vkr_set_switches(before | NO_SKIP)
            getattr(gpu, stage)()
            total += _check_outputs(case, stage, gpu, case.post[stage], outs)
            if skipping:
                no_skip = getattr(gpu, outs[0]).raw(0).copy()
                lib.vkr_set_switches(before & ~NO_SKIP)
                load(gpu, case.pre[stage])
                getattr(gpu, stage)()
                gpu.sync()
                differ = (getattr(gpu, outs[0]).raw(0)[..., :3] != no_skip[..., :3]).any(axis=-1)
                print(f"[content] {case.name} {case.size} {stage}: skip vs no-skip differ in {int(differ.sum())} texels")
                if case.name in gc.SKIP_EXACT:
                    assert not case.nonfinite_weight.any(), "the class was to hold no roughness code 0 and no depth code 0"
                    assert not differ.any(), f"{stage}: the empty-tile skip changed {int(differ.sum())} texels of a frame whose weights are all finite"
                else:
                    assert not (differ & ~_near(case.nonfinite_weight, 13)).any(), f"{stage}: skip and no-skip differ away from every non-finite weight"
    finally:
        lib.vkr_set_switches(before)
    print(f"[content] {case.name} {case.size} stagewise: texels outside tolerance over all stages: {total}")


def test_trace_schedules(case):
    """vkr_sssr_trace_split with 0..4 compacted rounds in the head launch against the single launch: `rays` and `raw` byte
    for byte, texels neither schedule writes included (both images start as 0x5A).  The parked-ray queue sees no ray,
    every ray, and rays in every second pixel / tile / block."""
    gpu = case.product()
    load(gpu, case.pre["ssr_trace"])

    def run(split):
        for img in (gpu.rays, gpu.raw):
            img.upload(np.full(img.nbytes, 0x5A, dtype=np.uint8))
        gpu.ssr_trace(split=split)
        gpu.sync()
        return gpu.rays.to_host().copy(), gpu.raw.to_host().copy()

    want_rays, want_raw = run(None)
    for rounds in (0, 1, 2, 3, 4):
        rays, raw = run(rounds)
        assert np.array_equal(rays, want_rays), f"{case.name} {case.size}: rays differ with {rounds} rounds in the head launch"
        assert np.array_equal(raw, want_raw), f"{case.name} {case.size}: raw differs with {rounds} rounds in the head launch"


def test_path_switches(case, parity_table):
    """The blur's three tap loops (wave-uniform sigma where a ballot finds one, rows, per-lane loops) and the TAA's two
    footprint instantiations, each against the oracle; the blur images among themselves within one UNORM8 code.  The
    blur runs without its empty-tile skip, as in test_stagewise: the oracle is its reference only then."""
    lib = abi.product()
    before = lib.vkr_get_switches()
    gpu = case.product()
    images = {}
    try:
        clear = (before | NO_SKIP) & ~(abi.SWITCH_BLUR_GENERIC | abi.SWITCH_BLUR_LANE_LOOPS)
        for path, bits in (("default", 0), ("generic", abi.SWITCH_BLUR_GENERIC), ("lane_loops", abi.SWITCH_BLUR_GENERIC | abi.SWITCH_BLUR_LANE_LOOPS)):
            lib.vkr_set_switches(clear | bits)
            load(gpu, case.pre["ssr_blur"])
            gpu.ssr_blur()
            _check_outputs(case, f"blur[{path}]", gpu, case.post["ssr_blur"], ("blurred",))
            images[path] = gpu.blurred.raw(0).astype(np.int32)
        for generic in (False, True):
            lib.vkr_set_switches((before | abi.SWITCH_TAA_GENERIC) if generic else (before & ~abi.SWITCH_TAA_GENERIC))
            load(gpu, case.pre["taa"])
            gpu.taa()
            _check_outputs(case, f"taa[generic={generic}]", gpu, case.post["taa"], ("taa_target",))
    finally:
        lib.vkr_set_switches(before)
    for a, b in (("default", "generic"), ("generic", "lane_loops"), ("default", "lane_loops")):
        d = np.abs(images[a] - images[b])
        print(f"[content] {case.name} {case.size} blur {a} vs {b}: {int((d != 0).any(axis=-1).sum())} texels differ, max {int(d.max())} code")
        assert int(d.max()) <= 1


_BRDF = {}


def test_widened_rows(case, parity_table):
    """The rows either side of the hot path (tests/test_fuzz_gpu.py::test_random_parameters_widened_rows) with fixed
    parameters; the classification with max_roughness 0.7 and glossy_value 0.5, which material_extremes straddles."""
    ref, gpu = case.oracle(), case.product()
    load(gpu, case.final)
    if "host" not in _BRDF:  # the split-sum LUT depends on nothing of the frame: restated once
        ref.preintegrate_brdf()
        _BRDF["host"] = ref.brdf.to_host().copy()
    for c in (ref, gpu):
        c.brdf = ImageBuf(abi.FMT_RG16_SFLOAT, PDF_LUT_SIZE, PDF_LUT_SIZE, device=c.device)
        c.brdf.upload(_BRDF["host"])

    def check(what, name):
        gpu.sync()
        r, g = getattr(ref, name), getattr(gpu, name)
        nbad, bad = _report(what, r.format, g.decode(), r.decode())
        where = [(int(x), int(y)) for y, x in zip(*np.nonzero(bad))][:4]
        assert nbad <= _cap(r.width * r.height), f"{case.name} {case.size} {what}: {nbad} texels outside tolerance, first at (x, y) {where}"

    angle = 0.3125
    ref.gtao_main_graphics(angle_offset=angle)
    gpu.gtao_main_graphics(angle_offset=angle)
    check("gtao_graphics", "raw")
    for c in (ref, gpu):
        c._layer_descs(2)
    ref.deinterleave_depth(2)
    gpu.deinterleave_depth(2)
    gpu.sync()
    for lr, lg in zip(ref.deint_layers, gpu.deint_layers):
        assert np.array_equal(lg.raw(0).view(np.uint32), lr.raw(0).view(np.uint32)), "deinterleaved depth layers must be bit-exact"
    ref.gtao_main_deinterleaved(layer=6, angle_offset=angle)
    gpu.gtao_main_deinterleaved(layer=6, angle_offset=angle)
    check("gtao_deinterleaved", "raw")
    # ScreenSpaceTrace
    st = dict(angle_offset=0.4375, random_offset=0.625)
    ref.screen_trace(**st)
    gpu.screen_trace(**st)
    check("screen_trace", "st_raw")
    gpu.st_raw.copy_from(ref.st_raw)
    ref.screen_trace_filter()
    gpu.screen_trace_filter()
    check("screen_trace_filter", "st_filtered")
    gpu.st_filtered.copy_from(ref.st_filtered)
    ref.screen_trace_accumulate()
    gpu.screen_trace_accumulate()
    check("screen_trace_accumulate", "st_accumulated")
    # simple SSR and the deferred-shading composite
    ref.ssr_simple()
    gpu.ssr_simple()
    check("ssr_simple", "ssr_out")
    sh = dict(min_roughness=0.1, max_roughness=0.7, show_ao=0)
    ref.shading(**sh)
    gpu.shading(**sh)
    check("shading", "color_out")
    # tile classification (sets and counts) + indirect trace
    cl = dict(max_roughness=0.7, glossy_value=0.5)
    ref.ssr_classify(**cl)
    gpu.ssr_classify(**cl)
    gpu.sync()
    for kind in ("reflective", "glossy"):
        nr = int(ref.buffer_to_host(getattr(ref, kind + "_args"))[0])
        ng = int(gpu.buffer_to_host(getattr(gpu, kind + "_args"))[0])
        assert nr == ng, f"{case.name} {case.size}: {kind}_tiles count {ng} != {nr}"
        assert set(ref.buffer_to_host(getattr(ref, kind + "_tiles"))[:nr].tolist()) == set(gpu.buffer_to_host(getattr(gpu, kind + "_tiles"))[:ng].tolist())
        print(f"[content] {case.name} {case.size} {kind} tiles {nr}")
    ref.ssr_trace_indirect(frame_random=5, max_roughness=0.7)
    gpu.ssr_trace_indirect(frame_random=5, max_roughness=0.7)
    check("trace_indirect", "rays")
    # static AO reprojection (tests/test_variants_gpu.py): half of the frame keeps its depth, the history is random
    # (first the chain's own main pass without MIS — the configuration that stores the bare arc — on the same frame)
    for c in (ref, gpu):
        c.setup.use_mis = 0
    for n in SNAP:
        getattr(gpu, n).copy_from(getattr(ref, n))
    ref.gtao_main()
    gpu.gtao_main()
    check("gtao_main[non-MIS]", "raw")
    ref.gtao_filter()
    cur, prev = ref.depth.to_host().copy(), ref.prev_depth.to_host().copy()
    prev[: len(prev) // 2] = cur[: len(cur) // 2]
    ref.prev_depth.upload(prev)
    for c in (ref, gpu):
        c._half_img(abi.FMT_R16_SFLOAT, "ao_prev_frame")
        c._half_img(abi.FMT_R16_SFLOAT, "ao_output")
    hist = ref.ao_prev_frame.to_host()
    h16 = hist.view(np.uint16)
    h16[:] = np.random.default_rng(5).integers(0, 0x3C00, size=h16.shape, dtype=np.uint16)  # fp16 codes in [0, 1)
    ref.ao_prev_frame.upload(hist)
    for n in SNAP:
        getattr(gpu, n).copy_from(getattr(ref, n))
    gpu.ao_prev_frame.copy_from(ref.ao_prev_frame)
    ref.gtao_reproject()
    gpu.gtao_reproject()
    check("gtao_reproject", "ao_output")
