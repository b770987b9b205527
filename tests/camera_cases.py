"""Cameras other than the frozen benchmark one (vk-renderer_amd/camera.py: pitch 0, no roll, fovy 60 deg, aspect W / H, depth
range 0.05..80): named sets of FrameSetup keywords under which the parity tests run every pass that takes a camera as data, and
the texel class on which the reprojecting accumulation is ill-conditioned by construction (DESIGN_NUMERICS.md "Cameras").

A case holds only what it changes.  Angles in degrees, fovy in radians, as FrameSetup takes them.

Shared by tests/test_camera_cases.py (CPU: the oracle alone, every camera input observable, no case on a knife edge) and
tests/test_camera_cases_gpu.py (each kernel against the oracle on the oracle's pre-step bytes)."""
import functools
import math
import types

import numpy as np

from vk_renderer_amd import abi
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PDF_LUT_SIZE, PostFxChain
from vk_renderer_amd.images import ImageBuf

_case = types.MappingProxyType
CASES = types.MappingProxyType({
    # a view matrix without a row and a column of zeros and +-1: m[i][j] for m[j][i], view for transpose(inverse(view)) show
    "pitch_down": _case(dict(pitch=-35.0)),
    "pitch_down_roll": _case(dict(pitch=-35.0, roll=30.0)),
    # about half of the frame is sky
    "pitch_up": _case(dict(pitch=25.0)),
    # x and y of the view swap: an aspect applied to the wrong axis shows
    "roll_90": _case(dict(roll=90.0)),
    # tan(fovy / 2) = 0.13 and 1.73, the second above 1
    "narrow": _case(dict(fovy=math.radians(15.0))),
    "wide": _case(dict(fovy=math.radians(120.0))),
    # an aspect that is width / height of no extent the tests use
    "anamorphic": _case(dict(aspect=2.39)),
    # depth ranges: neither end is a literal of a reference shader, or only one is
    "deep_range": _case(dict(znear=0.5, zfar=5000.0)),
    "far_small": _case(dict(znear=0.05, zfar=8.0)),
    "near_small": _case(dict(znear=0.005, zfar=80.0)),
    # the previous frame pitched against the current one
    "prev_pitch": _case(dict(pitch=-20.0, prev_pitch_delta=1.5, prev_delta=(0.1, 0.05, -0.1))),
    # everything at once
    "all_moved": _case(dict(pitch=-25.0, roll=17.0, fovy=math.radians(75.0), aspect=1.6, znear=0.2, zfar=300.0,
                            prev_pitch_delta=1.0, prev_roll_delta=-0.7)),
    # what the twelve above leave as the frozen camera has it (tests/test_camera_cases.py found these unobservable without it): the
    # eye, so the translation column of the inverses; the yaw, so the entries that cos(90 deg) keeps at 1e-17; an aspect other than
    # W / H together with a previous frame far enough away for the reprojection tests of the blur and the TAA to decide
    "yaw_eye": _case(dict(eye=(-1.2, 3.0, -0.2), yaw=62.0, pitch=-15.0, roll=-40.0, aspect=1.25, prev_delta=(0.1, 0.05, -0.1),
                          prev_yaw_delta=1.0, prev_pitch_delta=-1.0)),
})

SMALL, RAGGED = (70, 38), (206, 226)  # 206x226: half-res 103x113, floor-dispatch extent 96x112
SIZES = (SMALL, RAGGED)


def setup(name, size, **more):
    """FrameSetup of case `name` ("default": the frozen camera) at `size`"""
    kw = dict(CASES[name]) if name != "default" else {}
    kw.update(more)
    return FrameSetup(*size, **kw)


class Extent(tuple):
    """(width, height) that names a camera case.  The G-buffer kits of the passes with exact restatements (tests/
    side_pass_content.py, tests/test_shadow_mask_rt_gpu.py and its kin) cache their inputs and expectations by size; an Extent is
    a size that compares and hashes together with its case, so the same kits serve under every camera, with frame_setup() where
    they build their FrameSetup and nothing else changed."""

    def __new__(cls, size, case):
        self = super().__new__(cls, size)
        self.case = case
        return self

    def __eq__(self, other):
        return tuple.__eq__(self, other) and getattr(other, "case", None) == self.case

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((tuple(self), self.case))


def frame_setup(size, width, height):
    """the FrameSetup a G-buffer kit builds for `size` at the extent it rasterises: the frozen camera, or the case an Extent names"""
    return setup(size.case, (width, height)) if isinstance(size, Extent) else FrameSetup(width, height)


def sky_half(depth, host=None):
    """The half-resolution texels whose depth code is 0xFFFFFF (nothing was drawn there): `depth` the chain's depth image with its
    mip 1 built, `host` its bytes if they are not the image's own.  gtao_accumulate linearises the reprojected ndc.z ~ 1 of such a
    texel and compares the result with 0.2: whether it keeps or drops its history there hangs on the last bit of the camera's
    scalars."""
    return (depth.raw(1, host)[..., 0] & 0xFFFFFF) == 0xFFFFFF


def cap(texels):
    # tests/test_fuzz_gpu.py: a texel may flip a hit / break decision through libm-vs-ocml ulps in the smooth part
    return max(1, int(2e-4 * texels))


# ---- steps: every pass of the flat chain that takes a camera, each run on the oracle's bytes -----------------------------------------
GBUFFER = ("depth", "prev_depth", "normal", "albedo", "material", "velocity")
CHAIN_IMAGES = GBUFFER + ("dn", "dv", "raw", "filtered", "acc_ao", "acc_hist", "rays", "reflections", "blurred", "blurred_hist", "taa_hist",
                          "taa_target")
# the images of the passes outside the frame loop (chain.py allocates them on first use: every chain here gets them up front)
EXTRA_IMAGES = ("st_raw", "st_filtered", "st_accumulated", "ao_prev_frame", "ao_output", "ssr_out", "color_out")
IMAGES = CHAIN_IMAGES + EXTRA_IMAGES
EXACT = ("depth", "dn", "dv")  # integer / index work, tests/test_parity_gpu.py


class Step:
    """One pass: run(chain) on any backend; outs: the images it writes; exact: every output is integer work (bit for bit);
    prepare(ref): what the oracle does to its own images before the step's inputs are recorded"""

    def __init__(self, name, run, outs, exact=False, prepare=None):
        self.name, self.run, self.outs, self.exact, self.prepare = name, run, outs, exact, prepare

    def is_exact(self, out):
        return self.exact or out in EXACT


def _stage(name, outs):
    return Step(name, lambda c: getattr(c, name)(), outs)


# the frame loop, tests/test_parity_gpu.py STAGES
CHAIN_STEPS = tuple(_stage(n, o) for n, o in (("downsample", ("depth", "dn", "dv")), ("ssr_trace", ("rays", "raw")), ("ssr_filter", ("reflections",)),
                                              ("ssr_blur", ("blurred",)), ("gtao_main", ("raw",)), ("gtao_filter", ("filtered",)),
                                              ("gtao_accumulate", ("acc_ao",)), ("taa", ("taa_target",))))
ANGLE = 0.3125


def _deinterleaved(c):
    c.deinterleave_depth(2)
    c.gtao_main_deinterleaved(layer=6, angle_offset=ANGLE)


def _trace_indirect(c):
    c.ssr_classify(max_roughness=0.7, glossy_value=0.5)
    c.ssr_trace_indirect(frame_random=5, max_roughness=0.7)


def _gtao_main_no_mis(c):
    c.setup.use_mis = 0
    try:
        c.gtao_main()
    finally:
        c.setup.use_mis = 1


def _nearly_static(ref, mip, seed):
    """prev_depth mip `mip` := the current depth moved by -2 .. 2 codes per texel (sky stays sky).  The two static reprojections
    blend where |linear(prev) - linear(cur)| < 1e-6; one D24 code is 1.2e-6 z^2 of linear depth under the frozen range, so the
    decision falls either way across the frame and depends on znear and zfar.  On the chain's own previous depth it never
    does: that differs everywhere by far more."""
    cur = ref.depth.raw(mip)[..., 0].astype(np.int64)
    code = cur & 0xFFFFFF
    moved = np.clip(code + np.random.default_rng(seed).integers(-2, 3, size=code.shape), 0, 0xFFFFFE)
    code = np.where(code == 0xFFFFFF, code, moved)
    ref.prev_depth.set_raw(((cur & 0xFF000000) | code).astype(np.uint32).reshape(code.shape + (1,)), mip)


def nearly_static(depth, prev_depth, mip, host=None, prev_host=None):
    """the texels that _nearly_static moved by one or two codes: there the static reprojections decide |linear(prev) -
    linear(cur)| < 1e-6 between floats a few ulps apart"""
    cur = depth.raw(mip, host)[..., 0].astype(np.int64) & 0xFFFFFF
    prev = prev_depth.raw(mip, prev_host)[..., 0].astype(np.int64) & 0xFFFFFF
    return (cur != prev) & (np.abs(cur - prev) <= 2)


def _random_history(img, seed):
    hist = img.to_host().copy()
    h16 = hist.view(np.uint16)
    h16[:] = np.random.default_rng(seed).integers(0, 0x3C00, size=h16.shape, dtype=np.uint16)  # fp16 codes in [0, 1)
    img.upload(hist)


def _prepare_screen_trace_accumulate(ref):
    _nearly_static(ref, 0, 7)
    _random_history(ref.st_accumulated, 3)


def _prepare_reproject(ref):
    """tests/test_variants_gpu.py test_gtao_reproject_variant: the filtered bare arcs of the non-MIS main pass, a random history;
    the previous depth a few codes from the current one"""
    ref.gtao_filter()
    _nearly_static(ref, 1, 11)
    _random_history(ref.ao_prev_frame, 5)


# the generator, the rows either side of the hot path (tests/test_content_gpu.py test_widened_rows) and the shading, on the state
# the frame loop leaves.
SIDE_STEPS = (
    Step("gtao_graphics", lambda c: c.gtao_main_graphics(angle_offset=ANGLE), ("raw",)),
    Step("gtao_deinterleaved", _deinterleaved, ("raw",)),
    Step("screen_trace", lambda c: c.screen_trace(angle_offset=0.4375, random_offset=0.625), ("st_raw",)),
    Step("screen_trace_filter", lambda c: c.screen_trace_filter(), ("st_filtered",)),
    Step("screen_trace_accumulate", lambda c: c.screen_trace_accumulate(), ("st_accumulated",), prepare=_prepare_screen_trace_accumulate),
    Step("ssr_simple", lambda c: c.ssr_simple(), ("ssr_out",)),
    Step("shading", lambda c: c.shading(min_roughness=0.1, max_roughness=0.7, show_ao=0), ("color_out",)),
    Step("shading_show_ao", lambda c: c.shading(show_ao=1), ("color_out",)),
    Step("trace_indirect", _trace_indirect, ("rays",)),
    Step("gtao_main_no_mis", _gtao_main_no_mis, ("raw",)),
    Step("gtao_reproject", lambda c: c.gtao_reproject(), ("ao_output",), prepare=_prepare_reproject),
)
SYNTH = Step("synth", lambda c: c.synth(), GBUFFER, exact=True)
STEPS = {s.name: s for s in (SYNTH,) + CHAIN_STEPS + SIDE_STEPS}


@functools.lru_cache(maxsize=None)
def _luts():
    """the two LUTs depend on nothing of the frame: the oracle's bytes, once"""
    c = PostFxChain(2, 2, backend="oracle")
    c.preintegrate_pdf()
    c.preintegrate_brdf()
    return c.pdf.to_host().copy(), c.brdf.to_host().copy()


def new_chain(size, backend, st, **kw):
    """a chain of `backend` with every image of IMAGES allocated and the oracle's LUTs in place"""
    c = PostFxChain(*size, backend=backend, setup=st, **kw)
    for n in ("st_raw", "st_filtered", "st_accumulated"):
        c._full_img(n)
    for n in ("ao_prev_frame", "ao_output"):
        c._half_img(abi.FMT_R16_SFLOAT, n)
    geometry = dict(device=c.device, full=c.albedo.full, origin=c.albedo.origin)
    c.ssr_out = ImageBuf(abi.FMT_RGBA8_UNORM, c.albedo.width, c.albedo.height, **geometry)
    c.color_out = ImageBuf(abi.FMT_RGBA8_SRGB, c.albedo.width, c.albedo.height, **geometry)
    c.brdf = ImageBuf(abi.FMT_RG16_SFLOAT, PDF_LUT_SIZE, PDF_LUT_SIZE, device=c.device)
    c._layer_descs(2)
    pdf, brdf = _luts()
    c.pdf.upload(pdf)
    c.brdf.upload(brdf)
    return c


def snapshot(chain, names=IMAGES):
    return {n: getattr(chain, n).to_host().copy() for n in names}


def load(chain, snap):
    for n, host_bytes in snap.items():
        getattr(chain, n).upload(host_bytes)


class Record:
    """The oracle under one case and size, step by step: the bytes of every image before each step and of the step's outputs after
    it.  The frame loop starts one whole frame after the seeded histories (tests/test_fuzz_gpu.py), so what the passes reproject
    is not a constant.  Shared between tests: never run on, never written to."""

    def __init__(self, name, size, side=True):
        self.name, self.size = name, size
        ref = new_chain(size, "oracle", setup(name, size))
        self.pre, self.post = {}, {}
        self._step(ref, SYNTH)
        ref.build_prev_hiz()
        ref.init_histories()
        ref.frame()
        ref.swap_histories()
        for step in CHAIN_STEPS:
            if step.name == "gtao_accumulate":  # the second reference value of the texels of sky_half: the history dropped
                before = ref.acc_ao.to_host().copy()
                ref.gtao_accumulate(clear_history=1)
                self.acc_ao_cleared = ref.acc_ao.to_host().copy()
                ref.acc_ao.upload(before)
            self._step(ref, step)
        self.sky = sky_half(ref.depth, self.pre["gtao_accumulate"]["depth"])[: ref.acc_ao.height, : ref.acc_ao.width]
        for step in SIDE_STEPS if side else ():
            self._step(ref, step)

    def _step(self, ref, step):
        if step.prepare is not None:
            step.prepare(ref)
        self.pre[step.name] = snapshot(ref)
        step.run(ref)
        self.post[step.name] = snapshot(ref, step.outs)

    def setup(self):
        return setup(self.name, self.size)

    def chain(self, backend, st=None, **kw):
        """a fresh chain of `backend` under the record's camera, or under `st`"""
        return new_chain(self.size, backend, st or self.setup(), **kw)

    def run(self, chain, step):
        """`step` on the record's bytes -> {output name: (image, the oracle's bytes)}"""
        load(chain, self.pre[step.name])
        step.run(chain)
        chain.sync()
        return {o: (getattr(chain, o), self.post[step.name][o]) for o in step.outs}


@functools.lru_cache(maxsize=None)
def record(name, size):
    return Record(name, size, side=size == SMALL)


def bits(img, mip, host):
    r = img.raw(mip, host)
    r = r.view(np.uint16) if r.dtype == np.float16 else r
    return r & 0xFFFFFF if img.format == abi.FMT_D24_UNORM_S8 else r  # the top byte of a D24S8 word is not depth
