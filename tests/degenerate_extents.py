"""Images too small to fill a pass's own structure: the sizes, the content and the oracle record the degenerate-extent
tests (tests/test_degenerate_extents.py on the oracle alone, tests/test_degenerate_extents_gpu.py on the kernels) share.

Below 70 x 38 the kernels take branches nothing else launches: a half-res image one texel wide or high (no pair loads),
a floor-dispatch extent (8 x 4 groups, floored: vkr_host.hpp floor_dispatch_w / _h) of zero, exactly one dispatch group,
the smallest ragged one, images smaller than one block, one wave, one 8 x 8 tile and one blur radius.

The content classes are those of tests/gbuffer_content.py that still mean something on a handful of texels, and one more:
the synthetic camera produces next to no reflections at these sizes (1 to 3 distinct `reflections` texels at 2 x 130 under
every class), so `stage_noise` — the synthetic scene itself — also overwrites the intermediate inputs of the later
stages with noise directly before the stage runs.  Both backends are given the same pre-stage bytes.
"""
import numpy as np

import gbuffer_content as gc
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PostFxChain

# full-res extent -> what it is the smallest case of (half-res in brackets)
SIZES = (
    (2, 2),     # (1 x 1) one texel everywhere, depth chain of 2 mips
    (2, 130),   # (1 x 65) one texel wide, higher than a block: no pair loads, depth1.w < 2 in the shading
    (130, 2),   # (65 x 1) one texel high, one lane more than a wave wide
    (4, 4),     # (2 x 2) the narrowest pair
    (6, 10),    # (3 x 5) odd on both axes, floor-dispatch width 0
    (14, 34),   # (7 x 17) floor-dispatch width 0, height non-zero
    (34, 6),    # (17 x 3) floor-dispatch height 0, width non-zero
    (16, 8),    # (8 x 4) exactly one dispatch group: the smallest image on the TILED GTAO path
    (18, 10),   # (9 x 5) the smallest ragged floor dispatch (8 x 4 of 9 x 5)
)
CLASSES = ("sky_all", "checker_px", "normal_poles", "material_extremes", "velocity_wild", "history_nonfinite", "all_noise", "stage_noise")
CASES = [(name, size) for name in CLASSES for size in SIZES]
IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]

EXACT = ("depth", "dn", "dv")  # integer outputs
STAGES = [("downsample", ("depth", "dn", "dv")), ("ssr_trace", ("rays", "raw")), ("ssr_filter", ("reflections",)), ("ssr_blur", ("blurred",)),
          ("gtao_main", ("raw",)), ("gtao_filter", ("filtered",)), ("gtao_accumulate", ("acc_ao",)), ("taa", ("taa_target",))]
FLOOR_STAGES = ("gtao_main", "gtao_filter")  # dispatched in floored 8 x 4 groups
SNAP = ("depth", "prev_depth", "normal", "albedo", "material", "velocity", "dn", "dv", "raw", "filtered", "acc_ao", "acc_hist", "rays",
        "reflections", "blurred", "blurred_hist", "taa_hist", "taa_target")  # every image but the LUT, which never changes


def floor_extent(w, h):
    """the extent a pass of floored 8 x 4 groups writes of a w x h image"""
    return (w // 8) * 8, (h // 4) * 4


def zero_dispatch(size):
    fw, fh = floor_extent(size[0] // 2, size[1] // 2)
    return fw == 0 or fh == 0


def written(stage, w, h):
    """[h, w] bool: the texels of a w x h output `stage` writes"""
    m = np.zeros((h, w), dtype=bool)
    fw, fh = floor_extent(w, h) if stage in FLOOR_STAGES else (w, h)
    m[:fh, :fw] = True
    return m


_PDF = {}


def pdf_lut():
    """the bytes of the preintegrated PDF LUT: one 1024^2 integration per process"""
    if "host" not in _PDF:
        c = PostFxChain(2, 2, backend="oracle", setup=FrameSetup(2, 2))
        c.preintegrate_pdf()
        _PDF["host"] = c.pdf.to_host().copy()
    return _PDF["host"]


def _f16_unit(rng, shape):
    return rng.random(shape, dtype=np.float32).astype(np.float16).clip(0, np.float16(0.99951171875))  # [0, 1) after rounding


def seed_stage(c, stage, size):
    """stage_noise: the inputs of `stage` that earlier stages produce, overwritten with noise (fixed seed per stage and size)"""
    rng = np.random.default_rng([0x57A6E, [s for s, _ in STAGES].index(stage), size[0], size[1]])
    if stage == "ssr_filter":
        c.rays.set_raw(rng.integers(0, 1 << 16, size=(c.rays.height, c.rays.width, 4), dtype=np.uint16))
        c.albedo.set_raw(rng.integers(0, 256, size=(c.albedo.height, c.albedo.width, 4), dtype=np.uint8))
    elif stage == "ssr_blur":
        for img in (c.reflections, c.blurred_hist):
            img.set_raw(rng.integers(0, 256, size=(img.height, img.width, 4), dtype=np.uint8))
    elif stage == "gtao_filter":
        c.raw.set_raw(_f16_unit(rng, (c.raw.height, c.raw.width, 4)))
    elif stage == "gtao_accumulate":
        c.filtered.set_raw(_f16_unit(rng, (c.filtered.height, c.filtered.width, 1)))


def prepare(name, size):
    """the oracle chain of the class before its first stage"""
    return gc.prepare(None if name == "stage_noise" else name, size, pdf=pdf_lut())


def snapshot(c):
    return {n: getattr(c, n).to_host().copy() for n in SNAP}


def load(chain, snap):
    for n in SNAP:
        getattr(chain, n).upload(snap[n])


class Case:
    """One oracle run of the class, stage by stage: what every image held before each stage (pre[stage], after the
    stage_noise hook) and what the stage's outputs held after it (post[stage])"""

    def __init__(self, name, size):
        self.name, self.size = name, size
        ref = prepare(name, size)
        self.pdf = pdf_lut()
        self.pre, self.post = {}, {}
        for stage, outs in STAGES:
            if name == "stage_noise":
                seed_stage(ref, stage, size)
            self.pre[stage] = snapshot(ref)
            getattr(ref, stage)()
            self.post[stage] = {o: getattr(ref, o).to_host().copy() for o in outs}
        self.final = snapshot(ref)
        self.ref = ref  # the record's own chain: read (formats, extents, raw()), never run on again
        # half-res texels holding a roughness code 0 or a depth code 0: where a filter / blur weight can be infinite or NaN
        bad = (ref.material.raw(0)[..., 1] == 0) | ((ref.depth.raw(0)[..., 0] & 0xFFFFFF) == 0)
        h2, w2 = ref.rays.height, ref.rays.width
        self.nonfinite_weight = bad.reshape(h2, 2, w2, 2).any(axis=(1, 3))

    def product(self):
        import torch

        assert torch.cuda.is_available()
        gpu = PostFxChain(*self.size, backend="product", device="cuda", setup=FrameSetup(*self.size))
        gpu.pdf.upload(self.pdf)
        return gpu


def ssao_case(w, h):
    """-> (depth words [h, w], setup, samples) of the SSAO cases: depth codes 0xFFFFFF - U[0, 2^16), far geometry whose
    sample tests sit close to the compare's threshold"""
    import ssao_reference

    rng = np.random.default_rng([0x55A0, w, h])
    depth = (np.uint32(0xFFFFFF) - rng.integers(0, 1 << 16, size=(h, w), dtype=np.uint32)).astype(np.uint32)
    return depth, FrameSetup(w, h), ssao_reference.fixed_samples()


def texels(img, mip, host):
    """[h, w, bpp] uint8: the stored bytes of every texel of one mip"""
    r = img.raw(mip, host)
    return np.ascontiguousarray(r).view(np.uint8).reshape(r.shape[0], r.shape[1], -1)
