"""Adversarial G-buffer and history content for the post-process chain.

Every parity test of the hot path used to see one picture (synth(): a floor, 24 spheres, sky).  The kernels decide a lot
by content — ballots over live lanes, compaction lists, empty-tile skips, wave-uniform sigma, shared bilinear footprints,
reprojection through a stored velocity — so the classes below overwrite the raw storage of an oracle-backed PostFxChain
with the content at which such decisions go wrong: nothing live, everything live, live and dead alternating per pixel /
tile / block, incoherent depth, normals on the octahedral seams, material codes on both sides of every threshold,
velocities out of the frame or not finite, histories holding Inf / NaN / 65504.

A class is a function (chain, rng).  prepare() builds the frame the tests run on: synth scene, one real oracle frame so
that the histories are real, the class, prev_depth's mips rebuilt.  Draws come from numpy.random.default_rng with a seed
fixed per (class, size), so the bytes are frozen.
"""
import numpy as np

from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PostFxChain

SKY = 0xFFFFFF
SIZES = ((70, 38), (206, 226))  # half-res 35x19 and 103x113: ragged against 8, 32 and 64


def _srgb_table():
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def threshold_codes():
    """The sRGB codes either side of every roughness threshold the chain compares a decoded material channel with:
    max_roughness 1.0 / 0.7 / 0.35 (trace, blur, classification) and the classification's glossy_value 0.5."""
    t = _srgb_table()
    codes = set()
    for thr in (1.0, 0.7, 0.35, 0.5):
        above = int(np.searchsorted(t, thr, side="left"))  # first code whose value is >= thr
        codes.update(c for c in (above - 1, above, above + 1) if 0 <= c <= 255)
    return sorted(codes)


def _set_depth(img, code, where=None):
    """D24 code into the low 24 bits of mip 0 (the stencil byte stays), everywhere or where `where` [h, w] is set"""
    d = img.raw(0)[..., 0].copy()
    new = (d & np.uint32(0xFF000000)) | (np.broadcast_to(np.asarray(code, dtype=np.uint32), d.shape) & np.uint32(SKY))
    img.set_raw(new if where is None else np.where(where, new, d))


def _grid(img):
    y, x = np.mgrid[0:img.height, 0:img.width]
    return x, y


def sky_all(c, rng):
    for img in (c.depth, c.prev_depth):
        _set_depth(img, SKY)


def near_all(c, rng):
    for img in (c.depth, c.prev_depth):
        _set_depth(img, 0)


def checker_px(c, rng):
    x, y = _grid(c.depth)
    for img in (c.depth, c.prev_depth):
        _set_depth(img, SKY, ((x + y) & 1) == 1)


def checker_tile(c, rng):
    x, y = _grid(c.depth)
    for img in (c.depth, c.prev_depth):
        _set_depth(img, SKY, (((x // 16) + (y // 16)) & 1) == 1)


def checker_block(c, rng):
    x, y = _grid(c.depth)
    for img in (c.depth, c.prev_depth):
        _set_depth(img, SKY, (((x // 64) + (y // 16)) & 1) == 1)


def depth_noise(c, rng):
    for img in (c.depth, c.prev_depth):
        _set_depth(img, rng.integers(0, 1 << 24, size=(img.height, img.width), dtype=np.uint32))


def depth_stripes(c, rng):
    x, _ = _grid(c.depth)
    for img in (c.depth, c.prev_depth):
        _set_depth(img, 0x800000, x % 3 == 0)
        _set_depth(img, 0xFFF000, x % 3 == 1)


def normal_noise(c, rng):
    c.normal.set_raw(rng.integers(0, 1 << 16, size=(c.normal.height, c.normal.width, 2), dtype=np.uint16))


def normal_poles(c, rng):
    codes = np.array([0, 1, 32767, 32768, 65534, 65535], dtype=np.uint16)
    c.normal.set_raw(rng.choice(codes, size=(c.normal.height, c.normal.width, 2)))


def material_extremes(c, rng):
    codes = np.array(sorted(set([0, 1, 254, 255] + threshold_codes())), dtype=np.uint8)
    c.material.set_raw(rng.choice(codes, size=(c.material.height, c.material.width, 4)))


_F16_WILD = np.array([0.0, -0.0, 6e-8, -6e-8, 0.5, -0.5, 2.0, -2.0, 65504.0, -65504.0, np.inf, -np.inf, np.nan], dtype=np.float16)
_F16_HIST = np.array([0.0, 1.0, 6e-8, 65504.0, -65504.0, np.inf, -np.inf, np.nan], dtype=np.float16)


def velocity_wild(c, rng):
    c.velocity.set_raw(rng.choice(_F16_WILD, size=(c.velocity.height, c.velocity.width, 2)))


def history_nonfinite(c, rng):
    for img, ch in ((c.acc_hist, 2), (c.acc_ao, 2), (c.taa_hist, 4)):
        img.set_raw(rng.choice(_F16_HIST, size=(img.height, img.width, ch)))
    c.blurred_hist.set_raw(rng.integers(0, 256, size=(c.blurred_hist.height, c.blurred_hist.width, 4), dtype=np.uint8))


def all_noise(c, rng):
    depth_noise(c, rng)
    normal_noise(c, rng)
    for img in (c.material, c.albedo):
        img.set_raw(rng.integers(0, 256, size=(img.height, img.width, 4), dtype=np.uint8))
    bits = rng.integers(0, 1 << 16, size=(c.velocity.height, c.velocity.width, 2), dtype=np.uint16)
    c.velocity.set_raw(bits.view(np.float16))
    history_nonfinite(c, rng)


CLASSES = {f.__name__: f for f in (sky_all, near_all, checker_px, checker_tile, checker_block, depth_noise, depth_stripes, normal_noise,
                                   normal_poles, material_extremes, velocity_wild, history_nonfinite, all_noise)}
NONFINITE = ("velocity_wild", "history_nonfinite", "all_noise")
FINITE = tuple(n for n in CLASSES if n not in NONFINITE)
# classes in which no roughness code and no depth code is 0, so no filter / blur weight is infinite or NaN and the
# empty-tile skips must not change a single texel (tests/test_parity_gpu.py::test_empty_tile_skip_against_no_skip)
SKIP_EXACT = ("sky_all", "checker_px", "checker_tile", "checker_block", "depth_stripes", "normal_noise", "normal_poles", "velocity_wild")
CASES = [(name, size) for name in CLASSES for size in SIZES]
# the images a class may touch (what a determinism check hashes)
INPUTS = ("depth", "prev_depth", "normal", "albedo", "material", "velocity", "acc_hist", "acc_ao", "taa_hist", "blurred_hist")


def seed_of(name, size):
    return [0xC0_47E47, list(CLASSES).index(name), size[0], size[1]]


def apply(chain, name, size):
    CLASSES[name](chain, np.random.default_rng(seed_of(name, size)))


def prepare(name, size, pdf=None, **setup_kw):
    """An oracle-backed chain holding class `name` at `size`, ready for any stage of the chain.  pdf: the bytes of an
    already preintegrated PDF LUT (it depends on nothing of the frame), uploaded instead of integrating the 1024^2 table again."""
    w, h = size
    ref = PostFxChain(w, h, backend="oracle", setup=FrameSetup(w, h, **setup_kw))
    ref.synth()
    ref.build_prev_hiz()
    ref.init_histories()
    if pdf is None:
        ref.preintegrate_pdf()
    else:
        ref.pdf.upload(pdf)
    ref.frame()
    ref.swap_histories()
    if name is not None:  # None: the synthetic scene as it is
        apply(ref, name, size)
    ref.build_prev_hiz()
    return ref


def input_bytes(chain):
    return b"".join(getattr(chain, n).to_host().tobytes() for n in INPUTS)
