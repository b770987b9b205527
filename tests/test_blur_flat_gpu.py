"""The blur's constant-normal-weight tap loops (vk-renderer_amd/csrc/ssr.hip, blur_uniform_sigma<R, true> / blur_rows<R, true>): a tile
whose staged normals — tile and apron, clamped footprints included — are ONE raw RG16 word takes them, every other tile the
per-tap normal weight of before.

Frames of 160x96 (half-res 80x48: three by two blur tiles of 32x32, so interior, edge and corner tiles) and a ragged 150x90.
Every case: random reflections, a depth ramp with one discontinuity, a random history.  The oracle is the blur's reference
without the empty-tile skip (tests/test_content_gpu.py), so those runs set VKR_SWITCH_BLUR_NO_SKIP; the tile counters
(vkr_debug_blur_paths) are read from runs with the skip as shipped.

Which tiles a full-res normal texel belongs to is restated here from the staging rule: staged half-res pixel p samples the
normal at uv = p / half extent, a footprint of the full-res texels 2p - 1 and 2p clamped into the image, and tile b stages
p = 32 b - 11 .. 32 b + 42.  Tiles overlap by their aprons, so every staged row of a tile but the frame's outermost lies in a
neighbour's region too: "the outermost apron row of a tile" below is row 32 b - 11 of tile row b = 1, whose texel row
2 (32 b - 11) - 1 no other staged row of that tile reads; the tile row above holds it as well, and the model says so.

VKR_SWITCH_BLUR_GENERIC must switch the flat loops off: its image is held bit for bit to the one of GENERIC | NO_FLAT, and it
runs no flat loop.  Against plain NO_FLAT it is held to one UNORM8 code: those two are the rows order and the column order of
the same sums, both from before the flat loops, and on these frames they already differ by one code in a texel now and then
(measured: one texel in 2 of the 22 plane frames).
"""
import numpy as np
import pytest

from vk_renderer_amd import abi
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PostFxChain

from parity import report

pytestmark = pytest.mark.gpu

SIZES = ((160, 96), (150, 90))
TILE, APRON = 32, 11
NO_SKIP, NO_FLAT, GENERIC, COUNT = abi.SWITCH_BLUR_NO_SKIP, abi.SWITCH_BLUR_NO_FLAT, abi.SWITCH_BLUR_GENERIC, abi.SWITCH_BLUR_COUNT_PATHS
BLUR_IMAGES = ("depth", "prev_depth", "normal", "material", "reflections", "blurred_hist", "dv", "blurred")
PLANE = (40000, 27000)  # an RG16 code pair off every octahedral seam


def _srgb_table():
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def radius_of(code, max_roughness=1.0):
    """blur.comp:45-53 for the roughness an sRGB code decodes to"""
    sigma = 0.4 + 3.6 * (_srgb_table()[code] * max_roughness)
    return min(int(np.floor(3.0 * sigma - 0.01)), APRON)


def code_for_radius(r):
    """the material code whose radius is r, as far from both neighbouring radii as codes allow"""
    codes = [c for c in range(256) if radius_of(c) == r]
    assert codes, f"no roughness code gives radius {r}"
    return codes[len(codes) // 2]


def tiles_of(size):
    w2, h2 = size[0] // 2, size[1] // 2
    return (w2 + TILE - 1) // TILE, (h2 + TILE - 1) // TILE


def tiles_holding(size, tx, ty):
    """the blur tiles whose staged region reads full-res normal texel (tx, ty)"""
    def along(n_full, n_tiles, t):
        out = []
        for b in range(n_tiles):
            read = set()
            for p in range(TILE * b - APRON, TILE * b + TILE + APRON):
                read.update((min(max(2 * p - 1, 0), n_full - 1), min(max(2 * p, 0), n_full - 1)))
            if t in read:
                out.append(b)
        return out
    nx, ny = tiles_of(size)
    return [(bx, by) for by in along(size[1], ny, ty) for bx in along(size[0], nx, tx)]


class Scene:
    """An oracle chain holding the blur's inputs, and a product chain to run them on"""

    def __init__(self, size, roughness_code):
        import torch

        assert torch.cuda.is_available(), "the blur tests need a GPU"
        self.size = size
        w, h = size
        rng = np.random.default_rng([0xF1A7, w, h])
        ref = PostFxChain(w, h, backend="oracle", setup=FrameSetup(w, h))
        ref.synth()
        ref.build_prev_hiz()
        ref.init_histories()
        ref.downsample()
        h2, w2 = ref.reflections.height, ref.reflections.width
        # a depth ramp with one discontinuity, the same in the previous frame (so the reprojection test passes somewhere)
        y, x = np.mgrid[0:h2, 0:w2]
        ramp = (0x600000 + 0x400 * x + 0x300 * y + np.where(x + y > (w2 + h2) // 2, 0x200000, 0)).astype(np.uint32)
        for img in (ref.depth, ref.prev_depth):
            d = img.raw(1)[..., 0]
            img.set_raw((d & np.uint32(0xFF000000)) | ramp, mip=1)
        ref.reflections.set_raw(rng.integers(0, 256, size=(h2, w2, 4), dtype=np.uint8))
        ref.blurred_hist.set_raw(rng.integers(0, 256, size=(h2, w2, 4), dtype=np.uint8))
        m = ref.material.raw(0).copy()
        m[..., 1] = roughness_code
        ref.material.set_raw(m)
        ref.normal.set_raw(np.broadcast_to(np.array(PLANE, dtype=np.uint16), (h, w, 2)))
        self.ref = ref
        self.gpu = PostFxChain(w, h, backend="product", device="cuda", setup=FrameSetup(w, h))
        self.lib = abi.product()
        self.before = self.lib.vkr_get_switches()
        self.mask = NO_SKIP | NO_FLAT | GENERIC | COUNT | abi.SWITCH_BLUR_LANE_LOOPS

    def oracle(self):
        self.ref.ssr_blur()
        return self.ref.blurred.decode(0).copy()

    def run(self, bits, count=True):
        """the product's blur on the oracle's input bytes under the switches `bits`: (raw RGB codes, decoded image, path counters);
        count=False: as shipped, without the counters (they must then stay 0)"""
        for n in BLUR_IMAGES:
            getattr(self.gpu, n).copy_from(getattr(self.ref, n))
        try:
            self.lib.vkr_set_switches((self.before & ~self.mask) | bits | (COUNT if count else 0))
            abi.debug_blur_paths(reset=True)
            self.gpu.ssr_blur()
            self.gpu.sync()
            paths = abi.debug_blur_paths(reset=True)
        finally:
            self.lib.vkr_set_switches(self.before)
        host = self.gpu.blurred.to_host()
        return self.gpu.blurred.raw(0, host)[..., :3].astype(np.int32), self.gpu.blurred.decode(0, host), paths

    def check(self, what, want_not_flat=()):
        """The rules every case shares.  want_not_flat: the tiles that must not be flat (all others must be); their texels
        must be the NO_FLAT run's bit for bit.  Returns the images by switch set."""
        nx, ny = tiles_of(self.size)
        n_tiles, n_not = nx * ny, len(set(want_not_flat))
        want = self.oracle()
        fmt = self.ref.blurred.format
        on, on_dec, paths = self.run(0)
        print(f"[blur flat] {what} {self.size}: paths (empty, flat, not flat, blocks on a flat loop) = {paths}")
        assert paths[0] == 0, "random reflections: no tile is empty"
        assert (paths[1], paths[2]) == (n_tiles - n_not, n_not), f"{what}: flat / not flat tiles {paths[1:3]}, expected {(n_tiles - n_not, n_not)}"
        assert paths[3] == paths[1], "every flat tile runs its live waves on a flat loop (uniform sigma or rows)"
        # the shipped configuration (counters off): the same bits, and nothing counted
        plain, _, paths_plain = self.run(0, count=False)
        assert paths_plain == (0, 0, 0, 0), f"counters off, yet counted {paths_plain}"
        assert np.array_equal(plain, on), f"{what}: the image changes with VKR_SWITCH_BLUR_COUNT_PATHS"
        off, off_dec, paths_off = self.run(NO_FLAT)
        assert paths_off[3] == 0 and paths_off[1:3] == paths[1:3], "NO_FLAT: the same tiles found flat, no flat loop run"
        # against the oracle (its reference: every tap evaluated), zero texels outside the rule, flat paths on and off
        for name, bits in (("flat", NO_SKIP), ("no_flat", NO_SKIP | NO_FLAT)):
            _, dec, p = self.run(bits)
            nbad, _ = report(f"{what}[{name}]", fmt, dec, want)
            assert nbad == 0, f"{what} {self.size} [{name}]: {nbad} texels outside the rule"
            assert p[0] == 0
        nbad, _ = report(f"{what}[flat, skipping]", fmt, on_dec, want)
        assert nbad == 0
        # on against off: one UNORM8 code per channel at the most; tiles that are not flat: the same bits
        d = np.abs(on - off)
        print(f"[blur flat] {what}: flat vs NO_FLAT differ in {int((d > 0).any(axis=-1).sum())} texels, max {int(d.max())} code")
        assert d.max() <= 1
        for bx, by in set(want_not_flat):
            t = d[by * TILE:(by + 1) * TILE, bx * TILE:(bx + 1) * TILE]
            assert not t.any(), f"{what}: tile {(bx, by)} is not flat and differs from NO_FLAT in {int((t > 0).any(axis=-1).sum())} texels"
        # GENERIC implies NO_FLAT: the same bits with and without it, and no flat loop
        gen, _, pg = self.run(GENERIC)
        gen_off, _, _ = self.run(GENERIC | NO_FLAT)
        assert pg[3] == 0, "GENERIC ran a flat loop"
        assert np.array_equal(gen, gen_off), "GENERIC and GENERIC | NO_FLAT differ"
        dg = np.abs(gen - off)
        print(f"[blur flat] {what}: GENERIC vs NO_FLAT differ in {int((dg > 0).any(axis=-1).sum())} texels, max {int(dg.max())} code")
        assert dg.max() <= 1
        return on, off


@pytest.fixture(params=SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def size(request, oracle_lib):
    return request.param


def test_tile_model():
    """the restated staging rule on the cases below (no GPU work)"""
    assert tiles_of((160, 96)) == (3, 2) and tiles_of((150, 90)) == (3, 2)
    assert tiles_holding((160, 96), 96, 20) == [(1, 0)]
    assert tiles_holding((160, 96), 96, 41) == [(1, 0), (1, 1)] and tiles_holding((160, 96), 96, 40) == [(1, 0)]
    assert tiles_holding((160, 96), 159, 20) == [(2, 0)] and tiles_holding((150, 90), 149, 20) == [(2, 0)]
    assert sorted(radius_of(code_for_radius(r)) for r in range(1, 12)) == list(range(1, 12))


@pytest.mark.parametrize("radius", range(1, 12))
def test_plane(size, radius):
    """Case 1: every normal texel one code pair, one roughness per run with radius 1 .. 11: every tile flat."""
    Scene(size, code_for_radius(radius)).check(f"plane r={radius}")


# (name, texel of a 160x96 / 150x90 frame as a function of the size)
ONE_OFF = {
    "interior": lambda w, h: (96, 20),                       # half-res pixel (48, 10): inside tile (1, 0), in no apron
    "outermost_apron_row": lambda w, h: (96, 2 * (TILE - APRON) - 1),  # read by staged row 21 alone: first apron row of tile row 1
    "clamped_footprint_only": lambda w, h: (w - 1, 20),      # the last column: read only through the clamp, by staged pixels past the frame
}


@pytest.mark.parametrize("radius", (3, 10, 11))
@pytest.mark.parametrize("channel", (0, 1))
@pytest.mark.parametrize("where", sorted(ONE_OFF))
def test_one_texel_off(size, where, channel, radius):
    """Case 2: the plane with one full-res normal texel one LSB off in one channel.  Every tile whose staged region reads it
    is not flat and leaves the NO_FLAT bits; every other tile stays flat."""
    s = Scene(size, code_for_radius(radius))
    tx, ty = ONE_OFF[where](*size)
    n = s.ref.normal.raw(0).copy()
    n[ty, tx, channel] += 1
    s.ref.normal.set_raw(n)
    holding = tiles_holding(size, tx, ty)
    assert holding, "the texel is read by no tile"
    if where == "clamped_footprint_only":
        w2 = size[0] // 2
        assert all(2 * p < tx for p in range(w2)), "an in-frame staged pixel reads the texel"
    s.check(f"one off {where} ch{channel} r={radius}", want_not_flat=holding)


@pytest.mark.parametrize("radius", (2, 10))
def test_flat_per_tile(size, radius):
    """Case 3: one code pair over each 32x32 tile alone, another in every neighbour: the aprons see the neighbours' codes, so
    no tile is flat and the image is the NO_FLAT one bit for bit."""
    s = Scene(size, code_for_radius(radius))
    h, w = size[1], size[0]
    y, x = np.mgrid[0:h, 0:w]
    tile = (y // (2 * TILE)) * 8 + x // (2 * TILE)
    s.ref.normal.set_raw(np.stack([PLANE[0] + 257 * tile, PLANE[1] - 131 * tile], axis=-1).astype(np.uint16))
    nx, ny = tiles_of(size)
    on, off = s.check(f"flat per tile r={radius}", want_not_flat=[(bx, by) for by in range(ny) for bx in range(nx)])
    assert np.array_equal(on, off)


def test_textured_roughness(size):
    """Case 4: roughness per texel on the plane (the content of VKR_SYNTH_TEXTURED_ROUGHNESS: the object's roughness +- 0.15):
    no wave shares one sigma, so the flat tiles run blur_rows<R, true>."""
    s = Scene(size, 0)
    rng = np.random.default_rng([0x7E57, *size])
    t = _srgb_table()
    rough = np.clip(0.45 + 0.3 * (rng.random((size[1], size[0])) - 0.5), 0.02, 1.0)
    m = s.ref.material.raw(0).copy()
    m[..., 1] = np.searchsorted(t, rough).clip(1, 255)
    s.ref.material.set_raw(m)
    s.check("textured roughness")


@pytest.mark.parametrize("code", ((0, 0), (32768, 32768), (65535, 0), (65535, 65535)))
def test_degenerate_code(size, code):
    """Case 5: the plane's code pair is the clear value (0, 0) or sits on the octahedral map's seams and centre, where the
    decode is least well behaved: the one weight nw0 is then whatever each tap's weight was."""
    s = Scene(size, code_for_radius(5))
    s.ref.normal.set_raw(np.broadcast_to(np.array(code, dtype=np.uint16), (size[1], size[0], 2)))
    s.check(f"degenerate code {code}")
