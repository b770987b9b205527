"""The shadow mask without a GPU: the C-ABI block and the program table, every refusal of vkr_shadow_mask and of
vkr_defered_shading_shadowed (validation never reaches a launch), and a known answer for the numpy restatement
(tests/shadow_mask_reference.py): a tilted floor under light A of tests/shadow_light.py with a smaller occluder between light and
floor, seen by a camera that looks at the edge of the shadow.

Known answer, measured here (oracle rasteriser, 128^2 map, 96 x 64 camera): radius 0 / 1 / 2: bias 585 / 1169 / 1751 codes,
2780 / 2625 / 2473 floor pixels at least radius + 2 texels inside the occluder's outline (all 0) and 2480 / 2348 / 2226 at least
as far outside it (all 255)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from vk_renderer_amd import abi, camera, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.chain import PostFxChain

import shadow_light as sl
import shadow_mask_reference as ref
from test_abi_errors import ERR_EXTENT, ERR_FORMAT, ERR_NULL, img

F32 = np.float32


# ---- struct size and symbols ------------------------------------------------------------------------------------------------------
def test_block_layout_and_symbols():
    txt = open(abi.ROOT + "/include/vkr_postfx.h").read()
    body = re.search(r"typedef struct vkr_shadow_mask_params \{(.*?)\} vkr_shadow_mask_params;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind, names = decl.split(None, 1)
        unit = {"vkr_mat4": 64, "float": 4, "uint32_t": 4}[kind]
        for name in names.split(","):
            m = re.search(r"\[(\d+)\]", name)
            size += unit * (int(m.group(1)) if m else 1)
    assert size == 352
    assert C.sizeof(abi.ShadowMaskParams) == size
    assert abi.ShadowMaskParams.fovy.offset == 320 and abi.ShadowMaskParams.layer_count.offset == 336
    assert "int vkr_shadow_mask(" in txt and "int vkr_defered_shading_shadowed(" in txt
    lib = abi.product()
    assert hasattr(lib, "vkr_shadow_mask") and hasattr(lib, "vkr_defered_shading_shadowed")


def test_programs_are_registered():
    assert host.lib().vkrh_has_program(b"shadow_mask") == 1
    assert host.lib().vkrh_has_program(b"defered_shading_shadowed") == 1
    assert host.lib().vkrh_has_program(b"defered_shading") == 1
    assert host.STAGE_SHADOW_MASK == 1 << 28
    assert hasattr(host.lib(), "vkrh_set_shadow_mask")


# ---- error paths ------------------------------------------------------------------------------------------------------------------
W, H, N = 64, 32, 48


def _params(**over):
    p = abi.shadow_mask_params(np.eye(4), [np.eye(4)] * over.pop("lights", 2), 1.0, 2.0, 0.05, 80.0, radius=1, bias=0)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _mask_call(depth="ok", layers="ok", params="ok", out="ok"):
    lib = abi.product()
    d = img(abi.FMT_D24_UNORM_S8, W, H) if depth == "ok" else depth
    o = img(abi.FMT_RGBA8_UNORM, W, H) if out == "ok" else out
    p = _params() if params == "ok" else params
    ls = [img(abi.FMT_D24_UNORM_S8, N, N), img(abi.FMT_D24_UNORM_S8, N, N)] if layers == "ok" else layers
    arr = (abi.VkrImg * len(ls))(*ls) if ls is not None else None
    byref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    rc = lib.vkr_shadow_mask(byref(d), arr, byref(p), byref(o), None)
    return rc, (lib.vkr_last_error() or b"").decode()


D24 = abi.FMT_D24_UNORM_S8
MASK_REFUSALS = {
    "depth NULL": (dict(depth=None), ERR_NULL, "depth is NULL"),
    "layers NULL": (dict(layers=None), ERR_NULL, "layers is NULL"),
    "params NULL": (dict(params=None), ERR_NULL, "params is NULL"),
    "out NULL": (dict(out=None), ERR_NULL, "out_mask is NULL"),
    "depth without memory": (dict(depth=img(D24, W, H, base=None)), ERR_NULL, "shadow_mask.depth: NULL image"),
    "layer without memory": (dict(layers=[img(D24, N, N), img(D24, N, N, base=None)]), ERR_NULL, "shadow_mask.layers: NULL image"),
    "depth format": (dict(depth=img(abi.FMT_R32_SFLOAT, W, H)), ERR_FORMAT, "shadow_mask.depth: format"),
    "out format": (dict(out=img(abi.FMT_RGBA8_SRGB, W, H)), ERR_FORMAT, "shadow_mask.out_mask: format"),
    "layer format": (dict(layers=[img(D24, N, N), img(abi.FMT_R32_SFLOAT, N, N)]), ERR_FORMAT, "shadow_mask.layers: format"),
    "extent mismatch": (dict(out=img(abi.FMT_RGBA8_UNORM, W, H + 1)), ERR_EXTENT, "one extent expected"),
    "layer not square": (dict(layers=[img(D24, N, N + 1), img(D24, N, N)]), ERR_EXTENT, "must be square and of one extent"),
    "layers of unequal extent": (dict(layers=[img(D24, N, N), img(D24, N + 1, N + 1)]), ERR_EXTENT, "must be square and of one extent"),
    "layer_count 0": (dict(params=_params(layer_count=0)), ERR_EXTENT, "layer_count 0"),
    "layer_count 5": (dict(params=_params(layer_count=5)), ERR_EXTENT, "layer_count 5"),
    "radius 3": (dict(params=_params(radius=3)), ERR_EXTENT, "radius 3"),
    "reserved": (dict(params=_params(reserved=7)), ERR_EXTENT, "reserved is 7"),
    "windowed depth": (dict(depth=img(D24, W, H, full=(W, 2 * H), origin=(0, 2))), ERR_EXTENT, "depth: windows are not supported"),
    "windowed out": (dict(out=img(abi.FMT_RGBA8_UNORM, W, H, full=(W, 2 * H), origin=(0, 0))), ERR_EXTENT, "out_mask: windows are not supported"),
    "windowed layer": (dict(layers=[img(D24, N, N, full=(N, 2 * N)), img(D24, N, N)]), ERR_EXTENT, "layers: windows are not supported"),
}


@pytest.mark.parametrize("name", sorted(MASK_REFUSALS))
def test_shadow_mask_refusals(name):
    kwargs, code, message = MASK_REFUSALS[name]
    rc, msg = _mask_call(**kwargs)
    assert rc == code, (name, rc, msg)
    assert message in msg, (name, msg)


def _shading_call(shadowed, **over):
    lib = abi.product()
    d = dict(albedo=img(abi.FMT_RGBA8_SRGB, W, H), normal=img(abi.FMT_RG16_UNORM, W, H), material=img(abi.FMT_RGBA8_SRGB, W, H),
             depth=img(D24, W, H, mips=2), consts=abi.ShadingParams(), occlusion=img(abi.FMT_RG16_SFLOAT, W // 2, H // 2),
             brdf=img(abi.FMT_RG16_SFLOAT, 32, 32), reflections=img(abi.FMT_RGBA8_UNORM, W // 2, H // 2),
             mask=img(abi.FMT_RGBA8_UNORM, W, H), out=img(abi.FMT_RGBA8_SRGB, W, H), push=abi.ShadingPush())
    d.update(over)
    byref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    names = ["albedo", "normal", "material", "depth", "consts", "occlusion", "brdf", "reflections"] + (["mask"] if shadowed else []) + ["out", "push"]
    fn = lib.vkr_defered_shading_shadowed if shadowed else lib.vkr_defered_shading
    rc = fn(*[byref(d[n]) for n in names], None)
    return rc, (lib.vkr_last_error() or b"").decode()


SHADING_REFUSALS = {
    "mask NULL": (dict(mask=None), ERR_NULL, "defered_shading_shadowed.shadow_mask: NULL image"),
    "mask without memory": (dict(mask=img(abi.FMT_RGBA8_UNORM, W, H, base=None)), ERR_NULL, "defered_shading_shadowed.shadow_mask: NULL image"),
    "mask format": (dict(mask=img(abi.FMT_RGBA8_SRGB, W, H)), ERR_FORMAT, "defered_shading_shadowed.shadow_mask: format"),
    "mask extent": (dict(mask=img(abi.FMT_RGBA8_UNORM, W, H - 2)), ERR_EXTENT, "one window expected"),
    "params NULL": (dict(consts=None), ERR_NULL, "defered_shading_shadowed: NULL params"),
    "albedo format": (dict(albedo=img(abi.FMT_RGBA8_UNORM, W, H)), ERR_FORMAT, "defered_shading_shadowed.albedo: format"),
}


@pytest.mark.parametrize("name", sorted(SHADING_REFUSALS))
def test_shadowed_shading_refusals(name):
    kwargs, code, message = SHADING_REFUSALS[name]
    rc, msg = _shading_call(True, **kwargs)
    assert rc == code, (name, rc, msg)
    assert message in msg, (name, msg)


def test_plain_shading_keeps_its_messages():
    """the existing entry names its bindings as before"""
    rc, msg = _shading_call(False, albedo=img(abi.FMT_RGBA8_UNORM, W, H))
    assert rc == ERR_FORMAT and "defered_shading.albedo: format" in msg
    rc, msg = _shading_call(False, push=None)
    assert rc == ERR_NULL and msg == "defered_shading: NULL params"


# ---- the host's double product -----------------------------------------------------------------------------------------------------
def test_light_matrix_is_the_double_product_rounded_once():
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=(4, 4)).astype(F32), rng.normal(size=(4, 4)).astype(F32)
    m = ref.light_matrix(a, b)
    exact = a.astype(np.float64) @ b.astype(np.float64)
    assert np.abs(m.astype(np.float64) - exact).max() <= np.abs(exact).max() * 2.0 ** -24
    assert np.array_equal(ref.light_matrix(a, np.eye(4)), a)
    a[1, 2] = np.inf
    with np.errstate(all="ignore"):
        m = ref.light_matrix(a, np.eye(4))
    assert np.isnan(m[1, 0]) and np.isinf(m[1, 2]) and np.array_equal(m[0], a[0])  # inf * 0 poisons the row, and only the row


# ---- the synthetic inputs of the GPU parity test, and what keeps that test from being vacuous ---------------------------------------
OUT_SIZES = [(70, 37), (16, 16), (1, 1), (257, 3)]  # no multiple of the block; one block; one pixel; many blocks in x, odd width
MAP_SIZES = [45, 1, 64]
RADII = [0, 1, 2]
BIASES = [0, 1, 1 << 24]
SYNTH_FAZZ = (F32(1.0), F32(1.5), F32(1.0), F32(3.0))  # view z in (-3, -1] over the whole depth range: every pixel is well conditioned
CLASSES = ("behind", "left", "right", "top", "bottom", "far", "near", "nan", "border_left", "border_right", "border_top", "border_bottom",
           "equal", "one_above", "sky", "tapped")


def _synth_inverse_camera():
    """a rigid view -> world matrix without a zero entry (so that an infinity in a light matrix reaches every entry of its row)"""
    a, b = 0.7, -0.4
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx @ ry
    m[:3, 3] = (0.3, -1.2, 2.5)
    return m.astype(F32)


def _synth_light(kind, inverse_camera):
    """a light matrix whose product with inverse_camera is (up to rounding) the view-space map A of its kind.  With the camera
    of SYNTH_FAZZ a pixel's view position is (xd * 0.8194 |z|, yd * 0.5463 |z|, z), xd and yd in (-1, 1), |z| in [1, 3).
    fit: ndc.xy = 0.9999 (xd, yd), ndc.z in (0.05, 0.95): every pixel takes taps, the outermost land in the border texels;
    wide: ndc.xy = 1.6 (xd, yd), ndc.z from -0.3 to 1.3: every frustum side, far and near;
    behind: clip.w changes sign across the picture;
    inf: `fit` with an infinity in its z row."""
    tg = np.tan(0.5)
    sx, sy = 1.0 / (1.5 * tg), 1.0 / tg
    A = np.zeros((4, 4))
    if kind in ("fit", "inf"):
        A[0, 0], A[1, 1] = 0.9999 * sx, 0.9999 * sy
        A[2, 2], A[2, 3] = -1.4, -1.35   # ndc.z = 1.4 - 1.35 / |z|
        A[3, 2] = -1.0
    elif kind == "wide":
        A[0, 0], A[1, 1] = 1.6 * sx, 1.6 * sy
        A[2, 2], A[2, 3] = -2.1, -2.4    # ndc.z = 2.1 - 2.4 / |z|
        A[3, 2] = -1.0
    elif kind == "behind":
        A[0, 0], A[1, 1] = 0.5, 0.5
        A[2, 2], A[2, 3] = -0.2, 0.1
        A[3, 0], A[3, 1], A[3, 3] = 1.0, 0.5, 0.2
    else:
        raise ValueError(kind)
    m = (A @ np.linalg.inv(inverse_camera.astype(np.float64))).astype(F32)
    if kind == "inf":
        m[2, 1] = np.inf
    return m


KINDS = ("fit", "wide", "behind", "inf")


@functools.lru_cache(maxsize=None)
def synthetic_launches(map_n, radius, bias):
    """The launches of one parity case: every output size x layer_count 1..4, the light kinds rotating through the layers.
    -> list of dict(size, depth words [h, w], maps [4, n, n] words, mvps, inverse_camera, fazz, expect [h, w, 4], classes).
    Depth: random D24 with a fifth of sky and random stencil bytes; maps: random 32-bit words (the top byte is noise), then one
    texel per light patched to code - bias (the compare holds with equality) or code - bias - 1 (code is one above) under a pixel
    that takes taps.  With bias = 2^24 neither can be built: code < 2^24 <= word + bias for every word."""
    arith = ref.Arith(int(abi.product().vkr_numeric_contract()))
    inv = _synth_inverse_camera()
    out = []
    for si, (w, h) in enumerate(OUT_SIZES):
        for k in range(1, 5):
            rng = np.random.default_rng(1000 * map_n + 100 * radius + 10 * si + k + (7 if bias else 0))
            depth = rng.integers(0, 1 << 24, size=(h, w), dtype=np.uint32)
            depth[rng.random((h, w)) < 0.2] = sl.D24_MAX
            depth |= rng.integers(0, 256, size=(h, w), dtype=np.uint32) << 24
            maps = rng.integers(0, 1 << 32, size=(4, map_n, map_n), dtype=np.uint64).astype(np.uint32)
            kinds = [KINDS[(si + k + j) % 4] for j in range(k)]
            mvps = [_synth_light(kind, inv) for kind in kinds]
            proj = ref.project(arith, depth, inv, mvps, *SYNTH_FAZZ, map_n)
            if bias < (1 << 24):
                for l in range(k):
                    cand = np.argwhere(~proj["lit"][l] & (proj["code"][l] >= bias + 2))
                    if len(cand):
                        y, x = cand[len(cand) // 2]
                        ty, tx, code = proj["ty"][l, y, x], proj["tx"][l, y, x], int(proj["code"][l, y, x])
                        word = code - bias - ((si + k + l) % 2)
                        maps[l, ty, tx] = (maps[l, ty, tx] & 0xFF000000) | np.uint32(word)
            stats = {}
            expect = ref.resolve(proj, maps, radius, bias, stats)
            tapped = ~proj["lit"]
            classes = {c: int(proj[c].sum()) for c in ("behind", "left", "right", "top", "bottom", "far", "near", "nan")}
            classes.update(border_left=int((tapped & (proj["tx"] <= radius)).sum()), border_right=int((tapped & (proj["tx"] >= map_n - 1 - radius)).sum()),
                           border_top=int((tapped & (proj["ty"] <= radius)).sum()), border_bottom=int((tapped & (proj["ty"] >= map_n - 1 - radius)).sum()),
                           equal=stats["equal"], one_above=stats["one_above"], sky=int(proj["sky"].sum()), tapped=int(tapped.sum()))
            out.append(dict(size=(w, h), depth=depth, maps=maps, mvps=mvps, kinds=kinds, inverse_camera=inv, fazz=SYNTH_FAZZ, expect=expect, classes=classes))
    return out


def synthetic_class_totals(map_n, radius, bias):
    total = dict.fromkeys(CLASSES, 0)
    for launch in synthetic_launches(map_n, radius, bias):
        for c in CLASSES:
            total[c] += launch["classes"][c]
    return total


def check_synthetic_classes(map_n, radius, bias):
    """every class of the rule occurs in the case; with bias = 2^24 the two equality classes are empty by arithmetic"""
    total = synthetic_class_totals(map_n, radius, bias)
    for c in CLASSES:
        if bias >= (1 << 24) and c in ("equal", "one_above"):
            assert total[c] == 0, (c, total)
        else:
            assert total[c] > 0, (f"class {c} does not occur with map {map_n}, radius {radius}, bias {bias}", total)
    return total


@pytest.mark.parametrize("map_n", MAP_SIZES)
@pytest.mark.parametrize("radius", RADII)
def test_synthetic_cases_hold_every_class(map_n, radius):
    for bias in BIASES:
        total = check_synthetic_classes(map_n, radius, bias)
        if bias == 0:
            print(f"[shadow mask] synthetic map {map_n} radius {radius}: {total}")
        values = np.unique(np.concatenate([l["expect"][..., :len(l["mvps"])].reshape(-1) for l in synthetic_launches(map_n, radius, bias)]))
        taps = (2 * radius + 1) ** 2
        assert set(values.tolist()) <= set(ref.encode_unorm8(np.arange(taps + 1, dtype=F32) / F32(taps)).tolist())
        if bias < (1 << 24) and radius > 0 and map_n > 1:  # (a 1 x 1 map has one texel: 8 or 9 of 9 taps pass)
            assert len(values) >= 3, values  # partial visibility occurs, not only 0 and 255
        for l in synthetic_launches(map_n, radius, bias):
            assert (l["expect"][..., len(l["mvps"]):] == 255).all()


# ---- known answer -----------------------------------------------------------------------------------------------------------------
MAP_N = 128
CAM_W, CAM_H = 96, 64
OCC = 0.4                        # the occluder's outline in the light's NDC: the square |x|, |y| <= OCC
Z_OCC = 0.975                    # its depth there
Z_FLOOR = (0.990, 0.994)         # the floor's depth at ndc.y = -FLOOR_REACH and +FLOOR_REACH: tilted, ~584 codes per texel of 128
FLOOR_REACH = 0.9


def _unproject(m, ndc):
    w = np.asarray(ndc, np.float64) @ np.linalg.inv(np.asarray(m, np.float64)).T
    return w[:, :3] / w[:, 3:4]


def _add_quad(scene, m, corners):
    """an untextured quad with identity model from four NDC corners unprojected through m (shadow_light.add_backdrop's way)"""
    pos = _unproject(m, corners).astype(F32)
    mesh = scene.add_mesh(pos, np.array([[0, 0, 1]] * 4, F32), np.zeros((4, 2), F32), np.array([0, 1, 2, 0, 2, 3], np.uint32))
    scene.add_draw(scene.add_transform(np.eye(4, dtype=F32)), mesh)


@functools.lru_cache(maxsize=None)
def occluder_case():
    """-> dict(map words [128, 128], depth words [64, 96], setup, light matrix, texel coordinates of every camera pixel in the
    map (float64, analytic), floor (the pixel shows the floor)).  Light A; floor and occluder from unprojected NDC corners; the
    camera sits 40 % of the way from the shadow's edge on the floor towards the light and looks at that edge, so the occluder is
    behind it and both sides of the edge fill its picture."""
    m = sl.mvp("A")
    sc = scn.Scene()
    r, (z0, z1) = FLOOR_REACH, Z_FLOOR
    _add_quad(sc, m, [[-r, -r, z0, 1], [r, -r, z0, 1], [r, r, z1, 1], [-r, r, z1, 1]])
    _add_quad(sc, m, [[-OCC, -OCC, Z_OCC, 1], [OCC, -OCC, Z_OCC, 1], [OCC, OCC, Z_OCC, 1], [-OCC, OCC, Z_OCC, 1]])
    words = sl.expected(sc, m, MAP_N)
    target = _unproject(m, [[OCC, 0.0, 0.5 * (z0 + z1), 1.0]])[0]
    eye = target + 0.4 * (sl.eye("A").astype(np.float64) - target)
    setup = FrameSetup(CAM_W, CAM_H)
    f32 = lambda a: np.asarray(a, dtype=F32).astype(np.float64)  # noqa: E731
    setup.view = f32(camera.look_at_rh(eye, target, (0.0, -1.0, 0.0)))
    setup.prev_view = setup.view
    setup.mvp = setup.prev_mvp = f32(setup.proj @ setup.view)
    setup.inv_view = setup.prev_inv_view = f32(np.linalg.inv(setup.view))
    chain = PostFxChain(CAM_W, CAM_H, backend="oracle", setup=setup)
    chain.raster(sc)
    depth = chain.depth.raw(0)[..., 0].astype(np.uint32)
    # where every camera pixel lies in the light's map, analytically in double
    gy, gx = np.mgrid[0:CAM_H, 0:CAM_W]
    d = (depth & sl.D24_MAX).astype(np.float64) / float(sl.D24_MAX)
    ndc = np.stack([(gx + 0.5) / CAM_W * 2 - 1, (gy + 0.5) / CAM_H * 2 - 1, d, np.ones_like(d)], axis=-1).reshape(-1, 4)
    world = _unproject(setup.mvp, ndc)
    clip = np.concatenate([world, np.ones((len(world), 1))], axis=1) @ m.astype(np.float64).T
    lndc = clip[:, :3] / clip[:, 3:4]
    texel = ((0.5 * lndc[:, :2] + 0.5) * MAP_N).reshape(CAM_H, CAM_W, 2)
    floor = ((depth & sl.D24_MAX) != sl.D24_MAX) & (lndc[:, 2].reshape(CAM_H, CAM_W) > 0.5 * (Z_OCC + Z_FLOOR[0]))
    return dict(words=words, depth=depth, setup=setup, mvp=m, texel=texel, floor=floor)


def occluder_bias(words, radius):
    """the largest difference in D24 codes between floor texels radius + 1 apart in the map, plus 1.  Floor texels: covered, and
    at least one texel outside the occluder's outline."""
    lo, hi = (0.5 - 0.5 * OCC) * MAP_N - 1, (0.5 + 0.5 * OCC) * MAP_N + 1
    idx = np.arange(MAP_N) + 0.5
    in_occ = (idx[None, :] > lo) & (idx[None, :] < hi) & (idx[:, None] > lo) & (idx[:, None] < hi)
    floor = (words != sl.D24_MAX) & ~in_occ
    w = words.astype(np.int64)
    s = radius + 1
    dx = np.abs(w[:, s:] - w[:, :-s])[floor[:, s:] & floor[:, :-s]]
    dy = np.abs(w[s:, :] - w[:-s, :])[floor[s:, :] & floor[:-s, :]]
    return int(max(dx.max(), dy.max())) + 1


def occluder_classes(case, radius):
    """(inside, outside): floor pixels that project at least radius + 2 texels inside / outside the occluder's outline"""
    lo, hi = (0.5 - 0.5 * OCC) * MAP_N, (0.5 + 0.5 * OCC) * MAP_N
    t, g = case["texel"], radius + 2
    inside = case["floor"] & (t[..., 0] >= lo + g) & (t[..., 0] <= hi - g) & (t[..., 1] >= lo + g) & (t[..., 1] <= hi - g)
    outside = case["floor"] & ((t[..., 0] <= lo - g) | (t[..., 0] >= hi + g) | (t[..., 1] <= lo - g) | (t[..., 1] >= hi + g))
    return inside, outside


def check_occluder_mask(case, radius, channel):
    """the two assertions of the known answer on light A's channel [h, w]"""
    inside, outside = occluder_classes(case, radius)
    figures = f"radius {radius}: bias {occluder_bias(case['words'], radius)}, {int(inside.sum())} pixels inside, {int(outside.sum())} outside"
    print("[shadow mask]", figures, "| values inside", np.unique(channel[inside]).tolist(), "outside", np.unique(channel[outside]).tolist())
    assert inside.sum() >= 100 and outside.sum() >= 100, figures
    assert (channel[inside] == 0).all(), figures
    assert (channel[outside] == 255).all(), figures


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_known_answer_occluder(radius):
    case = occluder_case()
    s = case["setup"]
    arith = ref.Arith(int(abi.product().vkr_numeric_contract()))
    stats = {}
    mask = ref.shadow_mask(arith, case["depth"], case["words"][None], s.inv_view, [case["mvp"]], *s.fazz, radius, occluder_bias(case["words"], radius), stats)
    assert (mask[..., 1:] == 255).all()
    assert stats["taps"] > 0
    check_occluder_mask(case, radius, mask[..., 0])
    sky = (case["depth"] & sl.D24_MAX) == sl.D24_MAX
    assert (mask[sky] == 255).all()
