"""The tile plane regression without a GPU: the C-ABI push block, the program table and the stage value, what the host mirror
records (vkrh_selftest_tile_regression), the formula of the numpy restatement (tests/tile_regression_reference.py) against
np.linalg.lstsq in float64, its summation order, the quirks the port keeps, and the properties of the restatement's result on
the synthetic depth that keep the GPU parity test (tests/test_tile_regression_gpu.py) from being vacuous."""
import ctypes as C

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd.chain import PostFxChain

import tile_regression_reference as ref
from gtao_rt_reference import butterfly_sum

F32 = np.float32


def test_push_layout_and_entry():
    assert C.sizeof(abi.TileRegressionPush) == 80
    assert abi.TileRegressionPush.fovy.offset == 64
    txt = open(abi.ROOT + "/include/vkr_postfx.h").read()
    assert "int vkr_tile_regression(" in txt and "vkr_tile_regression_push" in txt
    assert hasattr(abi.product(), "vkr_tile_regression")


def test_program_and_stage_are_registered():
    assert host.lib().vkrh_has_program(b"tile_regression") == 1
    assert host.STAGE_TILE_REGRESSION == 1 << 26
    assert not host.STAGE_CHAIN & host.STAGE_TILE_REGRESSION


def _malloc_allocator(l):
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    alloc = host._ALLOC(lambda n, u: libc.malloc(n))
    free = host._FREE(lambda p, u: libc.free(p))
    l.vkrh_set_allocator(alloc, free, None)
    return alloc, free


@pytest.fixture(scope="module")
def selftest():
    """{first word of the line: rest of the line}"""
    l = host.lib()
    keep = _malloc_allocator(l)
    try:
        buf = C.create_string_buffer(8192)
        assert l.vkrh_selftest_tile_regression(buf, 8192) == 0, l.vkrh_last_error().decode()
    finally:
        l.vkrh_set_allocator(host._ALLOC(0), host._FREE(0), None)
    del keep
    return dict(line.split(":", 1) for line in buf.value.decode().splitlines())


def test_mirror_records_the_references_task(selftest):
    """advanced_ssr.cpp:521-525: task "SSSR_Tile_Regression" samples depth mip 1 and stores into tile_planes mip 0; nothing else.
    The image is (64 / 16, 48 / 16) RGBA32F (VK_FORMAT_R32G32B32A32_SFLOAT = 109), allocated by the call."""
    words = selftest["images"].split()
    depth, planes = int(words[1]), int(words[3])
    assert selftest["SSSR_Tile_Regression"].split() == [f"R{depth}.1", f"W{planes}.0"], selftest
    assert [k for k in selftest if k not in ("images", "tile_planes", "push 80")] == ["SSSR_Tile_Regression"], selftest
    assert selftest["tile_planes"].split() == ["4x3", "format", "109"]


def test_push_holds_the_transposed_normal_matrix(selftest):
    """the selftest's normal matrix is column-major 1..16 (not symmetric): camera_to_world = transpose, then the four floats"""
    push = np.array([float(v) for v in selftest["push 80"].split()], F32)
    assert push.shape == (20,)
    normal_mat = np.arange(1, 17, dtype=F32).reshape(4, 4)  # [column, row] as stored
    assert np.array_equal(push[:16].reshape(4, 4), normal_mat.T)
    assert not np.array_equal(push[:16].reshape(4, 4), normal_mat)
    assert np.array_equal(push[16:], np.array([1.0, 1.5, 0.05, 80.0], F32))


def _contract():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


# a camera that is not axis-aligned: the fit runs on rotated vectors
CAMERA_TO_WORLD = np.array([[0.36, 0.48, -0.8, 3.0], [-0.8, 0.6, 0.0, -1.5], [0.48, 0.64, 0.6, 0.25], [0.0, 0.0, 0.0, 1.0]], F32)
FAZZ = (1.0, 16.0 / 9.0, 0.05, 80.0)
# view-space planes normal . p = -k that cover the whole 128 x 72 view inside the depth range (plane_depth_bits checks it):
# a wall at z = -2 (constant depth), a floor seen from a camera pitched down, a plane tilted about both axes
PLANES = {"wall": ((0.0, 0.0, 1.0), 2.0), "floor": ((0.0, 1.0, 0.7), 1.0), "tilted": ((0.4, 0.3, 1.0), 3.0)}


@pytest.mark.parametrize("name", sorted(PLANES))
def test_formula_against_lstsq_in_float64(name):
    """The float64 mode solves the normal equations N p = s with N = R^T R through the adjugate; lstsq solves min |R p - 1|
    through the SVD.  The normal equations lose cond(N) * eps of the solution, lstsq no more than that, so on coefficients of
    size 0.1 .. 1 the two agree within 100 * cond(N) * 2.2e-16 (100: the constants of both bounds, the 64-term sums and the
    cancellation in the cofactors).  The mean squared residual follows: |e^2 - e'^2| <= (|e| + |e'|) * |de| per lane, with
    |de| <= 3 * tol * |r|_max."""
    normal, k = PLANES[name]
    bits = ref.plane_depth_bits(128, 72, normal, k, *FAZZ)
    r = ref.tile_points(_contract(), bits, CAMERA_TO_WORLD, *FAZZ, mode="fp64").reshape(-1, 64, 3)
    plane, mean = ref.fit(_contract(), r, mode="fp64")
    worst = 0.0
    for t in range(r.shape[0]):
        cond = np.linalg.cond(r[t].T @ r[t])
        assert cond < 1e8, (name, t, cond)
        tol = 100.0 * cond * 2.2e-16
        want = np.linalg.lstsq(r[t], np.ones(64), rcond=None)[0]
        err = np.abs(plane[t] - want).max()
        worst = max(worst, err / tol)
        assert err <= tol, (name, t, plane[t], want, cond)
        e = r[t] @ want - 1.0
        de = 3.0 * tol * np.abs(r[t]).max()
        assert abs(mean[t] - np.mean(e * e)) <= (2.0 * np.abs(e).max() + de) * de + 1e-30, (name, t, mean[t], np.mean(e * e))
    print(f"[tile_regression] {name}: worst error / bound {worst:.3g}")


def test_tree_order_is_the_wave_butterfly_in_every_lane():
    """fp32 addition is commutative, so the xor butterfly leaves in EVERY lane the bits the shader's tree leaves in s[0]"""
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((257, 64)) * np.exp2(rng.integers(-20, 20, (257, 64)))).astype(F32)
    tree = ref.tree_sum(v)
    assert np.array_equal(tree.view(np.uint32), butterfly_sum(v).view(np.uint32))
    lanes = ref.xor_butterfly(v)
    assert np.array_equal(lanes.view(np.uint32), np.broadcast_to(tree[:, None], lanes.shape).view(np.uint32))
    assert not np.array_equal(tree, v.sum(axis=1, dtype=F32))  # and the order matters: numpy's own pairwise sum differs


def test_outside_lanes_count_in_the_mean():
    """125 x 71 view of the constant-depth wall: the right column of tiles has 3 columns outside (24 lanes), the bottom row one
    row (8 lanes), the corner 24 + 8 - 3 = 29.  The inside lanes lie on one plane, which the float64 fit reproduces to ~1e-12,
    an outside lane has r = 0 and the residual (0 - 1)^2 = 1: the mean is k / 64."""
    normal, k = PLANES["wall"]
    bits = ref.plane_depth_bits(125, 71, normal, k, *FAZZ)
    out = ref.tile_regression(_contract(), bits, CAMERA_TO_WORLD, *FAZZ, 16, 9, mode="fp64")
    lanes = np.zeros((9, 16))
    lanes[:, 15] += 24
    lanes[8, :] += 8
    lanes[8, 15] -= 3
    assert np.abs(out[..., 3] - lanes / 64.0).max() <= 1e-12, np.abs(out[..., 3] - lanes / 64.0).max()
    assert np.isfinite(out[..., :3]).all()
    # the fp32 mode counts the same lanes: its inside lanes miss the plane by the fit's fp32 error, never by as much as 1 / 64
    out32 = ref.tile_regression(_contract(), bits, CAMERA_TO_WORLD, *FAZZ, 16, 9)
    assert out32.dtype == F32 and (np.floor(out32[..., 3] * 64.0 + 0.5) == lanes).all()


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_nan_plane_gives_1e10(mode):
    """64 lanes of r = 0 (and 64 of NaN): det = 0, 1 / det = inf, cofactor 0 * inf = NaN; every residual is 1e10, so is the mean"""
    T = F32 if mode == "fp32" else np.float64
    r = np.zeros((2, 64, 3), T)
    r[1] = np.nan
    plane, mean = ref.fit(_contract(), r, mode)
    assert np.isnan(plane).all()
    assert mean.dtype == T and (mean == T(1e10)).all(), mean


def test_restatement_on_the_synthetic_depth_is_not_trivial():
    """Bounds from what the formula gives on this depth, not from any kernel: the synthetic scene is piecewise planar, so most
    tiles fit a finite plane (all 144 do) with a residual that is fp32 noise (10th percentile 2e-9), while tiles across a
    silhouette miss by a few tenths (99th percentile 0.28): eight decades.  Asserted: three quarters of the planes finite, three
    decades between those percentiles, and planes that differ from tile to tile — a constant image shows none of the three."""
    W, H = 256, 144
    chain = PostFxChain(W, H, backend="oracle")
    chain.synth()
    chain.downsample()
    depth = chain.depth.raw(1)[..., 0]
    assert depth.shape == (H // 2, W // 2)
    cam = np.linalg.inv(chain.setup.view.astype(np.float64)).astype(F32)
    out = ref.tile_regression(_contract(), depth, cam, *chain.setup.fazz, 16, 9)
    finite = np.isfinite(out[..., :3]).all(axis=-1)
    res = out[..., 3][finite]
    lo, hi = np.percentile(res, 10), np.percentile(res, 99)
    figures = f"finite planes {int(finite.sum())} of {finite.size}, residual p10 {lo:.3g} p99 {hi:.3g} max {res.max():.3g}, distinct planes {len(np.unique(out[..., 0]))}"
    print("[tile_regression]", figures)
    assert finite.sum() * 4 >= finite.size * 3, figures
    assert lo > 0 and hi >= 1000.0 * lo, figures
    assert len(np.unique(out[..., 0])) >= finite.size // 2, figures
