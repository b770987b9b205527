"""An exact reference of the frozen raster rules (DESIGN_NUMERICS.md, "Raster stage"), written from that prose and from nothing
else: test infrastructure for tests/test_raster_geometry.py and tests/test_raster_geometry_gpu.py.

What it is: every pixel centre of the viewport tested against every triangle with integer arithmetic, the fill rule stated
geometrically (through the triangle's third vertex, not through the direction of an oriented edge), the owner of a pixel found by
comparing all covering triangles at once, and the depth as the exact rational number sum(e_k z_k) / area2 evaluated in float64.
What it is not: it has no bounding box, no 8 x 8 blocks, no small / large split, no orientation swap, no depth buffer that
triangles are drawn into one after another and no fp32 interpolation; it knows nothing of attributes, textures or the near clip
(the caller clips; see raster_geometry.clip_near).  So a rule that the kernels, the oracle (oracle/raster.cpp) and the numpy cube
restatement (tests/cubemap_reference.py) all read wrongly in the same way does not pass here.

Input: clip positions float32 [T, 3, 4] in submission order (after the near clip), the viewport, and per triangle the submission
index it belongs to (the two halves of a clipped triangle share one) and whether it is drawn at all (a program may skip a draw).

Exactness of the float64 depth: e_k and area2 are integers below 2^60, converted to float64 with a relative error of 2^-53 each;
the three products, two sums and the quotient add 2^-53 each.  For z_k in [-2, 2] the result is within 2^-49 of the rational
depth, 2^-25 of a D24 code.  Where vertices and z_k are dyadic numbers with few bits (the tie classes) every step is exact.
"""
import numpy as np

F32 = np.float32
GUARD_PX = F32(1048576.0)
D24_SCALE = 16777215.0
EDGE_KINDS = ("top", "left", "bottom", "right", "sloped_accepting", "sloped_rejecting")
ACCEPTING = {"top": True, "left": True, "bottom": False, "right": False, "sloped_accepting": True, "sloped_rejecting": False}
LIMIT = 1 << 29  # every operand of an edge function stays at or below this, so a product is below 2^58 and a difference below 2^59


def depth_bound_codes(zmax=1.0):
    """By how many D24 codes rint(fp32 depth * 16777215) may differ from rint(exact depth * 16777215); derivation in
    DESIGN_NUMERICS.md ("Raster stage", depth bound).  With u = 2^-24 and |z_k| <= zmax: the rounding of l_k to fp32, the three
    products and the two sums each add at most u * zmax * (1 + 3u) to the depth, 4 u zmax (1 + 3u) in all, which is
    4 zmax (1 + 3u) codes; the product with 16777215 adds half an ulp of a number below 2^24 * zmax, 0.5 * zmax; each of the
    two rint adds 0.5.  The difference of two integers within 4 zmax (1 + 3u) + 0.5 zmax + 1 of each other is its floor."""
    zmax = max(1.0, float(zmax))
    return int(np.floor(4.0 * zmax * (1.0 + 3.0 * 2.0 ** -24) + 0.5 * zmax + 1.0))


def snap(clip, width, height):
    """clip float32 [T, 3, 4] -> (X, Y int64 [T, 3] in 1/256 px, z / w float32 [T, 3], kept bool [T]).  A triangle is kept when
    every corner has w > 0 and lies within the guard band; a NaN fails both tests."""
    clip = np.asarray(clip, F32)
    x, y, z, w = clip[..., 0], clip[..., 1], clip[..., 2], clip[..., 3]
    with np.errstate(all="ignore"):
        xs = ((x / w) * F32(0.5) + F32(0.5)) * F32(width)
        ys = ((y / w) * F32(0.5) + F32(0.5)) * F32(height)
        ok = (w > 0) & (np.abs(xs) <= GUARD_PX) & (np.abs(ys) <= GUARD_PX)
        kept = ok.all(axis=1)
        X = np.where(kept[:, None], np.rint(xs * F32(256.0)), 0).astype(np.int64)
        Y = np.where(kept[:, None], np.rint(ys * F32(256.0)), 0).astype(np.int64)
        zn = (z / w).astype(F32)
    return X, Y, zn, kept


def _edge(ax, ay, bx, by, px, py):
    for v in (bx - ax, py - ay, by - ay, px - ax):
        assert np.abs(v).max(initial=0) <= LIMIT, "an operand of an edge function exceeds 2^29"
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def edge_kind(ax, ay, bx, by, cx, cy):
    """the kind of edge a-b of the triangle whose third vertex is c (scalars, y down): a horizontal edge is a top edge when the
    triangle lies below it; any other edge is a left edge when the triangle lies to its right"""
    ax, ay, bx, by, cx, cy = (int(v) for v in (ax, ay, bx, by, cx, cy))
    if ay == by:
        return "top" if cy > ay else "bottom"
    # c.x minus the x of the line a-b at the height of c, times the positive number |b.y - a.y|
    right_of = ((cx - ax) * (by - ay) - (bx - ax) * (cy - ay)) * (1 if by > ay else -1)
    if ax == bx:
        return "left" if right_of > 0 else "right"
    return "sloped_accepting" if right_of > 0 else "sloped_rejecting"


class Result:
    """coverage bool [H, W]; owner int64 [H, W] (submission index, -1: none); depth float64 [H, W] (exact, NaN: none); d24 int64
    [H, W] (rint(depth * 16777215), 0xFFFFFF where uncovered); gap float64 [H, W]: by how many codes the second-nearest covering
    submission lies behind the owner (inf: none; 0: an exact tie between different submissions); layers int [H, W]: covering
    submissions; clip_band bool [H, W]: centres within the depth bound of the line along which the depth clip cuts a triangle;
    edge_hits {kind: count} of (centre, edge) pairs with the centre on that edge of a triangle's boundary;
    kept bool [T]: the triangle passed w > 0, the guard band, a finite depth and a non-zero area"""


def rasterise(clip, width, height, owner_ids=None, drawn=None, batch=128):
    clip = np.asarray(clip, F32).reshape(-1, 3, 4)
    T = len(clip)
    owner_ids = np.arange(T, dtype=np.int64) if owner_ids is None else np.asarray(owner_ids, np.int64)
    drawn = np.ones(T, bool) if drawn is None else np.asarray(drawn, bool)
    X, Y, zn, kept = snap(clip, width, height)
    kept = kept & drawn & np.isfinite(zn).all(axis=1)  # the depth clip rejects every fragment of a depth that is no number
    area2 = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    kept = kept & (area2 != 0)
    py, px = np.mgrid[0:height, 0:width]
    PX = (px.reshape(-1).astype(np.int64) << 8) + 128
    PY = (py.reshape(-1).astype(np.int64) << 8) + 128
    P = PX.size
    best_depth = np.full(P, np.inf)
    second_depth = np.full(P, np.inf)
    best_owner = np.full(P, -1, np.int64)
    layers = np.zeros(P, np.int64)
    band = np.zeros(P, bool)
    hits = {k: 0 for k in EDGE_KINDS}
    idx = np.nonzero(kept)[0]
    for start in range(0, len(idx), batch):
        t = idx[start:start + batch]
        B = len(t)
        sgn = np.sign(area2[t])[:, None]
        side = np.empty((3, B, P), np.int64)
        accept = np.empty((3, B), bool)
        kinds = []
        for k in range(3):  # edge k lies opposite corner k
            a, b = (k + 1) % 3, (k + 2) % 3
            side[k] = _edge(X[t, a][:, None], Y[t, a][:, None], X[t, b][:, None], Y[t, b][:, None], PX[None, :], PY[None, :]) * sgn
            kk = [edge_kind(X[i, a], Y[i, a], X[i, b], Y[i, b], X[i, k], Y[i, k]) for i in t]
            kinds.append(kk)
            accept[k] = [ACCEPTING[v] for v in kk]
        on_boundary = (side >= 0).all(axis=0)  # inside the closed triangle
        for k in range(3):
            on = on_boundary & (side[k] == 0)
            n = on.sum(axis=1)
            for i in np.nonzero(n)[0]:
                hits[kinds[k][i]] += int(n[i])
        inside = ((side > 0) | ((side == 0) & accept[:, :, None])).all(axis=0)
        z = zn[t].astype(np.float64)
        with np.errstate(all="ignore"):
            depth = ((side[0].astype(np.float64) * z[:, 0:1] + side[1].astype(np.float64) * z[:, 1:2]) + side[2].astype(np.float64) * z[:, 2:3]) \
                / np.abs(area2[t]).astype(np.float64)[:, None]
        # A triangle with a corner beyond a limit of the depth range is cut there along a line; which side of the cut a centre
        # within the depth bound of the line falls on is decided by fp32 rounding: such centres are reported in clip_band.  A
        # triangle whose corners all lie inside the range has no such line (its depth cannot leave the range of its corners).
        straddles = ((z.min(axis=1) < 0.0) | (z.max(axis=1) > 1.0))[:, None]
        eps = (depth_bound_codes(np.abs(z).max(initial=1.0)) + 1) / D24_SCALE
        with np.errstate(invalid="ignore"):
            band |= (inside & straddles & ((np.abs(depth) < eps) | (np.abs(depth - 1.0) < eps))).any(axis=0)
        inside &= (depth >= 0.0) & (depth <= 1.0)  # the depth clip per fragment
        depth = np.where(inside, depth, np.inf)
        # one after the other inside a batch: a later submission wins an exact tie
        for i in range(B):
            d, own = depth[i], owner_ids[t[i]]
            m = np.nonzero(inside[i])[0]
            if m.size == 0:
                continue
            dm = d[m]
            same = best_owner[m] == own  # the other half of a clipped triangle: one submission
            layers[m] += ~same
            wins = (dm < best_depth[m]) | ((dm == best_depth[m]) & (own >= best_owner[m]))
            # what becomes the runner-up: the old best where it is beaten by another submission, else the newcomer where it loses
            lose = m[~wins & ~same]
            second_depth[lose] = np.minimum(second_depth[lose], d[lose])
            w_other = m[wins & ~same]
            second_depth[w_other] = np.minimum(second_depth[w_other], best_depth[w_other])
            w_all = m[wins]
            best_depth[w_all] = d[w_all]
            best_owner[w_all] = own
    r = Result()
    covered = best_owner >= 0
    r.coverage = covered.reshape(height, width)
    r.owner = best_owner.reshape(height, width)
    r.depth = np.where(covered, best_depth, np.nan).reshape(height, width)
    with np.errstate(invalid="ignore"):
        r.d24 = np.where(covered, np.rint(np.where(covered, best_depth, 0.0) * D24_SCALE), 0xFFFFFF).astype(np.int64).reshape(height, width)
        r.gap = ((second_depth - best_depth) * D24_SCALE).reshape(height, width)
    r.gap[~r.coverage] = np.inf
    r.layers = layers.reshape(height, width)
    r.clip_band = band.reshape(height, width)
    r.edge_hits = hits
    r.kept = kept
    r.snapped = (X, Y, zn, area2)
    return r
