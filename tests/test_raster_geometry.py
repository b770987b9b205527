"""CPU tests of the constructed raster geometry (tests/raster_geometry.py): every class, for every program, through the program's
checker -- the oracle's G-buffer rasteriser (oracle/raster.cpp) for gbuf_opaque_taa and, under the light's matrix, for
default_shadow; the numpy restatement tests/cubemap_reference.py for cubemap_probe -- against the exact reference of the raster
rules (tests/raster_rules_reference.py): coverage equal as a set, the owner equal (read through the depth, and through the palette
colour where depths tie), the depth within the derived bound of the exact depth.  Every class's non-vacuity floor is asserted here,
on the reference alone, so the GPU tests (tests/test_raster_geometry_gpu.py) cannot go vacuous."""
import numpy as np
import pytest

import cubemap_reference as cref
import raster_geometry as rg
import raster_rules_reference as rr


def oracle_gbuf(scene, w, h):
    return rg.Gbuf(w, h, "oracle").raster(scene)


def variants(name, program):
    v = rg.CLASSES[name].get(program)
    if v is None:
        return []
    return v if isinstance(v, list) else [v]


CASES = [(name, program, args) for name in rg.CLASSES for program in ("gbuf", "shadow", "cube") for args in variants(name, program)]
IDS = [f"{n}-{p}-{'x'.join(str(a) for a in args)}" for n, p, args in CASES]


# ---- the rules themselves, on cases small enough to do by hand ----
def test_reference_fill_rule_by_hand():
    """The square [4, 12) x [2, 6) of pixel corners as two triangles: the 8 x 4 centres inside, each once.  Centres on the left and
    the top edge belong to it, those on the right and the bottom edge do not (there are none: corners, not centres); then the same
    square moved by half a pixel, so that every border lies on centres."""
    case = rg.Case("by_hand", 16, 8)
    case.tri(case.px([(4, 2), (12, 2), (12, 6)], 0.25))
    case.tri(case.px([(4, 2), (12, 6), (4, 6)], 0.5))
    r = case.reference()
    want = np.zeros((8, 16), bool)
    want[2:6, 4:12] = True
    assert np.array_equal(r.coverage, want) and (r.layers[want] == 1).all()
    assert r.d24[2, 11] == round(0.25 * 16777215) and r.d24[5, 4] == round(0.5 * 16777215)
    # the diagonal x - 4 = 2 (y - 2) passes through centres (x + .5 - 4) = 2 (y + .5 - 2): none (x would be a half), so move it
    case = rg.Case("by_hand_centres", 16, 8)
    case.tri(case.px([(4.5, 2.5), (12.5, 2.5), (12.5, 6.5)], 0.25))   # upper right: its diagonal is a left edge
    case.tri(case.px([(4.5, 2.5), (4.5, 6.5), (12.5, 6.5)], 0.5))     # lower left, other winding: the diagonal is a right edge
    r = case.reference()
    want = np.zeros((8, 16), bool)
    want[2:6, 4:12] = True  # centres 4.5 .. 11.5 x 2.5 .. 5.5: left column and top row in, right column (12.5) and bottom row (6.5) out
    assert np.array_equal(r.coverage, want) and (r.layers[want] == 1).all()
    # centres on the diagonal (x - 4) = 2 (y - 2): (4, 2), (6, 3), (8, 4), (10, 5) go to the upper right triangle
    for x, y in ((4, 2), (6, 3), (8, 4), (10, 5)):
        assert r.owner[y, x] == 0
    assert r.owner[3, 5] == 1 and r.owner[3, 7] == 0
    # centres on the closed boundary, corners included: 9 on each horizontal edge, 5 on each vertical one and on the diagonal
    assert r.edge_hits["top"] == 9 and r.edge_hits["left"] == 5 and r.edge_hits["right"] == 5 and r.edge_hits["bottom"] == 9
    assert r.edge_hits["sloped_accepting"] == 5 and r.edge_hits["sloped_rejecting"] == 5


def test_reference_owner_and_ties_by_hand():
    case = rg.Case("ties_by_hand", 8, 8)
    full = np.array([[-1, -1, 0.5], [3, -1, 0.5], [-1, 3, 0.5]], np.float32)
    for n in range(3):
        case.tri(full if n != 1 else full[[0, 2, 1]])
    near = full.copy()
    near[:, 2] = 0.25
    case.tri(near * np.array([0.25, 0.25, 1], np.float32))
    r = case.reference()
    assert r.coverage.all() and (r.layers >= 3).all()
    assert set(np.unique(r.owner)) == {2, 3} and (r.owner == 3).sum() >= 1
    assert (r.gap[r.owner == 2] == 0).all() and (r.gap[r.owner == 3] > 4e6).all()


def test_depth_bound_is_a_handful_of_codes():
    assert rr.depth_bound_codes(1.0) == 5 and rr.depth_bound_codes(1.5) == 7


def test_clip_near_of_the_classes_own_by_hand():
    """the class's Sutherland-Hodgman: counts for the eight masks, the crossing from the inside vertex, corners on the plane stay"""
    def tri(z):
        return np.array([[0, 0, z[0], 1], [1, 0, z[1], 1], [0, 1, z[2], 1]], np.float32)
    for mask in range(8):
        z = [0.5 if mask >> k & 1 else -0.5 for k in range(3)]
        n = len(rg.clip_near(tri(z)))
        assert n == {0: 0, 7: 3}.get(mask, 3 if bin(mask).count("1") == 1 else 4)
    poly = rg.clip_near(tri([0.5, -0.5, 0.5]))
    assert np.allclose(poly[1], [0.5, 0, 0, 1]) and np.allclose(poly[2], [0.5, 0.5, 0, 1])
    assert len(rg.clip_near(tri([-0.0, 0.0, 0.5]))) == 3 and len(rg.clip_near(tri([0.0, -0.5, -0.5]))) == 3


# ---- the floors: what each class must contain, by the reference alone ----
def _floors_world(name, case, r):
    """the classes placed in world space for the cube bake alone"""
    c = case.contains
    owned = np.bincount(r.owner[r.owner >= 0], minlength=len(case.pos))
    clip = case.clip()
    if name == "near_plane":
        assert len(c["masks"]) == 16
        for (mask, winding), i in c["masks"].items():
            inside = rg.inside_mask(clip[i][[0, 2, 1]] if winding else clip[i])
            assert inside == mask, (mask, winding, inside)
            assert (owned[i] > 0) == (mask != 0), (mask, winding, owned[i])
        for i, j in c["pairs"]:
            assert 0 < rg.inside_mask(clip[i]) < 7 and 0 < rg.inside_mask(clip[j]) < 7, "both triangles of a pair cross the plane"
        _union_of_pairs_is_covered(case, r)
    elif name == "guard_band":
        assert r.kept_submission[c["kept"]].all() and (owned[c["kept"]] > 0).all(), owned[c["kept"]]
        assert not r.kept_submission[c["dropped"]].any()
        assert (owned[c["neighbours"]] > 0).all()
        X, Y = r.snapped[0], r.snapped[1]
        assert max(np.abs(X).max(), np.abs(Y).max()) == 2 ** 28, "a corner on exactly 2^20 px"
    elif name == "depth_range":
        assert owned[c["far_cut"]] > 20 and owned[c["before_far"]] > 20 and owned[c["after_near"]] > 20 and owned[c["beyond"]] == 0
        assert r.kept_submission[c["beyond"]], "set up, and every fragment clipped"
        box = np.argwhere(r.owner == c["far_cut"])
        assert r.layers[box[:, 0].min():box[:, 0].max() + 1, box[:, 1].min():box[:, 1].max() + 1].min() == 0, "the cut leaves a part undrawn"
        assert r.d24[r.owner == c["before_far"]].min() > 0.999 * 16777215 and r.d24[r.owner == c["after_near"]].max() < 0.01 * 16777215
        assert r.clip_band.sum() < 0.1 * owned[c["far_cut"]]


def _floors(name, program, case, r):
    if getattr(case, "world", False):
        return _floors_world(name, case, r)
    c = case.contains
    T = len(case.pos)
    owned = np.bincount(r.owner[r.owner >= 0], minlength=T)
    if name == "centre_lattice":
        for kind in rr.EDGE_KINDS:
            assert r.edge_hits[kind] >= 20, (kind, r.edge_hits)
        assert sum(r.edge_hits.values()) >= c["min_on_edge_centres"]
        for x0, y0, x1, y1 in c["single_cover_regions"]:
            ys, xs = np.mgrid[0:case.height, 0:case.width]
            inside = (xs + 0.5 >= x0) & (xs + 0.5 < x1) & (ys + 0.5 >= y0) & (ys + 0.5 < y1)
            assert inside.sum() > 500 and (r.layers[inside] == 1).all(), "the mesh is closed: no gap, no double cover"
        # accepted centres in the last column / row of an 8 x 8 block on a left / top edge: what a block cull must keep
        ys, xs = np.nonzero(r.coverage)
        assert ((xs % 8 == 7).sum() > 100) and ((ys % 8 == 7).sum() > 100)
        assert (r.gap[r.coverage] > 2 * rr.depth_bound_codes() + 2).all()
    elif name == "exact_ties":
        last_a, last_b = c["same_in_draw"][-1], c["same_across_draws"][-1]
        assert owned[last_a] > 200 and owned[last_b] > 50, "the last copy owns the whole triangle"
        assert owned[c["same_in_draw"][:-1]].sum() == 0 and owned[c["same_across_draws"][:-1]].sum() == 0
        for first, second in c["coplanar_pairs"]:
            tied = (r.owner == second) & (r.gap == 0)
            assert tied.sum() >= c["min_tied_centres_per_pair"], int(tied.sum())
            assert owned[first] > 0 or owned[second] > tied.sum()
        assert ((r.gap == 0) | (r.gap > 2 * rr.depth_bound_codes() + 2))[r.coverage].all()
    elif name == "block_split":
        assert c["blocks"] == [1, 2, 64, 65, 72] and (owned[:8] > 0).all()
    elif name == "offscreen_reach":
        assert (owned[[i for i in c["covering"] if i != c["surrounding"][0]]] > 0).all(), owned  # the first surrounding one is hidden by the second
        assert owned[c["outside"]].sum() == 0
        assert r.coverage.all(), "the surrounding triangle covers what nothing else does"
        X, Y, _, _ = r.snapped[:4]
        assert np.abs(X).max() > 2 ** 27 and np.abs(Y).max() > 2 ** 27
    elif name == "guard_band":
        assert r.kept_submission[c["kept"]].all() and (owned[c["kept"]] > 0).all(), owned[c["kept"]]
        assert not r.kept_submission[c["dropped"]].any(), np.asarray(c["dropped"])[r.kept_submission[c["dropped"]]]
        assert (owned[c["neighbours"]] > 0).all()
    elif name == "slivers":
        assert owned[c["slivers"]].sum() == 0 and owned[c["nothing"]].sum() == 0
        assert (owned[c["one_centre"]] == 1).all(), owned[c["one_centre"]]
        assert c["needles"] or owned[c["ordinary"]] > 0.25 * case.width * case.height  # (the needles hide it: one per pixel)
        listed = sum(1 for i in c["slivers"][:40] if rg.centre_blocks(case, i) > 0)
        assert listed == 40, "a sliver's bounding box holds pixel centres: it is set up and listed"
        hidden = int((owned[c["needles"]] != 1).sum())  # the four one-centre slivers are nearer than the needles of their pixels
        assert hidden <= len(c["one_centre"]) and (owned[c["needles"]] <= 1).all()
        if program in ("shadow", "cube"):
            waves = rg.shadow_small_waves(T) if program == "shadow" else rg.cube_small_waves(T)
            records = len(c["needles"]) + len(c["slivers"]) + len(c["one_centre"])  # the ordinary triangle goes to the large list
            assert rg.centre_blocks(case, c["ordinary"]) > 64
            assert records - waves > len(c["slivers"]) + hidden, "the last turn of the small-list loop holds records that draw"
    elif name == "large_flood":
        assert (owned[c["large"]] >= c["min_owned_per_large"]).all(), owned[c["large"]].min()
        assert (r.gap[r.coverage] > 2 * rr.depth_bound_codes() + 2).all()
        if program == "gbuf":
            assert c["chunks"] > rg.RASTER_LARGE_WAVES, "the large kernel's loop takes a second turn"
    elif name == "near_plane":
        for (draw, mask, winding), i in c["masks"].items():
            assert rg.inside_mask(case.pos[i]) == mask
            assert (owned[i] > 0) == (mask != 0), (draw, mask, winding, owned[i])
        assert len(c["masks"]) == 32
        assert (owned[c["on_plane"][:3]] > 0).all()
        _union_of_pairs_is_covered(case, r)
    elif name == "depth_range":
        assert owned[c["z0"]] > 100 and owned[c["minus_zero"]] > 100 and owned[c["far_cut"]] > 100 and owned[c["z1"]] > 100
        assert r.clip_band.sum() < 0.1 * owned[c["far_cut"]], "the far cut is a line"
        box = np.argwhere(r.owner == c["far_cut"])
        assert r.layers[box[:, 0].min():box[:, 0].max() + 1, box[:, 1].min():box[:, 1].max() + 1].min() == 0, "the cut leaves a part undrawn"
        assert (r.d24[r.owner == c["z1"]] == 0xFFFFFF).all()
        assert (r.d24[r.owner == c["z0"]] == 0).all()
    elif name == "tiny_targets":
        assert r.coverage.all()


class _Plain:
    zmax = 1.0


@pytest.mark.parametrize("program,args", [(p, a) for p in ("gbuf", "shadow", "cube") for a in rg.TABLES[p]])
def test_tables_checker_agrees_with_the_exact_reference(program, args, oracle_lib):
    """1, 8, 9, 17 (33) draws, draws of 0, 1 and 2 indices first, in the middle and last, index counts that are no multiple of 3,
    offsets into the buffers, five small textures with one or all levels and uv far from [0, 1)"""
    sc, r, drawn = rg.tables_case(program, args)
    w, h = args[0], args[1]
    owned = np.bincount(r.owner[r.owner >= 0], minlength=args[2])
    assert (owned > 0).sum() >= min(drawn, 3) and (r.gap[r.coverage] > 2 * rr.depth_bound_codes() + 2).all()
    assert sum(1 for d in sc.draws if d["index_count"] < 3) == 4 and (args[2] == 1 or any(d["index_count"] % 3 for d in sc.draws if d["index_count"] > 3))
    label = f"tables {program} {args}"
    if program == "gbuf":
        out = oracle_gbuf(sc, w, h)
        rg.compare(label, _Plain, r, d24=out["depth"].astype(np.int64) & 0xFFFFFF, covered=out["albedo"][..., 3] != 0)
    elif program == "shadow":
        rg.compare(label, _Plain, r, d24=rg.oracle_shadow(sc, np.eye(4, dtype=np.float32), w).astype(np.int64))
    else:
        color, distance = cref.cubemap_probe(cref.Arith(2), sc, (0.0, 0.0, 0.0), w)
        rg.compare(label, _Plain, r, covered=distance[rg.CUBE_FACE] != cref.CLEAR_DISTANCE)


def _union_of_pairs_is_covered(case, r):
    """Each pair shares an edge that crosses the near plane.  Without any clip, in float64: every centre more than one pixel inside
    the union of the two triangles and more than one pixel in front of the plane must be covered by the clipped pieces (no crack
    along the shared edge, no piece lost by the clip); the one-pixel band left out is at most a tenth of the union's pixels."""
    clip = case.clip().astype(np.float64)
    ys, xs = np.mgrid[0:case.height, 0:case.width]
    ring = [(np.cos(a), np.sin(a)) for a in np.arange(16) * (2 * np.pi / 16)] + [(0.0, 0.0)]
    for i, j in case.contains["pairs"]:
        def front_inside(px, py):
            """inside the union at a depth in front of the plane (z / w is affine in screen space)"""
            out = np.zeros(px.shape, bool)
            inside_any = np.zeros(px.shape, bool)
            for t in (i, j):
                sx = (clip[t, :, 0] / clip[t, :, 3] * 0.5 + 0.5) * case.width
                sy = (clip[t, :, 1] / clip[t, :, 3] * 0.5 + 0.5) * case.height
                zn = clip[t, :, 2] / clip[t, :, 3]
                e = [(sx[(k + 2) % 3] - sx[(k + 1) % 3]) * (py - sy[(k + 1) % 3]) - (sy[(k + 2) % 3] - sy[(k + 1) % 3]) * (px - sx[(k + 1) % 3]) for k in range(3)]
                area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sy[1] - sy[0]) * (sx[2] - sx[0])
                lam = [ek / area for ek in e]
                ins = (lam[0] >= 0) & (lam[1] >= 0) & (lam[2] >= 0)
                z = lam[0] * zn[0] + lam[1] * zn[1] + lam[2] * zn[2]
                inside_any |= ins
                out |= ins & (z > 0)
            return out, inside_any
        deep = np.ones(xs.shape, bool)
        for dx, dy in ring:
            f, _ = front_inside(xs + 0.5 + dx, ys + 0.5 + dy)
            deep &= f
        front, union = front_inside(xs + 0.5, ys + 0.5)
        assert deep.sum() > 500
        missing = deep & ~np.isin(r.owner, (i, j))
        assert not missing.any(), f"pair {(i, j)}: {int(missing.sum())} centres inside the union are not covered, first {np.argwhere(missing)[:3].tolist()}"
        band = front & ~deep
        assert band.sum() <= case.contains["max_band_share"] * union.sum(), (int(band.sum()), int(union.sum()))


@pytest.mark.parametrize("name,program,args", CASES, ids=IDS)
def test_checker_agrees_with_the_exact_reference(name, program, args, oracle_lib):
    if program == "cube":
        case, sc, r = rg.cube_case(name, args)
    else:
        case, r = rg.get(name, args)
    _floors(name, program, case, r)
    label = f"{name} {program} {args}"
    if program == "gbuf":
        out = oracle_gbuf(case.scene(), case.width, case.height)
        rg.compare(label, case, r, d24=out["depth"].astype(np.int64) & 0xFFFFFF, albedo=out["albedo"], covered=out["albedo"][..., 3] != 0)
    elif program == "shadow":
        d = rg.oracle_shadow(case.scene(), np.eye(4, dtype=np.float32), case.width)
        rg.compare(label, case, r, d24=d.astype(np.int64))
    else:
        with np.errstate(invalid="ignore"):
            color, distance = cref.cubemap_probe(cref.Arith(2), sc, (0.0, 0.0, 0.0), case.width)
        f = rg.CUBE_FACE
        # covered: the alpha of the colour (cleared to 0, the palette's is 255); the stored distance may equal its clear value
        assert ((distance[f] != cref.CLEAR_DISTANCE) <= (color[f][..., 3] != 0)).all()
        rg.compare(label, case, r, covered=color[f][..., 3] != 0, albedo=color[f])
        assert (distance[4] == cref.CLEAR_DISTANCE).all(), "nothing lies behind the probe"
