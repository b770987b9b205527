"""The restated rules of the hit exchange (tests/hit_exchange_reference.py) on the constructed cases of tests/hit_exchange_cases.py:
against the oracle twin oracle/passes_hit.cpp (counts, request sets per owner, replies and scattered frame images byte for byte),
that every class reaches what it was built to reach, that every wrong variant of a rule changes what some case emits, and
host.hit_capacities against its restatement.  No GPU."""
import dataclasses
import functools

import numpy as np
import pytest

import hit_exchange_cases as hc
import hit_exchange_reference as ref
import hit_round as hr
from vk_renderer_amd import host


@functools.lru_cache(maxsize=None)
def _case(geom, rank, name):
    return hc.make(geom, rank, name)


@functools.lru_cache(maxsize=None)
def _requests(geom, rank, name):
    return _case(geom, rank, name).requests()


def _of(name, geoms=None):
    return [c for c in hc.CASES if c[2] == name and (geoms is None or c[0] in geoms)]


@functools.lru_cache(maxsize=4)
def _owner_rigs(geom):
    """every strip of the geometry as the owner that answers: window albedo / downsampled normals of the frame's noise"""
    g = hc.GEOMETRIES[geom]
    rigs = []
    for o in range(g.world):
        rig = hc.HitRig(g, o, "oracle")
        hc.fill_owner(rig, *hc.frame_noise(geom))
        rigs.append(rig)
    return rigs


@pytest.mark.parametrize("case", hc.CASES, ids=hc.case_id)
def test_reference_against_the_oracle_twin(case, oracle_lib):
    geom, rank, name = case
    g, c, req = hc.GEOMETRIES[geom], _case(*case), _requests(*case)
    rig = hc.HitRig(g, rank, "oracle")
    c.fill(rig)
    bounds = list(g.bounds)
    counts = rig.hit_count(bounds)
    assert counts == req.counts, "pass 1"
    out, seg = rig.hit_write(bounds, counts)
    seg_ref, buf = ref.layout(req)
    assert seg == seg_ref
    out = np.asarray(out, dtype=np.uint32)
    for o in range(g.world):
        assert np.array_equal(np.sort(out[seg[o]: seg[o + 1]]), np.sort(buf[seg[o]: seg[o + 1]])), f"the requests for owner {o} differ as sets"
    # replies of every owner on the reference's list, then the scatter of all of them
    replies = np.zeros((buf.size, 4), dtype=np.uint32)
    owners = _owner_rigs(geom)
    for o in range(g.world):
        n = seg[o + 1] - seg[o]
        if n == 0:
            continue
        mine = np.ascontiguousarray(buf[seg[o]: seg[o + 1]])
        rep, err = owners[o].hit_reply(mine.copy(), n)
        want, err_ref = ref.reply(mine, *hc.window_texels(owners[o], "albedo"), *hc.window_texels(owners[o], "dn"))
        assert err == 0 and err_ref == 0, f"owner {o} was asked for texels it does not hold"
        assert np.array_equal(np.asarray(rep, dtype=np.uint32)[: 4 * n].reshape(n, 4), want), f"the replies of owner {o} differ"
        replies[seg[o]: seg[o + 1]] = want
    if buf.size:
        rig.hit_scatter(buf.copy(), replies.reshape(-1).copy(), int(buf.size))
    fa, fn = c.frame_images()
    ref.scatter_unordered(buf, replies, fa, fn)
    got_a, got_n = hc.frame_texels(rig)
    assert np.array_equal(got_a, fa) and np.array_equal(got_n, fn), "the frame images differ after the scatter"
    # every requested texel now holds what the frame holds there, nothing else was touched
    asked_a, asked_n = fa != hc.POISON * 0x01010101, fn != hc.POISON * 0x01010101
    assert np.array_equal(fa[asked_a], c.albedo[asked_a]) and np.array_equal(fn[asked_n], c.normals[asked_n])


def test_scatter_in_order_and_unordered_agree():
    c, req = _case("ragged3", 0, "noise"), _requests("ragged3", 0, "noise")
    owners = _owner_rigs("ragged3")
    seg, buf = ref.layout(req)
    replies = np.concatenate([ref.reply(buf[seg[o]: seg[o + 1]], *hc.window_texels(owners[o], "albedo"), *hc.window_texels(owners[o], "dn"))[0]
                              for o in range(3)])
    a, b = c.frame_images(), c.frame_images()
    ref.scatter(buf, replies, *a)
    ref.scatter_unordered(buf, replies, *b)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_reply_reference_refuses_what_the_window_does_not_hold():
    owners = _owner_rigs("ragged3")
    albedo, normals = hc.window_texels(owners[1], "albedo"), hc.window_texels(owners[1], "dn")  # rows [48, 166) / [24, 83)
    q = np.array([47, 48, 165, 165 | ref.BOTH_ROWS, 164 | ref.BOTH_ROWS, 48 | (204 << 14), 48 | (205 << 14), ref.NO_REQUEST,
                  23 | ref.NORMAL, 24 | ref.NORMAL, 82 | ref.NORMAL | ref.BOTH_ROWS, 82 | ref.NORMAL | (101 << 14), 82 | ref.NORMAL | (102 << 14)], dtype=np.uint32)
    rep, err = ref.reply(q, *albedo, *normals)
    bad = [0, 3, 6, 8, 10, 12]
    assert err == len(bad) and not rep[bad].any() and not rep[7].any()
    assert all(rep[i].any() for i in (1, 2, 4, 5, 9, 11))
    assert ref.reply(q, *albedo, None, 0)[1] == len([0, 3, 6]) + 5


# ---- every class reaches what it was built for ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", _of("four"), ids=hc.case_id)
def test_four_has_rays_with_four_requests(case):
    req = _requests(*case)
    assert (req.per_ray == 4).sum() > 100
    four = np.nonzero(req.per_ray == 4)[0][0]
    mine = req.ray == four
    assert sorted(req.k[mine]) == [0, 1, 2, 3] and len(set(req.owner[mine])) >= 2 and (req.code[mine] & ref.NORMAL).astype(bool).sum() == 2


@pytest.mark.parametrize("case", _of("edge_rows"), ids=hc.case_id)
def test_edge_rows_has_single_rows_and_split_pairs(case):
    geom, rank, _ = case
    g, req = hc.GEOMETRIES[geom], _requests(*case)
    win0, win1 = g.window(rank)
    kinds = {s: set(req.kind[(req.code & ref.NORMAL != 0) == s]) for s in (False, True)}
    for s in (False, True):
        if win0 > 0:
            assert ref.KIND_ROW0 in kinds[s], "no request from want0 alone"  # the footprint's lower row is the window's first
        if win1 < g.H:
            assert ref.KIND_ROW1 in kinds[s], "no request from want1 alone"
        if hc.foreign_pairs(g, rank):
            assert {ref.KIND_SPLIT0, ref.KIND_SPLIT1} <= kinds[s], "no pair split between two owners"
    # every aimed code is carried: each uv.y code by a hit ray, each hit uv.y by a pending ray, each x value by a ray that asks
    c = _case(*case)
    ycodes, xcodes, hys, hxs = hc.edge_lists(g, rank)
    hit, pend = c.rays[..., 3] != 0xFFFF, c.mask != 0
    asks_a, asks_n = np.zeros(c.mask.size + 1, dtype=bool), np.zeros(c.mask.size + 1, dtype=bool)
    asks_a[req.ray[(req.code & ref.NORMAL) == 0]] = True
    asks_n[req.ray[(req.code & ref.NORMAL) != 0]] = True
    asks_a, asks_n = asks_a[:-1].reshape(c.mask.shape), asks_n[:-1].reshape(c.mask.shape)
    assert set(ycodes) <= set(c.rays[..., 1][hit].tolist()) and set(xcodes) <= set(c.rays[..., 0][hit & asks_a].tolist())
    bits = lambda a: set(np.asarray(a, dtype=np.float32).view(np.uint32).tolist())
    assert bits(hys) <= bits(c.data[..., 5][pend]) and bits(hxs) <= bits(c.data[..., 4][pend & asks_n])
    rows, xs = req.code & 0x3FFF, (req.code >> 14) & 0x3FFF
    alb = (req.code & ref.NORMAL) == 0
    assert xs[alb].min() == 0 and xs[alb].max() == g.W - 2 and xs[~alb].max() == g.W // 2 - 2
    foreign = hc.foreign_rows(g, rank)
    assert rows[alb].min() == foreign.min() and rows[alb].max() == foreign.max(), "the frame's first / last foreign row is asked for"


def test_edge_rows_codes_are_the_extreme_ones():
    """the smallest and largest uv.y code of a row are one code away from the neighbouring rows' (scanned with the reference)"""
    for extent in (226, 76, 512, 64, 16384):
        t = hc.index_table(extent)
        assert t[0] == -1 and t[65535] == extent - 1 and (np.diff(t) >= 0).all()
        for row in (0, extent // 2, extent - 1):
            lo, hi = hc.codes_for(row, extent)
            assert t[lo - 1] == row - 1 and (hi == 65535 or t[hi + 1] == row + 1)


@pytest.mark.parametrize("case", _of("owner_salad"), ids=hc.case_id)
def test_owner_salad_has_waves_naming_many_owners(case):
    req = _requests(*case)
    wave = req.tile * 16 + req.wave
    most = max(len(set(req.owner[wave == w])) for w in np.unique(wave))
    assert most >= 8, most


def test_tiles1080_has_blocks_with_five_tiles_and_blocks_with_four():
    for case in _of("noise", ("tiles1080",)) + _of("every_code", ("tiles1080",)):
        req = _requests(*case)
        assert req.tiles == 1080 and req.blocks == 256
        # (blocks 48 .. 55 have five tiles too, the fifth in the apron row, where this rank, holding row 0, asks for nothing)
        per_block = [len(set(req.tile[req.block == b])) for b in (0, 47, 56, 255)]
        assert per_block[0] == 5 and per_block[1] == 5 and per_block[2] == 4 and per_block[3] == 4, per_block
    assert _requests("tiles256", 1, "noise").tiles == 256 and _requests("tiles256", 1, "noise").blocks == 256
    r = _requests("tiles257", 1, "noise")
    assert r.tiles == 257 and r.blocks == 256 and set(r.tile[r.block == 0]) == {0, 256} and len(set(r.tile[r.block == 1])) == 1
    # the apron request stands in the last row of tiles: in `misses` on a rank that does not hold row 0 it is all there is
    m = _requests("ragged3", 2, "misses")
    assert m.counts == [1, 0, 0] and m.tile[0] == 2 * 3 and m.ray[0] == 46 * 103


def test_every_code_has_every_code():
    c = _case("tiles1080", 0, "every_code")
    assert np.unique(c.rays[..., 0]).size == 65536 and np.unique(c.rays[..., 1]).size == 65536


@pytest.mark.parametrize("case", _of("pending_floats"), ids=hc.case_id)
def test_pending_floats_stay_inside_the_frame(case):
    geom, rank, _ = case
    g, c, req = hc.GEOMETRIES[geom], _case(*case), _requests(*case)
    uv = c.hit_uv[c.mask != 0]
    assert np.isnan(uv).any() and np.isposinf(uv).any() and np.isneginf(uv).any() and (np.abs(uv) == np.float32(1e30)).any()
    assert ((uv != 0) & (np.abs(uv) < np.float32(1.2e-38))).any(), "denormals"
    nrm = (req.code & ref.NORMAL) != 0
    assert nrm.sum() + 1 >= req.code.size  # every request but the apron's comes from a raw float
    rows, xs = req.code & 0x3FFF, (req.code >> 14) & 0x3FFF
    last = rows + ((req.code & ref.BOTH_ROWS) != 0)
    assert (last[nrm] < g.H // 2).all() and (xs[nrm] <= g.W // 2 - 2).all()
    assert (last[~nrm] < g.H).all() and (xs[~nrm] <= g.W - 2).all()


@pytest.mark.parametrize("case", hc.CASES, ids=hc.case_id)
def test_every_request_names_texels_of_the_frame_that_the_window_lacks(case):
    """what the scatter (which has no guard) relies on, for every case the GPU file hands it"""
    geom, rank, _ = case
    g, req = hc.GEOMETRIES[geom], _requests(*case)
    win0, win1 = g.window(rank)
    nrm, both = (req.code & ref.NORMAL) != 0, (req.code & ref.BOTH_ROWS) != 0
    rows, xs = (req.code & 0x3FFF).astype(np.int64), (req.code >> 14) & 0x3FFF
    h, w = np.where(nrm, g.H // 2, g.H), np.where(nrm, g.W // 2, g.W)
    lo, hi = np.where(nrm, win0 // 2, win0), np.where(nrm, win1 // 2, win1)
    assert (rows + both < h).all() and (xs + 1 < w).all()
    assert ((rows < lo) | (rows >= hi)).all() and ((rows + both < lo) | (rows + both >= hi)).all()
    b = np.asarray(g.bounds)
    shift = nrm.astype(np.int64)
    assert ((b[req.owner] <= rows << shift) & ((rows + both) << shift < b[req.owner + 1])).all(), "a request goes to the strip that owns its rows"
    assert (req.owner != rank).all()


def test_world1_and_misses_ask_for_nothing():
    for case in _of("misses") + [c for c in hc.CASES if c[0] == "world1"]:
        req = _requests(*case)
        holds_row0 = hc.GEOMETRIES[case[0]].window(case[1])[0] == 0
        assert sum(req.counts) == (0 if holds_row0 else 1), case
    assert _requests("world1", 0, "noise").counts == [0] and ref.layout(_requests("world1", 0, "noise"))[1].size == 0


def test_noise_uses_every_mask_byte_and_half_the_rays_miss():
    c = _case("ragged3", 1, "noise")
    assert set(np.unique(c.mask)) == {0, 1, 0x80, 0xFF}
    assert 0.4 < (c.rays[..., 3] == 0xFFFF).mean() < 0.6 and c.hit_uv.min() < -0.2 and c.hit_uv.max() > 1.2


def test_tile_checker_has_tiles_with_one_request():
    c, req = _case("ragged3", 1, "tile_checker"), _requests("ragged3", 1, "tile_checker")  # 103 x 59 rays: 2 x 4 tiles, ragged both ways
    asking = req.per_ray[:-1].reshape(c.mask.shape) > 0
    per_tile = {(ty, tx): asking[ty * 16: ty * 16 + 16, tx * 64: tx * 64 + 64] for ty in range(4) for tx in range(2)}
    assert all(t.all() for (ty, tx), t in per_tile.items() if (tx + ty) % 2 == 0), "loud tiles: every ray asks"
    ones = [k for k, t in per_tile.items() if t.sum() == 1]
    assert any(per_tile[k][0, 0] for k in ones) and any(per_tile[k][-1, -1] for k in ones) and len(ones) >= 3
    assert per_tile[(3, 1)].shape == (11, 39)


# ---- wrong variants of the rules ---------------------------------------------------------------------------------------
MUTANTS = [f.name for f in dataclasses.fields(ref.Rules)]
SMALL = [c for c in hc.CASES if c[0] in ("ragged3", "small3", "world16", "thin16", "world1")]


def _outcome(case, rules):
    """everything the tests compare: the ordered request buffer with its segments and the bounded pass one slot short"""
    req = _case(*case).requests(rules)
    seg, buf = ref.layout(req)
    short = ref.layout_bounded(req, hc.capacity_vectors(_requests(*case).counts)["one_short"], rules)
    return seg, buf.tobytes(), short[1].tobytes(), short[2]


@functools.lru_cache(maxsize=None)
def _oracle_sets(case):
    """(counts, sorted requests per owner) of the oracle twin"""
    g = hc.GEOMETRIES[case[0]]
    rig = hc.HitRig(g, case[1], "oracle")
    _case(*case).fill(rig)
    counts = rig.hit_count(list(g.bounds))
    out, seg = rig.hit_write(list(g.bounds), counts)
    out = np.asarray(out, dtype=np.uint32)
    return counts, [np.sort(out[seg[o]: seg[o + 1]]).tobytes() for o in range(g.world)]


ORDER_MUTANTS = ("lane_then_k", "keep_last")  # (the twin's order is its own: these two have nothing to disagree with there)
# for the two order mutants also the launches with a tile per block, with two, and with five
TILED = [("tiles256", 1, "noise"), ("tiles257", 1, "noise"), ("tiles1080", 0, "noise")]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_wrong_rule_is_noticed(mutant, oracle_lib):
    """no mutant is exempt: each changes the bytes of at least one class, and each mutant of what is emitted also disagrees with
    the oracle twin's counts or request sets on a class that kills it"""
    rules = ref.Rules(**{mutant: True})
    cases = SMALL + (TILED if mutant in ORDER_MUTANTS else [])
    killing = [case for case in cases if _outcome(case, rules) != _outcome(case, ref.EXACT)]
    killers = sorted({case[2] for case in killing})
    print(f"[mutant] {mutant}: killed by {killers}")
    assert killers, f"no class notices {mutant}"
    if mutant in ORDER_MUTANTS:
        assert {case[0] for case in killing} >= {"tiles256", "tiles257", "tiles1080"}
        return
    against_twin = 0
    for case in killing:
        req = _case(*case).requests(rules)
        counts, sets = _oracle_sets(case)
        against_twin += req.counts != counts or any(np.sort(req.of_owner(o)).tobytes() != sets[o] for o in range(req.world))
    print(f"[mutant] {mutant}: disagrees with the oracle twin on {against_twin} of {len(killing)} killing cases")
    assert against_twin == len(killing)


def test_the_nine_rules_of_the_issue_are_all_mutated():
    assert len(MUTANTS) == 9


# ---- the bounded pass ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in SMALL if c[2] in ("noise", "edge_rows")], ids=hc.case_id)
def test_bounded_layout(case):
    req = _requests(*case)
    counts = req.counts
    for name, caps in hc.capacity_vectors(counts).items():
        seg, buf, dropped = ref.layout_bounded(req, caps)
        assert dropped == int(any(c > k for c, k in zip(counts, caps))), name
        for o, (c, k) in enumerate(zip(counts, caps)):
            mine = buf[seg[o]: seg[o + 1]]
            assert np.array_equal(mine[: min(c, k)], req.of_owner(o)[: min(c, k)]) and (mine[min(c, k):] == ref.NO_REQUEST).all()
    assert ref.layout_bounded(req, hc.capacity_vectors(counts)["exact"])[1].tobytes() == ref.layout(req)[1].tobytes()


# ---- the room of the next frame's segments ---------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3, 16])
@pytest.mark.parametrize("percent", [30, 100, 125])
def test_hit_capacities(world, percent):
    rng = np.random.default_rng([0xCA9, world, percent])
    values = [0, 1, 63, 64, 65, 2 ** 31]
    matrices = [[v] * (world * world) for v in values]                          # the diagonal holds a count too: it gets no room
    matrices += [[int(v) for v in rng.choice(values, size=world * world)] for _ in range(8)]
    matrices += [[int(v) for v in rng.integers(0, 5000, size=world * world)]]
    zero_pairs = [int(v) for v in rng.integers(1, 200, size=world * world)]     # adjacent and distant pairs that asked for nothing
    for r in range(world):
        for o in (r - 1, r + 1, r + 2, r - 3):
            if 0 <= o < world:
                zero_pairs[r * world + o] = 0
    matrices.append(zero_pairs)
    for m in matrices:
        got, want = host.hit_capacities(m, world, percent), ref.hit_capacities(m, world, percent)
        assert got == want, (m, got, want)
    caps = ref.hit_capacities(zero_pairs, world, percent)
    for r in range(world):
        for o in range(world):
            k = caps[r * world + o]
            assert k == (0 if r == o or (abs(r - o) > 1 and zero_pairs[r * world + o] == 0) else k) and k % 64 == 0
            if abs(r - o) == 1:
                assert k >= 64
            if r != o and zero_pairs[r * world + o]:
                assert k >= zero_pairs[r * world + o] * percent // 100 + 64 and k < zero_pairs[r * world + o] * percent // 100 + 128


# ---- content through the whole round on three uneven strips: the oracle half ---------------------------------------------------
@pytest.mark.parametrize("case", hr.CASES, ids=hr.case_id)
def test_oracle_round_on_three_strips_equals_the_plain_frame(case, oracle_lib):
    """DESIGN_MULTIGPU.md: the windowed trace evaluates first what needs nothing remote and the deferred normal test last — "the
    result is a conjunction" — so windowed + validated rays are the plain trace's, whatever the content, and once every requested
    texel has arrived the filter of a strip computes the plain frame's reflections"""
    name, size = case
    bounds, _ = hr.CUTS[size]
    plain, ranks = hr.oracle_round(*case)
    for rank, r in enumerate(ranks):
        oy, h = r["row0"], r["rays"].shape[0]
        assert r["errors"] == 0, f"rank {rank}: an owner was asked for texels it does not hold"
        assert np.array_equal(r["validated"], plain.rays.raw(0)[oy: oy + h]), f"rank {rank}: validated rays differ from the plain trace"
        assert np.array_equal(r["reflections"][hr.interior(size, rank, oy)], plain.reflections.raw(0)[bounds[rank] // 2: bounds[rank + 1] // 2]), \
            f"rank {rank}: reflections of the strip differ from the plain frame"


def test_oracle_rounds_ask_neighbours_and_distant_strips(oracle_lib):
    """Over the classes the middle rank asks both neighbours and some rank asks a strip that is not its neighbour.

    sky_all does NOT come down to the apron's texel pair: the trace has no early-out for a pixel of sky, and on a pyramid that is
    far everywhere its rays pass every test but the hit-normal one, which the plain trace fails them on (its rays are all misses)
    and the windowed trace defers where the footprint is foreign — 992 / 477 / 757 of the three windows' rays at 206 x 226 are
    provisional hits that ask for their normal and albedo footprints (995 / 478 / 764 requests) and become misses in validate.
    That is the round doing what the header says (DESIGN_MULTIGPU.md records it), so what is asserted is: every ray that is not
    pending is a miss and has no request, the apron has at most one, and no hit is left after the deferred test."""
    both = distant = 0
    for case in hr.CASES:
        _, ranks = hr.oracle_round(*case)
        counts = [r["counts"] for r in ranks]
        both += counts[1][0] > 0 and counts[1][2] > 0
        distant += counts[0][2] > 0 or counts[2][0] > 1  # (rank 2 always asks strip 0 for the apron pair)
        assert all(c[rank] == 0 for rank, c in enumerate(counts))
        if case[0] == "sky_all":
            for r in ranks:
                assert (r["rays"][..., 3][r["mask"] == 0] == 0xFFFF).all() and (r["validated"][..., 3] == 0xFFFF).all()
            bounds, halo = hr.CUTS[case[1]]
            for rank, r in enumerate(ranks):  # exactly: no ray that is not pending has a request, the apron has at most one
                _, win0, _, wh = hr.window(bounds, rank, halo, *case[1])
                req = ref.emit(r["rays"], r["mask"], r["pend"][..., 4:6], case[1][0], case[1][1], win0, win0 + wh, bounds)
                assert req.counts == r["counts"] and not req.per_ray[:-1][r["mask"].reshape(-1) == 0].any() and req.per_ray[-1] <= 1
    print(f"[round] the middle rank asks both neighbours in {both} of {len(hr.CASES)} cases, a rank asks a non-adjacent strip in {distant}")
    assert both > 0 and distant > 0


@pytest.mark.parametrize("case", hr.CASES, ids=hr.case_id)
def test_reference_on_traced_rays(case, oracle_lib):
    """the restated rules on what the windowed trace really stores (rays, mask, raw float hit uv) against the oracle twin's requests"""
    name, size = case
    bounds, halo = hr.CUTS[size]
    _, ranks = hr.oracle_round(*case)
    for rank, r in enumerate(ranks):
        _, win0, _, wh = hr.window(bounds, rank, halo, *size)
        req = ref.emit(r["rays"], r["mask"], r["pend"][..., 4:6], size[0], size[1], win0, win0 + wh, bounds)
        assert req.counts == r["counts"]
        for o in range(3):
            assert np.array_equal(np.sort(req.of_owner(o)), r["requests"][o]), f"rank {rank}: the requests for owner {o} differ"


def test_oracle_twin_answers_and_skips_unused_slots(oracle_lib):
    """include/vkr_postfx.h: vkr_hit_reply answers VKR_HIT_NO_REQUEST with zeros and counts no error, vkr_hit_scatter skips it"""
    case = ("ragged3", 1, "noise")
    g, c, req = hc.GEOMETRIES[case[0]], _case(*case), _requests(*case)
    seg, buf, dropped = ref.layout_bounded(req, hc.capacity_vectors(req.counts)["roomy"])
    owners = _owner_rigs(case[0])
    rig = hc.HitRig(g, case[1], "oracle")
    c.fill(rig)
    replies = np.zeros((buf.size, 4), dtype=np.uint32)
    for o in (0, 2):
        mine = np.ascontiguousarray(buf[seg[o]: seg[o + 1]])
        rep, err = owners[o].hit_reply(mine.copy(), int(mine.size))
        want, _ = ref.reply(mine, *hc.window_texels(owners[o], "albedo"), *hc.window_texels(owners[o], "dn"))
        assert err == 0 and np.array_equal(np.asarray(rep, dtype=np.uint32).reshape(-1, 4), want) and not want[req.counts[o]:].any()
        replies[seg[o]: seg[o + 1]] = want
    rig.hit_scatter(buf.copy(), replies.reshape(-1).copy(), int(buf.size))
    fa, fn = c.frame_images()
    ref.scatter_unordered(buf, replies, fa, fn)
    got_a, got_n = hc.frame_texels(rig)
    assert dropped == 0 and np.array_equal(got_a, fa) and np.array_equal(got_n, fn)
