"""The kernels of the hit exchange (csrc/hit_exchange.hip: vkr_hit_requests, vkr_hit_requests_bounded, vkr_hit_reply,
vkr_hit_scatter) and vkr_sssr_validate_unless on the constructed cases of tests/hit_exchange_cases.py, byte for byte against the
restated rules of tests/hit_exchange_reference.py — the ORDER of the requests included, which the kernel's comment promises and
the bounded pass depends on.

vkr_hit_scatter has no bounds check, so it is only ever given a request list that the same test has compared equal to the
reference (whose every code tests/test_hit_exchange_cases.py shows to lie inside the frame): a test that finds pass 2 different
fails there and launches nothing more."""
import ctypes as C
import functools

import numpy as np
import pytest

import hit_exchange_cases as hc
import hit_exchange_reference as ref
import hit_round as hr
from parity import mismatches
from vk_renderer_amd import abi

pytestmark = pytest.mark.gpu

GUARD, GUARD_WORDS = 0x6B6B6B6B, 64


@functools.lru_cache(maxsize=None)
def _case(geom, rank, name):
    return hc.make(geom, rank, name)


@functools.lru_cache(maxsize=2)
def _owner_rigs(geom):
    g = hc.GEOMETRIES[geom]
    rigs = []
    for o in range(g.world):
        rig = hc.HitRig(g, o, "product", "cuda")
        hc.fill_owner(rig, *hc.frame_noise(geom))
        rigs.append(rig)
    return rigs


def _dev(words, fill=None):
    """a device buffer of uint32 words: the given ones, or `words` of them holding `fill`"""
    import torch

    if fill is not None:
        return torch.full((int(words),), int(np.uint32(fill).view(np.int32)), dtype=torch.int32, device="cuda")
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32).copy()).cuda()


def _host(rig, t):
    return rig.buffer_to_host(t).view(np.uint32)


def _u32(values):
    return (C.c_uint32 * len(values))(*[int(v) for v in values])


def _count(rig, bounds):
    """pass 1 with a workspace that holds garbage (the header: no initialisation needed) and guard words behind counts and workspace"""
    world = len(bounds) - 1
    counts = _dev(world + GUARD_WORDS, fill=0)
    rig._hit_workspace = _dev(abi.HIT_WORKSPACE_WORDS + GUARD_WORDS, fill=0x5A5A5A5A)
    rig.call("hit_requests", C.byref(rig._hit_sources(True)), _u32(bounds), world, rig._buf_ptr(counts), rig._buf_ptr(rig._hit_workspace), None, None)
    got = _host(rig, counts)
    assert not got[world:].any(), "pass 1 wrote behind the counts"
    assert (_host(rig, rig._hit_workspace)[abi.HIT_WORKSPACE_WORDS:] == 0x5A5A5A5A).all(), "pass 1 wrote behind the workspace"
    return [int(v) for v in got[:world]]


def _write(rig, bounds, seg):
    world = len(bounds) - 1
    out = _dev(seg[-1] + GUARD_WORDS, fill=GUARD)
    rig.call("hit_requests", C.byref(rig._hit_sources(True)), _u32(bounds), world, None, rig._buf_ptr(rig._hit_workspace), _u32(seg[:world]), rig._buf_ptr(out))
    return _host(rig, out)


def _write_bounded(rig, bounds, caps):
    world = len(bounds) - 1
    seg = [0]
    for c in caps:
        seg.append(seg[-1] + int(c))
    out = _dev(seg[-1] + GUARD_WORDS, fill=ref.NO_REQUEST)
    out[seg[-1]:] = GUARD
    dropped = _dev(1 + GUARD_WORDS, fill=0)
    rig.call("hit_requests_bounded", C.byref(rig._hit_sources(True)), _u32(bounds), world, rig._buf_ptr(rig._hit_workspace), _u32(seg), _u32(caps),
             rig._buf_ptr(out), rig._buf_ptr(dropped))
    flag = _host(rig, dropped)
    assert not flag[1:].any()
    return seg, _host(rig, out), int(flag[0])


def _reply(rig, requests):
    """-> (replies [n, 4], the three error words)"""
    n = int(requests.size)
    q, replies, errors = _dev(requests), _dev(4 * n + GUARD_WORDS, fill=GUARD), _dev(3 + GUARD_WORDS, fill=0)
    rig.call("hit_reply", C.byref(rig.albedo.desc()), C.byref(rig.dn.desc()), rig._buf_ptr(q), n, rig._buf_ptr(replies), rig._buf_ptr(errors))
    rep, err = _host(rig, replies), _host(rig, errors)
    assert (rep[4 * n:] == GUARD).all() and not err[3:].any(), "the reply wrote behind its buffers"
    return rep[: 4 * n].reshape(n, 4), err[:3]


@pytest.mark.parametrize("case", hc.CASES, ids=hc.case_id)
def test_requests_replies_scatter_byte_for_byte(case, oracle_lib):
    geom, rank, name = case
    g, c = hc.GEOMETRIES[geom], _case(*case)
    req = c.requests()
    bounds = list(g.bounds)
    rig = hc.HitRig(g, rank, "product", "cuda")
    c.fill(rig)
    # pass 1
    counts = _count(rig, bounds)
    assert counts == req.counts, "pass 1: counts"
    # pass 2: the layout, order included; twice; nothing behind the last segment
    seg, buf = ref.layout(req)
    first = _write(rig, bounds, seg)
    differing = int((first[: seg[-1]] != buf).sum())
    assert differing == 0, f"pass 2: {differing} of {seg[-1]} slots differ from the reference's layout" + \
        (" (the sets per owner are equal: only the order differs)" if all(np.array_equal(np.sort(first[seg[o]: seg[o + 1]]), np.sort(buf[seg[o]: seg[o + 1]])) for o in range(g.world)) else "")
    assert (first[seg[-1]:] == GUARD).all(), "pass 2 wrote behind the last segment"
    assert np.array_equal(_write(rig, bounds, seg), first), "pass 2: a second run gives other bytes"
    # bounded pass 2 under each vector of rooms
    vectors = hc.capacity_vectors(counts)
    roomy = None
    for label, caps in vectors.items():
        bseg, want, want_dropped = ref.layout_bounded(req, caps)
        gseg, got, dropped = _write_bounded(rig, bounds, caps)
        assert gseg == bseg and np.array_equal(got[: bseg[-1]], want), f"bounded pass 2, rooms '{label}': the segments differ"
        assert (got[bseg[-1]:] == GUARD).all(), f"bounded pass 2, rooms '{label}': wrote behind the last segment"
        assert dropped == want_dropped, f"bounded pass 2, rooms '{label}': dropped flag {dropped}"
        if label == "one_short":
            for o, k in enumerate(counts):  # what is missing is the last request in order
                assert np.array_equal(got[bseg[o]: bseg[o + 1]], buf[seg[o]: seg[o + 1] - (1 if k else 0)])
        if label == "roomy":
            roomy = (bseg, got)
    # replies of every owner on its (verified) roomy segment: the requests, then 100 slots that say "no request"
    owners = _owner_rigs(geom)
    bseg, got = roomy
    replies = np.zeros((buf.size, 4), dtype=np.uint32)
    for o in range(g.world):
        if o == rank:
            continue
        mine = got[bseg[o]: bseg[o + 1]]
        want, err_ref = ref.reply(mine, *hc.window_texels(owners[o], "albedo"), *hc.window_texels(owners[o], "dn"))
        rep, err = _reply(owners[o], mine)
        assert err_ref == 0 and err[0] == 0, f"owner {o} counts errors"
        assert np.array_equal(rep, want), f"the replies of owner {o} differ"
        assert not rep[counts[o]:].any() and (counts[o] == 0 or rep[: counts[o]].any())
        replies[seg[o]: seg[o + 1]] = rep[: counts[o]]
    # scatter: the list equals the reference's (compared above), so every code names texels of the frame
    if buf.size:
        rig.hit_scatter(_dev(buf), _dev(replies.reshape(-1)), int(buf.size))
    fa, fn = c.frame_images()
    ref.scatter_unordered(buf, replies, fa, fn)
    got_a, got_n = hc.frame_texels(rig)
    assert np.array_equal(got_a, fa), "frame_albedo differs after the scatter"
    assert np.array_equal(got_n, fn), "frame_normals differs after the scatter"


def test_scatter_skips_no_request_slots(oracle_lib):
    """a roomy segment as the wire carries it: the unused slots (and their all-zero replies) leave the frame images alone"""
    case = ("ragged3", 1, "noise")
    g, c = hc.GEOMETRIES[case[0]], _case(*case)
    req = c.requests()
    rig = hc.HitRig(g, case[1], "product", "cuda")
    c.fill(rig)
    seg, buf, dropped = ref.layout_bounded(req, hc.capacity_vectors(req.counts)["roomy"])
    owners = _owner_rigs(case[0])
    replies = np.concatenate([ref.reply(buf[seg[o]: seg[o + 1]], *hc.window_texels(owners[o], "albedo"), *hc.window_texels(owners[o], "dn"))[0] for o in range(3)])
    rig.hit_scatter(_dev(buf), _dev(replies.reshape(-1)), int(buf.size))
    fa, fn = c.frame_images()
    ref.scatter_unordered(buf, replies, fa, fn)
    got_a, got_n = hc.frame_texels(rig)
    assert dropped == 0 and np.array_equal(got_a, fa) and np.array_equal(got_n, fn)


@pytest.mark.parametrize("case", hc.CASES, ids=hc.case_id)
def test_reply_refuses_what_the_window_does_not_hold(case, oracle_lib):
    """k_hit_reply checks bounds before it loads: an owner given EVERY owner's requests answers its own, zeros to the rest, and
    counts them exactly; the asking rank itself, which holds none of the rows it asked for, answers zeros to all of them; the
    diagnostics name one of the refused requests"""
    c = _case(*case)
    seg, buf = ref.layout(c.requests())
    if buf.size == 0:  # (world1, and `misses` on a rank that holds row 0: there is no list to hand to anybody)
        return
    o = next(o for o in range(c.geom.world) if o != case[1] and seg[o + 1] > seg[o])
    for who in (o, case[1]):
        owner = _owner_rigs(case[0])[who]
        want, err_ref = ref.reply(buf, *hc.window_texels(owner, "albedo"), *hc.window_texels(owner, "dn"))
        rep, err = _reply(owner, buf)
        assert int(err[0]) == err_ref and np.array_equal(rep, want)
        if who == case[1]:
            assert err_ref == buf.size and not rep.any()
        if err_ref:
            bad = np.nonzero(~want.any(axis=1))[0]
            assert int(err[2]) in bad and int(err[1]) in set(buf[bad].tolist())  # (two words, written by whichever refused threads came last)
    # without a normal image every normal request is an error
    import torch

    n = int(buf.size)
    q, replies, errors = _dev(buf), _dev(4 * n, fill=GUARD), _dev(3, fill=0)
    owner.call("hit_reply", C.byref(owner.albedo.desc()), None, owner._buf_ptr(q), n, owner._buf_ptr(replies), owner._buf_ptr(errors))
    torch.cuda.synchronize()
    want, err_ref = ref.reply(buf, *hc.window_texels(owner, "albedo"), None, 0)
    assert int(_host(owner, errors)[0]) == err_ref and np.array_equal(_host(owner, replies).reshape(n, 4), want)


@pytest.mark.parametrize("case", hc.CASES, ids=hc.case_id)
def test_validate_unless(case, oracle_lib):
    """vkr_sssr_validate_unless: with the flag word set the launch leaves `rays` alone; with 0 it is vkr_sssr_validate — on every
    case, the raw NaN / infinite / 1e30 / denormal hit uv of `pending_floats` included (the sampler clamps every tap to the edge)"""
    g, c = hc.GEOMETRIES[case[0]], _case(*case)
    rig = hc.HitRig(g, case[1], "product", "cuda")
    c.fill(rig)
    rig.frame_normals.upload(hc._rows(rig.frame_normals, c.normals))  # (every hit normal has arrived)
    rays = c.rays.copy()
    rays[..., 3] &= 0xFFFE  # every ray a hit (`pending_floats` stores misses only): a ray that fails the test shows
    rig.rays.upload(hc._rows(rig.rays, rays))
    before = rig.rays.to_host().copy()
    fn = rig.lib.vkr_sssr_validate_unless
    img = C.POINTER(abi.VkrImg)
    fn.argtypes, fn.restype = [img, img, img, img, C.POINTER(abi.TraceParams), C.c_void_p, C.c_void_p], C.c_int
    tp = rig.setup.trace_params()
    descs = [rig.rays.desc(), rig.pend_mask.desc(), rig.pend_data.desc(), rig.frame_normals.desc()]

    def run(flag):
        word = _dev(1, fill=flag)
        abi.check(fn(*[C.byref(d) for d in descs], C.byref(tp), rig._buf_ptr(word), rig.stream), rig.lib)
        rig.sync()
        return rig.rays.to_host().copy()

    for flag in (1, 0x80000000, 0xFFFFFFFF):
        assert np.array_equal(run(flag), before), f"flag {flag:#x}: the rays changed"
    unless = run(0)
    rig.rays.upload(before)
    rig.ssr_validate()
    rig.sync()
    plain = rig.rays.to_host()
    assert np.array_equal(unless, plain), "flag 0 differs from vkr_sssr_validate"
    changed = bool((unless != before).any())
    pending = int((c.mask != 0).sum())
    if pending >= 50:  # (R is drawn uniformly from [-1, 1]^3: about half of the pending rays face away)
        assert changed, "no pending ray failed the test: nothing shows that the launch ran"
    if pending == 0:
        assert not changed
    # only w of pending rays may change, and only to 0xFFFF
    r0, r1 = rig.rays.raw(0, before), rig.rays.raw(0, unless)
    assert np.array_equal(r0[..., :3], r1[..., :3]) and ((r1[..., 3] == r0[..., 3]) | ((r1[..., 3] == 0xFFFF) & (c.mask != 0))).all()


# ---- content through the whole round on three uneven strips ----------------------------------------------------------------
@pytest.mark.parametrize("case", hr.CASES, ids=hr.case_id)
def test_round_on_three_strips_against_the_oracle_twin(case, oracle_lib):
    """every rank's windowed trace, counts, requests, replies from each owner's window, scatter, deferred normal test and filter
    on the adversarial G-buffer content of tests/gbuffer_content.py, cut into three uneven strips: what the windowed trace stores
    equals the oracle twin's bit for bit ((occlusion, pdf) under the rule of tests/parity.py with the cap of tests/test_fuzz_gpu.py),
    the validated rays are the plain trace's rows and the strip's reflections the plain frame's"""
    name, size = case
    bounds, halo = hr.CUTS[size]
    plain, twin = hr.oracle_round(*case)
    ranks = hr.strip_chains(plain, "product", "cuda", bounds, halo, plain.pdf.to_host())
    got = hr.run_round(ranks, bounds)
    for rank, (g, r) in enumerate(zip(got, twin)):
        what = f"{hr.case_id(case)} rank {rank}"
        oy, h = r["row0"], r["rays"].shape[0]
        assert np.array_equal(g["rays"], r["rays"]), f"{what}: the windowed trace's rays differ"
        assert np.array_equal(g["mask"], r["mask"]), f"{what}: pending masks differ"
        pend = r["mask"] != 0
        assert np.array_equal(g["pend"][pend][:, [0, 1, 2, 4, 5]].view(np.uint32), r["pend"][pend][:, [0, 1, 2, 4, 5]].view(np.uint32)), f"{what}: pending R / hit uv differ"
        bad = int(mismatches(ranks[rank].raw.format, g["raw"], r["raw"]).sum())
        print(f"[round] {what}: (occlusion, pdf): {bad} of {g['raw'].shape[0] * g['raw'].shape[1]} texels outside tolerance; requests {g['counts']}")
        assert bad <= max(1, int(2e-4 * g["raw"].shape[0] * g["raw"].shape[1])), f"{what}: (occlusion, pdf): {bad} texels outside tolerance"
        assert g["counts"] == r["counts"] and g["errors"] == 0
        for o in range(3):
            assert np.array_equal(g["requests"][o], r["requests"][o]), f"{what}: the requests for owner {o} differ"
        for image in ("frame_albedo", "frame_normals"):
            assert np.array_equal(g[image], r[image]), f"{what}: {image} differs after the scatter"
        want = plain.rays.raw(0)[oy: oy + h]
        assert np.array_equal(r["validated"], want), f"{what}: oracle: validated rays differ from the plain trace"
        assert np.array_equal(g["validated"], want), f"{what}: product: validated rays differ from the plain trace"
        rows = hr.interior(size, rank, oy)
        assert np.array_equal(g["reflections"][rows], plain.reflections.raw(0)[bounds[rank] // 2: bounds[rank + 1] // 2]), f"{what}: reflections of the strip differ from the plain frame"
