"""vkr_accel_occluded_cutout and vkr_accel_closest_cutout on the GPU: their answers must be those of the numpy brute force
(tests/ray_cutout_reference.py) bit for bit — the hit flag, and t, u, v as uint32 views and the index — on every constructed case
of tests/ray_cutout_cases.py (a: nearest transparent and a farther one opaque; b: coincident triangles; c: a leaf whose first
triangle is transparent, and transparent below the root's first child with opaque below the second; d: everything transparent;
e: uv_hit on texel centres, on the boundary between alpha 0 and alpha code 1, deep inside a hole; f: attribute uv outside [0, 1)
and negative; g: alpha_lod 0, where the hole has vanished, beyond the chain; h: no texture and an index beyond the table; i: the
mask bit; j: tmin == tmax at a transparent and at an opaque candidate), over hierarchies of 1, 2, 3, 4 and 40 triangles and the
textures 1 x 1 alpha 0, 1 x 1 alpha 255, a 2 x 2 checker, 8 x 8 with a mip chain that averages the hole away, 3 x 5 and the
alpha-code-1 edge; and, on seeded rays against the 40-triangle scene in batches of 1, 63, 64, 65 and 257: the brute force again,
texture_count 0 and the mask of all ones equal to vkr_accel_occluded / vkr_accel_closest bit for bit, `closest.index != miss`
equal to the any hit, and no cutout hit nearer than the opaque hit of its ray.  Records behind the last ray keep a guard value."""
import functools

import numpy as np
import pytest

from vk_renderer_amd import abi
from vk_renderer_amd import scene as scn

import ray_cutout_cases as cs
import ray_cutout_reference as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 0x0BADBEEF
BATCHES = [1, 63, 64, 65, 257]


def _arith():
    return ref.Arith(int(abi.product().vkr_numeric_contract()))


@functools.lru_cache(maxsize=None)
def _textures():
    """the texture table on the host and on the device: -> (list of chains, RasterScene, keep-alive)"""
    sc = scn.Scene()
    sc.textures = cs.textures()
    rs, keep = sc.upload(device="cuda")
    return sc.textures, rs, keep


@functools.lru_cache(maxsize=None)
def _scratch():
    import torch

    n = abi.accel_cutout_scratch_bytes(cs.TEXTURE_COUNT)
    return n, torch.empty(n, dtype=torch.uint8, device="cuda")


def _run(tris, attribs, o, d, tmin, tmax, lod, mask, count=cs.TEXTURE_COUNT, accel=None):
    """-> (vkr_accel_closest_cutout's records HIT_DTYPE [n], vkr_accel_occluded_cutout's answers bool [n])"""
    import torch

    n = len(o)
    accel = accel or abi.Accel(tris)
    _, rs, _ = _textures()
    nbytes, scratch = _scratch()
    stream = torch.cuda.current_stream().cuda_stream
    to, td = torch.from_numpy(np.ascontiguousarray(o)).to("cuda"), torch.from_numpy(np.ascontiguousarray(d)).to("cuda")
    att = torch.from_numpy(np.ascontiguousarray(attribs).view(np.uint8).copy()).to("cuda")
    cut = abi.ray_cutout(lod, mask)
    out = torch.full((n + 64, 4), GUARD, dtype=torch.int32, device="cuda")
    occ = torch.full((n + 64,), 9, dtype=torch.int32, device="cuda")
    tex = rs.textures if count else None
    abi.accel_closest_cutout(accel, to, td, tmin, tmax, att.data_ptr(), len(attribs), tex, count, cut, out, scratch.data_ptr(), nbytes, stream)
    abi.accel_occluded_cutout(accel, to, td, tmin, tmax, att.data_ptr(), len(attribs), tex, count, cut, occ, scratch.data_ptr(), nbytes, stream)
    torch.cuda.synchronize()
    h = out.cpu().numpy().view(np.uint32)
    flags = occ.cpu().numpy()
    assert (h[n:] == GUARD).all() and (flags[n:] == 9).all(), "records past the last ray were written"
    assert set(np.unique(flags[:n]).tolist()) <= {0, 1}
    return np.ascontiguousarray(h[:n]).view(ref.HIT_DTYPE).reshape(n), flags[:n].astype(bool)


def _same_bits(got, want, what):
    g, w = got.view(np.uint32).reshape(-1, 4), want.view(np.uint32).reshape(-1, 4)
    bad = (g != w).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(g)} records differ, first ray {int(np.argmax(bad))}: {got[bad][:3]} != {want[bad][:3]}"


CASES = cs.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed_case(name):
    c = CASES[name]
    textures = _textures()[0][:c["texture_count"]]
    rec = ref.triangle_records(c["tris"])
    args = (c["o"], c["d"], c["tmin"], c["tmax"], rec, c["attribs"], textures, c["lod"], c["mask"])
    want = ref.brute_force_closest_cutout(_arith(), *args)
    want_any = ref.brute_force_any_hit_cutout(_arith(), *args)
    if c["expect"] is not None:
        assert (want["index"] == c["expect"]).all(), "the reference's own known answer"
    got, got_any = _run(c["tris"], c["attribs"], c["o"], c["d"], c["tmin"], c["tmax"], c["lod"], c["mask"], c["texture_count"])
    print(f"[ray cutout] {name}: index {got['index'].tolist()[:8]} any {got_any.astype(int).tolist()[:8]}")
    _same_bits(got, want, name)
    assert (got_any == want_any).all(), (name, got_any, want_any)
    miss = got[got["index"] == cs.MISS]
    assert (miss["t"] == 0).all() and (miss["u"] == 0).all() and (miss["v"] == 0).all()


@functools.lru_cache(maxsize=None)
def _forty():
    tris, attribs = cs.forty()
    o, d = cs.random_rays(257)
    return tris, attribs, o, d, ref.triangle_records(tris), abi.Accel(tris)


@functools.lru_cache(maxsize=None)
def _forty_expected(lod):
    tris, attribs, o, d, rec, _ = _forty()
    return ref.brute_force_closest_cutout(_arith(), o, d, 0.0, 1.0, rec, attribs, _textures()[0], lod, 0)


@pytest.mark.parametrize("lod", [0, 2])
@pytest.mark.parametrize("n", BATCHES)
def test_random_rays_against_the_brute_force(n, lod):
    tris, attribs, o, d, rec, accel = _forty()
    want = _forty_expected(lod)[:n]
    got, got_any = _run(tris, attribs, o[:n], d[:n], 0.0, 1.0, lod, 0, accel=accel)
    _same_bits(got, want, f"{n} rays, level {lod}")
    assert (got_any == (want["index"] != cs.MISS)).all()


def test_the_random_rays_meet_holes():
    """the properties below are not vacuous: some rays change their answer, some lose it altogether"""
    import closest_hit_reference as closest

    tris, attribs, o, d, rec, _ = _forty()
    opaque = closest.brute_force_closest(o, d, 0.0, 1.0, rec)
    cut = _forty_expected(0)
    changed = cut["index"] != opaque["index"]
    lost = changed & (cut["index"] == cs.MISS)
    print(f"[ray cutout] 257 rays on 40 triangles: {int((opaque['index'] != cs.MISS).sum())} opaque hits, {int(changed.sum())} change, {int(lost.sum())} miss")
    assert changed.sum() >= 5 and lost.any() and (changed & ~lost).any()
    nodes = abi.accel_layout(tris)[0].view(np.uint32).reshape(-1, 8)
    assert (nodes[:, 7] > 1).any(), "leaves that hold more than one triangle"


@pytest.mark.parametrize("n", BATCHES)
def test_properties_on_random_rays(n):
    import torch

    tris, attribs, o, d, rec, accel = _forty()
    o, d = o[:n], d[:n]
    to, td = torch.from_numpy(np.ascontiguousarray(o)).to("cuda"), torch.from_numpy(np.ascontiguousarray(d)).to("cuda")
    out = torch.full((n, 4), GUARD, dtype=torch.int32, device="cuda")
    occ = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    accel.closest(to, td, 0.0, 1.0, out, stream)
    accel.occluded(to, td, 0.0, 1.0, occ, stream)
    torch.cuda.synchronize()
    opaque = np.ascontiguousarray(out.cpu().numpy().view(np.uint32)).view(ref.HIT_DTYPE).reshape(n)
    opaque_any = occ.cpu().numpy().astype(bool)
    # without textures, and with every texture masked, the outputs are the opaque entries' bit for bit
    for what, kw in (("texture_count 0", dict(mask=0, count=0)), ("mask of all ones", dict(mask=0xFFFFFFFF))):
        got, got_any = _run(tris, attribs, o, d, 0.0, 1.0, 0, accel=accel, **kw)
        _same_bits(got, opaque, what)
        assert (got_any == opaque_any).all(), what
    got, got_any = _run(tris, attribs, o, d, 0.0, 1.0, 0, 0, accel=accel)
    assert ((got["index"] != cs.MISS) == got_any).all(), "closest_cutout.index != miss equals occluded_cutout"
    hit = got["index"] != cs.MISS
    assert (opaque["index"][hit] != cs.MISS).all(), "a cutout hit is a candidate of the opaque query too"
    assert (got["t"][hit] >= opaque["t"][hit]).all(), "a cutout hit is never nearer than the opaque hit of the same ray"
