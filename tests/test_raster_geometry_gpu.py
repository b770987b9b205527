"""GPU tests of the constructed raster geometry (tests/raster_geometry.py): every class through the three HIP rasterisers
(gbuf_opaque_taa, default_shadow, cubemap_probe), compared with both references -- depth words bit-equal to the program's checker
(the oracle, the numpy cube restatement), coverage and owner equal to the exact reference of the raster rules
(tests/raster_rules_reference.py), the shaded attachments by the rule of tests/parity.py with no texel outside tolerance (the
allow-list is empty).  The floors that keep these tests from going vacuous are asserted on the CPU, in
tests/test_raster_geometry.py.  The table of every comparison is written through the parity_table fixture.

Measured on an MI355X (profiles/parity_raster_geometry.json): 51 class / program / extent rows, every texel of every image bit-equal
to its checker, none outside tolerance, depth at most 2 codes from the exact depth (derived bound 5); the file runs in 11 s."""
import time

import numpy as np
import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.images import ArrayImageBuf

import cubemap_reference as cref
import parity
import probe_reference as pref
import raster_geometry as rg

pytestmark = pytest.mark.gpu

IDENTITY = np.eye(4, dtype=np.float32)
FORMATS = {"albedo": abi.FMT_RGBA8_SRGB, "normal": abi.FMT_RG16_UNORM, "material": abi.FMT_RGBA8_SRGB, "velocity": abi.FMT_RG16_SFLOAT}


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch

    torch.cuda.synchronize()


def _triangles(sc):
    return sum(d["index_count"] // 3 for d in sc.draws)


def shadow_gpu(sc, mvps, n):
    import torch

    s, keep = sc.upload("cuda")
    array = ArrayImageBuf(abi.FMT_D24_UNORM_S8, n, n, len(mvps), device="cuda", fill=0x5A)
    nbytes = abi.default_shadow_scratch_bytes(n, len(mvps), _triangles(sc))
    scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    abi.default_shadow(s, mvps, [array.desc(l) for l in range(len(mvps))], scratch.data_ptr(), nbytes, _stream())
    _sync()
    return array.raw()[..., 0]


def cube_gpu(sc, size):
    import torch

    s, keep = sc.upload("cuda")
    color = ArrayImageBuf(abi.FMT_RGBA8_SRGB, size, size, 6, device="cuda", fill=0x5A)
    distance = ArrayImageBuf(abi.FMT_R16_SFLOAT, size, size, 6, device="cuda", fill=0x5A)
    nbytes = abi.cubemap_probe_scratch_bytes(size, _triangles(sc))
    scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    abi.cubemap_probe(s, (0.0, 0.0, 0.0), color.descs(), distance.descs(), scratch.data_ptr(), nbytes, _stream())
    _sync()
    return color.raw(), distance.raw()[..., 0]


def _decode_color(codes):
    out = np.empty(codes.shape, np.float32)
    out[..., :3] = pref.SRGB[codes[..., :3]]
    out[..., 3] = codes[..., 3].astype(np.float32) / np.float32(255.0)
    return out


def _row(label, texels, bit_equal, outside, worst_depth):
    parity.record(label, texels, bit_equal, outside, worst_depth, "depth bit-equal to the checker; max_abs_diff: codes from the exact depth")


def check_gbuf(label, sc, w, h, case, r, albedo_owner=True):
    got = rg.Gbuf(w, h, "product").raster(sc)
    want = rg.Gbuf(w, h, "oracle").raster(sc)
    same = got["depth"] == want["depth"]
    assert (got["depth"] >> 24 == 0).all()
    assert same.all(), f"{label}: {int((~same).sum())} depth words differ from the oracle, first (y, x) {np.argwhere(~same)[:5].tolist()}"
    covered = got["albedo"][..., 3] != 0
    _, worst = rg.compare(label, case, r, d24=got["depth"].astype(np.int64), albedo=got["albedo"] if albedo_owner else None, covered=covered)
    _row(label + ".depth", same.size, int(same.sum()), 0, worst)
    for name in ("albedo", "normal", "material", "velocity"):
        n, bad = parity.report(f"{label}.{name}", FORMATS[name], got["decoded"][name], want["decoded"][name])
        assert n == 0, f"{label}: {name}: {n} texels outside tolerance, first (y, x) {np.argwhere(bad)[:5].tolist()}"
    return got


def check_shadow(label, got, want, case, r):
    assert (got >> 24 == 0).all(), f"{label}: a stored word has a top byte"
    same = got == want
    assert same.all(), f"{label}: {int((~same).sum())} texels differ from the oracle, first (y, x) {np.argwhere(~same)[:5].tolist()}"
    _, worst = rg.compare(label, case, r, d24=got.astype(np.int64))
    _row(label + ".depth", same.size, int(same.sum()), 0, worst)


def check_cube(label, sc, size, case, r, albedo_owner=True):
    got_c, got_d = cube_gpu(sc, size)
    contract = int(abi.product().vkr_numeric_contract())
    assert contract == 2 or not getattr(case, "world", False), "the reference of a world-space class is computed under contract 2"
    with np.errstate(invalid="ignore"):
        ref_c, ref_d = cref.cubemap_probe(cref.Arith(contract), sc, (0.0, 0.0, 0.0), size)
    cov_g, cov_r = got_d != cref.CLEAR_DISTANCE, ref_d != cref.CLEAR_DISTANCE
    assert (cov_g == cov_r).all(), f"{label}: coverage differs from the restatement on {int((cov_g != cov_r).sum())} texels"
    f = rg.CUBE_FACE
    # covered: the alpha of the colour (cleared to 0, the palette's and every tables texture's is 255)
    assert (cov_g[f] <= (got_c[f][..., 3] != 0)).all()
    rg.compare(label, case, r, covered=got_c[f][..., 3] != 0, albedo=got_c[f] if albedo_owner else None)
    for face in range(6):
        n_c, _ = parity.report(f"{label}.color{face}", abi.FMT_RGBA8_SRGB, _decode_color(got_c[face]), _decode_color(ref_c[face]))
        n_d, _ = parity.report(f"{label}.dist{face}", abi.FMT_R16_SFLOAT, got_d[face].astype(np.float32)[..., None], ref_d[face].astype(np.float32)[..., None])
        assert n_c == 0 and n_d == 0, f"{label} face {face}: {n_c} colour and {n_d} distance texels outside tolerance"


def _variants(name, program):
    v = rg.CLASSES[name].get(program)
    return [] if v is None else (v if isinstance(v, list) else [v])


@pytest.mark.parametrize("name", list(rg.CLASSES))
def test_class_on_the_three_programs(name, parity_table, oracle_lib):
    t0 = time.perf_counter()
    for args in _variants(name, "gbuf"):
        case, r = rg.get(name, args)
        check_gbuf(f"{name}.gbuf.{case.width}x{case.height}", case.scene(), case.width, case.height, case, r)
    for args in _variants(name, "shadow"):
        case, r = rg.get(name, args)
        sc = case.scene()
        label = f"{name}.shadow.{case.width}"
        check_shadow(label, shadow_gpu(sc, [IDENTITY], case.width)[0], rg.oracle_shadow(sc, IDENTITY, case.width), case, r)
    for args in _variants(name, "cube"):
        case, sc, r = rg.cube_case(name, args)
        check_cube(f"{name}.cube.{case.width}", sc, case.width, case, r)
    print(f"[raster-geometry] {name}: {time.perf_counter() - t0:.2f} s")


class _Plain:
    zmax = 1.0


def test_tables_on_the_three_programs(parity_table, oracle_lib):
    for args in rg.TABLES["gbuf"]:
        sc, r, _ = rg.tables_case("gbuf", args)
        check_gbuf(f"tables.gbuf.{args[2]}draws", sc, args[0], args[1], _Plain, r, albedo_owner=False)
    for args in rg.TABLES["shadow"]:
        sc, r, _ = rg.tables_case("shadow", args)
        check_shadow(f"tables.shadow.{args[2]}draws", shadow_gpu(sc, [IDENTITY], args[0])[0], rg.oracle_shadow(sc, IDENTITY, args[0]), _Plain, r)
    for args in rg.TABLES["cube"]:
        sc, r, _ = rg.tables_case("cube", args)
        check_cube(f"tables.cube.{args[2]}draws", sc, args[0], _Plain, r, albedo_owner=False)


def _counters(scratch, size_of, triangles, records_per_triangle, list_bytes_per_record, records_before):
    """The list counters of a rasteriser, read back from its scratch; the offset comes from the program's own *_scratch_bytes
    (size_of(triangle count)), not from a constant.  A scratch is parts padded to 256 bytes: those that do not depend on the
    triangle count, the 256-byte block of the counters last among them, and those sized by the record count (the records, then
    the lists of list_bytes_per_record bytes per record in all).  For no triangles the size ends with the counter block.  For 64
    triangles every part is a multiple of 256 bytes, so the size grows by records x (record size + list bytes): that gives the
    record size.  records_before: the records lie before the counters (cubemap_probe, gbuf_opaque_taa) or after (default_shadow).
    A layout that this does not describe yields other bytes and the comparison with the geometry fails."""
    empty = int(size_of(0))
    at = empty - 256
    if records_before:
        record = (int(size_of(64)) - empty) // (64 * records_per_triangle) - list_bytes_per_record
        assert record > 0 and (int(size_of(64)) - empty) % (64 * records_per_triangle) == 0
        at += -(-(record * records_per_triangle * triangles) // 256) * 256
    return scratch[at:at + 16].view(np.uint64)


def test_lists_hold_what_the_geometry_says(oracle_lib):
    """Which list a record goes to cannot be seen in an image (either kernel draws any triangle right), so the counters are read
    back: large (entries << 32 | chunks) and, for the programs with a small list, small (entries).  block_split has bounding
    boxes of 1, 2, 64, 64 blocks (small: at most 64) and 65, 65, 72, 72 (large: 5 chunks of 16 each, the last one partial)."""
    import torch

    want = {"small": 4, "large": 4, "chunks": 20}
    for program, args in (("shadow", (203, 203)), ("cube", (203, 203)), ("gbuf", (203, 117))):
        if program == "cube":
            case, sc, _ = rg.cube_case("block_split", args)
        else:
            case, _ = rg.get("block_split", args)
            sc = case.scene()
        blocks = [rg.centre_blocks(case, i) for i in range(len(case.pos))]
        assert sorted(blocks) == [1, 2, 64, 64, 65, 65, 72, 72]
        s, keep = sc.upload("cuda")
        n = case.width
        if program == "shadow":
            nbytes = abi.default_shadow_scratch_bytes(n, 1, _triangles(sc))
            layout = (lambda t: abi.default_shadow_scratch_bytes(n, 1, t), 2, 12, False)
            scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            array = ArrayImageBuf(abi.FMT_D24_UNORM_S8, n, n, 1, device="cuda")
            abi.default_shadow(s, [IDENTITY], [array.desc(0)], scratch.data_ptr(), nbytes, _stream())
        elif program == "cube":
            nbytes = abi.cubemap_probe_scratch_bytes(n, _triangles(sc))
            layout = (lambda t: abi.cubemap_probe_scratch_bytes(n, t), 12, 12, True)
            scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            color = ArrayImageBuf(abi.FMT_RGBA8_SRGB, n, n, 6, device="cuda")
            distance = ArrayImageBuf(abi.FMT_R16_SFLOAT, n, n, 6, device="cuda")
            abi.cubemap_probe(s, (0.0, 0.0, 0.0), color.descs(), distance.descs(), scratch.data_ptr(), nbytes, _stream())
        else:
            lib = abi.product()
            h = case.height
            layout = (lambda t: lib.vkr_raster_scratch_bytes(n, h, t), 2, 8, True)
            g = rg.Gbuf(n, case.height, "product")
            scratch = g.raster(sc, keep_scratch=True)["scratch"]
        _sync()
        state = _counters(scratch.cpu().numpy(), layout[0], _triangles(sc), *layout[1:])
        got = {"large": int(state[0] >> np.uint64(32)), "chunks": int(state[0] & np.uint64(0xFFFFFFFF))}
        if program != "gbuf":  # gbuf_opaque_taa has no small list: a wave per triangle
            got["small"] = int(state[1])
        print(f"[raster-geometry] lists of block_split on {program}: {got}")
        assert got == {k: want[k] for k in got}, (program, got)


FOUR = ("near_plane", "centre_lattice", "exact_ties", "block_split")  # near_plane first: its w row needs the untranslated layer
FOUR_SIZE = 291


def test_four_layers_carry_four_classes(parity_table, oracle_lib):
    """One default_shadow call, four layers, one scene: class j sits 10 j NDC units to the right (its draws' model matrices) and
    layer l looks 10 l units to the right, so layer l shows class l alone -- the others lie outside its frustum, are rejected or
    listed empty in ITS lists.  A layer that read another layer's lists or records would show another class.  Every layer must be
    the oracle's map of its class alone, bit for bit (the classes are compared with the exact reference in their own test)."""
    cases = [rg.build(name, (FOUR_SIZE, FOUR_SIZE)) for name in FOUR]
    combined = rg.Case("four", FOUR_SIZE, FOUR_SIZE)
    for j, case in enumerate(cases):
        ids = {}
        for i, p in enumerate(case.pos):
            d = case.draw_of[i]
            if d not in ids:
                ids[d] = combined.draw(k=case.draws[d]["k"], c=case.draws[d]["c"])
                combined.draws[ids[d]]["tx"] = 10.0 * j
            combined.tri(p, ids[d])
    mvps = []
    for l in range(4):
        m = IDENTITY.copy()
        m[0, 3] = -10.0 * l
        mvps.append(m)
    got = shadow_gpu(combined.scene(), mvps, FOUR_SIZE)
    for l, case in enumerate(cases):
        want = rg.oracle_shadow(case.scene(), IDENTITY, FOUR_SIZE)
        same = got[l] == want
        assert (want != 0xFFFFFF).sum() > 1000
        assert same.all(), f"layer {l} ({FOUR[l]}): {int((~same).sum())} texels differ from the oracle's map of that class alone"
        _row(f"four_layers.{l}.{FOUR[l]}.depth", same.size, int(same.sum()), 0, 0.0)
    assert len({got[l].tobytes() for l in range(4)}) == 4


@pytest.mark.parametrize("name,size", [("large_flood", (328, 200)), ("centre_lattice", (204, 118))])
def test_host_frame_raster_stage(name, size, oracle_lib):
    """the same geometry through HostFrame with STAGE_RASTER (the C++ rendergraph mirror: clear, buffers, one draw per primitive)"""
    w, h = size
    case, r = rg.get(name, size)
    sc = case.scene()
    setup = FrameSetup(w, h)
    frame = host.HostFrame(setup, device="cuda")
    frame.load_scene(sc)
    frame.run(host.STAGE_LUT)
    frame.set_camera(IDENTITY, IDENTITY, IDENTITY, setup.fazz)
    frame.run(host.STAGE_RASTER)
    want = rg.Gbuf(w, h, "oracle").raster(sc)
    depth = frame.download("depth").raw(0)[..., 0].astype(np.uint32)
    albedo = frame.download("albedo").raw(0)
    frame.close()
    assert np.array_equal(depth & 0xFFFFFF, want["depth"] & 0xFFFFFF), f"{name}: depth differs from the oracle"
    rg.compare(f"{name}.host_frame", case, r, d24=(depth & 0xFFFFFF).astype(np.int64), albedo=albedo, covered=albedo[..., 3] != 0)
