"""GPU tests of the shadow-map pass (csrc/shadow.hip, program default_shadow) and of VKRH_STAGE_SHADOW: the kernel against the
oracle's G-buffer rasteriser under the light's matrix (tests/shadow_light.py), the solid shadow of a cutout, several layers in
one call, rays through the scene's acceleration structure, and the frame stage against the entry called by hand.  Procedural
scenes only.

Measured on an MI355X: 0 differing texels and no top byte in all 12 single-layer cases (lights A, B, C x 1024^2, 360^2 x the
cutout scene and detail 64; coverage 0.9444 / 1.0000 / 0.5941 and 0.9444 / 0.9726 / 0.5786); 1728 and 100403 texels differ
from the textured raster for A and B; 8553 to 16384 rays per case, none hitting before the surface, none missing it."""
import numpy as np
import pytest

from vk_renderer_amd import abi, camera, host
from vk_renderer_amd import scene as scn
from vk_renderer_amd.camera import FrameSetup
from vk_renderer_amd.images import ArrayImageBuf

import shadow_light as sl

pytestmark = pytest.mark.gpu

RAY_EPS = 1e-3  # of the distance eye -> surface; the cap on disagreeing rays is 0


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch

    torch.cuda.synchronize()


def _triangles(sc):
    return sum(d["index_count"] // 3 for d in sc.draws)


def render(sc, mvps, n, uploaded=None, array=None):
    """vkr_default_shadow with len(mvps) layers -> the whole words, uint32 [layers of the array, n, n]"""
    import torch

    s, keep = uploaded if uploaded is not None else sc.upload("cuda")
    if array is None:
        array = ArrayImageBuf(abi.FMT_D24_UNORM_S8, n, n, len(mvps), device="cuda", fill=0x5A)
    nbytes = abi.default_shadow_scratch_bytes(n, len(mvps), _triangles(sc))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    abi.default_shadow(s, mvps, [array.desc(l) for l in range(len(mvps))], scratch.data_ptr(), nbytes, _stream())
    _sync()
    return array.raw()[..., 0]


SCENES = {"cutout": lambda: scn.procedural_scene(cutout=True), "detail64": lambda: scn.procedural_scene(detail=64)}
# "backdrop": a quad that fills the map of light A behind the cutout scene.  At 200^2 the bounding box of each of its triangles
# is 25 x 25 = 625 blocks of 8 x 8: 39 chunks of 16 and a last one of 1 for the large kernel, on an extent that is no multiple
# of the chunk; lights B and C see the quad obliquely.
SCENES["backdrop"] = lambda: sl.add_backdrop(scn.procedural_scene(cutout=True), sl.mvp("A"))
CASES = [(name, n) for name in ("cutout", "detail64") for n in (1024, 360)] + [("backdrop", 200)]


@pytest.mark.parametrize("scene_name,n", CASES)
def test_single_layer_matches_the_oracle(scene_name, n):
    """bit for bit on the low 24 bits, top byte 0 everywhere, for the lights A, B, C"""
    sc = SCENES[scene_name]()
    uploaded = sc.upload("cuda")
    for name in "ABC":
        m = sl.mvp(name)
        got = render(sc, [m], n, uploaded)[0]
        want = sl.expected(sc, m, n)
        if scene_name == "backdrop" and name == "A":
            assert ((n + 7) // 8) ** 2 % 16 != 0 and (want != sl.D24_MAX).all(), "the quad fills the map: a partial last chunk"
        bad = int((got != want).sum())
        print(f"[shadow] {scene_name} {n} light {name}: covered {float((want != sl.D24_MAX).mean()):.4f}, differing texels {bad}, "
              f"texels with a top byte {int((got >> 24 != 0).sum())}")
        assert (got >> 24 == 0).all(), f"{scene_name} {n} {name}: a stored word has a top byte"
        assert bad == 0, f"{scene_name} {n} {name}: {bad} texels differ from the oracle"


def test_cutout_casts_a_solid_shadow():
    """the oracle's TEXTURED depth has the fence's holes; the shadow map does not"""
    sc = scn.procedural_scene(cutout=True)
    uploaded = sc.upload("cuda")
    for name in "AB":
        m = sl.mvp(name)
        got = render(sc, [m], 1024, uploaded)[0]
        textured = sl.oracle_depth(sc, m, 1024)
        differ = int((got != textured).sum())
        print(f"[shadow] light {name}: {differ} texels differ from the textured raster")
        assert differ >= 1
        assert (got <= textured).all(), "a solid fence can only be nearer than a fence with holes"


def test_four_layers_in_one_call():
    sc = scn.procedural_scene(cutout=True)
    uploaded = sc.upload("cuda")
    n = 360
    mats = [sl.mvp(k) for k in "ABCA"]
    together = render(sc, mats, n, uploaded)
    for l, m in enumerate(mats):
        alone = render(sc, [m], n, uploaded)[0]
        assert (together[l] == alone).all(), f"layer {l} of the 4-layer call differs from its own call"
    assert (together[0] == together[3]).all() and (together[0] != together[1]).any()
    # layer_count 2 on a 4-layer array: layers 2 and 3 keep what they held
    array = ArrayImageBuf(abi.FMT_D24_UNORM_S8, n, n, 4, device="cuda", fill=0xA7)
    two = render(sc, mats[:2], n, uploaded, array=array)
    assert (two[0] == together[0]).all() and (two[1] == together[1]).all()
    assert (two[2:] == 0xA7A7A7A7).all()
    assert (array.to_host().reshape(4, n, array.pitch[0])[2:] == 0xA7).all(), "row padding of the untouched layers included"


@pytest.mark.parametrize("n,step", [(1024, 8), (360, 3)])
def test_rays_agree_with_the_map(n, step):
    """On the kernel's own map: a ray from the light's eye to the unprojected centre of a covered texel hits nothing on
    t in [0, 1 - 1e-3] and something on [0, 1 + 1e-3] (vkr_accel_query over the scene's triangles), for every sampled texel."""
    import torch

    sc = scn.procedural_scene(cutout=True)
    uploaded = sc.upload("cuda")
    accel = abi.Accel.from_scene(sc)
    try:
        for name in "ABC":
            m = sl.mvp(name)
            got = render(sc, [m], n, uploaded)[0]
            pts = sl.sample_grid(got, step)
            o, d = sl.rays(name, pts, got, m)
            to, td = torch.from_numpy(np.ascontiguousarray(o)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()
            out = torch.zeros((len(o),), dtype=torch.int32, device="cuda")
            accel.query(to, td, 0.0, 1.0 - RAY_EPS, out, _stream())
            _sync()
            early = int(out.sum().item())
            accel.query(to, td, 0.0, 1.0 + RAY_EPS, out, _stream())
            _sync()
            missed = int((out == 0).sum().item())
            print(f"[shadow rays] {n} light {name}: {len(pts)} rays, {early} hit before the surface, {missed} miss it")
            assert len(pts) > 1000
            assert early == 0 and missed == 0
    finally:
        accel.close()


# ---- the frame stage ----------------------------------------------------------------------------------------------------------------
W, H = 256, 144


def _layer_words(frame, layer):
    return frame.download("shadows", layer).raw(0)[..., 0]


def test_frame_stage_fills_the_shadow_layers():
    sc = scn.procedural_scene(detail=12, cutout=True)
    frame = host.HostFrame(FrameSetup(W, H), device="cuda")
    try:
        frame.load_scene(sc)
        lights = frame.shadow_lights()
        assert len(lights) == 1 and np.array_equal(lights[0].view(np.uint32), camera.shadow_mvp().view(np.uint32))
        frame.run(host.STAGE_RASTER | host.STAGE_SHADOW)
        _sync()
        tasks = frame.last_tasks()
        assert tasks.count("ShadowPass") == 1 and tasks.index("GbufferPass") < tasks.index("ShadowPass")
        by_hand = render(sc, [camera.shadow_mvp()], 1024)[0]
        got = _layer_words(frame, 0)
        assert got.shape == (1024, 1024) and (got == by_hand).all(), f"{int((got != by_hand).sum())} texels differ from the entry called by hand"
        assert (got != sl.D24_MAX).mean() > 0.5
        # two lights of another size: layers 0 and 1
        frame.set_shadow_lights([sl.mvp("B"), sl.mvp("C")], 360)
        frame.run(host.STAGE_SHADOW)
        _sync()
        assert frame.last_tasks() == ["ShadowPass", "ShadowPass"]
        by_hand = render(sc, [sl.mvp("B"), sl.mvp("C")], 360)
        for layer in range(2):
            got = _layer_words(frame, layer)
            assert got.shape == (360, 360) and (got == by_hand[layer]).all(), f"layer {layer}: {int((got != by_hand[layer]).sum())} texels differ"
    finally:
        frame.close()


def test_raster_passes_share_a_lane_when_tasks_overlap():
    """set_async(True): GbufferPass and the ShadowPasses use the command context's one scratch allocation, so they stay on one
    lane, in order, and the maps equal those of the one-stream frame"""
    sc = scn.procedural_scene(detail=12, cutout=True)
    maps = {}
    for overlap in (False, True):
        frame = host.HostFrame(FrameSetup(W, H), device="cuda")
        try:
            frame.load_scene(sc)
            frame.set_async(overlap)
            frame.set_shadow_lights([sl.mvp("A"), sl.mvp("B")], 360)
            frame.run(host.STAGE_RASTER | host.STAGE_SHADOW | host.STAGE_DOWNSAMPLE)
            _sync()
            tasks, lanes = frame.last_tasks(), frame.last_lanes()
            assert tasks[:3] == ["GbufferPass", "ShadowPass", "ShadowPass"]
            assert lanes[0] == lanes[1] == lanes[2], (tasks, lanes)
            maps[overlap] = [_layer_words(frame, l) for l in range(2)] + [frame.download("depth").to_host().copy()]
        finally:
            frame.close()
    for a, b in zip(maps[False], maps[True]):
        assert np.array_equal(a, b)


def test_shading_output_does_not_depend_on_the_stage():
    """a full frame with and without STAGE_SHADOW: color_out and taa_target bit-identical (binding 5 is never read)"""
    outs = {}
    for shadow in (False, True):
        sc = scn.procedural_scene(detail=12, cutout=True)
        frame = host.HostFrame(FrameSetup(W, H), device="cuda")
        try:
            frame.load_scene(sc)
            frame.run(host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH)
            mask = host.STAGE_RASTER | host.STAGE_CHAIN | host.STAGE_SHADING | (host.STAGE_SHADOW if shadow else 0)
            for _ in range(2):
                frame.run(mask)
                tasks = frame.last_tasks()
                frame.end_frame()
            _sync()
            assert ("ShadowPass" in tasks) == shadow and "DeferedShading" in tasks
            if shadow:
                assert tasks.index("GbufferPass") < tasks.index("ShadowPass") < tasks.index("DownsampleGbuffer")
            outs[shadow] = {n: frame.download(n).to_host().copy() for n in ("color_out", "taa_target", "taa_hist")}
        finally:
            frame.close()
    for n in outs[False]:
        assert np.array_equal(outs[False][n], outs[True][n]), f"{n} changes with STAGE_SHADOW"
    assert outs[True]["color_out"].any()


def test_stage_refusals_on_a_device_frame():
    frame = host.HostFrame(FrameSetup(W, H), device="cuda")
    try:
        with pytest.raises(RuntimeError, match="without a loaded scene"):
            frame.run(host.STAGE_SHADOW)
        assert "ShadowPass" not in frame.last_tasks()
    finally:
        frame.close()
    tiled = host.HostFrame(FrameSetup(W, H), device="cuda", tiled=True)
    try:
        with pytest.raises(RuntimeError, match="tiled frame"):
            tiled.run(host.STAGE_SHADOW)
    finally:
        tiled.close()
