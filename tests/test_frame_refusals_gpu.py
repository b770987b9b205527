"""What PostFxFrame refuses before it records anything, with the exact messages: the stages and setters a tiled frame does not
take, the stages that need a scene, an acceleration structure, probes or shadow maps, the stages that write the same images,
and the names of the image table (vkrh_image, vkrh_create_image).  Nothing here launches a pass: every call is refused before
recording, or only describes an image.  The texts are written out: they are what callers (and the other tests) match on."""
import ctypes as C

import pytest

from vk_renderer_amd import abi, host
from vk_renderer_amd.camera import FrameSetup

W, H = 256, 144  # the frames of the test_frame_stage_is_refused_on_a_tiled_frame tests

TILED_STAGES = [
    (host.STAGE_CLEAR_PREV_DEPTH, "vkrh_run: VKRH_STAGE_CLEAR_PREV_DEPTH on a tiled frame (transfers take whole images)"),
    (host.STAGE_SSAO, "vkrh_run: VKRH_STAGE_SSAO on a tiled frame (a sample's reach is unbounded near the eye: SSAO runs on one GPU)"),
    (host.STAGE_TILE_REGRESSION,
     "vkrh_run: VKRH_STAGE_TILE_REGRESSION on a tiled frame (halved strip bounds are no multiples of 8: tiles would straddle owners)"),
    (host.STAGE_BACKBUFFER,
     "vkrh_run: VKRH_STAGE_BACKBUFFER on a tiled frame (the uv of a pixel spans the whole source: the backbuffer is drawn on one GPU)"),
    (host.STAGE_SHADOW_MASK_RT, "vkrh_run: VKRH_STAGE_SHADOW_MASK_RT on a tiled frame (the rays reach anywhere: ray-traced shadows run on one GPU)"),
    (host.STAGE_REFLECTIONS_RT,
     "vkrh_run: VKRH_STAGE_REFLECTIONS_RT on a tiled frame (the rays reach anywhere: ray-traced reflections run on one GPU)"),
    (host.STAGE_SHADOW_MASK, "vkrh_run: VKRH_STAGE_SHADOW_MASK on a tiled frame (the shadow maps are rendered on one GPU)"),
    (host.STAGE_SHADOW, "vkrh_run: VKRH_STAGE_SHADOW on a tiled frame (the shadow maps are rendered on one GPU)"),
    (host.STAGE_GTAO_RT, "vkrh_run: VKRH_STAGE_GTAO_RT on a tiled frame (ray-traced AO runs on one GPU)"),
    (host.STAGE_PROBE_TRACE, "vkrh_run: VKRH_STAGE_PROBE_TRACE on a tiled frame (probes are traced on one GPU)"),
    # several refused stages in one mask: the first check of vkrh_run decides
    (host.STAGE_PROBE_TRACE | host.STAGE_GTAO_RT | host.STAGE_SSAO,
     "vkrh_run: VKRH_STAGE_SSAO on a tiled frame (a sample's reach is unbounded near the eye: SSAO runs on one GPU)"),
    (host.STAGE_SHADOW | host.STAGE_SHADOW_MASK | host.STAGE_REFLECTIONS_RT | host.STAGE_SSR,
     "vkrh_run: VKRH_STAGE_REFLECTIONS_RT on a tiled frame (the rays reach anywhere: ray-traced reflections run on one GPU)"),
    (host.STAGE_SHADOW_MASK_RT | host.STAGE_SHADOW_MASK,
     "vkrh_run: VKRH_STAGE_SHADOW_MASK_RT on a tiled frame (the rays reach anywhere: ray-traced shadows run on one GPU)"),
    (host.STAGE_GTAO_RT | host.STAGE_GTAO | host.STAGE_SHADOW, "vkrh_run: VKRH_STAGE_SHADOW on a tiled frame (the shadow maps are rendered on one GPU)"),
]

SSR_STAGES = (host.STAGE_SSR, host.STAGE_SSR_CLASSIFIED, host.STAGE_SSR_RESOLVE, host.STAGE_SSR_TRACE, 1 << 18, 1 << 19)  # .. _TRACE_HEAD, _TRACE_RESUME
REFLECTIONS_WITH_SSR = ("vkrh_run: VKRH_STAGE_REFLECTIONS_RT together with an SSR stage (VKRH_STAGE_SSR, _SSR_CLASSIFIED, _SSR_RESOLVE, "
                        "_SSR_TRACE*: all write the images reflections / blurred)")
SHADOW_MASKS_TOGETHER = "vkrh_run: VKRH_STAGE_SHADOW_MASK_RT together with VKRH_STAGE_SHADOW_MASK (both write the image shadow_mask)"
GTAOS_TOGETHER = "vkrh_run: VKRH_STAGE_GTAO_RT together with VKRH_STAGE_GTAO (both write GTAO's raw, filtered and accumulated images)"

PLAIN_STAGES = [
    (host.STAGE_SHADOW_MASK_RT, "vkrh_run: VKRH_STAGE_SHADOW_MASK_RT without a loaded scene (vkrh_load_scene builds its acceleration structure)"),
    (host.STAGE_REFLECTIONS_RT,
     "vkrh_run: VKRH_STAGE_REFLECTIONS_RT without a loaded scene (vkrh_load_scene builds its acceleration structure and attribute table)"),
    (host.STAGE_SHADOW_MASK, "vkrh_run: VKRH_STAGE_SHADOW_MASK without rendered shadow maps (VKRH_STAGE_SHADOW for the lights in use)"),
    (host.STAGE_SHADOW, "vkrh_run: VKRH_STAGE_SHADOW without a loaded scene (vkrh_load_scene)"),
    (host.STAGE_SHADOW | host.STAGE_SHADOW_MASK, "vkrh_run: VKRH_STAGE_SHADOW without a loaded scene (vkrh_load_scene)"),  # the maps would be current
    (host.STAGE_GTAO_RT, "vkrh_run: VKRH_STAGE_GTAO_RT without a loaded scene (vkrh_load_scene builds its acceleration structure)"),
    (host.STAGE_PROBE_TRACE, "vkrh_run: VKRH_STAGE_PROBE_TRACE without baked probes (vkrh_bake_probes)"),
    (host.STAGE_RASTER, "vkrh_run: VKRH_STAGE_RASTER without a loaded scene"),
    # stages that write the same images
    (host.STAGE_SHADOW_MASK_RT | host.STAGE_SHADOW_MASK, SHADOW_MASKS_TOGETHER),
    (host.STAGE_GTAO_RT | host.STAGE_GTAO, GTAOS_TOGETHER),
] + [(host.STAGE_REFLECTIONS_RT | s, REFLECTIONS_WITH_SSR) for s in SSR_STAGES] + [
    # masks that trip several rules: the first check of vkrh_run decides
    (host.STAGE_GTAO_RT | host.STAGE_GTAO | host.STAGE_REFLECTIONS_RT | host.STAGE_SSR, REFLECTIONS_WITH_SSR),
    (host.STAGE_PROBE_TRACE | host.STAGE_GTAO_RT | host.STAGE_SHADOW | host.STAGE_SHADOW_MASK,
     "vkrh_run: VKRH_STAGE_SHADOW without a loaded scene (vkrh_load_scene)"),
    (host.STAGE_PROBE_TRACE | host.STAGE_GTAO_RT | host.STAGE_SHADOW_MASK,
     "vkrh_run: VKRH_STAGE_SHADOW_MASK without rendered shadow maps (VKRH_STAGE_SHADOW for the lights in use)"),
    (host.STAGE_PROBE_TRACE | host.STAGE_GTAO_RT | host.STAGE_GTAO, GTAOS_TOGETHER),
    (host.STAGE_PROBE_TRACE | host.STAGE_GTAO_RT, "vkrh_run: VKRH_STAGE_GTAO_RT without a loaded scene (vkrh_load_scene builds its acceleration structure)"),
    (host.STAGE_REFLECTIONS_RT | host.STAGE_SHADOW_MASK_RT | host.STAGE_SHADOW_MASK | host.STAGE_SSR, SHADOW_MASKS_TOGETHER),
    (host.STAGE_RASTER | host.STAGE_SHADOW, "vkrh_run: VKRH_STAGE_SHADOW without a loaded scene (vkrh_load_scene)"),
]

# the image table on a plain W x H frame that has run nothing: (width, height) of mip 0, or the refusal
IMAGES = {
    "depth": (W, H), "prev_depth": (W, H), "normal": (W, H), "albedo": (W, H), "material": (W, H), "velocity": (W, H),
    "dn": (W // 2, H // 2), "dv": (W // 2, H // 2), "raw": (W // 2, H // 2), "filtered": (W // 2, H // 2), "acc_ao": (W // 2, H // 2),
    "acc_hist": (W // 2, H // 2), "rays": (W // 2, H // 2), "reflections": (W // 2, H // 2), "blurred": (W // 2, H // 2),
    "blurred_hist": (W // 2, H // 2), "pdf": (1024, 1024), "taa_hist": (W, H), "taa_target": (W, H), "frame_hiz": (W, H),
    "frame_normals": (W // 2, H // 2), "frame_albedo": (W, H), "color_out": (W, H), "brdf": (1024, 1024), "ao_prev_frame": (W // 2, H // 2),
    "ao_output": (W // 2, H // 2), "deinterleaved_depth": (W // 8, H // 8), "st_raw": (W, H), "st_filtered": (W, H), "st_accumulated": (W, H),
    "pend_mask": "vkrh_image: 'pend_mask' only exists with hit normals by request",
    "probe_trace": "vkrh_image: 'probe_trace' only exists after VKRH_STAGE_PROBE_TRACE",
    "probe_color": "vkrh_image: 'probe_color' only exists after vkrh_bake_probes",
    "probe_depth": "vkrh_image: 'probe_depth' only exists after vkrh_bake_probes",
    "cubemap_color": "vkrh_image: 'cubemap_color' only exists after vkrh_bake_probes",
    "cubemap_distance": "vkrh_image: 'cubemap_distance' only exists after vkrh_bake_probes",
    "shadows": "vkrh_image: 'shadows' only exists after VKRH_STAGE_SHADOW",
    "readback": "vkrh_image: 'readback' only exists after a final-frame capture (vkrh_capture kind 3)",
    "ssao": "vkrh_image: 'ssao' only exists after VKRH_STAGE_SSAO or vkrh_set_ssao_samples",
    "tile_planes": "vkrh_image: 'tile_planes' only exists after VKRH_STAGE_TILE_REGRESSION",
    "backbuffer": "vkrh_image: 'backbuffer' only exists after VKRH_STAGE_BACKBUFFER",
    "shadow_mask": "vkrh_image: 'shadow_mask' only exists after VKRH_STAGE_SHADOW_MASK or VKRH_STAGE_SHADOW_MASK_RT",
}


def _call(fn, *args):
    """-> (status, message) of one vkrh_* call"""
    rc = fn(*args)
    return rc, host.lib().vkrh_last_error().decode() if rc != 0 else ""


def setters(h, count):
    """(name, status, message) of the first `count` of the calls that refuse a tiled frame (the seven setters first), with
    arguments a plain frame takes"""
    l = host.lib()
    f4, f48, f3 = (C.c_float * 4)(0, 1, 0, 1), (C.c_float * 48)(), (C.c_float * 3)(0, 0, 0)
    calls = [("vkrh_set_ssao_samples", (h, f48, 0)), ("vkrh_set_shadow_mask", (h, 0, 1, 0)), ("vkrh_set_shadow_rays", (h, f4, 1, 1e-3, 0.0)),
             ("vkrh_set_shadow_area_lights", (h, f4, 1, 16, 4)), ("vkrh_set_reflection_rays", (h, 0, 1e-3, 0.0, 0.0, 0)),
             ("vkrh_set_ray_cutouts", (h, 1, 0)), ("vkrh_set_backbuffer", (h, b"albedo", 0, 0, 0)),
             ("vkrh_bake_probes", (h, C.byref(f3), C.byref(f3), 4, 64, 64)),
             ("vkrh_create_image", (h, b"mine", abi.FMT_RGBA8_UNORM, 8, 8, 1, 1)), ("vkrh_transfer", (h, 1, b"depth", None, None))]
    return [(name,) + _call(getattr(l, name), *args) for name, args in calls[:count]]


TILED_SETTERS = [
    ("vkrh_set_ssao_samples", "vkrh_set_ssao_samples: on a tiled frame (VKRH_STAGE_SSAO runs on one GPU)"),
    ("vkrh_set_shadow_mask", "vkrh_set_shadow_mask: on a tiled frame (VKRH_STAGE_SHADOW_MASK runs on one GPU)"),
    ("vkrh_set_shadow_rays", "vkrh_set_shadow_rays: on a tiled frame (VKRH_STAGE_SHADOW_MASK_RT runs on one GPU)"),
    ("vkrh_set_shadow_area_lights", "vkrh_set_shadow_area_lights: on a tiled frame (VKRH_STAGE_SHADOW_MASK_RT runs on one GPU)"),
    ("vkrh_set_reflection_rays", "vkrh_set_reflection_rays: on a tiled frame (VKRH_STAGE_REFLECTIONS_RT runs on one GPU)"),
    ("vkrh_set_ray_cutouts", "vkrh_set_ray_cutouts: on a tiled frame (the ray-traced stages run on one GPU)"),
    ("vkrh_set_backbuffer", "vkrh_set_backbuffer: on a tiled frame (VKRH_STAGE_BACKBUFFER runs on one GPU)"),
    # the three calls beside the seven setters that carry the same refusal
    ("vkrh_bake_probes", "vkrh_bake_probes: on a tiled frame (probes are baked on one GPU)"),
    ("vkrh_create_image", "vkrh_create_image: on a tiled frame (transfers take whole images)"),
    ("vkrh_transfer", "vkrh_transfer: on a tiled frame (transfers take whole images)"),
]


def check_tiled(h):
    l = host.lib()
    for mask, text in TILED_STAGES:
        assert _call(l.vkrh_run, h, mask) == (1, text), hex(mask)
    assert l.vkrh_last_tasks(h) == b""  # nothing was ever submitted
    got = setters(h, 10)
    assert [(n, m) for n, rc, m in got] == TILED_SETTERS
    assert all(rc == 1 for n, rc, m in got)


def check_plain_stages(h):
    l = host.lib()
    for mask, text in PLAIN_STAGES:
        assert _call(l.vkrh_run, h, mask) == (1, text), hex(mask)
    assert l.vkrh_last_tasks(h) == b""
    # a plain frame takes the seven setters (with the same arguments)
    assert [rc for n, rc, m in setters(h, 7)] == [0] * 7


def describe(h, name):
    d = abi.VkrImg()
    rc, msg = _call(host.lib().vkrh_image, h, name.encode(), 0, 1, C.byref(d))
    return msg if rc else (d.width, d.height)


def check_images(h):
    l = host.lib()
    want = IMAGES
    assert len(want) == 42
    got = {n: describe(h, n) for n in want}
    assert got == want, {n: (got[n], want[n]) for n in want if got[n] != want[n]}
    assert describe(h, "no_such_image") == "vkrh_image: unknown image 'no_such_image'"
    assert describe(h, "") == "vkrh_image: unknown image ''"
    # vkrh_create_image: a built-in name, a built-in name whose image does not exist yet, and a user's name are all taken
    create = lambda name, fmt=abi.FMT_RGBA8_UNORM: _call(l.vkrh_create_image, h, name, fmt, 8, 4, 1, 1)  # noqa: E731
    assert create(b"depth") == (1, "vkrh_create_image: the name 'depth' is taken")
    assert create(b"st_accumulated") == (1, "vkrh_create_image: the name 'st_accumulated' is taken")
    assert create(b"ssao") == (1, "vkrh_create_image: the name 'ssao' is taken")
    assert create(b"pend_mask") == (1, "vkrh_create_image: the name 'pend_mask' is taken")
    assert describe(h, "ssao") == IMAGES["ssao"]  # asking did not create it
    assert create(b"mine", 9999) == (1, "vkrh_create_image: unknown format 9999")  # a free name: the next check is reached
    assert describe(h, "mine") == "vkrh_image: unknown image 'mine'"
    assert create(b"mine") == (0, "")
    assert describe(h, "mine") == (8, 4)
    assert create(b"mine") == (1, "vkrh_create_image: the name 'mine' is taken")


@pytest.mark.gpu
def test_tiled_frame_refuses_stages_and_setters_with_their_messages():
    tiled = host.HostFrame(FrameSetup(W, H), device="cuda",
                           native_tiled=dict(rank=0, world=1, halo=48, gathered_mips=4, force_tiled=True, comm=None, row_bounds=None))
    try:
        check_tiled(tiled.h)
    finally:
        tiled.close()


@pytest.mark.gpu
def test_plain_frame_refuses_stages_without_their_inputs_and_names_its_images():
    plain = host.HostFrame(FrameSetup(W, H), device="cuda")
    try:
        check_images(plain.h)
        check_plain_stages(plain.h)
        assert describe(plain.h, "ssao") == (W, H)  # vkrh_set_ssao_samples made it appear
    finally:
        plain.close()
