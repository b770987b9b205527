"""ctypes binding of the C++ host mirror (host/libvkr_host.so): the reference's pass structs
(Gbuffer, DownsamplePass, AdvancedSSR, GTAO, TAA) on the rendergraph mirror, driven one stage at
a time.  Device memory for every graph image comes from torch through the allocator hook, so
the launcher can hand the same memory to torch.distributed (RCCL) without copies."""
import ctypes as C
import os

import numpy as np

from . import abi

STAGE_LUT, STAGE_GBUFFER, STAGE_PREV_DEPTH, STAGE_DOWNSAMPLE = 1, 2, 4, 8
STAGE_HIZ_TAIL, STAGE_SSR, STAGE_GTAO, STAGE_TAA = 16, 32, 64, 128
STAGE_SHADING, STAGE_BRDF_LUT, STAGE_GTAO_MAIN_ONLY = 256, 512, 1024
STAGE_GTAO_GRAPHICS, STAGE_GTAO_DEINTERLEAVED, STAGE_SCREEN_TRACE = 2048, 4096, 8192
STAGE_SSR_CLASSIFIED, STAGE_SSR_TRACE, STAGE_SSR_RESOLVE = 16384, 32768, 65536
STAGE_RASTER = 131072
STAGE_GTAO_RT = 1 << 21  # ray-traced AO (main.cpp:379-388 use_rt_ao): needs load_scene(); not with STAGE_GTAO, not tiled
STAGE_PROBE_TRACE = 1 << 22  # ProbeTracePass::run through the grid of bake_probes() -> image "probe_trace"; not tiled
STAGE_SHADOW = 1 << 23  # SceneRenderer::render_shadow per configured light -> layers of image "shadows"; needs load_scene(); not tiled
STAGE_CLEAR_PREV_DEPTH = 1 << 24  # clear_depth(graph, gbuffer.prev_depth) (main.cpp:306), before every other stage; not tiled
TEXTURE_GEN_MIPS = 1  # vkrh_scene_texture.flags: only level 0 comes from the host, the frame builds the others (vkr_gen_mipmaps)
STAGE_SSAO = 1 << 25  # SSAOPass::draw: depth mip 0 -> image "ssao" (R8_UNORM); after the G-buffer / raster / shadow stages, before the downsample; not tiled
STAGE_TILE_REGRESSION = 1 << 26  # AdvancedSSR::run_tile_regression_pass: depth mip 1 -> image "tile_planes" (RGBA32_SFLOAT, (W/16, H/16)); after the downsample; not tiled
STAGE_BACKBUFFER = 1 << 27  # add_backbuffer_subpass + add_present_subpass: the TAA output (or set_backbuffer's image) -> image "backbuffer" (RGBA8_SRGB); last; not tiled
STAGE_SHADOW_MASK_RT = 1 << 29  # ShadowMaskPass::run_rt: depth mip 0 + normal + the loaded scene's acceleration structure -> image "shadow_mask" (the image and slot of STAGE_SHADOW_MASK), one ray per pixel and light of set_shadow_rays; needs load_scene(); not with STAGE_SHADOW_MASK, not tiled
STAGE_REFLECTIONS_RT = 1 << 30  # AdvancedSSR::run_rt: depth mip 1 + the half-resolution normals + the loaded scene's acceleration structure, attribute table and textures -> images "reflections" and "blurred": ReflectionsRT -> SSSR_blur, or with set_reflection_rays(fill_misses=True) SSSR_trace -> SSSR_filter -> ReflectionsRT -> SSSR_blur; needs load_scene(); not with any SSR stage, not tiled
STAGE_SHADOW_MASK = 1 << 28  # ShadowMaskPass::run: depth mip 0 + the layers of "shadows" -> image "shadow_mask" (RGBA8_UNORM, channel l = light l); after the raster / shadow stages, before the shading; needs the maps of STAGE_SHADOW; not tiled
STAGE_CHAIN = STAGE_DOWNSAMPLE | STAGE_SSR | STAGE_GTAO | STAGE_TAA


class HostConfig(C.Structure):
    _fields_ = [("full_width", C.c_uint32), ("full_height", C.c_uint32), ("origin_x", C.c_int32), ("origin_y", C.c_int32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("tiled", C.c_uint32), ("stream", C.c_void_p)]


class TiledConfig(C.Structure):
    _fields_ = [("full_width", C.c_uint32), ("full_height", C.c_uint32), ("rank", C.c_uint32), ("world", C.c_uint32),
                ("halo", C.c_uint32), ("gathered_mips", C.c_uint32), ("force_tiled", C.c_uint32), ("albedo_by_gather", C.c_uint32),
                ("stream", C.c_void_p), ("comm", C.c_void_p), ("row_bounds", C.POINTER(C.c_uint32))]


class GatherPart(C.Structure):
    _fields_ = [("send", C.c_void_p), ("recv", C.c_void_p), ("bytes", C.c_uint64)]


class HaloPeer(C.Structure):
    _fields_ = [("peer", C.c_int32), ("reserved", C.c_uint32), ("send", C.c_void_p), ("send_bytes", C.c_uint64),
                ("recv", C.c_void_p), ("recv_bytes", C.c_uint64)]


class HostCamera(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("prev_view", C.c_float * 16), ("projection", C.c_float * 16),
                ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float)]


class SceneDraw(C.Structure):
    _fields_ = [("transform", C.c_float * 16), ("vertex_offset", C.c_uint32), ("index_offset", C.c_uint32), ("index_count", C.c_uint32),
                ("albedo_tex_index", C.c_uint32), ("metalic_roughness_index", C.c_uint32), ("clip_alpha", C.c_uint32)]


class SceneTexture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("mip_levels", C.c_uint32), ("flags", C.c_uint32),
                ("levels", C.c_void_p * 16)]


_ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_uint64, C.c_void_p)
_FREE = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
_lib = None


def lib():
    global _lib
    if _lib is None:
        l = abi._load(abi.HOST_LIB, "host library libvkr_host.so")
        l.vkrh_create.argtypes = [C.POINTER(HostConfig)]
        l.vkrh_create.restype = C.c_void_p
        l.vkrh_destroy.argtypes = [C.c_void_p]
        l.vkrh_last_error.restype = C.c_char_p
        l.vkrh_set_camera.argtypes = [C.c_void_p, C.POINTER(HostCamera)]
        l.vkrh_pin_randoms.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32]
        l.vkrh_has_program.argtypes = [C.c_char_p]
        l.vkrh_set_gtao_mode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        l.vkrh_set_synth_flags.argtypes = [C.c_void_p, C.c_uint32]
        l.vkrh_set_gathered_mips.argtypes = [C.c_void_p, C.c_uint32]
        l.vkrh_run.argtypes = [C.c_void_p, C.c_uint32]
        l.vkrh_end_frame.argtypes = [C.c_void_p, C.c_uint32]
        l.vkrh_image.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(abi.VkrImg)]
        l.vkrh_image_layer.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(abi.VkrImg)]
        l.vkrh_pin_screen_trace.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint32]
        l.vkrh_capture.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p]
        l.vkrh_read_buffer.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        l.vkrh_load_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(SceneDraw), C.c_uint32,
                                      C.POINTER(SceneTexture), C.c_uint32]
        l.vkrh_last_tasks.argtypes = [C.c_void_p]
        l.vkrh_last_tasks.restype = C.c_char_p
        l.vkrh_last_lanes.argtypes = [C.c_void_p]
        l.vkrh_last_lanes.restype = C.c_char_p
        l.vkrh_set_async.argtypes = [C.c_void_p, C.c_uint32]
        l.vkrh_enable_task_timing.argtypes = [C.c_void_p, C.c_uint32]
        l.vkrh_enable_task_timing_only.argtypes = [C.c_void_p, C.c_char_p]
        l.vkrh_collect_task_times.argtypes = [C.c_void_p]
        l.vkrh_collect_task_times.restype = C.c_char_p
        l.vkrh_set_allocator.argtypes = [_ALLOC, _FREE, C.c_void_p]
        l.vkrh_tiled_create.argtypes = [C.POINTER(TiledConfig)]
        l.vkrh_tiled_create.restype = C.c_void_p
        l.vkrh_tiled_destroy.argtypes = [C.c_void_p]
        l.vkrh_tiled_frame.argtypes = [C.c_void_p]
        l.vkrh_tiled_frame.restype = C.c_void_p
        l.vkrh_tiled_step.argtypes = [C.c_void_p]
        l.vkrh_tiled_flush.argtypes = [C.c_void_p]
        l.vkrh_tiled_phase.argtypes = [C.c_void_p, C.c_uint32]
        l.vkrh_tiled_gather_parts.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(GatherPart), C.c_uint32, C.POINTER(C.c_uint32)]
        l.vkrh_tiled_halo_peers.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(HaloPeer), C.c_uint32, C.POINTER(C.c_uint32)]
        l.vkrh_tiled_hit_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        l.vkrh_tiled_hit_requests.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(HaloPeer), C.c_uint32, C.POINTER(C.c_uint32)]
        l.vkrh_tiled_hit_replies.argtypes = [C.c_void_p, C.POINTER(HaloPeer), C.c_uint32, C.POINTER(C.c_uint32)]
        l.vkrh_tiled_hit_finish.argtypes = [C.c_void_p]
        l.vkrh_tiled_hit_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        l.vkrh_tiled_hit_rounds.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        l.vkrh_tiled_local_first.argtypes = [C.c_void_p]
        l.vkrh_hit_capacities.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        l.vkrh_tiled_emulate_wire.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        l.vkrh_tiled_hit_errors.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        l.vkrh_tiled_time_waits.argtypes = [C.c_void_p, C.c_uint32]
        l.vkrh_tiled_wait_times.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        l.vkrh_balance_rows.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        l.vkrh_balance_rows.restype = C.c_int
        # ray-traced AO entries: typed where the loaded library exports them.  VKR_HOST_LIB may name a build of the mirror made
        # by another recipe (tests/test_reference_passes_gpu.py loads oracle/_ref/libvkr_host_refpasses.so) that predates them;
        # frames that never ask for them must still load it.  Calling one that is missing raises AttributeError.
        for name, args in (("vkrh_gtao_rt_params", [C.c_void_p, C.POINTER(abi.GtaoRtParams)]),
                           ("vkrh_gtao_directions", [C.c_void_p, C.c_uint32]),
                           ("vkrh_selftest_ray_query", [C.c_char_p, C.c_uint32]),
                           # the probe bake (same rule: typed where exported)
                           ("vkrh_bake_probes", [C.c_void_p, C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), C.c_uint32, C.c_uint32, C.c_uint32]),
                           # the shadow pass (same rule)
                           ("vkrh_set_shadow_lights", [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_uint32]),
                           ("vkrh_shadow_lights", [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
                           # image transfers (same rule)
                           ("vkrh_scene_texture_image", [C.c_void_p, C.c_uint32, C.POINTER(abi.VkrImg)]),
                           ("vkrh_create_image", [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
                           ("vkrh_transfer", [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.POINTER(C.c_float)]),
                           # deferred shading in the tiled frame (same rule)
                           ("vkrh_tiled_set_shading", [C.c_void_p, C.c_uint32]),
                           ("vkrh_tiled_shading", [C.c_void_p]),
                           # the SSAO pass (same rule)
                           ("vkrh_set_ssao_samples", [C.c_void_p, C.POINTER(C.c_float), C.c_uint32]),
                           ("vkrh_selftest_ssao", [C.c_char_p, C.c_uint32]),
                           # the tile plane regression (same rule)
                           ("vkrh_selftest_tile_regression", [C.c_char_p, C.c_uint32]),
                           # the backbuffer texdraw pass (same rule)
                           ("vkrh_set_backbuffer", [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]),
                           ("vkrh_selftest_texdraw", [C.c_char_p, C.c_uint32]),
                           # the shadow mask (same rule)
                           ("vkrh_set_shadow_mask", [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
                           # the ray-traced shadow mask (same rule)
                           ("vkrh_set_shadow_rays", [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_float, C.c_float]),
                           # area lights in the ray-traced shadow mask (same rule)
                           ("vkrh_set_shadow_area_lights", [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32]),
                           # the edge-aware filter of the shadow mask (same rule)
                           ("vkrh_set_shadow_mask_filter", [C.c_void_p, C.c_uint32, C.c_float, C.c_float]),
                           # the temporal accumulation of the shadow mask (same rule)
                           ("vkrh_set_shadow_mask_accumulate", [C.c_void_p, C.c_uint32, C.c_float, C.c_uint32]),
                           # the ray-traced reflections (same rule)
                           ("vkrh_set_reflection_rays", [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32]),
                           # alpha cutouts in the rays of the two ray-traced stages (same rule)
                           ("vkrh_set_ray_cutouts", [C.c_void_p, C.c_uint32, C.c_uint32]),
                           # lit hits in the ray-traced reflections, and the scene's normal table as the device holds it (same rule)
                           ("vkrh_set_reflection_lights", [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                           C.c_float, C.c_float]),
                           ("vkrh_scene_hit_normals", [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
                           # moving draws: the raster table and a refit of the ray-query structure (same rule)
                           ("vkrh_set_draw_transforms", [C.c_void_p, C.POINTER(C.c_float), C.c_uint32]),
                           # the matrices derived from the camera (same rule)
                           ("vkrh_camera_matrices", [C.c_void_p, C.POINTER(C.c_float)]),
                           # the first refusal of every program of the table (same rule)
                           ("vkrh_selftest_programs", [C.c_char_p, C.c_uint32])):
            if hasattr(l, name):
                getattr(l, name).argtypes = args
        _lib = l
    return _lib


def hit_capacities(counts, world, percent=125):
    """frame.hpp vkrh_hit_capacities: the segment room of the next frame's hit round from this frame's world x world counts"""
    flat = (C.c_uint32 * len(counts))(*counts)
    out = (C.c_uint32 * len(counts))()
    if lib().vkrh_hit_capacities(flat, world, percent, out) != 0:
        raise RuntimeError("host error: " + lib().vkrh_last_error().decode())
    return list(out)


def balance_rows(ms, bounds, align=16, min_rows=64):
    """frame.hpp vkrh_balance_rows: new strip bounds from the compute time each rank measured with `bounds`."""
    world = len(ms)
    assert len(bounds) == world + 1
    out = (C.c_uint32 * (world + 1))()
    rc = lib().vkrh_balance_rows((C.c_float * world)(*[float(v) for v in ms]), (C.c_uint32 * (world + 1))(*bounds), world, align, min_rows, out)
    if rc != 0:
        raise RuntimeError("vkrh_balance_rows: " + lib().vkrh_last_error().decode())
    return list(out)


class TorchAllocator:
    """Backs graph images with torch uint8 tensors (keeps them alive until the graph frees them)."""

    def __init__(self, device):
        import torch

        self.torch = torch
        self.device = device
        self.live = {}
        self._alloc = _ALLOC(self.alloc)
        self._free = _FREE(self.free)

    def alloc(self, nbytes, _user):
        t = self.torch.zeros((int(nbytes),), dtype=self.torch.uint8, device=self.device)
        self.live[t.data_ptr()] = t
        return t.data_ptr()

    def free(self, ptr, _user):
        self.live.pop(ptr, None)

    def install(self):
        lib().vkrh_set_allocator(self._alloc, self._free, None)

    def tensor_at(self, ptr):
        """(tensor, byte offset) of the allocation containing `ptr`."""
        for base, t in self.live.items():
            if base <= ptr < base + t.numel():
                return t, ptr - base
        raise KeyError(hex(ptr))


def _mat16(m):
    a = (C.c_float * 16)()
    flat = np.asarray(m, dtype=np.float32).T.reshape(-1)
    for i in range(16):
        a[i] = float(flat[i])
    return a


class HostFrame:
    def __init__(self, setup, device="cuda", window=None, tiled=False, stream=None, native_tiled=None):
        """native_tiled: None, or dict(rank, world, halo, gathered_mips, force_tiled, comm) — the frame then lives inside
        the C++ tiled frame (frame.hpp vkrh_tiled_*: strips, exchanges issued from C++ on their own stream); `window` is
        derived there."""
        import torch

        self.setup = setup
        W, H = setup.width, setup.height
        ox, oy, ww, wh = window or (0, 0, W, H)
        self.allocator = TorchAllocator(device)
        self.allocator.install()
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        self.tiled_handle = None
        self.albedo_by_gather, self.gather_mode = True, 1  # only the C++ tiled frame has the request / reply exchanges
        if native_tiled is not None:
            nt = native_tiled
            comm = nt.get("comm")
            bounds = nt.get("row_bounds")  # world + 1 strip boundaries (rows), or None for equal strips
            arr = (C.c_uint32 * len(bounds))(*bounds) if bounds is not None else None
            # 0 (default): hit colours and hit normals by request / reply; 1: albedo and normals all-gathered (round 2);
            # 2: albedo by request, normals gathered
            mode = nt.get("gather_mode")
            if mode is None:
                mode = int(os.environ.get("VKR_TILED_GATHER_MODE", "1" if os.environ.get("VKR_TILED_ALBEDO_GATHER") == "1" else "0"))
            self.gather_mode = int(mode)
            self.albedo_by_gather = self.gather_mode == 1
            tc = TiledConfig(W, H, nt["rank"], nt["world"], nt["halo"], nt["gathered_mips"], 1 if nt.get("force_tiled") else 0, self.gather_mode,
                             C.c_void_p(stream), C.c_void_p(comm.handle if comm is not None else None),
                             C.cast(arr, C.POINTER(C.c_uint32)) if arr is not None else None)
            self.comm = comm  # keep the communicator alive as long as the frame
            self.tiled_handle = lib().vkrh_tiled_create(C.byref(tc))
            if not self.tiled_handle:
                raise RuntimeError("vkrh_tiled_create failed: " + lib().vkrh_last_error().decode())
            self.h = lib().vkrh_tiled_frame(self.tiled_handle)
        else:
            cfg = HostConfig(W, H, ox, oy, ww, wh, 1 if tiled else 0, C.c_void_p(stream))
            self.h = lib().vkrh_create(C.byref(cfg))
            if not self.h:
                raise RuntimeError("vkrh_create failed: " + lib().vkrh_last_error().decode())
        cam = HostCamera()
        cam.view, cam.prev_view, cam.projection = _mat16(setup.view), _mat16(setup.prev_view), _mat16(setup.proj)
        cam.fovy, cam.aspect, cam.znear, cam.zfar = [float(v) for v in setup.fazz]
        self._check(lib().vkrh_set_camera(self.h, C.byref(cam)))
        self.pin_randoms()
        self._check(lib().vkrh_set_gtao_mode(self.h, setup.use_mis, 0))
        self._check(lib().vkrh_set_synth_flags(self.h, getattr(setup, "synth_flags", 0)))

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError("host frame error: " + lib().vkrh_last_error().decode())

    def pin_randoms(self, angle_jitter=0.0, gtao_frame_count=0, ssr_counter=0):
        """angle_offset = table[frame_count % 12]/360 + jitter (gtao.cpp:109-111); SURVEY 8(d) pins 60/360 + 0."""
        self._check(lib().vkrh_pin_randoms(self.h, angle_jitter, gtao_frame_count, ssr_counter))

    def set_camera(self, view, prev_view, proj, fazz):
        cam = HostCamera()
        cam.view, cam.prev_view, cam.projection = _mat16(view), _mat16(prev_view), _mat16(proj)
        cam.fovy, cam.aspect, cam.znear, cam.zfar = [float(v) for v in fazz]
        self._check(lib().vkrh_set_camera(self.h, C.byref(cam)))

    def load_scene(self, sc, device_mips=False):
        """scene.Scene -> scene::CompiledScene + SceneRenderer inside the frame (main.cpp:250-259).  device_mips: only level 0 of
        every texture is handed over (TEXTURE_GEN_MIPS); the frame builds the chain on the device, as scene/images.cpp does."""
        verts = np.ascontiguousarray(sc.vertices, dtype=np.float32)
        idx = np.ascontiguousarray(sc.indices, dtype=np.uint32)
        draws = (SceneDraw * max(1, len(sc.draws)))()
        for i, d in enumerate(sc.draws):
            m = sc.transforms[d["transform"]][0]
            draws[i] = SceneDraw(_mat16(m), d["vertex_offset"], d["index_offset"], d["index_count"], d["albedo"], d["mr"], 1 if d["flags"] else 0)
        tex = (SceneTexture * max(1, len(sc.textures)))()
        keep = []
        for i, levels in enumerate(sc.textures):
            h, w = levels[0].shape[:2]
            tex[i].width, tex[i].height, tex[i].mip_levels = w, h, 1 if device_mips else len(levels)
            tex[i].flags = TEXTURE_GEN_MIPS if device_mips else 0
            for m, lv in enumerate(levels[:1] if device_mips else levels):
                a = np.ascontiguousarray(lv)
                keep.append(a)
                tex[i].levels[m] = a.ctypes.data
        self._check(lib().vkrh_load_scene(self.h, C.c_void_p(verts.ctypes.data), len(verts), C.c_void_p(idx.ctypes.data), len(idx),
                                          draws, len(sc.draws), tex, len(sc.textures)))

    def set_draw_transforms(self, models):
        """vkrh_set_draw_transforms: one 4 x 4 model matrix (maths convention, as scene.Scene keeps them) per draw of the scene
        given to load_scene, in its order — for a scene.Scene `sc`: [sc.transforms[d["transform"]][0] for d in sc.draws].  From the
        next run() the raster, shadow-map and cube stages and every ray-traced stage see that pose (the ray-query structure is
        refitted on the frame's stream, not rebuilt)."""
        flat = np.ascontiguousarray(np.stack([np.asarray(m, dtype=np.float32).T for m in models]).reshape(-1), dtype=np.float32) if len(models) else np.zeros(0, np.float32)
        self._check(lib().vkrh_set_draw_transforms(self.h, flat.ctypes.data_as(C.POINTER(C.c_float)), len(models)))

    def scene_texture(self, index):
        """vkrh_scene_texture_image: descriptor (every level) of texture `index` of the loaded scene"""
        d = abi.VkrImg()
        self._check(lib().vkrh_scene_texture_image(self.h, int(index), C.byref(d)))
        return d

    def download_desc(self, d):
        """host ImageBuf with the bytes of a device image described by `d` (a descriptor of one of the frame's allocations)"""
        from .images import ImageBuf, mip_extent

        buf = ImageBuf(d.format, d.width, d.height, d.mip_count)
        t, off = self.allocator.tensor_at(d.base)
        for i in range(d.mip_count):
            assert buf.pitch[i] == d.pitch_bytes[i], "layout rules diverged"
            n = buf.pitch[i] * mip_extent(d.height, i)
            buf.host[buf.offset[i]: buf.offset[i] + n] = t[off + d.mip_offset[i]: off + d.mip_offset[i] + n].cpu().numpy()
        return buf

    def create_image(self, name, fmt, width, height, mips=1, layers=1):
        """vkrh_create_image: an image of the caller's own in the frame's graph (fmt: abi.FMT_*), found by image() / download()"""
        self._check(lib().vkrh_create_image(self.h, name.encode(), int(fmt), int(width), int(height), int(mips), int(layers)))

    TRANSFER_GEN_MIPMAPS, TRANSFER_CLEAR_DEPTH, TRANSFER_CLEAR_COLOR, TRANSFER_BLIT = 0, 1, 2, 3

    def transfer(self, op, image, dst=None, value=None):
        """vkrh_transfer: one helper of util_passes.hpp on named images of the frame, recorded and submitted: gen_mipmaps(image),
        clear_depth(image, value), clear_color(image, value[4]), blit_image(image, dst)"""
        v = None
        if value is not None:
            vals = [float(value)] if np.isscalar(value) else [float(c) for c in value]
            v = (C.c_float * 4)(*(vals + [0.0] * (4 - len(vals))))
        self._check(lib().vkrh_transfer(self.h, int(op), image.encode(), dst.encode() if dst else None, v))

    def gtao_rt_params(self):
        """abi.GtaoRtParams that STAGE_GTAO_RT uses for the current camera (camera_to_world = inverse(view))"""
        p = abi.GtaoRtParams()
        self._check(lib().vkrh_gtao_rt_params(self.h, C.byref(p)))
        return p

    def set_gathered_mips(self, n):
        """tiled frames: how many whole-frame Hi-Z mips (image mips 1..n) arrive by all-gather; STAGE_HIZ_TAIL rebuilds the rest"""
        self._check(lib().vkrh_set_gathered_mips(self.h, n))

    def pin_screen_trace(self, angle_jitter=0.0, random_offset=0.25, frame_count=0):
        self._check(lib().vkrh_pin_screen_trace(self.h, angle_jitter, random_offset, frame_count))

    def bake_probes(self, pmin, pmax, grid_size=4, probe_size=256, cube_size=128):
        """vkrh_bake_probes: a grid_size x grid_size grid of octahedral probes from the loaded scene, in x and z between pmin and
        pmax at pmin's y.  Leaves images "probe_color" / "probe_depth" (download(name, layer)) for STAGE_PROBE_TRACE."""
        lo, hi = (C.c_float * 3)(*[float(v) for v in pmin]), (C.c_float * 3)(*[float(v) for v in pmax])
        self._check(lib().vkrh_bake_probes(self.h, C.byref(lo), C.byref(hi), int(grid_size), int(probe_size), int(cube_size)))

    def set_shadow_lights(self, mvps, size=0):
        """vkrh_set_shadow_lights: 1..4 light matrices (4x4, maths convention, e.g. camera.shadow_mvp(...)) for STAGE_SHADOW, light l
        -> layer l of image "shadows" (download("shadows", l)); size: edge of the map, 0 keeps 1024."""
        flat = (C.c_float * (16 * len(mvps)))()
        for i, m in enumerate(mvps):
            flat[16 * i: 16 * i + 16] = list(_mat16(m))
        self._check(lib().vkrh_set_shadow_lights(self.h, flat, len(mvps), int(size)))

    def set_shadow_mask(self, bias=0, radius=1, apply=0):
        """vkrh_set_shadow_mask: the lookup of STAGE_SHADOW_MASK: bias in D24 codes, radius 0, 1, 2 (a box of 1, 9, 25 taps);
        apply != 0: a STAGE_SHADING of a run that also has STAGE_SHADOW_MASK multiplies its direct term by light 0's channel
        (program defered_shading_shadowed); 0 (the default): the shading is what it is without the mask."""
        self._check(lib().vkrh_set_shadow_mask(self.h, int(bias), int(radius), 1 if apply else 0))

    def set_shadow_rays(self, lights, normal_offset=abi.SHADOW_RT_NORMAL_OFFSET, tmin=abi.SHADOW_RT_TMIN):
        """vkrh_set_shadow_rays: the rays of STAGE_SHADOW_MASK_RT: 1..4 lights of (x, y, z, w), w == 1 a point light at xyz, w == 0
        a directional light whose xyz is the vector from the surface towards the light (its length is the ray's reach); the origin
        is the surface point moved by normal_offset along the normal, the segment is t in [tmin, 1]."""
        flat = (C.c_float * max(4, 4 * len(lights)))()
        for i, v in enumerate(lights):
            flat[4 * i: 4 * i + 4] = [float(x) for x in v]
        self._check(lib().vkrh_set_shadow_rays(self.h, flat, len(lights), float(normal_offset), float(tmin)))

    def set_shadow_area_lights(self, radii, sample_count=16, pattern_side=4):
        """vkrh_set_shadow_area_lights: the sizes of the lights of STAGE_SHADOW_MASK_RT: one radius (world units) per light of
        set_shadow_rays, sample_count (1..64) rays per pixel and light with a radius, a tile of pattern_side^2 (1, 2 or 4) sample
        patterns from abi.shadow_disk_samples.  With any radius above 0 the stage records vkr_shadow_mask_rt_soft (task
        ShadowMaskRTSoft) and a channel holds 255 * visible / sample_count rounded half up; every radius 0 (the default) is the hard
        stage.  Not on a tiled frame."""
        flat = (C.c_float * max(4, len(radii)))(*[float(r) for r in radii])
        self._check(lib().vkrh_set_shadow_area_lights(self.h, flat, len(radii), int(sample_count), int(pattern_side)))

    def set_shadow_mask_filter(self, reach, normal_min_dot=abi.SHADOW_FILTER_NORMAL_MIN_DOT, plane_tolerance=abi.SHADOW_FILTER_PLANE_TOLERANCE):
        """vkrh_set_shadow_mask_filter: reach 1..4: STAGE_SHADOW_MASK and STAGE_SHADOW_MASK_RT record vkr_shadow_mask_filter (task
        ShadowMaskFilter) right after the mask, from image "shadow_mask" into image "shadow_mask_filtered", which the shadowed
        shading then reads; reach is the pattern_side of the area lights it reconstructs.  reach 0 (the default): off.  Not on a
        tiled frame."""
        self._check(lib().vkrh_set_shadow_mask_filter(self.h, int(reach), float(normal_min_dot), float(plane_tolerance)))

    def set_shadow_mask_accumulate(self, max_count=abi.SHADOW_ACCUM_MAX_COUNT, plane_tolerance=abi.SHADOW_FILTER_PLANE_TOLERANCE,
                                   pattern_frames=abi.SHADOW_ACCUM_PATTERN_FRAMES):
        """vkrh_set_shadow_mask_accumulate: max_count 1..255: STAGE_SHADOW_MASK and STAGE_SHADOW_MASK_RT record
        vkr_shadow_mask_accumulate (task ShadowMaskAccumulate) right after the mask and before the filter, from image "shadow_mask"
        and the histories "shadow_history" / "shadow_history_count" into "shadow_history_out" / "shadow_history_count_out" and
        "shadow_mask_accumulated"; end_frame swaps the history pairs; a traced soft mask cycles over pattern_frames sample
        tables.  max_count 0: off (the frame's default).  Not on a tiled frame."""
        self._check(lib().vkrh_set_shadow_mask_accumulate(self.h, int(max_count), float(plane_tolerance), int(pattern_frames)))

    def set_reflection_rays(self, fill_misses=False, normal_offset=abi.SHADOW_RT_NORMAL_OFFSET, tmin=abi.SHADOW_RT_TMIN, max_distance=None,
                            texture_lod=0):
        """vkrh_set_reflection_rays: the rays of STAGE_REFLECTIONS_RT: fill_misses False traces every pixel (ReflectionsRT -> blur),
        True only those whose screen-space ray is invalid (trace -> filter -> ReflectionsRT -> blur); the origin is the surface point
        moved by normal_offset along the normal, the ray runs t in [tmin, max_distance] along the unit mirror direction
        (max_distance None: the camera's zfar), a hit samples level texture_lod of its albedo texture."""
        self._check(lib().vkrh_set_reflection_rays(self.h, 1 if fill_misses else 0, float(normal_offset), float(tmin),
                                                   0.0 if max_distance is None else float(max_distance), int(texture_lod)))

    def set_reflection_lights(self, lights=None, colours=None, ambient=None, shadow_offset=abi.REFLECT_SHADOW_OFFSET,
                              shadow_tmin=abi.REFLECT_SHADOW_TMIN):
        """vkrh_set_reflection_lights: from now on STAGE_REFLECTIONS_RT lights and shadows the hit of the mirror ray (task
        "ReflectionsRTLit"): lights 0..4 of (x, y, z, w) in the convention of set_shadow_rays, colours one rgb per light, ambient an
        rgb.  With no argument at all: the default light, the direct diffuse term of defered_shading.  Composes with
        set_reflection_rays, set_ray_cutouts and set_draw_transforms.  Not on a tiled frame."""
        if lights is None and colours is None and ambient is None:
            self._check(lib().vkrh_set_reflection_lights(self.h, 1, None, None, None, float(shadow_offset), float(shadow_tmin)))
            return
        lights, colours = list(lights or []), list(colours or [])
        if len(colours) != len(lights) or ambient is None:
            raise RuntimeError(f"set_reflection_lights: {len(lights)} lights, {len(colours)} colours and ambient {ambient}: one colour per light and an ambient")
        fl = (C.c_float * max(1, 4 * len(lights)))(*[float(v[k]) for v in lights for k in range(4)])
        fc = (C.c_float * max(1, 3 * len(lights)))(*[float(v[k]) for v in colours for k in range(3)])
        fa = (C.c_float * 3)(*[float(ambient[k]) for k in range(3)])
        self._check(lib().vkrh_set_reflection_lights(self.h, len(lights), fl, fc, fa, float(shadow_offset), float(shadow_tmin)))

    def hit_normals(self):
        """vkrh_scene_hit_normals: the loaded scene's normal table as the device holds it now, a numpy array of abi.hit_normal_dtype()"""
        n = C.c_uint32(0)
        self._check(lib().vkrh_scene_hit_normals(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, abi.hit_normal_dtype())
        if n.value:
            self._check(lib().vkrh_scene_hit_normals(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def set_ray_cutouts(self, enable=True, alpha_lod=0):
        """vkrh_set_ray_cutouts: whether the rays of STAGE_SHADOW_MASK_RT and STAGE_REFLECTIONS_RT pass through triangles whose albedo
        alpha at the hit (level alpha_lod of the texture) is 0, as the rasteriser discards such fragments.  Default: off.
        STAGE_GTAO_RT stays opaque.  Not on a tiled frame."""
        self._check(lib().vkrh_set_ray_cutouts(self.h, 1 if enable else 0, int(alpha_lod)))

    def set_ssao_samples(self, samples, std140=0):
        """vkrh_set_ssao_samples: pins the 16 samples ([16, 3]) of STAGE_SSAO and their packing in the uniform block: std140 = 0
        the reference's (the shader sees samples 12..15 as zero and the others shifted), 1 one 16-byte slot per sample."""
        s = np.ascontiguousarray(np.asarray(samples, dtype=np.float32)[:, :3]).reshape(-1)
        if s.size != 48:
            raise RuntimeError(f"set_ssao_samples: {s.size} floats, expected 16 x 3")
        self._check(lib().vkrh_set_ssao_samples(self.h, (C.c_float * 48)(*[float(v) for v in s]), int(std140)))

    def set_backbuffer(self, source=None, flags=0, width=0, height=0):
        """vkrh_set_backbuffer: what STAGE_BACKBUFFER draws: `source` an image name (None: the TAA output), `flags` the DrawTex
        bits (abi.TEXDRAW_SHOW_*), width x height the backbuffer's extent (0, 0: the frame's)."""
        name = source.encode() if source else None
        self._check(lib().vkrh_set_backbuffer(self.h, name, int(flags), int(width), int(height)))

    def shadow_lights(self):
        """vkrh_shadow_lights: the light matrices in use as 4x4 float32 arrays (maths convention)"""
        out, n = (C.c_float * 64)(), C.c_uint32(0)
        self._check(lib().vkrh_shadow_lights(self.h, out, C.byref(n)))
        return [np.array(out[16 * i: 16 * i + 16], dtype=np.float32).reshape(4, 4).T.copy() for i in range(n.value)]

    def run(self, mask):
        self._check(lib().vkrh_run(self.h, mask))

    def end_frame(self, swap_depth=False):
        self._check(lib().vkrh_end_frame(self.h, 1 if swap_depth else 0))

    def image(self, name, base_mip=0, mip_count=0):
        d = abi.VkrImg()
        self._check(lib().vkrh_image(self.h, name.encode(), base_mip, mip_count, C.byref(d)))
        return d

    CAPTURE_DEPTH_CSV, CAPTURE_DEPTH_PNG, CAPTURE_RGBA_PNG, CAPTURE_FINAL_FRAME = 0, 1, 2, 3

    def capture(self, name, path, kind, mip=0):
        """ReadBackSystem + the capture writers of main.cpp:118-176."""
        self._check(lib().vkrh_capture(self.h, name.encode(), mip, kind, str(path).encode()))

    def capture_final(self, path, name="taa_target"):
        """The final frame as a PNG (main.cpp:392-396): `name` is blitted into the RGBA8_SRGB image "readback" on the device, which
        is read back and written with the RGBA PNG writer.  download("readback") shows the blitted image afterwards."""
        self.capture(name, path, self.CAPTURE_FINAL_FRAME)

    def read_buffer(self, name, max_bytes=1 << 24):
        """int32 contents of a named device buffer of the SSR pass (tile lists, indirect arguments)."""
        dst = np.zeros(max_bytes // 4, dtype=np.int32)
        n = C.c_uint64(0)
        self._check(lib().vkrh_read_buffer(self.h, name.encode(), C.c_void_p(dst.ctypes.data), dst.nbytes, C.byref(n)))
        return dst[: n.value // 4]

    def enable_task_timing(self, on=True, only=None):
        """HIP events around every task of each run() — or, with `only`, around the task of that name alone: an event
        pair costs ~3.5 us of queue time, so timing all nine passes slows a 1 ms frame by 7 %."""
        if on and only:
            self._check(lib().vkrh_enable_task_timing_only(self.h, only.encode()))
        else:
            self._check(lib().vkrh_enable_task_timing(self.h, 1 if on else 0))

    def collect_task_times(self):
        """{task name: (total_ms, launches)} measured with HIP events on the frame's stream since the last call."""
        txt = lib().vkrh_collect_task_times(self.h)
        if txt is None:
            raise RuntimeError("host frame error: " + lib().vkrh_last_error().decode())
        out = {}
        for line in txt.decode().splitlines():
            name, ms, n = line.rsplit(" ", 2)
            out[name] = (float(ms), int(n))
        return out

    def last_tasks(self):
        return lib().vkrh_last_tasks(self.h).decode().split()

    def last_lanes(self):
        """stream lane (0 = the frame's stream) of each task of the last run()"""
        return [int(v) for v in lib().vkrh_last_lanes(self.h).decode().split()]

    def set_async(self, on):
        """False (default): one in-order stream.  True: independent passes of one run() overlap on up to three streams."""
        self._check(lib().vkrh_set_async(self.h, 1 if on else 0))

    def download(self, name, layer=None):
        """Copies the named image (or one layer of an array image) into a host ImageBuf with the same layout rules (tests)."""
        from .images import ImageBuf

        if layer is None:
            d = self.image(name)
        else:
            d = abi.VkrImg()
            self._check(lib().vkrh_image_layer(self.h, name.encode(), layer, C.byref(d)))
        buf = ImageBuf(d.format, d.width, d.height, d.mip_count, full=(d.full_width, d.full_height), origin=(d.origin_x, d.origin_y))
        t, off = self.allocator.tensor_at(d.base)
        if layer is not None and d.mip_count > 1:
            # a layer of a mipped array: its mips lie an array's mip apart (arrays are mip-major), copied level by level
            from .images import mip_extent

            for i in range(d.mip_count):
                assert buf.pitch[i] == d.pitch_bytes[i], "layout rules diverged"
                n = buf.pitch[i] * mip_extent(d.height, i)
                buf.host[buf.offset[i]: buf.offset[i] + n] = t[off + d.mip_offset[i]: off + d.mip_offset[i] + n].cpu().numpy()
            return buf
        for i in range(d.mip_count):
            assert buf.pitch[i] == d.pitch_bytes[i] and buf.offset[i] == d.mip_offset[i], "layout rules diverged"
        buf.upload(t[off: off + buf.nbytes].cpu().numpy())
        return buf

    def upload(self, name, host_bytes):
        import torch

        d = self.image(name)
        t, off = self.allocator.tensor_at(d.base)
        src = torch.from_numpy(np.ascontiguousarray(host_bytes, dtype=np.uint8).reshape(-1))
        t[off: off + src.numel()].copy_(src)

    # ---- the C++ tiled frame (native_tiled) ---------------------------------------------------------------
    def tiled_step(self):
        self._check(lib().vkrh_tiled_step(self.tiled_handle))

    def tiled_flush(self):
        self._check(lib().vkrh_tiled_flush(self.tiled_handle))

    def tiled_phase(self, p):
        self._check(lib().vkrh_tiled_phase(self.tiled_handle, p))

    def tiled_time_waits(self, on=True):
        self._check(lib().vkrh_tiled_time_waits(self.tiled_handle, 1 if on else 0))

    def tiled_wait_times(self):
        """{exchange: ms the compute stream stood still for it since the last call} (frame.hpp vkrh_tiled_wait_times)"""
        out = (C.c_float * 5)()
        self._check(lib().vkrh_tiled_wait_times(self.tiled_handle, out))
        return dict(zip(("hiz_gather", "albedo_gather", "taa_halo", "ao_halo", "ssr_halo"), [float(v) for v in out]))

    def tiled_gather_parts(self, which):
        """[(send address, recv address, bytes)] of all-gather `which` (0: Hi-Z mips + normals, 1: albedo)"""
        out = (GatherPart * 8)()
        n = C.c_uint32(0)
        self._check(lib().vkrh_tiled_gather_parts(self.tiled_handle, which, out, 8, C.byref(n)))
        return [(out[i].send, out[i].recv, out[i].bytes) for i in range(n.value)]

    def tiled_halo_peers(self, surface):
        """[(peer rank, send address, recv address, bytes)] of halo refresh `surface` (0: TAA, 1: AO, 2: SSR)"""
        out = (HaloPeer * 2)()
        n = C.c_uint32(0)
        self._check(lib().vkrh_tiled_halo_peers(self.tiled_handle, surface, out, 2, C.byref(n)))
        return [(out[i].peer, out[i].send, out[i].recv, out[i].send_bytes) for i in range(n.value)]

    # the hit-colour request / reply of the C++ tiled frame, step by step (lockstep harness; frame.hpp)
    def tiled_hit_counts(self, world):
        row = (C.c_uint32 * world)()
        self._check(lib().vkrh_tiled_hit_counts(self.tiled_handle, row))
        return list(row)

    def _peer_list(self, out, n):
        return [(out[i].peer, out[i].send, out[i].send_bytes, out[i].recv, out[i].recv_bytes) for i in range(n.value)]

    def tiled_hit_requests(self, matrix):
        """matrix: world x world counts, row-major [requester][owner] -> [(peer, send address, send bytes, recv address, recv bytes)]"""
        flat = (C.c_uint32 * len(matrix))(*matrix)
        out, n = (HaloPeer * 16)(), C.c_uint32(0)
        self._check(lib().vkrh_tiled_hit_requests(self.tiled_handle, flat, out, 16, C.byref(n)))
        return self._peer_list(out, n)

    def tiled_hit_replies(self):
        out, n = (HaloPeer * 16)(), C.c_uint32(0)
        self._check(lib().vkrh_tiled_hit_replies(self.tiled_handle, out, 16, C.byref(n)))
        return self._peer_list(out, n)

    def tiled_hit_finish(self):
        self._check(lib().vkrh_tiled_hit_finish(self.tiled_handle))

    def tiled_hit_errors(self):
        e = C.c_uint32(0)
        self._check(lib().vkrh_tiled_hit_errors(self.tiled_handle, C.byref(e)))
        return int(e.value)

    def tiled_hit_rounds(self):
        """(rounds enqueued on the previous frame's capacities, exact rounds after a host round trip, rounds repeated after an overflow)"""
        r = (C.c_uint64 * 3)()
        self._check(lib().vkrh_tiled_hit_rounds(self.tiled_handle, r))
        return int(r[0]), int(r[1]), int(r[2])

    def tiled_pipelined(self):
        lib().vkrh_tiled_pipelined.argtypes = [C.c_void_p]
        return bool(lib().vkrh_tiled_pipelined(self.tiled_handle))

    def tiled_local_first(self):
        return bool(lib().vkrh_tiled_local_first(self.tiled_handle))

    def tiled_set_shading(self, on=True):
        """frame.hpp vkrh_tiled_set_shading: deferred shading at the end of the tiled frame, the TAA resolving color_out.  Needs
        STAGE_BRDF_LUT to have run; refused while a halo refresh is in flight (call before the first frame or after tiled_flush)"""
        self._check(lib().vkrh_tiled_set_shading(self.tiled_handle, 1 if on else 0))

    def tiled_shading(self):
        on = lib().vkrh_tiled_shading(self.tiled_handle)
        if on < 0:
            self._check(1)
        return bool(on)

    def tiled_emulate_wire(self, comm_handle, counts):
        """frame.hpp vkrh_tiled_emulate_wire: the harness-driven frame goes on natively on an emulated communicator"""
        flat = (C.c_uint32 * len(counts))(*counts) if counts is not None else None
        self._check(lib().vkrh_tiled_emulate_wire(self.tiled_handle, comm_handle, flat))

    def tiled_hit_bytes(self):
        b = C.c_uint64(0)
        self._check(lib().vkrh_tiled_hit_bytes(self.tiled_handle, C.byref(b)))
        return int(b.value)

    def close(self):
        if self.tiled_handle:
            lib().vkrh_tiled_destroy(self.tiled_handle)
            self.tiled_handle, self.h = None, None
        if self.h:
            lib().vkrh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
