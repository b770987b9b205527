"""ctypes mirror of include/vkr_postfx.h (the C-ABI of the HIP hot path).

Struct layouts must stay byte-identical to the header; tests/test_abi.py checks the
sizes against values the shared library reports and that every declared symbol is
exported.  Nothing here computes anything: it only declares types and loads libraries.
"""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# VKR_POSTFX_LIB: development only (tools/blur_timeline.py loads an instrumented build of the same sources)
PRODUCT_LIB = os.environ.get("VKR_POSTFX_LIB") or os.path.join(ROOT, "vk-renderer_amd", "csrc", "libvkr_postfx.so")
# VKR_HOST_LIB: tests only (tests/test_reference_passes_gpu.py loads the mirror built around the reference's own pass sources)
HOST_LIB = os.environ.get("VKR_HOST_LIB") or os.path.join(ROOT, "vk-renderer_amd", "host", "libvkr_host.so")

VKR_MAX_MIPS = 16
HALTON_SEQ_SIZE = 128

# vkr_format
FMT_D24_UNORM_S8 = 1
FMT_RG16_UNORM = 2
FMT_RG16_SFLOAT = 3
FMT_RGBA8_SRGB = 4
FMT_RGBA8_UNORM = 5
FMT_RGBA16_UNORM = 6
FMT_RGBA16_SFLOAT = 7
FMT_R16_SFLOAT = 8
FMT_R32_SFLOAT = 9
FMT_R8_UNORM = 10
FMT_RGBA32_SFLOAT = 11
FMT_R16_UNORM = 12
FORMAT_BYTES = {1: 4, 2: 4, 3: 4, 4: 4, 5: 4, 6: 8, 7: 8, 8: 2, 9: 4, 10: 1, 11: 16, 12: 2}

NORMALIZE_REFLECTIONS = 1
ACCUMULATE_REFLECTIONS = 2
BILATERAL_FILTER = 4
SYNTH_DEPTH_ONLY = 1
SYNTH_TEXTURED_ROUGHNESS = 2


class VkrImg(C.Structure):
    _fields_ = [
        ("base", C.c_void_p),
        ("format", C.c_uint32),
        ("mip_count", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("full_width", C.c_uint32),
        ("full_height", C.c_uint32),
        ("origin_x", C.c_int32),
        ("origin_y", C.c_int32),
        ("pitch_bytes", C.c_uint32 * VKR_MAX_MIPS),
        ("mip_offset", C.c_uint64 * VKR_MAX_MIPS),
    ]


class Mat4(C.Structure):
    _fields_ = [("m", C.c_float * 16)]

    @staticmethod
    def from_np(a):
        """a: 4x4 numpy array in maths (row, col) convention -> column-major storage."""
        import numpy as np

        m = Mat4()
        flat = np.asarray(a, dtype=np.float32).T.reshape(-1)
        for i in range(16):
            m.m[i] = float(flat[i])
        return m


class GtaoParams(C.Structure):
    _fields_ = [("normal_mat", Mat4), ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float)]


class GtaoPush(C.Structure):
    _fields_ = [("angle_offset", C.c_float), ("weight_ratio", C.c_float), ("use_mis", C.c_uint32),
                ("two_directions", C.c_uint32), ("reflections_only", C.c_uint32)]


class GtaoFilterPush(C.Structure):
    _fields_ = [("znear", C.c_float), ("zfar", C.c_float)]


class GtaoAccumParams(C.Structure):
    _fields_ = [("inverse_camera", Mat4), ("prev_inverse_camera", Mat4), ("mvp", Mat4),
                ("fovy_aspect_znear_zfar", C.c_float * 4)]


class GtaoAccumPush(C.Structure):
    _fields_ = [("clear_history", C.c_uint32)]


class TraceParams(C.Structure):
    _fields_ = [("normal_mat", Mat4), ("frame_random", C.c_uint32), ("fovy", C.c_float), ("aspect", C.c_float),
                ("znear", C.c_float), ("zfar", C.c_float)]


class TracePush(C.Structure):
    _fields_ = [("max_roughness", C.c_float)]


class FilterPush(C.Structure):
    _fields_ = [("render_flags", C.c_uint32)]


class BlurPush(C.Structure):
    _fields_ = [("max_roughness", C.c_float), ("accumulate", C.c_uint32), ("disable_blur", C.c_uint32)]


class ReprojectParams(C.Structure):
    _fields_ = [("inverse_camera", Mat4), ("prev_inverse_camera", Mat4), ("fovy_aspect_znear_zfar", C.c_float * 4)]


class SsrParams(C.Structure):
    _fields_ = [("normal_mat", Mat4), ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float)]


class ShadingParams(C.Structure):
    _fields_ = [("inverse_camera", Mat4), ("camera", Mat4), ("shadow_mvp", Mat4), ("fovy", C.c_float), ("aspect", C.c_float),
                ("znear", C.c_float), ("zfar", C.c_float)]


class ShadingPush(C.Structure):
    _fields_ = [("min_max_roughness", C.c_float * 2), ("show_ao", C.c_uint32)]


class ClassificationPush(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("max_roughness", C.c_float), ("glossy_value", C.c_float)]


class TraceIndirectPush(C.Structure):
    _fields_ = [("reflection_type", C.c_uint32), ("max_roughness", C.c_float)]


class GtaoGfxPush(C.Structure):
    _fields_ = [("angle_offset", C.c_float)]


class GtaoReprojection(C.Structure):
    _fields_ = [("camera_to_prev_frame", Mat4), ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float)]


class DeinterleavePush(C.Structure):
    _fields_ = [("pattern_step", C.c_int32)]


class GtaoDeinterleavedPush(C.Structure):
    _fields_ = [("pattern_n", C.c_int32), ("layer", C.c_uint32), ("angle_offset", C.c_float)]


class ScreenTraceParams(C.Structure):
    _fields_ = [("normal_mat", Mat4), ("random_offset", C.c_float), ("angle_offset", C.c_float), ("fovy", C.c_float),
                ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float)]


class ScreenTraceFilterPush(C.Structure):
    _fields_ = [("znear", C.c_float), ("zfar", C.c_float)]


class ScreenTraceAccumPush(C.Structure):
    _fields_ = [("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float)]


class RasterTransform(C.Structure):
    _fields_ = [("model", Mat4), ("normal", Mat4)]


class RasterDraw(C.Structure):
    _fields_ = [("transform_index", C.c_uint32), ("albedo_index", C.c_uint32), ("mr_index", C.c_uint32), ("flags", C.c_uint32),
                ("index_offset", C.c_uint32), ("index_count", C.c_uint32), ("vertex_offset", C.c_uint32), ("reserved", C.c_uint32)]


class GbufConst(C.Structure):
    _fields_ = [("view_projection", Mat4), ("prev_view_projection", Mat4), ("jitter", C.c_float * 4),
                ("fovy_aspect_znear_zfar", C.c_float * 4)]


class RasterScene(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("vertex_count", C.c_uint32), ("indices", C.c_void_p), ("index_count", C.c_uint32),
                ("transforms", C.c_void_p), ("transform_count", C.c_uint32), ("draws", C.c_void_p), ("draw_count", C.c_uint32),
                ("textures", C.c_void_p), ("texture_count", C.c_uint32)]


class SynthParams(C.Structure):
    _fields_ = [("camera_to_world", Mat4), ("prev_mvp", Mat4), ("mvp", Mat4), ("fovy", C.c_float), ("aspect", C.c_float),
                ("znear", C.c_float), ("zfar", C.c_float), ("seed", C.c_uint32), ("flags", C.c_uint32)]


P = C.POINTER
_IMG = P(VkrImg)


class TraceWindowPush(C.Structure):  # vkr_trace_window_push
    _fields_ = [("max_roughness", C.c_float), ("normal_row0", C.c_uint32), ("normal_row1", C.c_uint32)]


class HitSources(C.Structure):  # vkr_hit_sources
    _fields_ = [("rays", _IMG), ("albedo_width", C.c_uint32), ("albedo_height", C.c_uint32), ("window_row0", C.c_uint32),
                ("window_row1", C.c_uint32), ("pending_mask", _IMG), ("pending_data", _IMG),
                ("normal_width", C.c_uint32), ("normal_height", C.c_uint32), ("normal_row0", C.c_uint32), ("normal_row1", C.c_uint32)]


# ---- ray-traced AO: the acceleration structure (vkr_accel_*) and program gtao_rt_main ----
class AccelNode(C.Structure):  # vkr_accel_node
    _fields_ = [("lo", C.c_float * 3), ("first", C.c_uint32), ("hi", C.c_float * 3), ("count", C.c_uint32)]


class AccelTri(C.Structure):  # vkr_accel_tri
    _fields_ = [("v0", C.c_float * 3), ("index", C.c_uint32), ("e1", C.c_float * 3), ("e2", C.c_float * 3),
                ("lo", C.c_float * 3), ("hi", C.c_float * 3)]


class GtaoRtParams(C.Structure):  # vkr_gtao_rt_params == GTAORTParams
    _fields_ = [("camera_to_world", Mat4), ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float)]


class GtaoRtPush(C.Structure):  # vkr_gtao_rt_push
    _fields_ = [("rotation", C.c_float)]


# ---- octahedral probes: programs cube2oct, probe_downsample, trace_probe ----
class ProbeTraceConsts(C.Structure):  # vkr_probe_trace_consts == Constants (probe_renderer.cpp:332-341), 116 bytes
    _fields_ = [("inverse_view", Mat4), ("probe_min", C.c_float * 4), ("probe_max", C.c_float * 4), ("grid_size", C.c_uint32),
                ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float)]


# ---- image transfers: vkr_clear_image, vkr_blit_image, vkr_gen_mipmaps ----
class ClearValue(C.Structure):  # vkr_clear_value
    _fields_ = [("color", C.c_float * 4), ("depth", C.c_float), ("stencil", C.c_uint32)]


FILTER_NEAREST, FILTER_LINEAR = 0, 1


# ---- program ssao ----
class SsaoParams(C.Structure):  # vkr_ssao_params: the block as ssao/shader.frag reads it (std140), 336 bytes, samples at offset 80
    _fields_ = [("projection", Mat4), ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float),
                ("samples", (C.c_float * 4) * 16)]


# ---- program tile_regression ----
class TileRegressionPush(C.Structure):  # vkr_tile_regression_push: the push constants of advanced_ssr/regression.comp, 80 bytes
    _fields_ = [("camera_to_world", Mat4), ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float)]


# ---- program texdraw ----
class TexdrawPush(C.Structure):  # vkr_texdraw_push: the push constants of texdraw/shader.frag, 4 bytes
    _fields_ = [("flags", C.c_uint32)]


# ---- program shadow_mask ----
class ShadowMaskParams(C.Structure):  # vkr_shadow_mask_params, 352 bytes
    _fields_ = [("inverse_camera", Mat4), ("mvps", Mat4 * 4), ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float),
                ("zfar", C.c_float), ("layer_count", C.c_uint32), ("radius", C.c_uint32), ("bias", C.c_uint32), ("reserved", C.c_uint32)]


# ---- program shadow_mask_rt ----
# the defaults of the ray's offsets: the host frame's (host/frame.cpp), measured on a plane-only scene
SHADOW_RT_NORMAL_OFFSET, SHADOW_RT_TMIN = 1e-3, 0.0


class ShadowRtParams(C.Structure):  # vkr_shadow_rt_params, 160 bytes
    _fields_ = [("inverse_camera", Mat4), ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float),
                ("lights", (C.c_float * 4) * 4), ("light_count", C.c_uint32), ("normal_offset", C.c_float), ("tmin", C.c_float),
                ("reserved", C.c_uint32)]


class ShadowRtSoft(C.Structure):  # vkr_shadow_rt_soft, 40 bytes
    _fields_ = [("radius", C.c_float * 4), ("sample_count", C.c_uint32), ("pattern_side", C.c_uint32), ("samples", C.c_void_p),
                ("reserved", C.c_uint32 * 2)]


# ---- the edge-aware filter of the shadow mask ----
# the defaults of the accept test, the host frame's too (host/frame.cpp); DESIGN.md 7.13 says what they rest on
SHADOW_FILTER_NORMAL_MIN_DOT, SHADOW_FILTER_PLANE_TOLERANCE = 0.9, 0.01


class ShadowFilterParams(C.Structure):  # vkr_shadow_filter_params, 96 bytes
    _fields_ = [("inverse_camera", Mat4), ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float),
                ("reach", C.c_uint32), ("normal_min_dot", C.c_float), ("plane_tolerance", C.c_float), ("reserved", C.c_uint32)]


# ---- the temporal accumulation of the shadow mask ----
# the defaults of the frame and the chain (DESIGN.md 7.16 says what they rest on): the history weighs at most max_count - 1 frames,
# the sample patterns cycle over pattern_frames tables
SHADOW_ACCUM_MAX_COUNT, SHADOW_ACCUM_PATTERN_FRAMES = 8, 8


class ShadowAccumParams(C.Structure):  # vkr_shadow_accum_params, 160 bytes
    _fields_ = [("inverse_camera", Mat4), ("prev_inverse_camera", Mat4), ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float),
                ("zfar", C.c_float), ("max_count", C.c_uint32), ("plane_tolerance", C.c_float), ("reset", C.c_uint32), ("reserved", C.c_uint32)]


# ---- the closest-hit ray query and program reflections_rt ----
ACCEL_MISS = 0xFFFFFFFF  # vkr_accel_hit.index of a ray that hits nothing


class AccelHit(C.Structure):  # vkr_accel_hit, 16 bytes; numpy twin: accel_hit_dtype()
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("index", C.c_uint32)]


class HitAttrib(C.Structure):  # vkr_hit_attrib, 32 bytes, one per input triangle; numpy twin: hit_attrib_dtype()
    _fields_ = [("uv", (C.c_float * 2) * 3), ("albedo_index", C.c_uint32), ("reserved", C.c_uint32)]


REFLECT_RT_FILL_MISSES = 1  # VKR_REFLECT_RT_FILL_MISSES


class ReflectRtParams(C.Structure):  # vkr_reflect_rt_params, 112 bytes
    _fields_ = [("inverse_camera", Mat4), ("fovy", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float),
                ("normal_offset", C.c_float), ("tmin", C.c_float), ("max_distance", C.c_float), ("texture_lod", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


# ---- alpha cutouts in the ray query ----
class RayCutout(C.Structure):  # vkr_ray_cutout, 8 bytes
    _fields_ = [("alpha_lod", C.c_uint32), ("opaque_texture_mask", C.c_uint32)]


# ---- lit ray-traced reflections ----
class HitNormal(C.Structure):  # vkr_hit_normal, 48 bytes, one per input triangle; numpy twin: hit_normal_dtype()
    _fields_ = [("n", (C.c_float * 4) * 3)]


class ReflectLights(C.Structure):  # vkr_reflect_lights, 176 bytes
    _fields_ = [("lights", (C.c_float * 4) * 4), ("colour", (C.c_float * 4) * 4), ("ambient", C.c_float * 4), ("light_count", C.c_uint32),
                ("shadow_offset", C.c_float), ("shadow_tmin", C.c_float), ("reserved", C.c_uint32 * 5)]


# the offsets of the shadow ray cast from a reflection's hit: the host frame's defaults (host/frame.cpp), those of the shadow mask's rays
REFLECT_SHADOW_OFFSET, REFLECT_SHADOW_TMIN = 1e-3, 0.0


TEXDRAW_SHOW_ALL, TEXDRAW_SHOW_R, TEXDRAW_SHOW_G, TEXDRAW_SHOW_B, TEXDRAW_SHOW_A = 0, 1, 2, 4, 8  # VKR_TEXDRAW_*: DrawTex


HIT_BOTH_ROWS, HIT_NORMAL, HIT_REPLY_BYTES = 0x10000000, 0x20000000, 16
HIT_WORKSPACE_WORDS = 4096  # include/vkr_postfx.h VKR_HIT_WORKSPACE_WORDS

# name -> argument types *without* the trailing stream
ENTRY_ARGS = {
    "downsample_gbuffer": [_IMG, _IMG, _IMG, _IMG, _IMG],
    "depth_mips": [_IMG, C.c_uint32],
    "pdf_preintegrate": [_IMG],
    "sssr_trace": [_IMG, _IMG, _IMG, P(TraceParams), C.c_void_p, _IMG, _IMG, _IMG, P(TracePush)],
    # the same program in two launches (head + resume over a frame-wide queue of parked rays): workspace, bytes, park_after_rounds
    "sssr_trace_split": [_IMG, _IMG, _IMG, P(TraceParams), C.c_void_p, _IMG, _IMG, _IMG, P(TracePush), C.c_void_p, C.c_uint64, C.c_uint32],
    "sssr_filter": [_IMG, _IMG, _IMG, _IMG, _IMG, _IMG, P(TraceParams), P(FilterPush)],
    "sssr_blur": [_IMG, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG, _IMG, P(ReprojectParams), P(BlurPush)],
    "gtao_main": [_IMG, P(GtaoParams), _IMG, _IMG, _IMG, _IMG, P(GtaoPush)],
    "gtao_filter": [_IMG, _IMG, _IMG, P(GtaoFilterPush)],
    "gtao_accumulate": [_IMG, _IMG, _IMG, _IMG, _IMG, _IMG, P(GtaoAccumParams), P(GtaoAccumPush)],
    "taa_resolve": [_IMG, _IMG, _IMG, _IMG, _IMG, _IMG, P(ReprojectParams)],
    "synth_gbuffer": [_IMG, _IMG, _IMG, _IMG, _IMG, P(SynthParams)],
    "ssr": [_IMG, _IMG, _IMG, P(SsrParams), _IMG, _IMG],
    "brdf_preintegrate": [C.c_void_p, _IMG],
    "defered_shading": [_IMG, _IMG, _IMG, _IMG, P(ShadingParams), _IMG, _IMG, _IMG, _IMG, P(ShadingPush)],
    # G-buffer raster stage; trailing (scratch pointer, scratch bytes)
    "raster_gbuffer": [P(RasterScene), P(GbufConst), _IMG, _IMG, _IMG, _IMG, _IMG, C.c_void_p, C.c_uint64],
    # tile-classified trace: tile lists / indirect args are raw pointers
    "sssr_clear_indirect": [C.c_void_p, C.c_void_p],
    "sssr_classification": [_IMG, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(ClassificationPush)],
    "sssr_trace_indirect": [_IMG, _IMG, _IMG, P(TraceParams), C.c_void_p, _IMG, C.c_void_p, C.c_void_p, C.c_uint32, P(TraceIndirectPush)],
    # dormant GTAO variants; `layers` = array of per-layer descriptors + count
    "gtao_main_graphics": [_IMG, P(GtaoParams), _IMG, _IMG, P(GtaoGfxPush)],
    "gtao_reproject": [P(GtaoReprojection), _IMG, _IMG, _IMG, _IMG, _IMG],
    "deinterleave_depth": [_IMG, _IMG, C.c_uint32, P(DeinterleavePush)],
    "gtao_main_deinterleaved": [_IMG, C.c_uint32, P(GtaoParams), _IMG, _IMG, P(GtaoDeinterleavedPush)],
    # ScreenSpaceTrace (row R2)
    "screen_trace_main": [_IMG, _IMG, _IMG, _IMG, _IMG, P(ScreenTraceParams)],
    "screen_trace_filter": [_IMG, _IMG, _IMG, P(ScreenTraceFilterPush)],
    "screen_trace_accumulate": [_IMG, _IMG, _IMG, _IMG, P(ScreenTraceAccumPush)],
    # multi-GPU: hit colours / hit normals by request / reply (no reference counterpart)
    "sssr_trace_windowed": [_IMG, _IMG, _IMG, P(TraceParams), C.c_void_p, _IMG, _IMG, _IMG, _IMG, _IMG, P(TraceWindowPush)],
    # ... in two launches around the arrival of the whole-frame pyramid: local pyramid first; trailing (workspace, bytes[, park_after_rounds])
    "sssr_trace_windowed_head": [_IMG, _IMG, _IMG, _IMG, P(TraceParams), C.c_void_p, _IMG, _IMG, _IMG, _IMG, _IMG, P(TraceWindowPush), C.c_void_p, C.c_uint64, C.c_uint32],
    "sssr_trace_windowed_resume": [_IMG, _IMG, _IMG, P(TraceParams), C.c_void_p, _IMG, _IMG, _IMG, _IMG, _IMG, P(TraceWindowPush), C.c_void_p, C.c_uint64],
    "sssr_validate": [_IMG, _IMG, _IMG, _IMG, P(TraceParams)],
    "hit_requests": [P(HitSources), P(C.c_uint32), C.c_uint32, C.c_void_p, C.c_void_p, P(C.c_uint32), C.c_void_p],
    # pass 2 into segments of fixed room (workspace, segments, capacities, out, dropped flag); an overflowing segment keeps the
    # first requests in the fixed slot order of pass 2: no oracle twin, checked against tests/hit_exchange_reference.py
    "hit_requests_bounded": [P(HitSources), P(C.c_uint32), C.c_uint32, C.c_void_p, P(C.c_uint32), P(C.c_uint32), C.c_void_p, C.c_void_p],
    "hit_reply": [_IMG, _IMG, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "hit_scatter": [_IMG, _IMG, C.c_void_p, C.c_void_p, C.c_uint32],
    # lit ray-traced reflections: vkr_reflections_rt's arguments with (normals, normal_count) behind the attributes and the lights
    # behind params; trailing (scratch pointer, scratch bytes); and the scene's vertex normals made on the device
    "reflections_rt_lit": [_IMG, _IMG, _IMG, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, P(ReflectRtParams),
                           P(ReflectLights), _IMG, C.c_void_p, C.c_uint64],
    "reflections_rt_lit_cutout": [_IMG, _IMG, _IMG, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                  P(ReflectRtParams), P(ReflectLights), P(RayCutout), _IMG, C.c_void_p, C.c_uint64],
    "scene_triangle_normals": [P(RasterScene), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64],
}


# entries without a twin in a checker library: a different SCHEDULE of another entry (same images bit for bit), or a variant
# of pass 2 of the hit requests that the checker library does not restate (held to tests/hit_exchange_reference.py instead), or
# a ray-query entry without a reference program, held to the numpy restatement tests/reflections_rt_lit_reference.py
SCHEDULE_VARIANTS = {"sssr_trace_split": "sssr_trace", "sssr_trace_windowed_head": "sssr_trace_windowed", "sssr_trace_windowed_resume": "sssr_trace_windowed",
                     "hit_requests_bounded": "hit_requests", "reflections_rt_lit": None, "reflections_rt_lit_cutout": None, "scene_triangle_normals": None}


class RectCopy(C.Structure):  # vkr_rect_copy
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("src_pitch", C.c_uint32), ("dst_pitch", C.c_uint32),
                ("row_bytes", C.c_uint32), ("rows", C.c_uint32)]


class ExtensionMissing(RuntimeError):
    pass


def _load(path, what, needs_hip=True):
    if needs_hip:
        # torch ships its own libamdhip64.so.7; load it first so the extension binds to the same HIP
        # runtime torch uses for memory and streams (two runtimes in one process do not share devices)
        import torch  # noqa: F401
    if not os.path.exists(path):
        raise ExtensionMissing(
            f"{what} not built: {path} is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` first."
        )
    return C.CDLL(path)


_product = None


def product():
    """The HIP C-ABI library.  Fails loudly when it is missing — there is no fallback."""
    global _product
    if _product is None:
        lib = _load(PRODUCT_LIB, "HIP extension libvkr_postfx.so")
        for name, args in ENTRY_ARGS.items():
            fn = getattr(lib, "vkr_" + name)
            fn.argtypes = args + [C.c_void_p]
            fn.restype = C.c_int
        lib.vkr_stream_read.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.vkr_stream_read.restype = C.c_int
        lib.vkr_copy_rects.argtypes = [P(RectCopy), C.c_uint32, C.c_void_p]
        lib.vkr_comm_unique_id.argtypes = [C.c_void_p]
        lib.vkr_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, P(C.c_void_p)]
        lib.vkr_comm_destroy.argtypes = [C.c_void_p]
        lib.vkr_comm_create_emulated.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, P(C.c_void_p)]
        lib.vkr_comm_create_emulated.restype = C.c_int
        lib.vkr_comm_available.argtypes = []
        lib.vkr_get_switches.argtypes = []
        lib.vkr_get_switches.restype = C.c_uint32
        lib.vkr_set_switches.argtypes = [C.c_uint32]
        lib.vkr_set_switches.restype = None
        lib.vkr_debug_blur_paths.argtypes = [P(C.c_uint32), C.c_int]
        lib.vkr_debug_blur_paths.restype = C.c_int
        lib.vkr_comm_available.restype = C.c_int
        lib.vkr_copy_rects.restype = C.c_int
        lib.vkr_sssr_trace_workspace_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.vkr_sssr_trace_workspace_bytes.restype = C.c_uint64
        lib.vkr_raster_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        lib.vkr_raster_scratch_bytes.restype = C.c_uint64
        lib.vkr_halton23_fill.argtypes = [C.c_void_p, C.c_uint32]
        lib.vkr_halton23_fill.restype = None
        lib.vkr_version.restype = C.c_char_p
        lib.vkr_last_error.restype = C.c_char_p
        lib.vkr_format_bytes.argtypes = [C.c_uint32]
        lib.vkr_format_bytes.restype = C.c_uint32
        # ray-traced AO (no twin in the oracle: its checker is the numpy restatement of tests/test_gtao_rt_gpu.py)
        lib.vkr_accel_layout.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, P(C.c_uint32)]
        lib.vkr_accel_create.argtypes = [C.c_void_p, C.c_uint32, P(C.c_void_p)]
        lib.vkr_accel_destroy.argtypes = [C.c_void_p]
        lib.vkr_accel_info.argtypes = [C.c_void_p, P(C.c_uint32), P(C.c_uint32)]
        lib.vkr_accel_query.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.vkr_gtao_rt_main.argtypes = [P(GtaoRtParams), _IMG, _IMG, C.c_void_p, C.c_void_p, _IMG, P(GtaoRtPush), C.c_void_p]
        lib.vkr_accel_occluded.argtypes = lib.vkr_accel_query.argtypes
        # the ray-traced shadow mask (checked against the numpy restatement tests/shadow_mask_rt_reference.py)
        lib.vkr_shadow_mask_rt.argtypes = [_IMG, _IMG, C.c_void_p, P(ShadowRtParams), _IMG, C.c_void_p]
        for name in ("accel_layout", "accel_create", "accel_destroy", "accel_info", "accel_query", "gtao_rt_main", "accel_occluded", "shadow_mask_rt"):
            getattr(lib, "vkr_" + name).restype = C.c_int
        # the closest-hit query and the ray-traced reflections (checked against the numpy restatements tests/closest_hit_reference.py
        # and tests/reflections_rt_reference.py)
        lib.vkr_accel_closest.argtypes = lib.vkr_accel_query.argtypes
        lib.vkr_accel_closest.restype = C.c_int
        # refit (checked against the numpy restatement tests/accel_refit_reference.py) and the scene's triangles on the device
        lib.vkr_accel_refit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.vkr_accel_refit_layout.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.vkr_accel_download.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.vkr_accel_refit_schedule.argtypes = [C.c_void_p, P(C.c_uint32), C.c_uint32, P(C.c_uint32), P(C.c_uint32)]
        lib.vkr_scene_triangles_scratch_bytes.argtypes = [C.c_uint32]
        lib.vkr_scene_triangles_scratch_bytes.restype = C.c_uint64
        lib.vkr_scene_triangles.argtypes = [P(RasterScene), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        for name in ("accel_refit", "accel_refit_layout", "accel_download", "accel_refit_schedule", "scene_triangles"):
            getattr(lib, "vkr_" + name).restype = C.c_int
        lib.vkr_reflections_rt_scratch_bytes.argtypes = [C.c_uint32]
        lib.vkr_reflections_rt_scratch_bytes.restype = C.c_uint64
        lib.vkr_reflections_rt.argtypes = [_IMG, _IMG, _IMG, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, P(ReflectRtParams), _IMG,
                                           C.c_void_p, C.c_uint64, C.c_void_p]
        lib.vkr_reflections_rt.restype = C.c_int
        # alpha cutouts in the ray query (checked against the numpy restatement tests/ray_cutout_reference.py)
        cutout_tail = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, P(RayCutout), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.vkr_accel_cutout_scratch_bytes.argtypes = [C.c_uint32]
        lib.vkr_accel_cutout_scratch_bytes.restype = C.c_uint64
        lib.vkr_accel_occluded_cutout.argtypes = lib.vkr_accel_query.argtypes[:6] + cutout_tail
        lib.vkr_accel_closest_cutout.argtypes = lib.vkr_accel_query.argtypes[:6] + cutout_tail
        lib.vkr_shadow_mask_rt_cutout.argtypes = [_IMG, _IMG, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, P(ShadowRtParams), P(RayCutout),
                                                  _IMG, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.vkr_reflections_rt_cutout.argtypes = [_IMG, _IMG, _IMG, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, P(ReflectRtParams),
                                                  P(RayCutout), _IMG, C.c_void_p, C.c_uint64, C.c_void_p]
        for name in ("accel_occluded_cutout", "accel_closest_cutout", "shadow_mask_rt_cutout", "reflections_rt_cutout"):
            getattr(lib, "vkr_" + name).restype = C.c_int
        # area lights in the traced shadow mask (checked against the numpy restatement tests/shadow_mask_rt_soft_reference.py)
        lib.vkr_shadow_mask_rt_soft.argtypes = [_IMG, _IMG, C.c_void_p, P(ShadowRtParams), P(ShadowRtSoft), _IMG, C.c_void_p]
        lib.vkr_shadow_mask_rt_soft_cutout.argtypes = [_IMG, _IMG, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, P(ShadowRtParams),
                                                       P(RayCutout), P(ShadowRtSoft), _IMG, C.c_void_p, C.c_uint64, C.c_void_p]
        for name in ("shadow_mask_rt_soft", "shadow_mask_rt_soft_cutout"):
            getattr(lib, "vkr_" + name).restype = C.c_int
        lib.vkr_shadow_disk_samples.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        lib.vkr_shadow_disk_samples.restype = None
        # the edge-aware filter of the shadow mask (checked against the numpy restatement tests/shadow_mask_filter_reference.py)
        lib.vkr_shadow_mask_filter.argtypes = [_IMG, _IMG, _IMG, P(ShadowFilterParams), _IMG, C.c_void_p]
        lib.vkr_shadow_mask_filter.restype = C.c_int
        # the temporal accumulation of the shadow mask (checked against tests/shadow_mask_accumulate_reference.py)
        lib.vkr_shadow_mask_accumulate.argtypes = [_IMG] * 7 + [P(ShadowAccumParams)] + [_IMG] * 3 + [C.c_void_p]
        lib.vkr_shadow_mask_accumulate.restype = C.c_int
        lib.vkr_shadow_disk_samples_frame.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.vkr_shadow_disk_samples_frame.restype = None
        lib.vkr_selftest_accum_division.argtypes = [C.c_void_p, C.c_void_p]
        lib.vkr_selftest_accum_division.restype = C.c_int
        # octahedral probes (checked against the numpy restatement of tests/test_probe_gpu.py); array images: per-layer descriptors
        lib.vkr_cube2oct.argtypes = [_IMG, _IMG, _IMG, _IMG, C.c_void_p]
        lib.vkr_probe_downsample.argtypes = [_IMG, C.c_void_p]
        lib.vkr_trace_probe.argtypes = [_IMG, _IMG, _IMG, _IMG, C.c_uint32, P(ProbeTraceConsts), _IMG, C.c_void_p]
        for name in ("cube2oct", "probe_downsample", "trace_probe"):
            getattr(lib, "vkr_" + name).restype = C.c_int
        # the cube-face bake (checked against the numpy restatement tests/cubemap_reference.py)
        lib.vkr_cubemap_probe_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.vkr_cubemap_probe_scratch_bytes.restype = C.c_uint64
        lib.vkr_cubemap_probe.argtypes = [P(RasterScene), P(C.c_float * 3), _IMG, _IMG, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.vkr_cubemap_probe.restype = C.c_int
        # the shadow-map pass (checked against the oracle's G-buffer rasteriser: its depth attachment under the light's matrix)
        lib.vkr_default_shadow_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        lib.vkr_default_shadow_scratch_bytes.restype = C.c_uint64
        lib.vkr_default_shadow.argtypes = [P(RasterScene), P(Mat4), _IMG, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.vkr_default_shadow.restype = C.c_int
        # image transfers (checked against the numpy restatement tests/transfer_reference.py and scene.build_mips)
        lib.vkr_clear_image.argtypes = [_IMG, P(ClearValue), C.c_void_p]
        lib.vkr_blit_image.argtypes = [_IMG, _IMG, C.c_uint32, C.c_void_p]
        lib.vkr_gen_mipmaps.argtypes = [_IMG, C.c_void_p]
        for name in ("clear_image", "blit_image", "gen_mipmaps"):
            getattr(lib, "vkr_" + name).restype = C.c_int
        # the SSAO pass (checked against the numpy restatement tests/ssao_reference.py)
        lib.vkr_ssao.argtypes = [_IMG, P(SsaoParams), _IMG, C.c_void_p]
        lib.vkr_ssao.restype = C.c_int
        # the tile plane regression (checked against the numpy restatement tests/tile_regression_reference.py)
        lib.vkr_tile_regression.argtypes = [_IMG, _IMG, P(TileRegressionPush), C.c_void_p]
        lib.vkr_tile_regression.restype = C.c_int
        # the backbuffer texdraw pass (checked against the numpy restatement tests/texdraw_reference.py) and its encode's self-test
        lib.vkr_texdraw.argtypes = [_IMG, _IMG, P(TexdrawPush), C.c_void_p]
        lib.vkr_texdraw.restype = C.c_int
        lib.vkr_selftest_srgb_encode.argtypes = [C.c_void_p, C.c_void_p]
        lib.vkr_selftest_srgb_encode.restype = C.c_int
        # the shadow mask (checked against the numpy restatement tests/shadow_mask_reference.py) and the shading that applies it
        lib.vkr_shadow_mask.argtypes = [_IMG, _IMG, P(ShadowMaskParams), _IMG, C.c_void_p]
        lib.vkr_shadow_mask.restype = C.c_int
        lib.vkr_defered_shading_shadowed.argtypes = [_IMG, _IMG, _IMG, _IMG, P(ShadingParams), _IMG, _IMG, _IMG, _IMG, _IMG, P(ShadingPush), C.c_void_p]
        lib.vkr_defered_shading_shadowed.restype = C.c_int
        _product = lib
    return _product


def check(rc, lib=None):
    if rc != 0:
        msg = ""
        if lib is not None and hasattr(lib, "vkr_last_error"):
            msg = (lib.vkr_last_error() or b"").decode()
        raise RuntimeError(f"vkr call failed with code {rc}: {msg}")


def cubemap_probe_scratch_bytes(cube_size, triangle_count):
    """vkr_cubemap_probe_scratch_bytes: device scratch of one bake (triangles summed over all draws of the scene)"""
    return int(product().vkr_cubemap_probe_scratch_bytes(int(cube_size), int(triangle_count)))


def cubemap_probe(scene, pos, cube_color, cube_distance, scratch, scratch_bytes, stream=None):
    """vkr_cubemap_probe: bakes the six cube faces at `pos`.  scene: RasterScene; cube_color / cube_distance: (VkrImg * 6)
    arrays, the layers of one regular array image each (images.ArrayImageBuf.descs()); scratch: device pointer.  Raises
    RuntimeError with the library's message on a refusal."""
    lib = product()
    if len(cube_color) < 6 or len(cube_distance) < 6:
        raise RuntimeError("cubemap_probe: a cube has 6 layers")
    p = (C.c_float * 3)(float(pos[0]), float(pos[1]), float(pos[2]))
    check(lib.vkr_cubemap_probe(C.byref(scene), C.byref(p), cube_color, cube_distance, scratch, int(scratch_bytes), stream), lib)


def clear_image(img, color=(0.0, 0.0, 0.0, 0.0), depth=1.0, stencil=0, stream=None):
    """vkr_clear_image: every mip of the view `img` (VkrImg) to one value: `color` for colour formats (stored as the format
    stores it), rint(clamp(depth, 0, 1) * 16777215) | stencil << 24 for D24_UNORM_S8 (a NaN depth stores 0).  Raises RuntimeError with
    the library's message on a refusal."""
    lib = product()
    v = ClearValue((C.c_float * 4)(*[float(c) for c in color]), float(depth), int(stencil))
    check(lib.vkr_clear_image(C.byref(img), C.byref(v), stream), lib)


def blit_image(src, dst, filter=FILTER_LINEAR, stream=None):
    """vkr_blit_image: whole mip 0 of `src` onto whole mip 0 of `dst` (VkrImg), any colour formats and extents; FILTER_NEAREST or
    FILTER_LINEAR.  Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    check(lib.vkr_blit_image(C.byref(src), C.byref(dst), int(filter), stream), lib)


def gen_mipmaps(img, stream=None):
    """vkr_gen_mipmaps: levels 1 .. mip_count - 1 of the view from level 0 by the project's mip rule (scene.build_mips).  Raises
    RuntimeError with the library's message on a refusal."""
    lib = product()
    check(lib.vkr_gen_mipmaps(C.byref(img), stream), lib)


def default_shadow_scratch_bytes(size, layer_count, triangle_count):
    """vkr_default_shadow_scratch_bytes: device scratch of one call (edge of a layer, layers, triangles summed over all draws)"""
    return int(product().vkr_default_shadow_scratch_bytes(int(size), int(layer_count), int(triangle_count)))


def default_shadow(scene, mvps, layers, scratch, scratch_bytes, stream=None):
    """vkr_default_shadow: layer l := the depth of `scene` (RasterScene) seen through mvps[l].  mvps: a sequence of 4x4 arrays
    (maths convention, as camera.shadow_mvp returns them); layers: a (VkrImg * n) array or a sequence of VkrImg, one square
    D24_UNORM_S8 descriptor per matrix; scratch: device pointer.  Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    n = len(mvps)
    if len(layers) != n:
        raise RuntimeError(f"default_shadow: {n} matrices for {len(layers)} layers")
    mats = (Mat4 * max(1, n))(*[Mat4.from_np(m) for m in mvps])
    descs = (VkrImg * max(1, n))(*list(layers))
    check(lib.vkr_default_shadow(C.byref(scene), mats, descs, n, scratch, int(scratch_bytes), stream), lib)


def ssao_params(projection, fovy, aspect, znear, zfar, samples):
    """SsaoParams from a 4x4 projection (maths convention), the camera's four floats and 16 samples: an array of [16, 3] (w = 0)
    or [16, 4] (the block's 16-byte slots as they are)."""
    import numpy as np

    s = np.asarray(samples, dtype=np.float32)
    if s.shape not in ((16, 3), (16, 4)):
        raise RuntimeError(f"ssao_params: samples of shape {s.shape}, expected (16, 3) or (16, 4)")
    p = SsaoParams(Mat4.from_np(projection), float(fovy), float(aspect), float(znear), float(zfar))
    for i in range(16):
        for c in range(s.shape[1]):
            p.samples[i][c] = float(s[i, c])
    return p


def ssao(depth, params, out_occlusion, stream=None):
    """vkr_ssao: out_occlusion (R8_UNORM VkrImg, any extent) := the 16-sample SSAO of `depth` (D24_UNORM_S8 VkrImg, mip 0 of the
    view) under `params` (SsaoParams, e.g. ssao_params(...)).  Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    check(lib.vkr_ssao(C.byref(depth), C.byref(params), C.byref(out_occlusion), stream), lib)


def tile_regression_push(camera_to_world, fovy, aspect, znear, zfar):
    """TileRegressionPush from a 4x4 camera-to-world matrix (maths convention) and the camera's four floats"""
    return TileRegressionPush(Mat4.from_np(camera_to_world), float(fovy), float(aspect), float(znear), float(zfar))


def tile_regression(depth, out_planes, push, stream=None):
    """vkr_tile_regression: out_planes (RGBA32_SFLOAT VkrImg, at most ceil(w / 8) x ceil(h / 8)) := per 8 x 8 tile of `depth`
    (D24_UNORM_S8 VkrImg, mip 0 of the view: pass a view of the G-buffer depth's mip 1) the fitted plane and its mean squared
    residual under `push` (TileRegressionPush, e.g. tile_regression_push(...)).  Raises RuntimeError with the library's message
    on a refusal."""
    lib = product()
    check(lib.vkr_tile_regression(C.byref(depth), C.byref(out_planes), C.byref(push), stream), lib)


def texdraw_push(flags=TEXDRAW_SHOW_ALL):
    """TexdrawPush from the DrawTex flags (TEXDRAW_SHOW_*; the last set bit of R, G, B, A wins)"""
    return TexdrawPush(int(flags) & 0xFFFFFFFF)


def texdraw(target_tex, backbuffer, push=None, stream=None):
    """vkr_texdraw: backbuffer (RGBA8_SRGB or RGBA8_UNORM VkrImg of any extent) := texture(target_tex, pixel-centre uv) of
    `target_tex` (a VkrImg of any colour format, mip 0 of the view), all channels or the one `push` (TexdrawPush, e.g.
    texdraw_push(TEXDRAW_SHOW_R); default: all) selects.  Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    push = push if push is not None else TexdrawPush(TEXDRAW_SHOW_ALL)
    check(lib.vkr_texdraw(C.byref(target_tex), C.byref(backbuffer), C.byref(push), stream), lib)


def shadow_mask_params(inverse_camera, mvps, fovy, aspect, znear, zfar, radius=1, bias=0):
    """ShadowMaskParams from the camera's view -> world matrix and 1..4 light matrices (4x4, maths convention, the ones the
    layers were rendered with, e.g. camera.shadow_mvp(...)), the camera's four floats, the box radius (0, 1, 2) and the bias in
    D24 codes.  layer_count = len(mvps); radius and bias are passed on as given (the entry refuses what it does not take)."""
    p = ShadowMaskParams()
    p.inverse_camera = Mat4.from_np(inverse_camera)
    if len(mvps) > 4:
        raise RuntimeError(f"shadow_mask_params: {len(mvps)} light matrices, at most 4")
    for l, m in enumerate(mvps):
        p.mvps[l] = Mat4.from_np(m)
    p.fovy, p.aspect, p.znear, p.zfar = float(fovy), float(aspect), float(znear), float(zfar)
    p.layer_count, p.radius, p.bias, p.reserved = len(mvps), int(radius), int(bias), 0
    return p


def shadow_mask(depth, layers, params, out_mask, stream=None):
    """vkr_shadow_mask: out_mask (RGBA8_UNORM VkrImg) := per pixel of `depth` (D24_UNORM_S8 VkrImg of the same extent, mip 0 of
    the view) the visibility of light l in channel l, through `layers` (a (VkrImg * n) array or a sequence of square
    D24_UNORM_S8 VkrImg of one extent, n >= params.layer_count) under `params` (ShadowMaskParams, e.g. shadow_mask_params(...)).
    Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    descs = (VkrImg * max(1, len(layers)))(*list(layers))
    check(lib.vkr_shadow_mask(C.byref(depth), descs, C.byref(params), C.byref(out_mask), stream), lib)


def shadow_rt_params(inverse_camera, lights, fovy, aspect, znear, zfar, normal_offset=SHADOW_RT_NORMAL_OFFSET, tmin=SHADOW_RT_TMIN):
    """ShadowRtParams from the camera's view -> world matrix (4x4, maths convention), 1..4 lights of (x, y, z, w) — w == 1 a point
    light at xyz, w == 0 a directional light whose xyz is the vector from the surface towards the light — the camera's four floats
    and the two offsets of the ray.  light_count = len(lights); everything is passed on as given (the entry refuses what it does
    not take)."""
    p = ShadowRtParams()
    p.inverse_camera = Mat4.from_np(inverse_camera)
    if len(lights) > 4:
        raise RuntimeError(f"shadow_rt_params: {len(lights)} lights, at most 4")
    for l, v in enumerate(lights):
        for k in range(4):
            p.lights[l][k] = float(v[k])
    p.fovy, p.aspect, p.znear, p.zfar = float(fovy), float(aspect), float(znear), float(zfar)
    p.light_count, p.normal_offset, p.tmin, p.reserved = len(lights), float(normal_offset), float(tmin), 0
    return p


def shadow_mask_rt(depth, normal, accel, params, out_mask, stream=None):
    """vkr_shadow_mask_rt: out_mask (RGBA8_UNORM VkrImg) := per pixel of `depth` (D24_UNORM_S8 VkrImg, mip 0 of the view) and
    `normal` (RG16_UNORM VkrImg), all of one extent, channel l = 255 where the ray from the surface towards light l meets no
    triangle of `accel` (an Accel, or None to show the refusal) and 0 where it does or where the surface faces away, under
    `params` (ShadowRtParams, e.g. shadow_rt_params(...)).  Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    handle = accel.handle if accel is not None else None
    check(lib.vkr_shadow_mask_rt(C.byref(depth) if depth is not None else None, C.byref(normal) if normal is not None else None, handle,
                                 C.byref(params) if params is not None else None, C.byref(out_mask) if out_mask is not None else None,
                                 stream), lib)


def accel_occluded(accel, origins, dirs, tmin, tmax, out, stream=None):
    """vkr_accel_occluded: Accel.query on the walk for long rays — the same arguments (device tensors (n, 3) float32, out (n,)
    int32 / uint32) and the same answers."""
    accel.occluded(origins, dirs, tmin, tmax, out, stream)


def accel_hit_dtype():
    """the numpy dtype of vkr_accel_hit: view a (n, 16) uint8 / (n, 4) int32 download with it"""
    import numpy as np

    return np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32), ("index", np.uint32)])


def hit_attrib_dtype():
    """the numpy dtype of vkr_hit_attrib (32 bytes)"""
    import numpy as np

    return np.dtype([("uv", np.float32, (3, 2)), ("albedo_index", np.uint32), ("reserved", np.uint32)])


def reflect_rt_params(inverse_camera, fovy, aspect, znear, zfar, fill_misses=False, normal_offset=SHADOW_RT_NORMAL_OFFSET, tmin=SHADOW_RT_TMIN,
                      max_distance=None, texture_lod=0):
    """ReflectRtParams from the camera's view -> world matrix (4x4, maths convention), its four floats and the ray's settings:
    origin = world + normal_offset * normal, t in [tmin, max_distance] along the unit mirror direction (max_distance None: zfar),
    the mip level sampled at a hit, and the mode (fill_misses: only pixels whose screen-space ray is invalid are traced)."""
    p = ReflectRtParams()
    p.inverse_camera = Mat4.from_np(inverse_camera)
    p.fovy, p.aspect, p.znear, p.zfar = float(fovy), float(aspect), float(znear), float(zfar)
    p.normal_offset, p.tmin, p.max_distance = float(normal_offset), float(tmin), float(zfar if max_distance is None else max_distance)
    p.texture_lod, p.flags = int(texture_lod), REFLECT_RT_FILL_MISSES if fill_misses else 0
    return p


def reflections_rt_scratch_bytes(texture_count):
    """vkr_reflections_rt_scratch_bytes: the device scratch of one call (the texture table)"""
    return int(product().vkr_reflections_rt_scratch_bytes(int(texture_count)))


def reflections_rt(depth, normal, rays, accel, attribs, attrib_count, textures, texture_count, params, out_reflections, scratch, scratch_bytes,
                   stream=None):
    """vkr_reflections_rt: out_reflections (RGBA8_UNORM VkrImg) := per pixel of `depth` (D24_UNORM_S8 VkrImg, mip 0 of the view) and
    `normal` (RG16_UNORM VkrImg), all of one extent, the albedo at the closest hit of the mirror ray through `accel` (an Accel, or
    None to show the refusal); `rays` (RGBA16_UNORM VkrImg) only with REFLECT_RT_FILL_MISSES, else None.  attribs: device pointer
    to attrib_count vkr_hit_attrib records (scene_triangle_attributes order); textures: a (VkrImg * n) host array of RGBA8_SRGB
    mip chains or None; scratch: device pointer of reflections_rt_scratch_bytes(texture_count).  Raises RuntimeError with the
    library's message on a refusal."""
    lib = product()
    ref = lambda d: C.byref(d) if d is not None else None
    handle = accel.handle if accel is not None else None
    check(lib.vkr_reflections_rt(ref(depth), ref(normal), ref(rays), handle, attribs, int(attrib_count), textures, int(texture_count),
                                 ref(params), ref(out_reflections), scratch, int(scratch_bytes), stream), lib)


def ray_cutout(alpha_lod=0, opaque_texture_mask=0):
    """RayCutout: the mip level whose alpha decides a hole (clamped to each texture's chain) and the textures that are not to be
    tested (bit i set: textures[i] is opaque whatever its texels hold; scene_opaque_texture_mask(scene) for a Scene)"""
    return RayCutout(int(alpha_lod), int(opaque_texture_mask) & 0xFFFFFFFF)


def scene_opaque_texture_mask(sc):
    """The opaque_texture_mask of a scene.Scene: bit i set when no texel of any level of textures[i] has alpha 0 (what makes a
    draw carry VKR_RASTER_DRAW_OPAQUE_ALBEDO): such a texture can make no hole, so the ray query need not fetch from it."""
    mask = 0
    for i, levels in enumerate(sc.textures[:32]):
        if all(int(lv[..., 3].min()) > 0 for lv in levels):
            mask |= 1 << i
    return mask


def accel_cutout_scratch_bytes(texture_count):
    """vkr_accel_cutout_scratch_bytes: the device scratch of one call of a _cutout entry (the texture table)"""
    return int(product().vkr_accel_cutout_scratch_bytes(int(texture_count)))


def _cutout_tail(attribs, attrib_count, textures, texture_count, cutout):
    return attribs, int(attrib_count), textures, int(texture_count), (C.byref(cutout) if cutout is not None else None)


def accel_occluded_cutout(accel, origins, dirs, tmin, tmax, attribs, attrib_count, textures, texture_count, cutout, out, scratch, scratch_bytes,
                          stream=None):
    """vkr_accel_occluded_cutout: accel_occluded where a triangle whose albedo alpha at the hit is 0 is not there.  attribs: device
    pointer to attrib_count vkr_hit_attrib records (scene_triangle_attributes order); textures: a (VkrImg * n) host array of
    RGBA8_SRGB mip chains or None; cutout: a RayCutout; scratch: device pointer of accel_cutout_scratch_bytes(texture_count)."""
    lib = product()
    n = int(origins.shape[0])
    check(lib.vkr_accel_occluded_cutout(accel.handle, origins.data_ptr(), dirs.data_ptr(), float(tmin), float(tmax), n,
                                        *_cutout_tail(attribs, attrib_count, textures, texture_count, cutout), out.data_ptr(), scratch,
                                        int(scratch_bytes), stream), lib)


def accel_closest_cutout(accel, origins, dirs, tmin, tmax, attribs, attrib_count, textures, texture_count, cutout, out, scratch, scratch_bytes,
                         stream=None):
    """vkr_accel_closest_cutout: Accel.closest among the triangles that are not transparent at their own hit; the other arguments
    as accel_occluded_cutout, out as Accel.closest (n 16-byte records)."""
    lib = product()
    n = int(origins.shape[0])
    check(lib.vkr_accel_closest_cutout(accel.handle, origins.data_ptr(), dirs.data_ptr(), float(tmin), float(tmax), n,
                                       *_cutout_tail(attribs, attrib_count, textures, texture_count, cutout), out.data_ptr(), scratch,
                                       int(scratch_bytes), stream), lib)


def shadow_mask_rt_cutout(depth, normal, accel, attribs, attrib_count, textures, texture_count, params, cutout, out_mask, scratch, scratch_bytes,
                          stream=None):
    """vkr_shadow_mask_rt_cutout: shadow_mask_rt whose rays pass through the holes of alpha-tested triangles; attribs, textures,
    cutout and scratch as accel_occluded_cutout.  Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    ref = lambda d: C.byref(d) if d is not None else None
    handle = accel.handle if accel is not None else None
    check(lib.vkr_shadow_mask_rt_cutout(ref(depth), ref(normal), handle, attribs, int(attrib_count), textures, int(texture_count), ref(params),
                                        ref(cutout), ref(out_mask), scratch, int(scratch_bytes), stream), lib)


def shadow_disk_samples(sample_count, pattern_side):
    """vkr_shadow_disk_samples: the sample table of the area lights, float32 [pattern_side^2, sample_count, 2] of (u, v) in the
    unit disk — the table the host frame uses."""
    import numpy as np

    sample_count, pattern_side = int(sample_count), int(pattern_side)
    if not (1 <= sample_count <= 64) or pattern_side not in (1, 2, 4):
        raise RuntimeError(f"shadow_disk_samples: {sample_count} samples in a pattern tile of side {pattern_side}, needs 1..64 and 1, 2 or 4")
    out = np.zeros((pattern_side * pattern_side, sample_count, 2), np.float32)
    product().vkr_shadow_disk_samples(sample_count, pattern_side, out.ctypes.data)
    return out


def shadow_rt_soft(radii, sample_count, pattern_side, device=None, table=None):
    """ShadowRtSoft for shadow_mask_rt_soft: `radii` (up to 4, one per light; 0 keeps a light hard), S rays per pixel and light
    with a radius, a pattern tile of side P.  The table — `table` (anything numpy takes, P^2 * S * 2 values) or
    shadow_disk_samples(S, P) — is copied to `device` and kept alive by the returned block (attribute `table`); device None
    leaves samples NULL (to show the refusal).  Everything is passed on as given: the entry refuses what it does not take."""
    s = ShadowRtSoft()
    if len(radii) > 4:
        raise RuntimeError(f"shadow_rt_soft: {len(radii)} radii, at most 4")
    for l, r in enumerate(radii):
        s.radius[l] = float(r)
    s.sample_count, s.pattern_side = int(sample_count), int(pattern_side)
    s.table = None
    if device is not None:
        import numpy as np
        import torch

        host = np.ascontiguousarray(shadow_disk_samples(sample_count, pattern_side) if table is None else table, dtype=np.float32)
        s.table = torch.from_numpy(host.reshape(-1).copy()).to(device)
        s.samples = s.table.data_ptr()
    return s


def shadow_mask_rt_soft(depth, normal, accel, params, soft, out_mask, stream=None):
    """vkr_shadow_mask_rt_soft: shadow_mask_rt with area lights: channel l = 255 * (visible samples of light l's disk) / S, rounded
    half up, under `soft` (a ShadowRtSoft, e.g. shadow_rt_soft(...)); a light with radius 0 is traced as shadow_mask_rt traces it.
    Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    ref = lambda d: C.byref(d) if d is not None else None
    handle = accel.handle if accel is not None else None
    check(lib.vkr_shadow_mask_rt_soft(ref(depth), ref(normal), handle, ref(params), ref(soft), ref(out_mask), stream), lib)


def shadow_mask_rt_soft_cutout(depth, normal, accel, attribs, attrib_count, textures, texture_count, params, cutout, soft, out_mask, scratch,
                               scratch_bytes, stream=None):
    """vkr_shadow_mask_rt_soft_cutout: shadow_mask_rt_soft whose rays pass through the holes of alpha-tested triangles; attribs,
    textures, cutout and scratch as accel_occluded_cutout.  Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    ref = lambda d: C.byref(d) if d is not None else None
    handle = accel.handle if accel is not None else None
    check(lib.vkr_shadow_mask_rt_soft_cutout(ref(depth), ref(normal), handle, attribs, int(attrib_count), textures, int(texture_count), ref(params),
                                             ref(cutout), ref(soft), ref(out_mask), scratch, int(scratch_bytes), stream), lib)


def shadow_filter_params(inverse_camera, fovy, aspect, znear, zfar, reach, normal_min_dot=SHADOW_FILTER_NORMAL_MIN_DOT,
                         plane_tolerance=SHADOW_FILTER_PLANE_TOLERANCE):
    """ShadowFilterParams from the camera's view -> world matrix (4x4, maths convention), the camera's four floats, the reach R
    (taps at |dx|, |dy| < R; the pattern_side of the soft mask it reconstructs) and the two thresholds of the accept test.
    Everything is passed on as given (the entry refuses what it does not take)."""
    p = ShadowFilterParams()
    p.inverse_camera = Mat4.from_np(inverse_camera)
    p.fovy, p.aspect, p.znear, p.zfar = float(fovy), float(aspect), float(znear), float(zfar)
    p.reach, p.normal_min_dot, p.plane_tolerance, p.reserved = int(reach), float(normal_min_dot), float(plane_tolerance), 0
    return p


def shadow_mask_filter(depth, normal, mask, params, out_mask, stream=None):
    """vkr_shadow_mask_filter: out_mask (RGBA8_UNORM VkrImg) := per pixel the tent-weighted mean, rounded half up, of `mask`
    (RGBA8_UNORM VkrImg, other memory than out_mask) over the taps within params.reach that lie on the pixel's surface as `depth`
    (D24_UNORM_S8 VkrImg, mip 0 of the view) and `normal` (RG16_UNORM VkrImg) tell it, all of one extent, under `params`
    (ShadowFilterParams, e.g. shadow_filter_params(...)).  Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    ref = lambda d: C.byref(d) if d is not None else None
    check(lib.vkr_shadow_mask_filter(ref(depth), ref(normal), ref(mask), ref(params), ref(out_mask), stream), lib)


def shadow_accum_params(inverse_camera, prev_inverse_camera, fovy, aspect, znear, zfar, max_count=SHADOW_ACCUM_MAX_COUNT,
                        plane_tolerance=SHADOW_FILTER_PLANE_TOLERANCE, reset=False):
    """ShadowAccumParams from the view -> world matrices of this frame and of the frame that wrote prev_depth and the history (4x4,
    maths convention), the camera's four floats, max_count (the history weighs at most max_count - 1 frames), the tolerance of
    the plane test and whether no pixel has a history.  Everything is passed on as given (the entry refuses what it does not take)."""
    p = ShadowAccumParams()
    p.inverse_camera, p.prev_inverse_camera = Mat4.from_np(inverse_camera), Mat4.from_np(prev_inverse_camera)
    p.fovy, p.aspect, p.znear, p.zfar = float(fovy), float(aspect), float(znear), float(zfar)
    p.max_count, p.plane_tolerance, p.reset, p.reserved = int(max_count), float(plane_tolerance), int(reset), 0
    return p


def shadow_mask_accumulate(depth, normal, velocity, prev_depth, mask, history, history_count, params, out_history, out_count, out_mask, stream=None):
    """vkr_shadow_mask_accumulate: out_history (RGBA16_UNORM), out_count (R8_UNORM) and out_mask (RGBA8_UNORM) := per pixel the
    running mean of `mask` (RGBA8_UNORM) with the `history` / `history_count` of the texel its `velocity` (RG16_SFLOAT) points at,
    where `prev_depth` through params.prev_inverse_camera lies on the pixel's surface as `depth` (D24_UNORM_S8, mip 0) and `normal`
    (RG16_UNORM) tell it; all VkrImg of one extent, under `params` (ShadowAccumParams, e.g. shadow_accum_params(...)).  Raises
    RuntimeError with the library's message on a refusal."""
    lib = product()
    ref = lambda d: C.byref(d) if d is not None else None
    check(lib.vkr_shadow_mask_accumulate(ref(depth), ref(normal), ref(velocity), ref(prev_depth), ref(mask), ref(history), ref(history_count),
                                         ref(params), ref(out_history), ref(out_count), ref(out_mask), stream), lib)


def shadow_disk_samples_frame(sample_count, pattern_side, frame, frames):
    """vkr_shadow_disk_samples_frame: the table of shadow_disk_samples for frame `frame` of a cycle of `frames`:
    float32 [pattern_side^2, sample_count, 2]; frames == 1 is shadow_disk_samples bit for bit"""
    import numpy as np

    if not (1 <= int(sample_count) <= 64 and int(pattern_side) in (1, 2, 4) and 1 <= int(frames) <= 64):
        raise RuntimeError(f"shadow_disk_samples_frame: sample_count {sample_count} (1..64), pattern_side {pattern_side} (1, 2 or 4), frames {frames} (1..64)")
    out = np.zeros((int(pattern_side) ** 2, int(sample_count), 2), np.float32)
    product().vkr_shadow_disk_samples_frame(int(sample_count), int(pattern_side), int(frame), int(frames), out.ctypes.data)
    return out


def reflections_rt_cutout(depth, normal, rays, accel, attribs, attrib_count, textures, texture_count, params, cutout, out_reflections, scratch,
                          scratch_bytes, stream=None):
    """vkr_reflections_rt_cutout: reflections_rt whose mirror rays pass through the holes of alpha-tested triangles (cutout: a
    RayCutout); everything else as reflections_rt.  Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    ref = lambda d: C.byref(d) if d is not None else None
    handle = accel.handle if accel is not None else None
    check(lib.vkr_reflections_rt_cutout(ref(depth), ref(normal), ref(rays), handle, attribs, int(attrib_count), textures, int(texture_count),
                                        ref(params), ref(cutout), ref(out_reflections), scratch, int(scratch_bytes), stream), lib)


def hit_normal_dtype():
    """the numpy dtype of vkr_hit_normal (48 bytes): the world-space normals of a triangle's three vertices, .w unused"""
    import numpy as np

    return np.dtype([("n", np.float32, (3, 4))])


def reflect_lights(lights=(), colours=(), ambient=(1.0, 1.0, 1.0), shadow_offset=REFLECT_SHADOW_OFFSET, shadow_tmin=REFLECT_SHADOW_TMIN):
    """ReflectLights from 0..4 lights of (x, y, z, w) (the convention of shadow_rt_params), one rgb colour per light, the ambient rgb
    and the two offsets of the shadow ray cast from a hit.  Everything is passed on as given (the entry refuses what it does not
    take).  Without lights and with the default ambient the lit pass stores what reflections_rt stores."""
    if len(lights) > 4 or len(colours) != len(lights):
        raise RuntimeError(f"reflect_lights: {len(lights)} lights and {len(colours)} colours, at most 4 and as many of one as of the other")
    p = ReflectLights()
    for l, (v, c) in enumerate(zip(lights, colours)):
        for k in range(4):
            p.lights[l][k] = float(v[k])
        for k in range(3):
            p.colour[l][k] = float(c[k])
    for k in range(3):
        p.ambient[k] = float(ambient[k])
    p.light_count, p.shadow_offset, p.shadow_tmin = len(lights), float(shadow_offset), float(shadow_tmin)
    return p


def reflections_rt_lit(depth, normal, rays, accel, attribs, attrib_count, normals, normal_count, textures, texture_count, params, lights,
                       out_reflections, scratch, scratch_bytes, stream=None):
    """vkr_reflections_rt_lit: reflections_rt whose hit is lit by `lights` (a ReflectLights, e.g. reflect_lights(...)) and shadowed
    by one ray per light from the hit; normals: device pointer (16-byte aligned) to normal_count vkr_hit_normal records
    (scene_triangle_normals order); everything else as reflections_rt.  Raises RuntimeError with the library's message on a
    refusal."""
    lib = product()
    ref = lambda d: C.byref(d) if d is not None else None
    handle = accel.handle if accel is not None else None
    check(lib.vkr_reflections_rt_lit(ref(depth), ref(normal), ref(rays), handle, attribs, int(attrib_count), normals, int(normal_count), textures,
                                     int(texture_count), ref(params), ref(lights), ref(out_reflections), scratch, int(scratch_bytes), stream), lib)


def reflections_rt_lit_cutout(depth, normal, rays, accel, attribs, attrib_count, normals, normal_count, textures, texture_count, params, lights,
                              cutout, out_reflections, scratch, scratch_bytes, stream=None):
    """vkr_reflections_rt_lit_cutout: reflections_rt_lit whose mirror rays and shadow rays pass through the holes of alpha-tested
    triangles (cutout: a RayCutout).  Raises RuntimeError with the library's message on a refusal."""
    lib = product()
    ref = lambda d: C.byref(d) if d is not None else None
    handle = accel.handle if accel is not None else None
    check(lib.vkr_reflections_rt_lit_cutout(ref(depth), ref(normal), ref(rays), handle, attribs, int(attrib_count), normals, int(normal_count),
                                            textures, int(texture_count), ref(params), ref(lights), ref(cutout), ref(out_reflections), scratch,
                                            int(scratch_bytes), stream), lib)


def defered_shading_shadowed(albedo, normal, material, depth, consts, occlusion, brdf, reflections, shadow_mask, out, push, stream=None):
    """vkr_defered_shading_shadowed: vkr_defered_shading (same VkrImg bindings, ShadingParams and ShadingPush) with channel .x of
    `shadow_mask` (RGBA8_UNORM VkrImg at out's extent) on the direct term.  Raises RuntimeError with the library's message on a
    refusal."""
    lib = product()
    check(lib.vkr_defered_shading_shadowed(C.byref(albedo), C.byref(normal), C.byref(material), C.byref(depth), C.byref(consts),
                                           C.byref(occlusion), C.byref(brdf), C.byref(reflections), C.byref(shadow_mask), C.byref(out),
                                           C.byref(push), stream), lib)


COMM_ID_BYTES = 128
# measurement switches (include/vkr_postfx.h VKR_SWITCH_*): vkr_get_switches / vkr_set_switches
SWITCH_BLUR_NO_SKIP, SWITCH_FILTER_NO_SKIP, SWITCH_TAA_GENERIC, SWITCH_SHADING_GENERIC, SWITCH_BLUR_GENERIC, SWITCH_TRACE_ONE_LAUNCH, SWITCH_BLUR_LANE_LOOPS = 1, 2, 4, 8, 16, 32, 64
SWITCH_MIPS_PER_LEVEL, SWITCH_MIPS_FUSED = 128, 256  # vkr_gen_mipmaps: force one launch per level / the fused tiles (same bytes)
SWITCH_BLUR_NO_FLAT, SWITCH_BLUR_COUNT_PATHS = 512, 1024  # the blur without its constant-normal-weight loops / counting blocks per path


def debug_blur_paths(reset=True):
    """vkr_debug_blur_paths: (empty, lit flat, lit not flat, blocks with a wave on a flat loop) counted by the blur launches that
    ran with SWITCH_BLUR_COUNT_PATHS since the last reset."""
    lib = product()
    out = (C.c_uint32 * 4)()
    check(lib.vkr_debug_blur_paths(out, 1 if reset else 0), lib)
    return tuple(int(v) for v in out)


class Comm:
    """RCCL communicator of the C-ABI (include/vkr_postfx.h vkr_comm_*): the wire of the multi-GPU frame.  Rank 0 makes
    the id, `share` hands its bytes to every rank out of band (e.g. torch.distributed.broadcast_object_list over gloo),
    then every rank creates the communicator collectively with its device current.

    Every rank takes the same branch whatever fails where (a mismatch would leave the others blocked in a collective):
      * `agree(ok)` — optional, a collective AND over the ranks on the control plane — is asked whether RCCL loads on
        EVERY rank before anything collective happens;
      * every rank always calls `share` (rank 0 with None when it could not make the id) and raises after it;
      * `self_check(agree)` verifies a fresh communicator by moving known bytes through all three exchanges."""

    def __init__(self, rank, world, share, agree=None):
        lib = product()
        self.handle, self.rank, self.world = None, rank, world
        available = lib.vkr_comm_available() == 0
        why = "" if available else (lib.vkr_last_error() or b"").decode()
        if agree is not None and not agree(available):
            raise RuntimeError("RCCL is not available on every rank" + (f" (this rank: {why})" if why else ""))
        ident = None
        if rank == 0:
            buf = (C.c_uint8 * COMM_ID_BYTES)()
            if available and lib.vkr_comm_unique_id(buf) == 0:
                ident = bytes(buf)
            else:
                why = (lib.vkr_last_error() or b"").decode()
        ident = share(ident)  # rank 0 always reaches this, so nobody waits for an id that never comes
        if ident is None:
            raise RuntimeError("rank 0 could not make a communicator id" + (f": {why}" if why else ""))
        if not available:  # only without `agree`: the ranks that do have RCCL are about to block in vkr_comm_create — pass `agree`
            raise RuntimeError(f"RCCL is not available on this rank: {why}")
        assert len(ident) == COMM_ID_BYTES
        h = C.c_void_p(0)
        check(lib.vkr_comm_create((C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(ident), rank, world, C.byref(h)), lib)
        self.handle = h.value

    @classmethod
    def emulated(cls, rank, world, link_gbps=60.0, launch_us=15.0):
        """vkr_comm_create_emulated: moves nothing, holds the stream for the wire's time (tools/wire_emulation.py)"""
        self = cls.__new__(cls)
        lib = product()
        h = C.c_void_p(0)
        check(lib.vkr_comm_create_emulated(rank, world, link_gbps, launch_us, C.byref(h)), lib)
        self.handle = h.value
        return self

    def self_check(self, device, agree=None):
        """Moves rank-tagged patterns through vkr_all_gather, vkr_all_gather_v and vkr_halo_exchange and verifies every
        received byte (vkr_comm_selfcheck).  Returns True when the wire delivers what the tiled frame expects — on
        every rank, if `agree` (collective AND) is given."""
        import torch

        lib = product()
        lib.vkr_comm_selfcheck_bytes.argtypes = [C.c_int]
        lib.vkr_comm_selfcheck_bytes.restype = C.c_uint64
        lib.vkr_comm_selfcheck.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        scratch = torch.empty(int(lib.vkr_comm_selfcheck_bytes(self.world)), dtype=torch.uint8, device=device)
        stream = torch.cuda.current_stream(device)
        ok = lib.vkr_comm_selfcheck(C.c_void_p(self.handle), C.c_void_p(scratch.data_ptr()), C.c_void_p(stream.cuda_stream)) == 0
        self.self_check_error = "" if ok else (lib.vkr_last_error() or b"").decode()
        return agree(ok) if agree is not None else ok

    def close(self):
        if self.handle:
            check(product().vkr_comm_destroy(C.c_void_p(self.handle)), product())
            self.handle = None


# ---- the scene's acceleration structure, for tests and tools -------------------------------------------------------------
def scene_triangles(sc):
    """World-space triangles of a scene.Scene as (n, 3, 3) float32, in the order the host mirror's
    scene::SceneAccelerationStructure puts them into its structure (draw by draw, the draw's index range, vertex_offset added
    to every index), each vertex transformed in fp32 as ((m00 x + m01 y) + m02 z) + m03 per row (scene/scene_as.hpp)."""
    import numpy as np

    out = []
    for d in sc.draws:
        m = np.asarray(sc.transforms[d["transform"]][0], dtype=np.float32)
        n = d["index_count"] // 3 * 3
        idx = sc.indices[d["index_offset"]:d["index_offset"] + n].astype(np.int64) + d["vertex_offset"]
        p = sc.vertices[idx, :3].astype(np.float32)
        w = np.empty_like(p)
        for r in range(3):
            w[:, r] = ((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3]
        out.append(w.reshape(-1, 3, 3))
    return np.concatenate(out) if out else np.zeros((0, 3, 3), np.float32)


def scene_triangle_attributes(sc):
    """One vkr_hit_attrib per triangle of scene_triangles(sc), in its order, as a numpy array of hit_attrib_dtype(): the uv of the
    triangle's three vertices and the draw's albedo texture index (0xFFFFFFFF: none).  A mesh drawn by several nodes yields one
    record per instance (scene/scene_as.hpp)."""
    import numpy as np

    out = []
    for d in sc.draws:
        n = d["index_count"] // 3 * 3
        idx = sc.indices[d["index_offset"]:d["index_offset"] + n].astype(np.int64) + d["vertex_offset"]
        rec = np.zeros(n // 3, hit_attrib_dtype())
        rec["uv"] = sc.vertices[idx, 6:8].astype(np.float32).reshape(-1, 3, 2)
        rec["albedo_index"] = np.uint32(d["albedo"] & 0xFFFFFFFF)
        out.append(rec)
    return np.concatenate(out) if out else np.zeros(0, hit_attrib_dtype())


def scene_triangle_normals(sc):
    """One vkr_hit_normal per triangle of scene_triangles(sc), in its order, as a numpy array of hit_normal_dtype(): the normals of
    the triangle's three vertices under the draw's normal matrix, (m[r][0] x + m[r][1] y) + m[r][2] z per row in fp32 (no
    translation, nothing fused), not normalised; .w is 0."""
    import numpy as np

    out = []
    for d in sc.draws:
        m = np.asarray(sc.transforms[d["transform"]][1], dtype=np.float32)
        n = d["index_count"] // 3 * 3
        idx = sc.indices[d["index_offset"]:d["index_offset"] + n].astype(np.int64) + d["vertex_offset"]
        p = sc.vertices[idx, 3:6].astype(np.float32)
        rec = np.zeros(n // 3, hit_normal_dtype())
        w = np.zeros((n, 4), np.float32)
        for r in range(3):
            w[:, r] = (m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]
        rec["n"] = w.reshape(-1, 3, 4)
        out.append(rec)
    return np.concatenate(out) if out else np.zeros(0, hit_normal_dtype())


def accel_layout(triangles):
    """vkr_accel_layout on the host (no GPU): -> (nodes, tris) as numpy structured copies of the records"""
    import numpy as np

    tri = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    n = len(tri)
    cap = max(1, 2 * n - 1)
    nodes = (AccelNode * cap)()
    recs = (AccelTri * max(1, n))()
    count = C.c_uint32(0)
    lib = product()
    check(lib.vkr_accel_layout(tri.ctypes.data if n else None, n, nodes, cap, recs, C.byref(count)), lib)
    node_arr = np.frombuffer(bytes(nodes), dtype=np.uint8).reshape(cap, C.sizeof(AccelNode))[:count.value].copy()
    tri_arr = np.frombuffer(bytes(recs), dtype=np.uint8).reshape(max(1, n), C.sizeof(AccelTri))[:n].copy()
    return node_arr, tri_arr


def accel_refit_layout(nodes, tris, triangles):
    """vkr_accel_refit_layout on the host (no GPU): the arrays of accel_layout() (or Accel.download()) refitted to `triangles`
    ((n, 3, 3) float32 in input order) -> (nodes, tris), new arrays; the arguments are left as they are.  Raises RuntimeError
    where the library refuses the topology."""
    import numpy as np

    # any array of the records' bytes: the uint8 rows of accel_layout() or a structured view of them
    node_arr = np.frombuffer(np.ascontiguousarray(nodes).tobytes(), dtype=np.uint8).reshape(-1, C.sizeof(AccelNode)).copy()
    tri_arr = np.frombuffer(np.ascontiguousarray(tris).tobytes(), dtype=np.uint8).reshape(-1, C.sizeof(AccelTri)).copy()
    tri = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    lib = product()
    check(lib.vkr_accel_refit_layout(node_arr.ctypes.data if len(node_arr) else None, len(node_arr), tri_arr.ctypes.data if len(tri_arr) else None,
                                     len(tri_arr), tri.ctypes.data if len(tri) else None), lib)
    return node_arr, tri_arr


def scene_triangles_scratch_bytes(draw_count):
    """vkr_scene_triangles_scratch_bytes: the device scratch of one vkr_scene_triangles call (the draw table)"""
    return int(product().vkr_scene_triangles_scratch_bytes(int(draw_count)))


def scene_world_triangles(raster_scene, triangle_count, device="cuda", stream=None):
    """vkr_scene_triangles: the world-space triangles of a RasterScene (scene.Scene.to_device()'s descriptor, or one a test made)
    as a device tensor (triangle_count, 3, 3) float32 — scene_triangles() computed on the device, in its order.  A triangle with an
    index outside the vertex buffer is three NaN vertices."""
    import torch

    out = torch.zeros((int(triangle_count), 3, 3), dtype=torch.float32, device=device)
    nbytes = scene_triangles_scratch_bytes(raster_scene.draw_count)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    lib = product()
    check(lib.vkr_scene_triangles(C.byref(raster_scene), out.data_ptr(), int(triangle_count), scratch.data_ptr(), nbytes, stream), lib)
    # the call is asynchronous; the scratch tensor may be released only once the stream has passed it
    (torch.cuda.current_stream(out.device) if stream is None else torch.cuda.ExternalStream(stream)).synchronize()
    return out


def scene_world_normals(raster_scene, triangle_count, device="cuda", stream=None):
    """vkr_scene_triangle_normals: the vertex normals of a RasterScene's triangles as a device tensor (triangle_count, 3, 4) float32
    — scene_triangle_normals() computed on the device, in its order.  A triangle with an index outside the vertex buffer is three
    NaN normals."""
    import torch

    out = torch.zeros((int(triangle_count), 3, 4), dtype=torch.float32, device=device)
    nbytes = scene_triangles_scratch_bytes(raster_scene.draw_count)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    lib = product()
    check(lib.vkr_scene_triangle_normals(C.byref(raster_scene), out.data_ptr(), int(triangle_count), scratch.data_ptr(), nbytes, stream), lib)
    # the call is asynchronous; the scratch tensor may be released only once the stream has passed it
    (torch.cuda.current_stream(out.device) if stream is None else torch.cuda.ExternalStream(stream)).synchronize()
    return out


class Accel:
    """vkr_accel_create / _destroy around world-space triangles ((n, 3, 3) float32, e.g. scene_triangles(sc))."""

    def __init__(self, triangles):
        import numpy as np

        tri = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
        self.lib = product()
        self.handle = C.c_void_p()
        check(self.lib.vkr_accel_create(tri.ctypes.data if len(tri) else None, len(tri), C.byref(self.handle)), self.lib)

    @classmethod
    def from_scene(cls, sc):
        return cls(scene_triangles(sc))

    def info(self):
        nodes, tris = C.c_uint32(0), C.c_uint32(0)
        check(self.lib.vkr_accel_info(self.handle, C.byref(nodes), C.byref(tris)), self.lib)
        return nodes.value, tris.value

    def query(self, origins, dirs, tmin, tmax, out, stream=None):
        """origins, dirs: device tensors (n, 3) float32; out: device tensor (n,) int32 / uint32"""
        n = int(origins.shape[0])
        check(self.lib.vkr_accel_query(self.handle, origins.data_ptr(), dirs.data_ptr(), float(tmin), float(tmax), n, out.data_ptr(), stream), self.lib)

    def occluded(self, origins, dirs, tmin, tmax, out, stream=None):
        """vkr_accel_occluded: query() on the walk with the per-ray cull (long rays); the same answers"""
        n = int(origins.shape[0])
        check(self.lib.vkr_accel_occluded(self.handle, origins.data_ptr(), dirs.data_ptr(), float(tmin), float(tmax), n, out.data_ptr(), stream), self.lib)

    def closest(self, origins, dirs, tmin, tmax, out, stream=None):
        """vkr_accel_closest: origins, dirs as query(); out: device tensor of n 16-byte records (e.g. (n, 4) int32): t, u, v as
        float32 bits and the index of the input triangle, 0xFFFFFFFF for a miss (numpy: accel_hit_dtype())"""
        n = int(origins.shape[0])
        check(self.lib.vkr_accel_closest(self.handle, origins.data_ptr(), dirs.data_ptr(), float(tmin), float(tmax), n, out.data_ptr(), stream), self.lib)

    def refit(self, triangles, stream=None):
        """vkr_accel_refit: triangles: device tensor (n, 3, 3) / (n, 9) float32, contiguous, n = info()[1], in the order of the
        triangles this structure was created from.  Asynchronous on `stream`: what is queued there afterwards sees the new pose;
        the tensor must stay alive and unchanged until then."""
        import torch

        tris = self.info()[1]
        if tris and not (triangles.is_cuda and triangles.dtype == torch.float32 and triangles.is_contiguous() and triangles.numel() == 9 * tris):
            raise ValueError(f"refit: a contiguous float32 device tensor of 9 floats for each of the structure's {tris} triangles")
        check(self.lib.vkr_accel_refit(self.handle, triangles.data_ptr() if triangles is not None and tris else None, stream), self.lib)

    def download(self, stream=None):
        """vkr_accel_download (synchronises `stream`): -> (nodes, tris) as accel_layout() returns them"""
        import numpy as np

        n, t = self.info()
        nodes = np.zeros((n, C.sizeof(AccelNode)), np.uint8)
        tris = np.zeros((t, C.sizeof(AccelTri)), np.uint8)
        check(self.lib.vkr_accel_download(self.handle, nodes.ctypes.data if n else None, n, tris.ctypes.data if t else None, t, stream), self.lib)
        return nodes, tris

    def refit_schedule(self):
        """vkr_accel_refit_schedule: -> (level_sizes, tail_nodes): the number of nodes of every height and the size up to which a
        level is left to the single-workgroup tail launch of refit()"""
        sizes = (C.c_uint32 * 64)()
        count, tail = C.c_uint32(0), C.c_uint32(0)
        check(self.lib.vkr_accel_refit_schedule(self.handle, sizes, 64, C.byref(count), C.byref(tail)), self.lib)
        return list(sizes[:count.value]), tail.value

    def close(self):
        if self.handle:
            self.lib.vkr_accel_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
