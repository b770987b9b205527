/*
 * vkr_postfx.h — C-ABI of the MI355X post-process hot path (Hi-Z / SSR / GTAO / TAA).
 *
 * One entry point per reference compute/fragment *program* (src/shaders/config.json)
 * on the hot path.  Arguments follow the reference shader's binding order: POD image
 * views for sampled / storage images, a pointer to the exact UBO struct the reference
 * uploads, the exact push-constant struct, then the HIP stream.  Plain pointers and
 * sizes only; no torch / Vulkan / glm types.
 *
 * Conventions
 *   - all image memory is device (HBM) memory, pitch-linear, rows 256-B aligned,
 *     4 / 8 bytes per texel in the reference's storage format (vkr_format);
 *   - every call is asynchronous on `stream`; returns 0 or a non-zero hipError_t-style
 *     code (message via vkr_last_error()); nothing is allocated inside a call;
 *   - UBO / push-constant structs are read on the host at call time (they become
 *     kernel arguments), so they may live on the caller's stack;
 *   - a `vkr_img` is a *view*: mip 0 of the view is the first mip the reference binds
 *     (e.g. GTAO binds depth image-mip 1 as a 1-mip view, gtao.cpp:119);
 *   - multi-GPU tiling: an image may hold only a window of the frame.  `full_width/
 *     full_height` is the whole frame's extent at view-mip 0, `origin_x/origin_y` the
 *     window's position in it.  Single GPU: origin 0, full == width/height.  Output
 *     images define the set of pixels a kernel computes (their window).
 */
#ifndef VKR_POSTFX_H_INCLUDED
#define VKR_POSTFX_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VKR_MAX_MIPS 16
#define VKR_HALTON_SEQ_SIZE 128  /* advanced_ssr.cpp:6, trace.comp:18 */

/* Storage formats used by the path (scene_renderer.cpp:13-43, gtao.cpp:26-47,
 * advanced_ssr.cpp:62-92, taa.cpp:6).  Values are ours, not VkFormat. */
typedef enum vkr_format {
  VKR_FMT_UNDEFINED      = 0,
  VKR_FMT_D24_UNORM_S8   = 1,  /* uint32: depth in bits 0..23, stencil 24..31      */
  VKR_FMT_RG16_UNORM     = 2,  /* 2 x uint16                                       */
  VKR_FMT_RG16_SFLOAT    = 3,  /* 2 x fp16                                         */
  VKR_FMT_RGBA8_SRGB     = 4,  /* 4 x uint8, rgb sRGB-encoded, a linear            */
  VKR_FMT_RGBA8_UNORM    = 5,  /* 4 x uint8                                        */
  VKR_FMT_RGBA16_UNORM   = 6,  /* 4 x uint16                                       */
  VKR_FMT_RGBA16_SFLOAT  = 7,  /* 4 x fp16                                         */
  VKR_FMT_R16_SFLOAT     = 8,  /* 1 x fp16                                         */
  VKR_FMT_R32_SFLOAT     = 9,  /* 1 x fp32                                         */
  VKR_FMT_R8_UNORM       = 10, /* 1 x uint8 (create_gtao_texture, gtao.cpp:10)     */
  VKR_FMT_RGBA32_SFLOAT  = 11, /* 4 x fp32: AdvancedSSR::tile_planes (advanced_ssr.cpp:85), written by vkr_tile_regression */
  VKR_FMT_R16_UNORM      = 12  /* 1 x uint16: the octahedral probe depth (probe_renderer.cpp:284,302) */
} vkr_format;

/* bytes per texel of a vkr_format (0 for unknown) */
uint32_t vkr_format_bytes(uint32_t format);

typedef struct vkr_img {
  void*    base;                       /* device pointer, start of view-mip 0       */
  uint32_t format;                     /* vkr_format                                */
  uint32_t mip_count;                  /* mips in this view (>=1)                   */
  uint32_t width, height;              /* extent of view-mip 0 held in memory       */
  uint32_t full_width, full_height;    /* extent of view-mip 0 of the whole frame   */
  int32_t  origin_x, origin_y;         /* window origin inside the frame, view-mip 0*/
  uint32_t pitch_bytes[VKR_MAX_MIPS];  /* row pitch of each mip: < 16 MiB, rows < 2^24, and pitch x rows of the mip < 4 GiB (the kernels
                                          address texels with 32-bit offsets; VKR_ERR_LAYOUT otherwise)  */
  uint64_t mip_offset[VKR_MAX_MIPS];   /* byte offset of each mip from `base`       */
} vkr_img;

/* 4x4 column-major float matrix, memory-compatible with glm::mat4 */
typedef struct vkr_mat4 { float m[16]; } vkr_mat4;

/* ---- UBO structs, byte-compatible with what the reference uploads ------------------ */

/* GTAOParams, gtao.hpp:12-18 / main.comp:7-13 */
typedef struct vkr_gtao_params {
  vkr_mat4 normal_mat;
  float fovy, aspect, znear, zfar;
} vkr_gtao_params;

/* push constants of gtao_compute_main, gtao.cpp:101-113 / main.comp:20-26 */
typedef struct vkr_gtao_push {
  float    angle_offset;
  float    weight_ratio;
  uint32_t use_mis;
  uint32_t two_directions;
  uint32_t reflections_only;
} vkr_gtao_push;

/* push constants of gtao_filter, gtao.cpp:210-215 / filter.comp:12-15 */
typedef struct vkr_gtao_filter_push { float znear, zfar; } vkr_gtao_filter_push;

/* AccumConstants, gtao.cpp:300-305 / accum.comp:16-21 */
typedef struct vkr_gtao_accum_params {
  vkr_mat4 inverse_camera;
  vkr_mat4 prev_inverse_camera;
  vkr_mat4 mvp;
  float    fovy_aspect_znear_zfar[4];
} vkr_gtao_accum_params;

typedef struct vkr_gtao_accum_push { uint32_t clear_history; } vkr_gtao_accum_push;

/* TraceParams, advanced_ssr.cpp:138-145 / trace.comp:9-16 (std140: mat4, uint, 4 floats) */
typedef struct vkr_trace_params {
  vkr_mat4 normal_mat;
  uint32_t frame_random;
  float fovy, aspect, znear, zfar;
} vkr_trace_params;

typedef struct vkr_trace_push  { float max_roughness; } vkr_trace_push;     /* trace.comp:24-26  */
typedef struct vkr_filter_push { uint32_t render_flags; } vkr_filter_push;  /* filter.comp:28-30 */
/* multi-GPU trace: `normal` holds frame rows [normal_row0, normal_row1) only when the march ends (vkr_sssr_trace_windowed) */
typedef struct vkr_trace_window_push { float max_roughness; uint32_t normal_row0, normal_row1; } vkr_trace_window_push;
#define VKR_NORMALIZE_REFLECTIONS  1u   /* filter.comp:22-24 */
#define VKR_ACCUMULATE_REFLECTIONS 2u
#define VKR_BILATERAL_FILTER       4u

/* blur.comp:16-20 / advanced_ssr.cpp:388-392 */
typedef struct vkr_blur_push {
  float    max_roughness;
  uint32_t accumulate;
  uint32_t disable_blur;
} vkr_blur_push;

/* ReprojectConsts (blur.comp:22-26) == TAAUniforms (resolve.comp:11-15, taa.cpp:24-28) */
typedef struct vkr_reproject_params {
  vkr_mat4 inverse_camera;
  vkr_mat4 prev_inverse_camera;
  float    fovy_aspect_znear_zfar[4];
} vkr_reproject_params;

/* SSRParams of the simple SSR pass, ssr.hpp:8-15 / ssr/shader.frag:9-16 */
typedef struct vkr_ssr_params {
  vkr_mat4 normal_mat;
  float fovy, aspect, znear, zfar;
} vkr_ssr_params;

/* ShaderConstants of the deferred-shading composite, defered_shading.cpp:4-12 / shader.frag:15-23 */
typedef struct vkr_shading_params {
  vkr_mat4 inverse_camera;
  vkr_mat4 camera;
  vkr_mat4 shadow_mvp;
  float fovy, aspect, znear, zfar;
} vkr_shading_params;

/* push constants, defered_shading.cpp:68-72 / shader.frag:30-33 (vec2 + uint) */
typedef struct vkr_shading_push {
  float    min_max_roughness[2];
  uint32_t show_ao;
} vkr_shading_push;

/* ---- tile-classified trace -------------------------------------------------- */
/* classification.comp:26-30 (advanced_ssr.cpp:463-471)                                             */
typedef struct vkr_classification_push { int32_t width, height; float max_roughness, glossy_value; } vkr_classification_push;
/* trace_indirect.comp:25-28 (advanced_ssr.cpp:231-236)                                             */
typedef struct vkr_trace_indirect_push { uint32_t reflection_type; float max_roughness; } vkr_trace_indirect_push;

/* ---- dormant GTAO variants ------------------------------------------- */
/* gtao/main.frag:17-19 push constants (gtao.cpp:355-357)                                           */
typedef struct vkr_gtao_gfx_push { float angle_offset; } vkr_gtao_gfx_push;
/* gtao/reproject.comp:11-17 == GTAOReprojection (gtao.hpp:28-34)                                   */
typedef struct vkr_gtao_reprojection {
  vkr_mat4 camera_to_prev_frame;
  float fovy, aspect, znear, zfar;
} vkr_gtao_reprojection;
/* gtao_opt/deinterleave.comp:6-8 (gtao.cpp:464)                                                    */
typedef struct vkr_deinterleave_push { int32_t pattern_step; } vkr_deinterleave_push;
/* gtao_opt/main_deinterleaved.comp:17-21 (gtao.cpp:474-478)                                        */
typedef struct vkr_gtao_deinterleaved_push { int32_t pattern_n; uint32_t layer; float angle_offset; } vkr_gtao_deinterleaved_push;

/* ---- ScreenSpaceTrace ------------------------------------------------- */
/* screen_trace/trace.comp:14-22 == GpuParams (screen_trace.cpp:30-38)                              */
typedef struct vkr_screen_trace_params {
  vkr_mat4 normal_mat;
  float random_offset, angle_offset, fovy, aspect, znear, zfar;
} vkr_screen_trace_params;
/* screen_trace/filter.comp:8-11 (screen_trace.cpp:103-106)                                         */
typedef struct vkr_screen_trace_filter_push { float znear, zfar; } vkr_screen_trace_filter_push;
/* screen_trace/accumulate.comp:7-12 (screen_trace.cpp:148-153)                                     */
typedef struct vkr_screen_trace_accum_push { float fovy, aspect, znear, zfar; } vkr_screen_trace_accum_push;

/* ---- G-buffer raster stage --------------------------------------------------- */
/* scene::Vertex, scene/scene.hpp:15-19                                                              */
typedef struct vkr_raster_vertex { float pos[3], norm[3], uv[2]; } vkr_raster_vertex;
/* Transform, gbuf/opaque_taa.vert:15-18                                                             */
typedef struct vkr_raster_transform { vkr_mat4 model, normal; } vkr_raster_transform;
/* one draw_indexed of scene_renderer.cpp:196-214 with its push constants (:132-137)                 */
typedef struct vkr_raster_draw {
  uint32_t transform_index, albedo_index, mr_index, flags;   /* PushData; 0xFFFFFFFF = no texture    */
  uint32_t index_offset, index_count, vertex_offset, reserved;  /* reserved: VKR_RASTER_DRAW_* hints */
} vkr_raster_draw;
/* opaque_taa.frag:32-34 discards fragments whose filtered albedo alpha is 0 (no depth, no colour written); the stage
 * evaluates that for every draw with an albedo texture.  Hint: the caller guarantees that no texel of any mip level of
 * the draw's albedo texture has alpha 0, so the discard cannot fire and the test is skipped (same result, cheaper). */
#define VKR_RASTER_DRAW_OPAQUE_ALBEDO 1u
/* GbufConst, scene_renderer.cpp:148-153 / opaque_taa.vert:7-12                                      */
typedef struct vkr_gbuf_const {
  vkr_mat4 view_projection, prev_view_projection;
  float    jitter[4];
  float    fovy_aspect_znear_zfar[4];
} vkr_gbuf_const;
/* vertices / indices / transforms: device memory; draws and textures: host arrays (launch params).
 * Textures are RGBA8_SRGB images with full mip chains (scene/images.cpp:32-49), sampled with the
 * scene sampler (scene_renderer.cpp:77-81: bilinear, linear mip, REPEAT).                          */
typedef struct vkr_raster_scene {
  const vkr_raster_vertex*    vertices;   uint32_t vertex_count;
  const uint32_t*             indices;    uint32_t index_count;
  const vkr_raster_transform* transforms; uint32_t transform_count;
  const vkr_raster_draw*      draws;      uint32_t draw_count;
  const vkr_img*              textures;   uint32_t texture_count;
} vkr_raster_scene;

/* Parameters of the synthetic G-buffer generator (replaces the raster stage
 * scene_renderer.cpp:140-220 + gbuf/opaque_taa.{vert,frag}). */
typedef struct vkr_synth_params {
  vkr_mat4 camera_to_world;   /* inverse view matrix of the frame being generated    */
  vkr_mat4 prev_mvp;          /* projection * previous view (velocity, opaque_taa.vert)*/
  vkr_mat4 mvp;               /* projection * current view                           */
  float    fovy, aspect, znear, zfar;
  uint32_t seed;              /* PCG32 stream for the checker / per-object material  */
  uint32_t flags;             /* VKR_SYNTH_*                                          */
} vkr_synth_params;
#define VKR_SYNTH_DEPTH_ONLY 1u          /* depth attachment only (used for prev_depth)                                        */
/* Second material mode: the roughness of an object is perturbed PER TEXEL (+-0.15, PCG hash of the pixel), like a roughness
 * texture: the blur's sigma (blur.comp:44-75) and the trace's lobe then vary inside every wavefront.  The default scene has
 * one roughness per object, which the SSR blur's wave-uniform-sigma path and empty-tile skips exploit.                    */
#define VKR_SYNTH_TEXTURED_ROUGHNESS 2u

/* ---- entry points ------------------------------------------------------------------- */

const char* vkr_version(void);
const char* vkr_last_error(void);
/* Version of the numeric contract the library was built with (csrc/vkr_device.hpp): 2 = the accumulation steps of the
 * shared helpers (dot, mix, mat4*vec4, cross, madd, texel coordinates ...) are fused multiply-adds, which GLSL without
 * `precise` allows every Vulkan driver to do; 1 = nothing fused (`make CONTRACT=1`).  Results of the two contracts
 * differ in the last bits; a checker must be built with the same one.                                              */
uint32_t vkr_numeric_contract(void);

/* program "downsample_gbuffer": downsample_pass.cpp:25-92 + downsample_gbuffer.frag:12-37.
 * depth: full image (view mip 0 = image mip 0, >=2 mips); writes depth mip 1.           */
int vkr_downsample_gbuffer(const vkr_img* depth, const vkr_img* normal, const vkr_img* velocity,
                           const vkr_img* out_normal, const vkr_img* out_velocity, void* stream);

/* program "depth_mips": downsample_pass.cpp:94-131 + depth_mips.frag:7-15.
 * Builds mips src_mip+1 .. mip_count-1, each the 2x2 min of its parent.                 */
int vkr_depth_mips(const vkr_img* depth, uint32_t src_mip, void* stream);

/* program "pdf_preintegrate": advanced_ssr.cpp:95-114 + preintegrate.comp:45-84          */
int vkr_pdf_preintegrate(const vkr_img* out_pdf, void* stream);

/* Fills the HaltonBuffer UBO of sssr_trace (host memory, `count` x vec4): xy = Halton(2,3) of index
 * i+1 exactly as advanced_ssr.cpp:8-34 builds it; zw — unused (0) in the reference — carry
 * (float)cos((double)phi), (float)sin((double)phi) with phi = (2*PI)*y, the two transcendentals
 * sampleGGXVNDF (brdf.glsl:146-148) needs per ray: 128 values evaluated once on the host instead
 * of per pixel on the device.  vkr_sssr_trace requires a buffer filled by this function.          */
void vkr_halton23_fill(float* host_vec4, uint32_t count);

/* program "sssr_trace": advanced_ssr.cpp:147-214 + trace.comp (bindings 0..7)            */
int vkr_sssr_trace(const vkr_img* depth, const vkr_img* normal, const vkr_img* material,
                   const vkr_trace_params* params, const float* halton_vec4 /*device, 128 x vec4*/,
                   const vkr_img* out_ray, const vkr_img* out_occlusion, const vkr_img* pdf_tex,
                   const vkr_trace_push* push, void* stream);

/* "sssr_trace" in two launches, same images as vkr_sssr_trace bit for bit.  The head launch runs every ray's prologue, its 16
 * pinned steps and `park_after_rounds` (0..4) of the compacted 16-step rounds, and finishes the pixels whose rays have ended;
 * a ray that has not is PARKED: written, with what the rest of its march and its epilogue need (80 bytes), to a frame-wide
 * queue in `workspace`.  The resume launch gives every parked ray a lane of its own — the stragglers of many tiles side by side
 * in full waves — marches them to their end and writes their pixels.  workspace: device memory of at least
 * vkr_sssr_trace_workspace_bytes(rays width, rays height) bytes, 16-byte aligned, no initialisation needed; a workspace
 * belongs to one stream at a time.                                                                                      */
uint64_t vkr_sssr_trace_workspace_bytes(uint32_t rays_width, uint32_t rays_height);
int vkr_sssr_trace_split(const vkr_img* depth, const vkr_img* normal, const vkr_img* material,
                         const vkr_trace_params* params, const float* halton_vec4, const vkr_img* out_ray,
                         const vkr_img* out_occlusion, const vkr_img* pdf_tex, const vkr_trace_push* push,
                         void* workspace, uint64_t workspace_bytes, uint32_t park_after_rounds, void* stream);

/* Multi-GPU variant of "sssr_trace" (no reference counterpart; host/frame.hpp): `normal` is the whole-frame image but only
 * frame rows [normal_row0, normal_row1) of it are in memory when the march ends (the rank's window).  A ray that passes
 * every other validity test and whose hit-normal footprint (trace.comp:103-109) has a row outside them is stored as a
 * provisional hit: pending_mask (R8, the rays' extent; written for every pixel: 1 = pending) marks it and pending_data
 * (RGBA32F, twice the rays' width: two texels per pixel) keeps R and the hit uv.  Once the missing rows have arrived
 * (vkr_hit_requests / _reply / _scatter below) vkr_sssr_validate runs the deferred test and turns the rays that fail it
 * into misses — the stored rays are then bit-identical to vkr_sssr_trace's on a complete `normal`.                    */
int vkr_sssr_trace_windowed(const vkr_img* depth, const vkr_img* normal, const vkr_img* material,
                            const vkr_trace_params* params, const float* halton_vec4, const vkr_img* out_ray,
                            const vkr_img* out_occlusion, const vkr_img* pdf_tex, const vkr_img* pending_mask,
                            const vkr_img* pending_data, const vkr_trace_window_push* push, void* stream);
/* vkr_sssr_trace_windowed in two launches AROUND the arrival of the whole-frame pyramid (the depth all-gather of the tiled frame):
 * the head launch marches on `local_depth` alone — the levels of the pyramid this rank built itself, as the window image
 * holds them: full-width strips of the frame's levels, rows [origin_y, origin_y + height) each — and parks a ray in
 * `workspace` (vkr_sssr_trace_split above: same queue, same records) at its first fetch of a texel of the frame that is not
 * there: a row outside the strip, or a level the window image does not have.  A ray whose march has ended is parked as well
 * when its hit-depth sample (trace.comp:111-117) needs such a row; rays still marching after park_after_rounds compacted
 * rounds are parked as in the split.  `frame_depth` gives the head launch the frame's extents and level count only (not
 * read); once it is complete the resume launch finishes every parked ray on it.  Both launches take the arguments of
 * vkr_sssr_trace_windowed and leave, together, exactly its images.                                                      */
int vkr_sssr_trace_windowed_head(const vkr_img* local_depth, const vkr_img* frame_depth, const vkr_img* normal, const vkr_img* material,
                                 const vkr_trace_params* params, const float* halton_vec4, const vkr_img* out_ray,
                                 const vkr_img* out_occlusion, const vkr_img* pdf_tex, const vkr_img* pending_mask,
                                 const vkr_img* pending_data, const vkr_trace_window_push* push, void* workspace,
                                 uint64_t workspace_bytes, uint32_t park_after_rounds, void* stream);
int vkr_sssr_trace_windowed_resume(const vkr_img* frame_depth, const vkr_img* normal, const vkr_img* material,
                                   const vkr_trace_params* params, const float* halton_vec4, const vkr_img* out_ray,
                                   const vkr_img* out_occlusion, const vkr_img* pdf_tex, const vkr_img* pending_mask,
                                   const vkr_img* pending_data, const vkr_trace_window_push* push, void* workspace,
                                   uint64_t workspace_bytes, void* stream);
int vkr_sssr_validate(const vkr_img* rays, const vkr_img* pending_mask, const vkr_img* pending_data, const vkr_img* frame_normals,
                      const vkr_trace_params* params, void* stream);
/* the same, unless *skip_if_set (a device word, read by the launch) is non-zero: a round of requests that dropped some (see
 * vkr_hit_requests_bounded) has not delivered every hit normal, and the test must wait for the exact round               */
int vkr_sssr_validate_unless(const vkr_img* rays, const vkr_img* pending_mask, const vkr_img* pending_data, const vkr_img* frame_normals,
                             const vkr_trace_params* params, const uint32_t* skip_if_set, void* stream);

/* program "sssr_filter": advanced_ssr.cpp:308-369 + filter.comp (bindings 0..6)          */
int vkr_sssr_filter(const vkr_img* rays, const vkr_img* depth, const vkr_img* albedo,
                    const vkr_img* normal, const vkr_img* material, const vkr_img* out_reflections,
                    const vkr_trace_params* params, const vkr_filter_push* push, void* stream);

/* program "sssr_blur": advanced_ssr.cpp:371-438 + blur.comp (bindings 0..8)              */
int vkr_sssr_blur(const vkr_img* depth, const vkr_img* normal, const vkr_img* reflections,
                  const vkr_img* material, const vkr_img* history, const vkr_img* velocity,
                  const vkr_img* history_depth, const vkr_img* out_blurred,
                  const vkr_reproject_params* params, const vkr_blur_push* push, void* stream);


/* program "gtao_compute_main": gtao.cpp:84-148 + gtao/main.comp (bindings 0..5)          */
int vkr_gtao_main(const vkr_img* depth, const vkr_gtao_params* params, const vkr_img* normal,
                  const vkr_img* material, const vkr_img* pdf_tex, const vkr_img* gtao_inout,
                  const vkr_gtao_push* push, void* stream);

/* program "gtao_filter": gtao.cpp:198-239 + gtao/filter.comp (bindings 0..2)             */
int vkr_gtao_filter(const vkr_img* depth, const vkr_img* raw_gtao, const vkr_img* out_filtered,
                    const vkr_gtao_filter_push* push, void* stream);

/* program "gtao_accumulate": gtao.cpp:286-347 + gtao/accum.comp (bindings 0..6)          */
int vkr_gtao_accumulate(const vkr_img* depth, const vkr_img* prev_depth, const vkr_img* current_ao,
                        const vkr_img* out_accumulated, const vkr_img* velocity, const vkr_img* history,
                        const vkr_gtao_accum_params* params, const vkr_gtao_accum_push* push,
                        void* stream);

/* program "taa_resolve": taa.cpp:19-63 + taa/resolve.comp (bindings 0..6)                */
int vkr_taa_resolve(const vkr_img* history_color, const vkr_img* history_depth,
                    const vkr_img* current_depth, const vkr_img* velocity, const vkr_img* color,
                    const vkr_img* out_color, const vkr_reproject_params* params, void* stream);

/* program "ssr": ssr.cpp:10-73 + ssr/shader.frag:27-102 (bindings 0 normal, 1 depth [NEAREST,
 * clamp-to-border U], 2 frame colour, 3 SSRParams, 4 material; colour attachment RGBA8_UNORM).
 * depth: all mips of the full-res depth image.                                                  */
int vkr_ssr(const vkr_img* normal, const vkr_img* depth, const vkr_img* frame, const vkr_ssr_params* params,
            const vkr_img* material, const vkr_img* out, void* stream);

/* program "brdf_preintegrate": advanced_ssr.cpp:116-136 + preintegrate_ssr.comp:12-44 (split-sum LUT,
 * RG16F; consumed by the deferred-shading composite).  halton: the HaltonBuffer of vkr_sssr_trace.   */
int vkr_brdf_preintegrate(const float* halton_vec4 /*device*/, const vkr_img* out_brdf, void* stream);

/* program "defered_shading": defered_shading.cpp:47-118 + defered_shading/shader.frag:41-130
 * (bindings 0 albedo, 1 normal, 2 material, 3 depth [all mips], 4 Constants, 5 shadow map — bound by
 * the reference but never sampled, omitted here —, 6 occlusion, 7 brdf LUT, 8 reflections; colour
 * attachment RGBA8_SRGB).  SURVEY.md 8(f) #1.                                                        */
int vkr_defered_shading(const vkr_img* albedo, const vkr_img* normal, const vkr_img* material, const vkr_img* depth,
                        const vkr_shading_params* consts, const vkr_img* occlusion, const vkr_img* brdf,
                        const vkr_img* reflections, const vkr_img* out, const vkr_shading_push* push, void* stream);

/* SSSR_Clear (advanced_ssr.cpp:440-452): VkDispatchIndirectCommand{0,1,1} into both 3-word device
 * argument buffers.                                                                                */
int vkr_sssr_clear_indirect(uint32_t* reflective_args, uint32_t* glossy_args, void* stream);

/* program "sssr_classification": advanced_ssr.cpp:454-495 + classification.comp:38-98.  Appends
 * every 8x8 tile of the half-res extent (push->width/height = extent of `rays`) to the reflective
 * list when its mean roughness is below push->glossy_value, else to the glossy list; the tile
 * counts accumulate in word 0 of the argument buffers.  List order is unspecified (atomics), as in
 * the reference.  Bindings 0 material, 1/2 tile lists, 3/4 indirect arguments.                      */
int vkr_sssr_classification(const vkr_img* material, int32_t* reflective_tiles, int32_t* glossy_tiles,
                            uint32_t* reflective_args, uint32_t* glossy_args,
                            const vkr_classification_push* push, void* stream);

/* program "sssr_trace_indirect": advanced_ssr.cpp:216-302 + trace_indirect.comp:43-135, one
 * dispatch_indirect (push->reflection_type 0 = mirror: march from mip 0, <= 50 steps; 1 = glossy:
 * from mip 1, <= 25 steps).  Bindings 0 depth (view of mips 1..L-1), 1 normal, 2 material,
 * 3 TraceParams, 4 Halton, 5 rays, 6 tile list.  `indirect_args` word 0 is read on the device;
 * `max_tiles` = capacity of the tile list (launch bound).                                          */
int vkr_sssr_trace_indirect(const vkr_img* depth, const vkr_img* normal, const vkr_img* material,
                            const vkr_trace_params* params, const float* halton_vec4 /*device*/, const vkr_img* out_rays,
                            const int32_t* tiles /*device*/, const uint32_t* indirect_args /*device*/, uint32_t max_tiles,
                            const vkr_trace_indirect_push* push, void* stream);

/* program "gtao_main" (graphics): gtao.cpp:349-413 + gtao/main.frag:45-48,164-196 — full-screen
 * triangle into `raw`; one slice, 20 samples, radius min(200/|P|, 32) px, sky -> 1.  Bindings 0 depth
 * (view mip depth_lod), 1 GTAOParams, 2 normal; colour attachment RGBA16F (only .r is written by the
 * shader; the unwritten components are frozen to 0).  The debug heat-map of trace_samples.glsl
 * (binding 7, compiled out on the host side by GTAO_TRACE_SAMPLES 0) is not reproduced.            */
int vkr_gtao_main_graphics(const vkr_img* depth, const vkr_gtao_params* params, const vkr_img* normal,
                           const vkr_img* out_raw, const vkr_gtao_gfx_push* push, void* stream);

/* program "gtao_reproject": gtao.cpp:241-284 + gtao/reproject.comp:27-66 (STATIC_REPROJECT mode:
 * same-pixel history, mix 0.05 when |z_prev - z_cur| < 1e-6).  Bindings 0 params, 1 depth, 2 prev
 * depth, 3 current ao (filtered), 4 previous ao, 5 out (R16F).  Floor dispatch (w/8, h/4).           */
int vkr_gtao_reproject(const vkr_gtao_reprojection* params, const vkr_img* depth, const vkr_img* prev_depth,
                       const vkr_img* current_ao, const vkr_img* prev_ao, const vkr_img* out, void* stream);

/* program "deinterleave_depth": gtao.cpp:445-470 + gtao_opt/deinterleave.comp:10-21.  `layers` is the
 * R32F array image, one descriptor per layer (layer = ((y & m) << step) + (x & m)).  The dispatch is
 * (layer_w/8, layer_h/4) groups exactly as the reference records it (gtao.cpp:468), so only source
 * texels below that extent are scattered.                                                          */
int vkr_deinterleave_depth(const vkr_img* depth, const vkr_img* layers, uint32_t layer_count,
                           const vkr_deinterleave_push* push, void* stream);

/* program "main_deinterleaved": gtao.cpp:472-526 + gtao_opt/main_deinterleaved.comp:38-124.  One
 * dispatch of (out_w/8, out_h/4) groups for push->layer; stores outside `out` are dropped.          */
int vkr_gtao_main_deinterleaved(const vkr_img* layers, uint32_t layer_count, const vkr_gtao_params* params,
                                const vkr_img* normal, const vkr_img* out_raw,
                                const vkr_gtao_deinterleaved_push* push, void* stream);

/* program "screen_trace_main": screen_trace.cpp:23-95 + screen_trace/trace.comp:27-37,230-343
 * (trace_tangent_space, 1 direction).  Bindings 0 depth (mip 0), 1 normal, 2 colour, 3 material,
 * 4 out RGBA16F, 5 Params.  Floor dispatch (w/8, h/8).  The 8x8 tile exchange through shared memory
 * is resolved as if `barrier()` followed the stores (trace.comp:310-311 has only a memory barrier);
 * slots of sky pixels, which return before writing theirs, read as "no hit".                       */
int vkr_screen_trace_main(const vkr_img* depth, const vkr_img* normal, const vkr_img* color, const vkr_img* material,
                          const vkr_img* out_raw, const vkr_screen_trace_params* params, void* stream);

/* program "screen_trace_filter": screen_trace.cpp:97-140 + screen_trace/filter.comp:13-39.           */
int vkr_screen_trace_filter(const vkr_img* raw, const vkr_img* depth, const vkr_img* out_filtered,
                            const vkr_screen_trace_filter_push* push, void* stream);

/* program "screen_trace_accumulate": screen_trace.cpp:142-181 + screen_trace/accumulate.comp:21-40
 * (accum is read and written in place).                                                            */
int vkr_screen_trace_accumulate(const vkr_img* depth, const vkr_img* prev_depth, const vkr_img* current,
                                const vkr_img* accum_inout, const vkr_screen_trace_accum_push* push, void* stream);

/* program "gbuf_opaque_taa": SceneRenderer::draw_taa (scene_renderer.cpp:140-220) + gbuf/opaque_taa.{vert,frag}
 * as a compute rasterizer: attachments cleared (colour 0, depth 1), every triangle of every draw
 * rasterised into a 64-bit visibility buffer (depth | triangle) with atomics, then resolved per pixel
 * (perspective-correct attributes, trilinear sRGB textures, octahedral normal, velocity).  Frozen
 * raster rules: pixel centres, top-left fill rule, 8 sub-pixel bits, cull none, depth LESS_OR_EQUAL
 * in D24 (gpu/pipelines.hpp:113-128), near-plane clipping in clip space, implicit LOD from forward
 * differences of the interpolated uv.  `scratch`: vkr_raster_scratch_bytes() of device memory (the
 * visibility buffer + two records per drawn triangle).                           */
uint64_t vkr_raster_scratch_bytes(uint32_t width, uint32_t height, uint32_t triangle_count /* summed over all draws */);
int vkr_raster_gbuffer(const vkr_raster_scene* scene, const vkr_gbuf_const* consts, const vkr_img* albedo,
                       const vkr_img* normal, const vkr_img* material, const vkr_img* velocity, const vkr_img* depth,
                       void* scratch, uint64_t scratch_bytes, void* stream);

/* program "default_shadow": SceneRenderer::render_shadow (scene_renderer.cpp:222-274) + shadows/default.{vert,frag} as a
 * depth-only compute rasteriser: layer l of `layers` is the scene's depth seen through mvps[l], with the vertex stage
 * clip = (mvps[l] * model) * vec4(pos, 1) and an empty fragment stage.  Each layer is cleared to depth 1, stencil 0 (the word
 * 0x00FFFFFF) and then drawn; every stored word has its top byte 0.  The raster rules are those of vkr_raster_gbuffer (pixel
 * centres, vertices snapped to 8 sub-pixel bits, top-left fill rule, cull none, near-plane clip in clip space, per-fragment depth
 * clip, D24 = rint(z * (2^24 - 1)), LESS_OR_EQUAL), so a layer equals the depth attachment of vkr_raster_gbuffer run with
 * view_projection = mvps[l], zero jitter and no textures.  Only pos, the indices, the model matrices and transform_index /
 * index_offset / index_count / vertex_offset of each draw are read: textures, albedo_index, mr_index, flags and reserved are
 * ignored (textures == NULL with texture_count == 0 is valid), and a cutout casts a solid shadow as the empty fragment shader
 * makes it.  A triangle with an index outside the vertex buffer is not drawn.  There is no visibility buffer and no resolve:
 * coverage issues atomic mins of the 24-bit depth straight into the layers.  layers: layer_count (1..8) D24_UNORM_S8 descriptors,
 * square, of one extent, not windowed (single-GPU pass); they need not be the layers of one array.  All layers go through one set
 * of launches.  `scratch`: vkr_default_shadow_scratch_bytes(edge of a layer, layer_count, triangles summed over all draws) of
 * device memory.  At most 1024 draws. */
uint64_t vkr_default_shadow_scratch_bytes(uint32_t size, uint32_t layer_count, uint32_t triangle_count);
int vkr_default_shadow(const vkr_raster_scene* scene, const vkr_mat4* mvps /* [layer_count] */, const vkr_img* layers /* [layer_count] */,
                       uint32_t layer_count, void* scratch, uint64_t scratch_bytes, void* stream);

/* program "ssao": SSAOPass::draw (ssao.cpp:54-97) + ssao/shader.{vert,frag}, the reference's first ambient-occlusion pass.
 * The uniform block as the SHADER reads it (std140: a vec3 array has a 16-byte stride), 336 bytes; .w of a sample is not read. */
typedef struct vkr_ssao_params {
  vkr_mat4 projection;
  float fovy, aspect, znear, zfar;
  float samples[16][4];
} vkr_ssao_params;
/* Bindings in shader order: 0 depth (D24_UNORM_S8; mip 0 of the view, ssao.cpp:62), 1 the block, colour attachment
 * out_occlusion (R8_UNORM, any extent: the shader works in uv).  Per output pixel g, shader.frag:21-41 in this order:
 * screen_uv = (g + 0.5) / extent; frag_depth = texture(depth, screen_uv); camera_pos = reconstruct_view_vec(screen_uv,
 * frag_depth, ...); for each of the 16 samples pos = camera_pos + 0.05 * sample (one fused multiply-add per component under
 * numeric contract 2), ndc = projection * (pos, 1), ndc.xyz / ndc.w (IEEE division: w = 0, infinities and NaN as they fall),
 * sample_uv = 0.5 * ndc.xy + 0.5, counted when ndc.z < texture(depth, sample_uv) + 0.0000001 (the sum rounded to float, then
 * compared; a NaN on either side does not count); stored: count / 16 as UNORM8 = rint(x * 255), ties to even (8 / 16 -> 128).
 * texture(): bilinear, clamp-to-edge, float -> int saturating with NaN -> 0.  Every texel of out_occlusion is written.
 * Refused before any launch: a NULL argument, a descriptor without memory, other formats, a zero extent, an output wider or
 * higher than 65535, and a windowed descriptor on either side (the taps reach anywhere: a single-GPU pass). */
int vkr_ssao(const vkr_img* depth, const vkr_ssao_params* params, const vkr_img* out_occlusion, void* stream);

/* program "tile_regression": AdvancedSSR::run_tile_regression_pass (advanced_ssr.cpp:497-538) + advanced_ssr/regression.comp, the
 * per-tile plane fit of the tile-classified SSR experiment.  The push constants as the shader declares them, 80 bytes. */
typedef struct vkr_tile_regression_push { vkr_mat4 camera_to_world; float fovy, aspect, znear, zfar; } vkr_tile_regression_push;
/* Bindings in shader order: 0 depth (D24_UNORM_S8; mip 0 of the view is read: the caller passes a view of mip 1 of the G-buffer
 * depth, advanced_ssr.cpp:523), 1 out_planes (RGBA32_SFLOAT, one texel per 8 x 8 tile of the depth view; any extent up to
 * ceil(w / 8) x ceil(h / 8); the reference allocates (W / 16, H / 16) of the full-resolution frame, rounded down).  Per tile,
 * regression.comp:22-101 in the order DESIGN_NUMERICS.md (Tile regression) freezes: lane i = ly * 8 + lx takes pixel
 * p = 8 * tile + (lx, ly); screen_uv = vec2(p) / vec2(size) (no half-texel offset, IEEE division, pixel 0 gives 0);
 * r = (camera_to_world * (reconstruct_view_vec(screen_uv, texelFetch(depth, p), ...), 1) - camera_to_world * (0, 0, 0, 1)).xyz;
 * a lane whose pixel lies outside the view contributes r = 0 and is still one of the 64; depth 1 (sky) has no special case.
 * The sums of r, r * r and (r.x r.y, r.x r.z, r.y r.z) follow the shader's tree s[i] += s[i + off], off = 32 .. 1;
 * plane = inverse(mat3 of the sums) * sum r with the inverse as the adjugate over the determinant (GLM's layout, nothing fused,
 * 1 / det an IEEE division: det = 0 gives infinities, and plane is stored as it falls); each lane's squared residual
 * (dot(plane, r) - 1)^2, 1e10 where that is NaN, so an outside lane adds 1; .w = their tree sum / 64.
 * Every texel of out_planes is written and nothing outside its rows.  Refused before any launch: a NULL argument, a descriptor
 * without memory, other formats, a zero extent, an out_planes wider or higher than ceil(w / 8) x ceil(h / 8) (such a tile has no
 * pixel and the reference never dispatches it) or higher than 65535, and a windowed descriptor on either side. */
int vkr_tile_regression(const vkr_img* depth, const vkr_img* out_planes, const vkr_tile_regression_push* push, void* stream);

/* program "texdraw": add_backbuffer_subpass (backbuffer_subpass2.cpp:15-52) + texdraw/shader.{vert,frag}, the last pass of the
 * reference's frame and its debug view: any colour image, all channels or one, onto an 8-bit surface of the window's extent.
 * The push constants as the shader declares them, 4 bytes. */
typedef struct vkr_texdraw_push { uint32_t flags; } vkr_texdraw_push;   /* texdraw/shader.frag:15-17 */
enum { VKR_TEXDRAW_SHOW_ALL = 0, VKR_TEXDRAW_SHOW_R = 1, VKR_TEXDRAW_SHOW_G = 2, VKR_TEXDRAW_SHOW_B = 4, VKR_TEXDRAW_SHOW_A = 8 };
/* Binding 0 target_tex (any colour format vkr_blit_image takes as a source; mip 0 of the view is sampled), colour attachment
 * backbuffer (RGBA8_SRGB or RGBA8_UNORM, any extent: the shader works in uv).  Per destination pixel g (DESIGN_NUMERICS.md,
 * Texdraw): uv = (g + 0.5) / extent per axis (IEEE division); c = texture(target_tex, uv): texel coordinate uv * size - 0.5 (one
 * fused multiply-add under numeric contract 2), floor, fraction by subtraction, float -> int saturating with NaN -> 0,
 * clamp-to-edge, the decoded RGBA (absent channels 0, 0, 0, 1; RGBA8_SRGB rgb through the EOTF table, alpha linear) mixed rows
 * first, then columns, all four channels; then the shader's four ifs in order, so the LAST set bit of R, G, B, A wins
 * (flags = 3 shows G, 15 shows A, bits above 8 are ignored) and a shown channel goes to all four outputs; stored as the
 * backbuffer stores: RGBA8_SRGB rgb by the threshold rule and alpha as UNORM8, RGBA8_UNORM rint(clamp(x, 0, 1) * 255); NaN -> 0.
 * The reference's clear of the attachment to 0 is never visible (the triangle covers every pixel) and is not executed.
 * Every texel of the backbuffer is written.  Refused before any launch: a NULL argument, a descriptor without memory,
 * D24_UNORM_S8 or an unknown format as source, any other destination format, a zero extent, a destination wider or higher than
 * 65535, a windowed descriptor on either side, and target_tex == backbuffer (the same memory). */
int vkr_texdraw(const vkr_img* target_tex, const vkr_img* backbuffer, const vkr_texdraw_push* push, void* stream);

/* program "shadow_mask" (no reference program: the reference renders its shadow maps and never samples them).  The lookup half of
 * the shadow pipeline: for every full-resolution pixel the visibility of up to four lights through the D24 layers that
 * vkr_default_shadow rendered, one RGBA8_UNORM texel per pixel, channel l = light l, channels at or beyond layer_count = 255. */
typedef struct vkr_shadow_mask_params {
  vkr_mat4 inverse_camera;          /* view -> world, as in vkr_shading_params      */
  vkr_mat4 mvps[4];                 /* the matrices the layers were rendered with   */
  float    fovy, aspect, znear, zfar;
  uint32_t layer_count;             /* 1..4                                         */
  uint32_t radius;                  /* 0, 1, 2: 1, 9 or 25 taps                     */
  uint32_t bias;                    /* in D24 codes, added to the map's side        */
  uint32_t reserved;                /* 0                                            */
} vkr_shadow_mask_params;
/* depth: the G-buffer depth (D24_UNORM_S8, mip 0 of the view) at out_mask's extent; layers: layer_count square D24_UNORM_S8
 * descriptors of one extent `size`; out_mask: RGBA8_UNORM.  Per pixel g and light l (DESIGN_NUMERICS.md, Shadow mask):
 * uv = (g + 0.5) / extent; d = the exact decode of depth texel g (by index, unfiltered); d >= 1 stores 255 in every channel;
 * view = reconstruct_view_vec(uv, d, ...); clip = M_l * (view, 1) with M_l = mvps[l] * inverse_camera taken on the host in
 * double and rounded once to float (16 multiply-adds per light in the order of every mat4 * vec4 here); ndc = clip.xyz / clip.w
 * (IEEE division).  Lit without taps when clip.w <= 0, ndc.x or ndc.y outside [-1, 1], ndc.z > 1, or any of them NaN; nowhere
 * else.  Otherwise code = rint(clamp(ndc.z, 0, 1) * 16777215) (the rasteriser's depth quantisation), the centre texel
 * t = floor((0.5 * ndc.xy + 0.5) * size) (float -> int: truncate, saturating) clamped to [0, size - 1], and each of the
 * (2 radius + 1)^2 taps t + (dx, dy) passes when it lies outside the map or code <= (word & 0xFFFFFF) + bias (an integer
 * compare without wrap-around: the top byte of a word is ignored, bias >= 2^24 passes everything); the channel is
 * passes / taps as UNORM8 = rint(x * 255), ties to even.  Every texel of out_mask is written, nothing outside its rows.
 * Refused before any launch: a NULL argument, a descriptor without memory, other formats, depth and out_mask of different
 * extents, an extent above 65535, a windowed descriptor anywhere (the taps reach anywhere: a single-GPU pass), layers that are
 * not square or not of one extent, layer_count outside 1..4, radius > 2, reserved != 0. */
int vkr_shadow_mask(const vkr_img* depth, const vkr_img* layers /* [layer_count] */, const vkr_shadow_mask_params* params,
                    const vkr_img* out_mask, void* stream);

/* program "defered_shading_shadowed": vkr_defered_shading with one more binding, shadow_mask (RGBA8_UNORM at the extent and
 * window of `out`, as vkr_shadow_mask writes it).  Channel .x of the pixel's own texel, read by index as code / 255, multiplies
 * the direct term of shader.frag:91 (Lo before the reflection is added) and nothing else: the ambient term, the reflection term
 * and the show_ao branch are those of vkr_defered_shading.  The shading light is the shader's hard-coded LIGHT_POS, the eye of
 * the default shadow light (main.cpp:295), so the channel used is light 0 of the mask; the other channels are not read.  A
 * mask of 255 everywhere gives the bytes of vkr_defered_shading. */
int vkr_defered_shading_shadowed(const vkr_img* albedo, const vkr_img* normal, const vkr_img* material, const vkr_img* depth,
                                 const vkr_shading_params* consts, const vkr_img* occlusion, const vkr_img* brdf,
                                 const vkr_img* reflections, const vkr_img* shadow_mask, const vkr_img* out,
                                 const vkr_shading_push* push, void* stream);

/* synthetic G-buffer generator (no reference program).  Any of the
 * colour outputs may be NULL when VKR_SYNTH_DEPTH_ONLY is set.                          */
int vkr_synth_gbuffer(const vkr_img* depth, const vkr_img* normal, const vkr_img* albedo,
                      const vkr_img* material, const vkr_img* velocity,
                      const vkr_synth_params* params, void* stream);

/* ---- ray-traced AO (gtao.cpp:150-196 + gtao/rt_main.frag) over the project's own acceleration structure ---------------------
 * MI355X has no ray-tracing hardware: the scene's triangles, transformed to world space on the host, go into one bounding-
 * volume hierarchy (binned SAH, built on the host: deterministic, the same triangles always give the same bytes), traversed in
 * software.  Every ray is an ANY-hit query of the segment origin + t * dir, t in [tmin, tmax], against all triangles: opaque,
 * no facing culling, nothing but "was anything hit" is reported.  The frozen fp32 triangle test (DESIGN_NUMERICS.md, the one
 * device helper both entries below use): Moller-Trumbore in a fixed operation order, det == 0 a miss, inclusive edges
 * (u >= 0, v >= 0, u + v <= 1), tmin <= t <= tmax, and the computed point origin + t * dir inside the triangle's bounding box
 * widened by (max |coordinate| + 1) * 2^-12 — which makes every box test of the traversal provably conservative, so the
 * result does not depend on the hierarchy.                                                                                  */
typedef struct vkr_accel_node {  /* 32 bytes; count == 0: interior node whose children are nodes first and first + 1    */
  float    lo[3];                /* count > 0: leaf of the triangle records [first, first + count)                        */
  uint32_t first;
  float    hi[3];
  uint32_t count;
} vkr_accel_node;
typedef struct vkr_accel_tri {   /* 64 bytes: v0, its edges e1 = v1 - v0, e2 = v2 - v0 (fp32), the widened box, and the     */
  float    v0[3];                /* index of the triangle in the caller's input                                            */
  uint32_t index;
  float    e1[3], e2[3];
  float    lo[3], hi[3];
} vkr_accel_tri;
typedef struct vkr_accel vkr_accel;
/* Pure host function, no GPU: the hierarchy of tri_count world-space triangles (tri_vertices: tri_count x 3 vertices x xyz,
 * host memory) into caller-provided host arrays: at most max(1, 2 * tri_count - 1) nodes (node_capacity), exactly tri_count
 * triangle records.  *node_count receives the number of nodes written (0 for an empty scene).  Vertices that are not finite
 * are accepted (a loader can meet them): the build stays deterministic, a node box takes no NaN bound, and such a triangle is
 * hit exactly where the frozen test says so, where "NaN is a miss" (DESIGN_NUMERICS.md, "Ray query, scenes and scale").        */
int vkr_accel_layout(const float* tri_vertices, uint32_t tri_count, vkr_accel_node* nodes, uint32_t node_capacity,
                     vkr_accel_tri* tris, uint32_t* node_count);
/* layout + upload (synchronous, allocates device memory): the handle the ray-query kernels take                               */
int vkr_accel_create(const float* tri_vertices, uint32_t tri_count, vkr_accel** out);
int vkr_accel_destroy(vkr_accel* accel);
int vkr_accel_info(const vkr_accel* accel, uint32_t* node_count, uint32_t* tri_count);
/* any-hit of n arbitrary rays (origins, dirs: device, n x xyz floats): out_hit[i] = 1 when the frozen test reports a hit for
 * some triangle, else 0.  A wave of 64 rays traverses the hierarchy together (node order on a stack in LDS).                   */
int vkr_accel_query(const vkr_accel* accel, const float* origins, const float* dirs, float tmin, float tmax, uint32_t n,
                    uint32_t* out_hit, void* stream);
/* GTAORTParams, gtao.hpp:20-26 / rt_main.frag:11-17 */
typedef struct vkr_gtao_rt_params {
  vkr_mat4 camera_to_world;
  float fovy, aspect, znear, zfar;
} vkr_gtao_rt_params;
typedef struct vkr_gtao_rt_push { float rotation; } vkr_gtao_rt_push;  /* rt_main.frag:29-31 */
/* program "gtao_rt_main": gtao.cpp:150-196 + gtao/rt_main.frag — full-screen triangle into `raw` (RGBA16F, half resolution).
 * Bindings 0 GTAORTParams, 1 depth (view mip depth_lod), 2 normal (full resolution), 3 the acceleration structure, 4 the 64
 * random directions (device, 64 x vec4, gtao.cpp:415-443); push: rotation.  Per pixel: (2 * sum / 64, 1, 0, 0) of the
 * 64 visibility-weighted cosines of rays 0.2 long; sky (depth >= 1): (0, 1, 0, 0).  The 16 (cos, sin) pairs of
 * 2 PI (rotation + k / 16) are evaluated on the host.  One wave per pixel, one lane per direction.                        */
int vkr_gtao_rt_main(const vkr_gtao_rt_params* params, const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel,
                     const float* directions, const vkr_img* out_raw, const vkr_gtao_rt_push* push, void* stream);
/* vkr_accel_query for long rays: the arguments, the gates and the answers of vkr_accel_query, bit for bit.  The walk culls
 * a node per ray (the segment-box term of vkr_accel_query AND a slab test against the node box widened by a per-ray margin,
 * rounded outward; DESIGN_NUMERICS.md, "Ray query, the per-ray cull"), which is what keeps a wave of metres-long rays from
 * descending nearly everywhere.                                                                                               */
int vkr_accel_occluded(const vkr_accel* accel, const float* origins, const float* dirs, float tmin, float tmax, uint32_t n,
                       uint32_t* out_hit, void* stream);
/* The CLOSEST hit of n arbitrary rays (DESIGN_NUMERICS.md, "Ray query, closest hit"): of all triangles the frozen test accepts
 * for the ray (the test of vkr_accel_query: its operation order, inclusive edges, det == 0 a miss, the widened-box clause, NaN a
 * miss) the one with the smallest fp32 t; of equal t (==, so -0 == +0) the one with the smallest index in the caller's input,
 * never the one the hierarchy happens to meet first.  t, u, v are that triangle's values as the frozen sequence computed them
 * (the hit point is v0 + u e1 + v e2 = (1 - u - v) v0 + u v1 + v v2), index its position in the input of vkr_accel_create.   */
typedef struct vkr_accel_hit { float t, u, v; uint32_t index; } vkr_accel_hit;  /* 16 bytes; a miss: index 0xFFFFFFFF, t = u = v = 0 */
/* The arguments and gates of vkr_accel_occluded; out_hits: device, n records, 16-byte aligned (one 16-byte store per ray);
 * records past n are not written.  An empty structure is legal: every ray misses.  hit.index != 0xFFFFFFFF is
 * vkr_accel_occluded's answer for the ray.                                                                                    */
int vkr_accel_closest(const vkr_accel* accel, const float* origins, const float* dirs, float tmin, float tmax, uint32_t n,
                      vkr_accel_hit* out_hits, void* stream);

/* ---- refit: moving geometry under the topology of vkr_accel_create (DESIGN_NUMERICS.md "Ray query: refit") ------
 * The structure keeps the hierarchy the host builder chose; only the bytes that depend on vertex positions are recomputed, on the
 * device, from tri_vertices (device, tri_count x 9 floats, in the order of the INPUT of vkr_accel_create; tri_count as created:
 * triangles are neither added nor removed).  Every record slot keeps its place and its `index`; its v0, e1, e2, lo, hi become what
 * vkr_accel_layout computes for triangle `index` of tri_vertices (the same operations in the same order, the margin
 * (max |coordinate| + 1) * 2^-12).  Every node keeps `first` and `count`; a leaf's box becomes the union of its records' boxes, an
 * interior node's the union of its two children's, both from +-inf with the builder's minimum / maximum, so a NaN bound never
 * enters a node.  Boxes are recomputed on every call, never grown: what one pose put into them (a NaN, an infinity, a far vertex)
 * is gone after the next.  Since every answer of the ray query is that of the frozen test over all triangles whatever the
 * hierarchy, the refitted structure answers bit for bit like one created from tri_vertices; a walk may take longer where the old
 * topology no longer fits the moved triangles (the escape is to create the structure again).
 * Ordering: asynchronous on `stream`.  Queries (and passes that take the structure) submitted to the same stream after the call
 * see the refitted structure, those submitted before it the earlier one; tri_vertices must stay valid and unchanged until the
 * call's work has run.  Work on other streams that uses the structure is the caller's to order against the refit.
 * An empty structure is a no-op; a NULL handle, or NULL vertices for a structure with triangles, is VKR_ERR_NULL.               */
int vkr_accel_refit(vkr_accel* accel, const float* tri_vertices, void* stream);
/* The same rule as a pure host function, no GPU: applied in place to the arrays of vkr_accel_layout (or of vkr_accel_download)
 * from tri_vertices (host, tri_count x 9, input order).  A malformed topology — an interior node whose children are not stored
 * behind it inside the array, a leaf whose record range or a record whose input index leaves the arrays — is refused with
 * VKR_ERR_EXTENT before anything is written or read outside the arrays.                                                        */
int vkr_accel_refit_layout(vkr_accel_node* nodes, uint32_t node_count, vkr_accel_tri* tris, uint32_t tri_count, const float* tri_vertices);
/* For tests and tools: synchronises `stream`, then copies the device arrays into host arrays (vkr_accel_info gives the counts;
 * a capacity below them is VKR_ERR_EXTENT).                                                                                     */
int vkr_accel_download(const vkr_accel* accel, vkr_accel_node* nodes, uint32_t node_capacity, vkr_accel_tri* tris, uint32_t tri_capacity,
                       void* stream);
/* For tests and tools: how vkr_accel_refit walks the hierarchy.  level_sizes[h]: the number of nodes of height h (a leaf has
 * height 0, an interior node 1 + the larger height of its children; at most 49 levels), *level_count their number (0 for an empty
 * structure).  A refit is one launch over the records, one launch per level of more than *tail_nodes nodes (level sizes never
 * grow with the height, so these are the first ones), and one single-workgroup launch for all remaining levels up to the root.  */
int vkr_accel_refit_schedule(const vkr_accel* accel, uint32_t* level_sizes, uint32_t level_capacity, uint32_t* level_count, uint32_t* tail_nodes);
/* The world-space triangles of a raster scene, on the device, as vkr_accel_create / vkr_accel_refit take them: draw by draw,
 * index_count / 3 triangles per draw, vertex k of triangle j of a draw = vertices[indices[index_offset + 3 j + k] + vertex_offset]
 * .pos, transformed by m = transforms[transform_index].model as ((m[0][r] x + m[1][r] y) + m[2][r] z) + m[3][r] per row r, every
 * product and sum rounded on its own (no fused multiply-add under either numeric contract).  out_tri_vertices: device, room for
 * out_tri_capacity triangles of 9 floats; scratch: device, vkr_scene_triangles_scratch_bytes(draw_count) (the draw table, which
 * travels as kernel arguments: no host staging, nothing synchronises).  The gates of the rasterisers' scenes apply (NULL arrays,
 * a draw outside the index or transform arrays); texture indices are not read.  A triangle with an index outside the vertex buffer
 * gets three NaN vertices, so no ray hits it, and nothing is read outside the buffer.  Only pos, the
 * indices, model and the four range fields of a draw are read.                                                                  */
uint64_t vkr_scene_triangles_scratch_bytes(uint32_t draw_count);
int vkr_scene_triangles(const vkr_raster_scene* scene, float* out_tri_vertices, uint64_t out_tri_capacity, void* scratch, uint64_t scratch_bytes,
                        void* stream);

/* program "reflections_rt" (no reference program): the `reflections` image of AdvancedSSR (RGBA8_UNORM, half resolution in the
 * frame) traced through the scene's ray-query structure: per pixel the mirror ray of the view direction, its closest hit, and the
 * albedo of the hit triangle there ("radiance = albedo at the hit", as ssr/filter.comp; alpha 0 as the filter stores it).  Where
 * the screen-space trace goes black (the ray leaves the screen or passes behind geometry) this one still has an answer.       */
typedef struct vkr_hit_attrib {         /* 32 bytes, one per INPUT triangle of the structure, in input order (device memory) */
  float    uv[3][2];                    /* the texture coordinates of the triangle's three vertices */
  uint32_t albedo_index;                /* index into `textures`; 0xFFFFFFFF or >= texture_count: untextured, (0.5, 0.5, 0.5) */
  uint32_t reserved;
} vkr_hit_attrib;
#define VKR_REFLECT_RT_FILL_MISSES 1u   /* flags: only pixels whose screen-space ray is invalid (.w code of `rays` == 65535) are traced */
typedef struct vkr_reflect_rt_params {  /* 112 bytes */
  vkr_mat4 inverse_camera;              /* view -> world; its translation column is the eye */
  float    fovy, aspect, znear, zfar;
  float    normal_offset;               /* origin = world + normal_offset * normal */
  float    tmin, max_distance;          /* the ray is origin + t * dir, dir of unit length, t in [tmin, max_distance] */
  uint32_t texture_lod;                 /* the mip level sampled at a hit, clamped to the texture's chain */
  uint32_t flags;                       /* VKR_REFLECT_RT_* */
  uint32_t reserved[3];                 /* 0 */
} vkr_reflect_rt_params;
uint64_t vkr_reflections_rt_scratch_bytes(uint32_t texture_count);
/* depth: D24_UNORM_S8 (mip 0 of the view); normal: RG16_UNORM; rays: RGBA16_UNORM (NULL unless VKR_REFLECT_RT_FILL_MISSES);
 * out_reflections: RGBA8_UNORM; one extent (the frame binds the half-resolution set).  Per pixel g (DESIGN_NUMERICS.md,
 * Reflections, ray traced): d = the exact decode of depth texel g (by index); d >= 1 stores (0, 0, 0, 0).  With FILL_MISSES a
 * pixel whose `rays` texel has a .w code other than 65535 (a valid screen-space hit, filter.comp:94) is LEFT UNTOUCHED and casts
 * nothing: in-place use on the filter's output.  uv = (g + 0.5) / extent; world = (inverse_camera * (reconstruct_view_vec(uv, d),
 * 1)).xyz; n = decode_normal(normal texel g); origin = world + normal_offset * n; eye = inverse_camera's translation column;
 * V = world - eye; R = V - (2 dot(n, V)) n; dir = normalize(R); unless dot(n, dir) > 0 (a surface seen from behind, a grazing
 * zero, any NaN) the texel is 0.  Otherwise the closest hit of (origin, dir, tmin, max_distance) (vkr_accel_closest's answer): a
 * miss stores 0; a hit on triangle `index` at (u, v) shades a = attribs[index]: w = (1 - u) - v, uv_hit = (w uv0 + u uv1) + v uv2
 * per component, every operation rounded on its own; colour (0.5, 0.5, 0.5) when a.albedo_index is 0xFFFFFFFF or >=
 * texture_count, else the bilinear REPEAT sample of level min(texture_lod, levels - 1) of textures[a.albedo_index] (RGBA8_SRGB,
 * as vkr_raster_scene's) at uv_hit; stored as rint(255 x) per channel, alpha 0.  textures: host array (NULL only with
 * texture_count 0, at most 32); its table goes into `scratch` (device, vkr_reflections_rt_scratch_bytes(texture_count)): nothing
 * is allocated.  Refused before any launch: a NULL argument (rays only without the flag), other formats, different extents, an
 * extent above 65535, a windowed descriptor anywhere (the rays reach anywhere: a single-GPU pass), attrib_count != the structure's
 * triangle count, unknown flag bits, reserved != 0, tmin or max_distance NaN, scratch_bytes too small.                        */
int vkr_reflections_rt(const vkr_img* depth, const vkr_img* normal, const vkr_img* rays, const vkr_accel* accel,
                       const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                       const vkr_reflect_rt_params* params, const vkr_img* out_reflections, void* scratch, uint64_t scratch_bytes,
                       void* stream);

/* program "shadow_mask_rt" (no reference program): the shadow mask of vkr_shadow_mask traced through the scene's ray-query
 * structure instead of looked up in a shadow map: exact hard shadows of up to four point or directional lights, no map, no
 * frustum, no depth bias.  One RGBA8_UNORM texel per pixel, channel l = light l, 0 or 255.                                   */
typedef struct vkr_shadow_rt_params {   /* 160 bytes */
  vkr_mat4 inverse_camera;              /* view -> world */
  float    fovy, aspect, znear, zfar;
  float    lights[4][4];                /* xyz, w: w == 1 a point light at xyz; w == 0 directional: xyz is the vector from the
                                           surface towards the light, its length is the reach of the ray */
  uint32_t light_count;                 /* 1..4 */
  float    normal_offset;               /* origin = world + normal_offset * normal */
  float    tmin;                        /* the segment is origin + t * dvec, t in [tmin, 1] */
  uint32_t reserved;                    /* 0 */
} vkr_shadow_rt_params;
/* depth: D24_UNORM_S8 (mip 0 of the view); normal: RG16_UNORM at full resolution; out_mask: RGBA8_UNORM; one extent.  Per pixel
 * g (DESIGN_NUMERICS.md, Shadow mask, ray traced): d = the exact decode of depth texel g (by index, unfiltered); d >= 1 stores
 * 255 in every channel.  uv = (g + 0.5) / extent; view = reconstruct_view_vec(uv, d, ...); world = (inverse_camera * (view, 1)).xyz
 * in the order of every mat4 * vec4 here; n = decode_normal(the exact decode of normal texel g, by index);
 * origin = world + normal_offset * n (one multiply-add per component under contract 2).  Per light l < light_count:
 * dvec = lights[l].xyz - origin for a point light (three subtractions), lights[l].xyz for a directional one; facing = dot(n, dvec);
 * unless facing > 0 the channel is 0 and no ray is cast (a surface facing away, a light at the surface point, any NaN); otherwise
 * the channel is 0 when the frozen any-hit of (origin, dvec, tmin, 1) reports a hit (vkr_accel_query's answer for that ray) and
 * 255 when not.  Channels at or beyond light_count are 255.  Every texel of out_mask is written, nothing outside its rows.
 * An empty structure is legal: every ray misses.  Refused before any launch: a NULL argument, a descriptor without memory, other
 * formats, different extents, an extent above 65535, a windowed descriptor anywhere (the rays reach anywhere: a single-GPU
 * pass), light_count outside 1..4, a light whose w is neither 0 nor 1, reserved != 0, tmin NaN.                               */
int vkr_shadow_mask_rt(const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel, const vkr_shadow_rt_params* params,
                       const vkr_img* out_mask, void* stream);

/* ---- alpha cutouts in the ray query (DESIGN_NUMERICS.md, "Ray query, cutouts") ---------------------------------------------------
 * The rasterisers discard a fragment whose albedo alpha is 0; these entries ask the same of a ray.  A CANDIDATE is a triangle
 * `index` that the frozen test accepts for the ray at (t, u, v).  It is TRANSPARENT for that ray when a = attribs[index] has
 * a.albedo_index < texture_count, bit a.albedo_index of opaque_texture_mask is clear, and the alpha of the bilinear REPEAT sample
 * of level min(alpha_lod, levels - 1) of textures[a.albedo_index] at uv_hit is == 0.0f; uv_hit and the sample are those of
 * vkr_reflections_rt (w = (1 - u) - v, (w uv0 + u uv1) + v uv2, every operation rounded on its own; alpha decoded as UNORM8 and
 * mixed in the sampler's order).  A compare with a NaN is false: opaque.  An untextured triangle is opaque.  A set mask bit means
 * "do not test this texture": the triangle is opaque whatever its texels hold (set it for textures without an alpha-0 texel and
 * the fetch is skipped; a wrong hint is a defined answer, not an error).
 *   any hit:     does a triangle exist that the frozen test accepts and that is not transparent at its own (u, v)?
 *   closest hit: of those triangles the one with the smallest fp32 t, of equal t the smallest input index.
 * Both are defined over ALL triangles: the answers do not depend on the hierarchy.                                            */
typedef struct vkr_ray_cutout { uint32_t alpha_lod; uint32_t opaque_texture_mask; } vkr_ray_cutout;  /* 8 bytes */
/* the device scratch of one call of any _cutout entry (the texture table; equal to vkr_reflections_rt_scratch_bytes) */
uint64_t vkr_accel_cutout_scratch_bytes(uint32_t texture_count);
/* vkr_accel_occluded / vkr_accel_closest with the queries above: their arguments and gates, plus those vkr_reflections_rt has
 * for attribs (attrib_count == the structure's triangle count), textures (whole-frame RGBA8_SRGB chains, at most 32: the mask is
 * one word) and scratch; a NULL cutout is VKR_ERR_NULL; n == 0 is VKR_OK whatever else is passed.  With texture_count 0 or a
 * mask of all ones the outputs are those of the opaque entries, bit for bit.                                                  */
int vkr_accel_occluded_cutout(const vkr_accel* accel, const float* origins, const float* dirs, float tmin, float tmax, uint32_t n,
                              const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                              const vkr_ray_cutout* cutout, uint32_t* out_hit, void* scratch, uint64_t scratch_bytes, void* stream);
int vkr_accel_closest_cutout(const vkr_accel* accel, const float* origins, const float* dirs, float tmin, float tmax, uint32_t n,
                             const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                             const vkr_ray_cutout* cutout, vkr_accel_hit* out_hits, void* scratch, uint64_t scratch_bytes, void* stream);
/* vkr_shadow_mask_rt with "the frozen any-hit" replaced by the any hit above: the light passes through holes.  Every channel is
 * at least vkr_shadow_mask_rt's on the same input.  The gates of vkr_shadow_mask_rt, then those of the two entries above.     */
int vkr_shadow_mask_rt_cutout(const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel, const vkr_hit_attrib* attribs,
                              uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count, const vkr_shadow_rt_params* params,
                              const vkr_ray_cutout* cutout, const vkr_img* out_mask, void* scratch, uint64_t scratch_bytes, void* stream);
/* vkr_reflections_rt with "the closest hit" replaced by the closest hit above: the mirror ray goes on through holes and what it
 * meets behind them is shaded as vkr_reflections_rt shades a hit (at params->texture_lod; alpha_lod only decides the holes).
 * The gates of vkr_reflections_rt, and a NULL cutout is VKR_ERR_NULL.                                                          */
int vkr_reflections_rt_cutout(const vkr_img* depth, const vkr_img* normal, const vkr_img* rays, const vkr_accel* accel,
                              const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                              const vkr_reflect_rt_params* params, const vkr_ray_cutout* cutout, const vkr_img* out_reflections,
                              void* scratch, uint64_t scratch_bytes, void* stream);

/* ---- lit ray-traced reflections (DESIGN_NUMERICS.md, "Reflections, ray traced, lit") ----------------------------------------------
 * vkr_reflections_rt whose hit is lit and shadowed before it is stored: up to four point or directional lights (the convention of
 * vkr_shadow_rt_params), one shadow ray per light from the hit, a constant ambient term, and the albedo of the hit times the sum.
 * Everything up to and including the closest hit is vkr_reflections_rt's, bit for bit (vkr_reflections_rt_cutout's in the _cutout
 * entry).  For a hit (t, u, v, index) of ray (origin, dir), every operation rounded on its own, cfma the multiply-add contract 2
 * fuses:  P = cfma(t, dir, origin);  w = (1 - u) - v, Ni = (w n0 + u n1) + v n2 with n0..n2 = normals[index].n, Ns = normalize(Ni);
 * N = -Ns when dot(Ns, dir) > 0, else Ns (two-sided; a NaN normal stays NaN and is lit by ambient alone);  Po = P + shadow_offset N;
 * acc = ambient.rgb;  per light l < light_count in index order: dvec = lights[l].xyz - Po (w == 1) or lights[l].xyz (w == 0);
 * unless dot(N, dvec) > 0 the light adds nothing and casts no ray; it adds nothing when the frozen any-hit of (Po, dvec,
 * shadow_tmin, 1) reports a hit (vkr_accel_occluded's answer; vkr_accel_occluded_cutout's in the _cutout entry); otherwise
 * ld2 = dot(dvec, dvec), L = normalize(dvec), ndl = dot(N, L) or 0 unless ndl > 0, k = ndl for a directional light and
 * ndl * min'(1 / ld2, 1) for a point light (min'(q, 1) = q < 1 ? q : 1), acc.c = cfma(k, colour[l].c, acc.c).  The texel is
 * rint(255 clamp(albedo.c * acc.c)) per channel, alpha 0, albedo as vkr_reflections_rt computes it.  With light_count 0 and
 * ambient (1, 1, 1) the image is vkr_reflections_rt's.                                                                            */
typedef struct vkr_hit_normal { float n[3][4]; } vkr_hit_normal;   /* 48 bytes, one per INPUT triangle, in input order (device memory,
                                                                      16-byte aligned): the world-space normals of the three
                                                                      vertices, not normalised; n[k][3] is not read */
typedef struct vkr_reflect_lights {     /* 176 bytes */
  float    lights[4][4];                /* as vkr_shadow_rt_params.lights */
  float    colour[4][4];                /* rgb of light l; .w must be 0 */
  float    ambient[4];                  /* rgb; .w must be 0 */
  uint32_t light_count;                 /* 0..4 */
  float    shadow_offset;               /* the shadow ray starts at P + shadow_offset * N */
  float    shadow_tmin;                 /* its segment is Po + t * dvec, t in [shadow_tmin, 1] */
  uint32_t reserved[5];                 /* 0 */
} vkr_reflect_lights;
/* The arguments, scratch (vkr_reflections_rt_scratch_bytes) and gates of vkr_reflections_rt / vkr_reflections_rt_cutout, then,
 * still before any launch: lights NULL; normals NULL with triangles present; normals not 16-byte aligned; normal_count != the
 * structure's triangle count; light_count > 4; a light in use whose w is neither 0 nor 1; a non-zero .w of colour / ambient or a
 * non-zero reserved; shadow_offset or shadow_tmin NaN; a NaN in ambient or in the colour of a light in use.                     */
int vkr_reflections_rt_lit(const vkr_img* depth, const vkr_img* normal, const vkr_img* rays, const vkr_accel* accel,
                           const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_hit_normal* normals, uint32_t normal_count,
                           const vkr_img* textures, uint32_t texture_count, const vkr_reflect_rt_params* params,
                           const vkr_reflect_lights* lights, const vkr_img* out_reflections, void* scratch, uint64_t scratch_bytes,
                           void* stream);
int vkr_reflections_rt_lit_cutout(const vkr_img* depth, const vkr_img* normal, const vkr_img* rays, const vkr_accel* accel,
                                  const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_hit_normal* normals, uint32_t normal_count,
                                  const vkr_img* textures, uint32_t texture_count, const vkr_reflect_rt_params* params,
                                  const vkr_reflect_lights* lights, const vkr_ray_cutout* cutout, const vkr_img* out_reflections,
                                  void* scratch, uint64_t scratch_bytes, void* stream);
/* The twin of vkr_scene_triangles for vertex normals: one vkr_hit_normal per triangle, in its order, with its scratch
 * (vkr_scene_triangles_scratch_bytes) and its gates.  n[k] = transforms[t].normal * (norm, 0) of vertex k, computed as
 * (m[0][r] x + m[1][r] y) + m[2][r] z per row r: no translation, no fused multiply-add under either numeric contract, not
 * normalised (the pass normalises after interpolation); n[k][3] = 0.  A triangle with an index outside the vertex buffer gets NaN
 * normals, and nothing is read outside the buffer.  out: device, 16-byte aligned, room for out_capacity records.               */
int vkr_scene_triangle_normals(const vkr_raster_scene* scene, vkr_hit_normal* out, uint64_t out_capacity, void* scratch, uint64_t scratch_bytes,
                               void* stream);

/* ---- area lights in the traced shadow mask (DESIGN_NUMERICS.md, "Shadow mask, ray traced, area lights") ---------------------------
 * A light with a radius is a disk that faces the surface point; the channel is the share of S points of the disk that the surface
 * point sees, in 255ths.  Everything but the per-light step is vkr_shadow_mask_rt's.  Light l with radius[l] == 0 is traced as
 * vkr_shadow_mask_rt traces it (one ray, 0 or 255).  Otherwise, with dvec as there: wv = normalize(dvec); tangent_frame(wv, &T, &B);
 * the pattern slot of pixel (x, y) is p = (y & (P - 1)) * P + (x & (P - 1)); for k < S with (u, v) = samples[(p * S + k) * 2 ..]:
 * e = fma(v, B, u * T) per component, dvec_k = fma(radius[l], e, dvec) per component (multiply-adds as contract 2 fuses them),
 * sample k is cast when dot(n, dvec_k) > 0 and visible when cast and the frozen any-hit of (origin, dvec_k, tmin, 1) reports none.
 * With V visible samples the channel is (510 V + S) / (2 S) in unsigned integers: 255 V / S rounded half up.  A light at the
 * pixel's origin makes the frame NaN: no sample casts, the channel is 0.  For a directional light the disk sits at the tip of xyz:
 * radius / |xyz| is the tangent of its angular radius.  The table is data: any finite (u, v) is legal.                          */
typedef struct vkr_shadow_rt_soft {   /* 40 bytes */
  float        radius[4];      /* per light, world units; 0 = this light is traced as vkr_shadow_mask_rt traces it */
  uint32_t     sample_count;   /* S, 1..64 */
  uint32_t     pattern_side;   /* P: 1, 2 or 4 */
  const float* samples;        /* device, P*P*S*2 floats: (u, v) of sample k of pattern p at [(p*S + k)*2] */
  uint32_t     reserved[2];    /* 0 */
} vkr_shadow_rt_soft;
/* The gates of vkr_shadow_mask_rt, then: soft or soft->samples NULL, sample_count outside 1..64, pattern_side not 1, 2 or 4, a
 * radius (of a light in use) that is negative, NaN or infinite, reserved != 0.                                                */
int vkr_shadow_mask_rt_soft(const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel, const vkr_shadow_rt_params* params,
                            const vkr_shadow_rt_soft* soft, const vkr_img* out_mask, void* stream);
/* the same with the any hit of the cutout entries: the gates of vkr_shadow_mask_rt_cutout, then those above.  Every channel is at
 * least vkr_shadow_mask_rt_soft's on the same input.                                                                          */
int vkr_shadow_mask_rt_soft_cutout(const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel, const vkr_hit_attrib* attribs,
                                   uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                                   const vkr_shadow_rt_params* params, const vkr_ray_cutout* cutout, const vkr_shadow_rt_soft* soft,
                                   const vkr_img* out_mask, void* scratch, uint64_t scratch_bytes, void* stream);
/* Host only: the sample table the frame uses.  Pattern p, sample k: rho = sqrt((k + 0.5) / S), phi = k * 2.399963229728653 +
 * 2 pi * ((7 p) mod P^2) / P^2, (u, v) = (rho cos phi, rho sin phi), computed in double and rounded to fp32; out: P*P*S*2 floats.
 * Nothing is written for a NULL out, S outside 1..64 or P not 1, 2 or 4.                                                       */
void vkr_shadow_disk_samples(uint32_t sample_count, uint32_t pattern_side, float* out);

/* ---- the edge-aware filter of the shadow mask (DESIGN_NUMERICS.md, "Shadow mask, filter") ------------------------------------------
 * No reference program.  The reconstruction filter of a mask whose neighbouring pixels carry different sample patterns
 * (vkr_shadow_mask_rt_soft with pattern_side P; the box taps of vkr_shadow_mask): per pixel the tent-weighted mean of the mask over
 * the taps that lie on the pixel's own surface.  With reach == P every one of the P * P patterns enters a fully accepted pixel
 * with the same weight: (R - |d|) over |d| < R gives every residue class mod R the total weight R.                             */
typedef struct vkr_shadow_filter_params {   /* 96 bytes */
  vkr_mat4 inverse_camera;                  /* view -> world, as in vkr_shadow_rt_params */
  float    fovy, aspect, znear, zfar;
  uint32_t reach;                           /* R, 1..4: taps at |dx|, |dy| < R; 1 copies the mask */
  float    normal_min_dot;                  /* a tap is accepted only if dot(n_g, n_t) >= this */
  float    plane_tolerance;                 /* ... and |dot(n_g, W_t - W_g)| <= plane_tolerance * |view_g.z| */
  uint32_t reserved;                        /* 0 */
} vkr_shadow_filter_params;
/* depth: D24_UNORM_S8 (mip 0 of the view); normal: RG16_UNORM; mask, out_mask: RGBA8_UNORM; whole frames of one extent.  Per pixel g:
 * d_g = the exact decode of depth texel g; d_g >= 1 (sky) stores mask[g].  Otherwise view_g, W_g = world and n_g are those of
 * vkr_shadow_mask_rt for pixel g (uv = (g + 0.5) / extent, reconstruct_view_vec, inverse_camera * (view, 1), decode_normal of the
 * texel by index).  Tap t = g + (dx, dy), |dx|, |dy| < R, has the integer weight w = (R - |dx|)(R - |dy|).  The centre tap is always
 * accepted; another tap is accepted when it lies inside the image, d_t < 1, dot(n_g, n_t) >= normal_min_dot and
 * |dot(n_g, W_t - W_g)| <= plane_tolerance * |view_g.z| (W_t - W_g three subtractions, each dot product x, then y, then z with the
 * multiply-adds contract 2 fuses, the bound one multiplication; a compare with a NaN is false: the tap is rejected).  In unsigned
 * integers, A = the sum of w and V_c = the sum of w * mask[t].c over the accepted taps (one accept set for the four channels):
 * out[g].c = (2 V_c + A) / (2 A), the weighted mean rounded half up.  Every texel of out_mask is written, nothing outside it.
 * Refused before any launch: a NULL argument, a descriptor without memory, other formats, different extents, an extent above
 * 65535, a windowed descriptor anywhere (the taps cross strip borders: a single-GPU pass), reach outside 1..4, normal_min_dot or
 * plane_tolerance NaN, reserved != 0, mask and out_mask whose memory overlaps (the taps read neighbours: never in place).      */
int vkr_shadow_mask_filter(const vkr_img* depth, const vkr_img* normal, const vkr_img* mask, const vkr_shadow_filter_params* params,
                           const vkr_img* out_mask, void* stream);

/* ---- the temporal accumulation of the shadow mask (DESIGN_NUMERICS.md, "Shadow mask, temporal accumulation") ----------------------
 * No reference program.  The running mean of the mask over the frames in which a pixel saw the same world point: what makes the
 * sample patterns of consecutive frames (vkr_shadow_disk_samples_frame) one larger pattern.  It runs after the mask and before
 * vkr_shadow_mask_filter.                                                                                                        */
typedef struct vkr_shadow_accum_params {   /* 160 bytes */
  vkr_mat4 inverse_camera;                 /* view -> world, this frame (as vkr_shadow_rt_params) */
  vkr_mat4 prev_inverse_camera;            /* view -> world, the frame that wrote prev_depth and the history */
  float    fovy, aspect, znear, zfar;      /* one lens for both frames, as vkr_gtao_accumulate assumes */
  uint32_t max_count;                      /* 1..255: the history weighs at most max_count - 1 frames; 1 copies the mask */
  float    plane_tolerance;                /* as vkr_shadow_filter_params.plane_tolerance */
  uint32_t reset;                          /* 0 or 1: 1 = no pixel has a history (camera cut, moved light) */
  uint32_t reserved;                       /* 0 */
} vkr_shadow_accum_params;
/* depth, prev_depth: D24_UNORM_S8 (mip 0 of the view); normal: RG16_UNORM; velocity: RG16_SFLOAT (prev_uv - uv); mask, out_mask:
 * RGBA8_UNORM; history, out_history: RGBA16_UNORM (the running mean per light in 65535ths: a mask code m is 257 m); history_count,
 * out_count: R8_UNORM (the raw byte is the number n of frames in the mean, 0 = none); whole frames of one extent w x h.  Per pixel g:
 * m = mask[g]; d_g, uv_g, view_g, W_g, n_g as vkr_shadow_mask_filter has them; vel = the exact decode of velocity texel g;
 * p = uv_g + vel, f = (p.x * (float)w, p.y * (float)h), every operation rounded on its own; q = floor(f), inside when
 * 0 <= f.x < w and 0 <= f.y < h on the floats (a compare with a NaN is false).  The history of g is valid when reset == 0,
 * d_g < 1, q is inside, n = history_count[q] >= 1, d_q = prev_depth[q] < 1 and
 * |dot(n_g, W'_q - W_g)| <= plane_tolerance * |view_g.z| with W'_q = prev_inverse_camera * (reconstruct_view_vec(uv_q, d_q), 1),
 * subtraction, dot and bound as in the filter's plane test (a NaN: invalid).  In unsigned integers per channel c: without a valid
 * history n' = 1 and H'_c = 257 m_c; with one n' = min(n, max_count - 1) + 1 and H'_c = (H_c (n' - 1) + 257 m_c + (n' >> 1)) / n',
 * H = history[q].  out_history[g] = H', out_count[g] = n', out_mask[g].c = (255 H'_c + 32767) / 65535.  Every texel of the three
 * outputs is written, nothing outside them.
 * Refused before any launch: a NULL argument, a descriptor without memory, other formats, different extents, an extent above
 * 65535, a windowed descriptor anywhere (the reprojection reaches across strips: a single-GPU pass), max_count outside 1..255,
 * reset > 1, reserved != 0, plane_tolerance NaN, an output whose memory overlaps another image's — but mask and out_mask may be
 * one image (same memory, same pitch): a pixel reads and writes only its own texel of them.                                      */
int vkr_shadow_mask_accumulate(const vkr_img* depth, const vkr_img* normal, const vkr_img* velocity, const vkr_img* prev_depth,
                               const vkr_img* mask, const vkr_img* history, const vkr_img* history_count,
                               const vkr_shadow_accum_params* params,
                               const vkr_img* out_history, const vkr_img* out_count, const vkr_img* out_mask, void* stream);
/* Host only: vkr_shadow_disk_samples for frame `frame` of a cycle of T = frame_count frames: the same layout and rho,
 * phi = k * 2.399963229728653 + 2 pi * (((7 p) mod P^2) * T + (frame mod T)) / (P^2 * T): the T tables together are P^2 * T evenly
 * spaced rotations, and T == 1 gives the floats of vkr_shadow_disk_samples bit for bit.  Nothing is written for a NULL out,
 * S outside 1..64, P not 1, 2 or 4, or T outside 1..64.                                                                         */
void vkr_shadow_disk_samples_frame(uint32_t sample_count, uint32_t pattern_side, uint32_t frame, uint32_t frame_count, float* out);

/* ---- octahedral probes (probe_renderer.{hpp,cpp}: programs cubemap_probe, cube2oct, probe_downsample, trace_probe) ------------------------
 * Array images follow vkr_deinterleave_depth: one descriptor per layer.  The layers of one array must share format, extent,
 * mip count and pitches, and lie at regular distances: for every mip m, layer l starts at layer 0's mip m plus l times one
 * per-mip stride (the layout of an array image).  A cube is 6 layers in face order +X, -X, +Y, -Y, +Z, -Z, sampled with the
 * frozen seamless rules of DESIGN_NUMERICS.md (face ties x over y over z; a corner tap is the average of its three texels).  */
#define VKR_PROBE_ZNEAR 0.05f  /* cube2oct/shader.comp:10-11, trace_probe/shader.comp:117-118 */
#define VKR_PROBE_ZFAR  80.0f
/* program "cube2oct": probe_renderer.cpp:171-202 + cube2oct/shader.comp.  cube_color: 6 RGBA8_SRGB layers, cube_distance: 6
 * R16F layers (one square extent); oct_color RGBA8_UNORM and oct_depth R16_UNORM (mip 0 is written) of one extent.  Only the
 * dispatch extent floor(w/8)*8 x floor(h/4)*4 is written, with uv = pixel / that extent.                                     */
int vkr_cube2oct(const vkr_img* cube_color, const vkr_img* cube_distance, const vkr_img* oct_color, const vkr_img* oct_depth,
                 void* stream);
/* program "cubemap_probe": ProbeRenderer::render_cubemap / render_side (probe_renderer.cpp:72-160) + cubemap_probe/shader.{vert,
 * frag} as a compute rasteriser: the six faces of the cube at `pos` from one set of launches.  Face f (+X, -X, +Y, -Y, +Z, -Z) is
 * drawn with view = lookAt(pos, pos + fwd, up) of calc_matrix (up (0,-1,0); +Y: (0,0,1), -Y: (0,0,-1)) and projection =
 * perspective(radians(90), 1, 0.05, 80), both evaluated on the host in fp32; the vertex stage is view_pos = (view * model) * pos,
 * clip = projection * view_pos.  A draw whose albedo_index is 0xFFFFFFFF is skipped.  The raster rules are those of
 * vkr_raster_gbuffer (pixel centres, top-left fill rule, 8 sub-pixel bits, cull none, D24 LESS_OR_EQUAL with the later triangle
 * winning a tie, near-plane clip, implicit LOD, the alpha-0 discard at coverage time, VKR_RASTER_DRAW_OPAQUE_ALBEDO).  Colour: the
 * trilinear sRGB albedo as RGBA8_SRGB; distance: length of the interpolated view-space position as fp16 (round to nearest even).
 * Clears: colour codes (255, 0, 0, 0) (the reference clears to (100, 0, 0, 0)), distance 100.0.  cube_color / cube_distance: 6
 * descriptors each, the layers of one regular array (one square extent, one pitch, one stride between consecutive layers).
 * `scratch`: vkr_cubemap_probe_scratch_bytes(cube size, triangles summed over ALL draws of the scene) of device memory. */
uint64_t vkr_cubemap_probe_scratch_bytes(uint32_t cube_size, uint32_t triangle_count);
int vkr_cubemap_probe(const vkr_raster_scene* scene, const float pos[3], const vkr_img* cube_color /* 6 x RGBA8_SRGB */,
                      const vkr_img* cube_distance /* 6 x R16_SFLOAT */, void* scratch, uint64_t scratch_bytes, void* stream);
/* program "probe_downsample": probe_renderer.cpp:204-236 + probe_downsample/shader.frag.  Mip i >= 1 of the R16_UNORM view is
 * the min of the 2 x 2 texels of mip i - 1 at min(2 * pixel + o, size) (not size - 1: a fetch past the edge reads 0).        */
int vkr_probe_downsample(const vkr_img* depth_layer_all_mips, void* stream);
/* Constants, probe_renderer.cpp:332-341 / trace_probe/shader.comp:12-22 (116 bytes) */
typedef struct vkr_probe_trace_consts {
  vkr_mat4 inverse_view;       /* camera -> world */
  float    probe_min[4], probe_max[4];
  uint32_t grid_size;
  float    fovy, aspect, znear, zfar;
} vkr_probe_trace_consts;
/* program "trace_probe": probe_renderer.cpp:323-394 + trace_probe/shader.comp:48-82, 101-115, 175-347, 410-441.  Bindings 0
 * depth (D24, full resolution, mip 0), 1 normal (RG16_UNORM), 2 the probe colour array (RGBA8_UNORM), 3 the probe depth array
 * (R16_UNORM, all mips), 4 consts, 5 out (RGBA8_UNORM).  layer_count >= grid_size^2, grid_size >= 2.  Only the dispatch extent
 * floor(w/8)*8 x floor(h/4)*4 of `out` is written.  A hit stores the bilinear probe colour, a miss, an unresolved trace and sky
 * store 0.  Single-GPU images only (no windows).                                                                              */
int vkr_trace_probe(const vkr_img* depth, const vkr_img* normal, const vkr_img* color_layers, const vkr_img* depth_layers,
                    uint32_t layer_count, const vkr_probe_trace_consts* consts, const vkr_img* out, void* stream);

/* ---- image transfers (util_passes.cpp: clear_depth, clear_color, blit_image, gen_mipmaps; scene/images.cpp:93-160) -----------------------
 * Whole-image operations: every entry refuses, before it launches anything, a NULL descriptor, an unknown format and a descriptor
 * that is a window of a larger frame (origin != 0 or full_* != width / height).  Conversions use the library's codecs: a texel
 * decodes to float RGBA with absent channels 0, 0, 0, 1 (UNORM: the correctly rounded k / (2^b - 1); RGBA8_SRGB: rgb through the
 * EOTF table, alpha linear) and is stored as that format stores: sRGB threshold rule for the rgb of RGBA8_SRGB, UNORM
 * rint(clamp(x, 0, 1) * (2^b - 1)), fp16 round to nearest even, fp32 unchanged (DESIGN_NUMERICS.md, "Image transfers").        */
typedef struct vkr_clear_value {
  float    color[4];   /* colour formats                                    */
  float    depth;      /* D24_UNORM_S8: rint(clamp(depth, 0, 1) * 16777215), NaN -> 0 */
  uint32_t stencil;    /* ... | (stencil & 0xFF) << 24                      */
} vkr_clear_value;
/* vkCmdClearColorImage / vkCmdClearDepthStencilImage over every mip of the view, one launch.  Only the texels of a row are written
 * (not the padding up to the pitch), so clearing one layer's descriptor of an array image leaves the other layers alone.          */
int vkr_clear_image(const vkr_img* img, const vkr_clear_value* value, void* stream);
#define VKR_FILTER_NEAREST 0u
#define VKR_FILTER_LINEAR  1u
/* vkCmdBlitImage of whole mip 0 of `src` onto whole mip 0 of `dst` (what both callers of the reference do, util_passes.cpp:152-179),
 * between any two colour formats and any two extents.  Destination texel (i, j) samples the source at u = (i + 0.5) * (src_w /
 * dst_w), v alike: NEAREST takes texel floor(u); LINEAR takes the taps floor(u - 0.5) and that plus one, clamped to the edge, with
 * weight frac(u - 0.5), mixed like the sampler's bilinear filter.  D24_UNORM_S8 blits only to D24_UNORM_S8, only with NEAREST and
 * only at equal extents (the stored words are copied).  src and dst must not be the same memory.                                */
int vkr_blit_image(const vkr_img* src, const vkr_img* dst, uint32_t filter, void* stream);
/* Levels 1 .. mip_count - 1 of the view from level 0, by the project's one mip rule (vk-renderer_amd/scene.py build_mips), which
 * is NOT a Vulkan blit on odd extents: level extents max(1, s / 2); destination texel (X, Y) is ((a + b) + (c + d)) * 0.25 in fp32
 * of the source texels (2X, 2Y), (min(2X + 1, w - 1), 2Y) and the same in the row min(2Y + 1, h - 1), per channel, decoded from
 * the stored previous level and stored again (RGBA8_SRGB: rgb through the EOTF table, alpha linear).  Formats: RGBA8_SRGB,
 * RGBA8_UNORM, RGBA16_SFLOAT, RG16_SFLOAT, R16_SFLOAT, R32_SFLOAT, R8_UNORM; D24_UNORM_S8 is refused (vkr_depth_mips is the depth
 * pyramid).  Two schedules that leave the same bytes: one launch per level, or 64 x 64 source tiles reduced through LDS over up
 * to six levels per launch (VKR_SWITCH_MIPS_PER_LEVEL / VKR_SWITCH_MIPS_FUSED force one).                                       */
int vkr_gen_mipmaps(const vkr_img* img, void* stream);

/* Multi-GPU exchange helper (the reference is single-GPU, so there is no program this
 * replaces): copies `count` pitch-linear byte rectangles on `stream`, VKR_MAX_RECTS per launch.  Used to pack
 * a tile's surfaces for the all-gather, to scatter the gathered tiles into the whole-frame images and to
 * pack / unpack the halo rings of the history surfaces.  Addresses are device addresses; addresses, pitches
 * and row lengths must be multiples of 4 bytes (16 selects the wide path).  `rects` is host memory.       */
#define VKR_MAX_RECTS 64
typedef struct vkr_rect_copy {
  uint64_t src, dst;
  uint32_t src_pitch, dst_pitch; /* bytes between rows */
  uint32_t row_bytes, rows;
} vkr_rect_copy;
int vkr_copy_rects(const vkr_rect_copy* rects, uint32_t count, void* stream);

/* ---- the wire of the multi-GPU frame: RCCL over xGMI (SURVEY.md 8(b) "vkr_halo_exchange", 8(e)) -------------
 * One process per GPU.  Rank 0 makes an id (vkr_comm_unique_id) and hands its bytes to every rank out of band (a
 * file, a TCP store, MPI ...); every rank then calls vkr_comm_create, collectively, with its device current.  RCCL is
 * loaded with dlopen on first use (librccl.so.1, or $VKR_RCCL_LIBRARY): the library does not link against it.
 * Both exchanges are ONE grouped RCCL launch on `stream` and return at once; buffers are device memory.          */
#define VKR_COMM_ID_BYTES 128
typedef struct vkr_comm vkr_comm;
int vkr_comm_unique_id(uint8_t* id_bytes /* [VKR_COMM_ID_BYTES] */);
int vkr_comm_create(const uint8_t* id_bytes, int rank, int world, vkr_comm** out);
int vkr_comm_destroy(vkr_comm* comm);
int vkr_comm_rank(const vkr_comm* comm, int* rank, int* world);
/* 0 when RCCL can be loaded in this process (nothing collective happens); a launcher checks this on EVERY rank and
 * agrees on the result over its control plane before the collective vkr_comm_create, so that a rank without RCCL
 * cannot leave the others blocked inside ncclCommInitRank                                                          */
int vkr_comm_available(void);
/* A communicator that moves NOTHING and takes the time a fully connected xGMI node would (measurement facility, no RCCL
 * needed): every exchange enqueues, on the caller's stream, a one-wave kernel that holds the stream for
 * launch_us + (bytes on the busiest link) / link_gbps — each peer on a link of its own, full duplex: an all-gather costs
 * the largest share any peer sends, a point-to-point group the largest per-peer total — and copies the rank's own share of
 * an out-of-place all-gather into its slot.  What the peers would have sent is whatever the receive buffers already hold:
 * with a static scene and buffers filled once by real peers (the in-process lockstep harness) every frame receives what it
 * would have received, so the frame's stream / event schedule runs against realistic wire times on ONE GPU
 * (tools/wire_emulation.py, vkrh_tiled_emulate_wire).                                                                   */
int vkr_comm_create_emulated(int rank, int world, float link_gbps, float launch_us, vkr_comm** out);
/* Start-up check of a fresh communicator, collective: every rank gathers a rank-tagged pattern through vkr_all_gather
 * and vkr_all_gather_v (shares of different sizes, in place) and trades one with each neighbour rank through
 * vkr_halo_exchange, on `stream`, then verifies every byte it received (synchronises the stream).  0 = the wire delivers
 * what the tiled frame expects.  scratch: device memory of at least vkr_comm_selfcheck_bytes(world) bytes.          */
uint64_t vkr_comm_selfcheck_bytes(int world);
int vkr_comm_selfcheck(vkr_comm* comm, void* scratch, void* stream);
/* all-gather of several surfaces at once: recv receives [rank][bytes] from every rank's send (out of place; with
 * horizontal strips a tile's rows of a surface are contiguous, so recv can be the whole-frame image itself)       */
typedef struct vkr_gather_part { const void* send; void* recv; uint64_t bytes; } vkr_gather_part;
int vkr_all_gather(vkr_comm* comm, const vkr_gather_part* parts, uint32_t count, void* stream);
/* the same for shares of different sizes (strips balanced by cost): rank r's share of a surface lies at
 * recv + offsets[r] .. recv + offsets[r + 1] (offsets: world + 1 entries in host memory, identical on every rank; an
 * empty share is allowed); `send` is this rank's share where it lies now.  One grouped launch: every share sent straight
 * to each peer and received into place (ncclSend / ncclRecv: on a fully connected xGMI node a share crosses one link once;
 * RCCL fuses the point-to-point operations of a group), the own share copied on the stream.  VKR_GATHER_V_BROADCAST=1
 * (read at the first call) selects one ncclBroadcast per share, rooted at its owner, instead.                        */
typedef struct vkr_gather_v_part { const void* send; void* recv; const uint64_t* offsets; } vkr_gather_v_part;
int vkr_all_gather_v(vkr_comm* comm, const vkr_gather_v_part* parts, uint32_t count, void* stream);
/* halo refresh of one history surface: per neighbour the packed slice to send and the buffer to receive into
 * (either may be empty); pack / unpack with vkr_copy_rects around it                                               */
typedef struct vkr_halo_peer { int32_t peer; uint32_t reserved; const void* send; uint64_t send_bytes; void* recv; uint64_t recv_bytes; } vkr_halo_peer;
int vkr_halo_exchange(vkr_comm* comm, const vkr_halo_peer* peers, uint32_t count, void* stream);

/* ---- hit colours and hit normals by request / reply (multi-GPU; instead of all-gathering whole-frame surfaces) --------
 * filter.comp:112-134 reads the albedo bilinearly at the hit position of every valid ray, trace.comp:103-109 the downsampled
 * normal at the hit position of every candidate — anywhere in the frame.  A rank asks the owning ranks for exactly the
 * footprint rows it does not hold and writes the answers into its whole-frame images where an all-gather would have put
 * them (csrc/hit_exchange.hip; host/frame.hpp drives the steps and moves requests and replies with vkr_halo_exchange).
 * Strips: rank r owns full-res frame rows [row_bounds[r], row_bounds[r + 1]) (even numbers) and the half-res rows at half
 * of them.  A request is 4 bytes — bits 0..13 the frame row, 14..27 the left texel of the texel pair (<= width - 2),
 * VKR_HIT_BOTH_ROWS: also the row below (the two rows of a footprint usually have one owner), VKR_HIT_NORMAL: the
 * half-res normal image instead of the full-res albedo — and is answered with 16 bytes: the pair of the row and of the row
 * below it.  Frames up to 16384 x 16384.                                                                                */
typedef uint32_t vkr_hit_request;
#define VKR_HIT_BOTH_ROWS 0x10000000u
#define VKR_HIT_NORMAL    0x20000000u
typedef struct vkr_hit_sources {
  const vkr_img* rays;            /* RGBA16_UNORM, the rank's half-res window: albedo rows for every ray with w != 1           */
  uint32_t albedo_width, albedo_height;
  uint32_t window_row0, window_row1;   /* the full-res frame rows this rank holds                                             */
  const vkr_img* pending_mask;    /* or NULL: no normal requests.  R8 + RGBA32F of vkr_sssr_trace_windowed: normal rows for   */
  const vkr_img* pending_data;    /* every pending ray, outside half-res rows [normal_row0, normal_row1)                       */
  uint32_t normal_width, normal_height, normal_row0, normal_row1;
} vkr_hit_sources;
/* Two passes over the same `src` and bounds.  Pass 1 (out == NULL): counts[o] += number of requests this rank has for
 * owner o (counts: device, world entries, zeroed by the caller); with a workspace (device, VKR_HIT_WORKSPACE_WORDS uint32,
 * no initialisation needed) it also leaves there what pass 2 needs.  Pass 2 (out != NULL; workspace as pass 1 filled it):
 * writes the requests, owner o's from out[segments[o]] on (segments: host, world entries, the prefix sums of counts).    */
#define VKR_HIT_WORKSPACE_WORDS 4096u
int vkr_hit_requests(const vkr_hit_sources* src, const uint32_t* row_bounds, uint32_t world, uint32_t* counts, uint32_t* workspace,
                     const uint32_t* segments, vkr_hit_request* out, void* stream);
/* Pass 2 into segments of FIXED capacity (sized from the previous frame's counts, so that both ends of the exchange know the
 * message sizes without waiting for this frame's): owner o's requests from out[segments[o]] on, at most capacities[o] of them —
 * what does not fit is dropped (the caller compares this frame's counts with the capacities afterwards and repeats the round
 * exactly if any segment overflowed).  Slots a segment does not use must hold VKR_HIT_NO_REQUEST (fill `out` with 0xFF bytes
 * first): vkr_hit_reply answers such a slot with zeros and counts no error, vkr_hit_scatter skips it.                      */
#define VKR_HIT_NO_REQUEST 0xFFFFFFFFu
int vkr_hit_requests_bounded(const vkr_hit_sources* src, const uint32_t* row_bounds, uint32_t world, uint32_t* workspace,
                             const uint32_t* segments, const uint32_t* capacities, vkr_hit_request* out,
                             uint32_t* dropped_flag /* device word, zeroed by the caller: set to 1 when a request was dropped */, void* stream);
/* replies (device, 16 bytes each, 16-byte aligned): the texel pair(s) of requests[i] from this rank's albedo / downsampled-
 * normal window (normals may be NULL when no normal request can arrive); a request for texels the window does not hold
 * answers 0, increments error_counter[0] and leaves one such request and its index in error_counter[1], [2] (3 words)                                                                              */
#define VKR_HIT_REPLY_BYTES 16u
int vkr_hit_reply(const vkr_img* albedo, const vkr_img* normals, const vkr_hit_request* requests, uint32_t count, void* replies,
                  uint32_t* error_counter, void* stream);
int vkr_hit_scatter(const vkr_img* frame_albedo, const vkr_img* frame_normals, const vkr_hit_request* requests, const void* replies,
                    uint32_t count, void* stream);

/* Measurement switches — the library's only process-wide state.  The environment (VKR_BLUR_NO_SKIP, VKR_FILTER_NO_SKIP,
 * VKR_TAA_GENERIC, VKR_SHADING_GENERIC, VKR_BLUR_GENERIC, VKR_BLUR_LANE_LOOPS, VKR_TRACE_ONE_LAUNCH, VKR_MIPS_PER_LEVEL, VKR_MIPS_FUSED, VKR_BLUR_NO_FLAT, VKR_BLUR_COUNT_PATHS) is read once, at the first launch that asks; afterwards only vkr_set_switches
 * changes them.  NO_SKIP: evaluate every tap of the blur / filter even in tiles without a reflection / hit (a
 * content-independent time; the stored texels are the same wherever every weight is finite).  GENERIC: the TAA /
 * shading instantiations that do not assume equal window layouts.                                                  */
#define VKR_SWITCH_BLUR_NO_SKIP    1u
#define VKR_SWITCH_FILTER_NO_SKIP  2u
#define VKR_SWITCH_TAA_GENERIC     4u
#define VKR_SWITCH_SHADING_GENERIC 8u
#define VKR_SWITCH_BLUR_GENERIC    16u /* every wave of the blur on the per-lane Gaussian loop (no wave-uniform-sigma path) */
#define VKR_SWITCH_BLUR_LANE_LOOPS 64u /* waves that do not share one sigma on the per-lane tap loops of rounds 1-3 instead of the transposed packed rows (blur_rows) */
#define VKR_SWITCH_TRACE_ONE_LAUNCH 32u /* read by the HOST layer (host/gpu): program "sssr_trace" as one launch (vkr_sssr_trace) instead of
                                          * head + resume (vkr_sssr_trace_split); the library's entries do what their names say either way */
#define VKR_SWITCH_MIPS_PER_LEVEL 128u /* vkr_gen_mipmaps: one launch per level ... */
#define VKR_SWITCH_MIPS_FUSED     256u /* ... or the fused tiles, whatever the default is (per level wins if both are set); same bytes */
#define VKR_SWITCH_BLUR_NO_FLAT   512u /* blur tiles whose staged normals are one RG16 code on the per-tap normal weight, like every other tile (BLUR_GENERIC implies it) */
#define VKR_SWITCH_BLUR_COUNT_PATHS 1024u /* every blur block adds itself to the counters vkr_debug_blur_paths reads (one atomic per block; off: none) */
uint32_t vkr_get_switches(void);
void vkr_set_switches(uint32_t mask);
/* Blocks of the blur launches since the last reset that ran with VKR_SWITCH_BLUR_COUNT_PATHS: out[0] empty tiles (skipped), [1] lit
 * tiles whose staged normals are one code ("flat"), [2] the other lit tiles, [3] blocks with at least one wave on a
 * constant-normal-weight tap loop.  Waits for the device; reset != 0 zeroes the counters afterwards.                        */
int vkr_debug_blur_paths(uint32_t out[4], int reset);

/* float4 streaming-read microbenchmark: the measured-roofline denominator of
 * SURVEY.md 8(d).  Reads `bytes` from `src`, writes one float per block to `sink`.      */
int vkr_stream_read(const void* src, uint64_t bytes, float* sink, uint32_t sink_len, void* stream);

/* Test hook: counts (into 5 device uint32, zeroed by the caller) where the kernels' cheap exact
 * arithmetic — normal-range division, UNORM decodes — disagrees with its IEEE definition.        */
int vkr_selftest_division(uint32_t* device_counters5, float znear, float zfar, void* stream);
/* Test hook: counts (into one device uint32, zeroed by the caller) the pixel centres g < size, size = 1..max_size (<= 65535),
 * whose uv = (g + 0.5) / size differs between the kernels' normal-range division and IEEE '/'.     */
int vkr_selftest_pixel_uv(uint32_t* device_counter, uint32_t max_size, void* stream);
/* Test hook: [0] counts the floats x in [2^-96, FLT_MAX] — all of them — whose cheap exact square root (vkr_device.hpp
 * sqrt_ieee) differs from sqrtf(x); [1] the floats s in [2^-48, 2^64] whose cheap exact reciprocal differs from 1.0f / s
 * (two device uint32, zeroed by the caller)                                                                       */
int vkr_selftest_sqrt(uint32_t* device_counters2, void* stream);
/* Test hook: counts (into one device uint32, zeroed by the caller) the fp32 bit patterns — all 2^32 of them: NaNs, +-0,
 * negatives, denormals, values >= 1 and infinities included — for which the texdraw pass's sRGB encode (vkr_device.hpp
 * float_to_srgb8_fast: an arithmetic estimate of the code corrected by one threshold compare) differs from the binary search
 * of the blit and the mips (float_to_srgb8_lds).                                                                   */
int vkr_selftest_srgb_encode(uint32_t* device_counter, void* stream);
/* Test hook: counts (into one device uint32, zeroed by the caller) the pairs (numerator < 2^24, n' in 1..255) — all of them — for
 * which the division of vkr_shadow_mask_accumulate (an fp32 reciprocal estimate corrected by its remainder) differs from '/'.  */
int vkr_selftest_accum_division(uint32_t* device_counter, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKR_POSTFX_H_INCLUDED */
