// frame.hpp — headless frame driver: the per-frame pass order of the reference's main loop
// (src/main.cpp:261-274 construction, :345-391 passes, :416-420 history remaps) around the
// rendergraph mirror, plus a flat C interface (vkrh_*) so Python launchers (bench.py, tests,
// the multi-GPU driver) can run it one stage at a time and interleave RCCL exchanges.
#ifndef VKR_HOST_FRAME_HPP_INCLUDED
#define VKR_HOST_FRAME_HPP_INCLUDED
#include <stdint.h>
#include "../../include/vkr_postfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vkrh_config {
  uint32_t full_width, full_height;  /* whole frame                                        */
  int32_t  origin_x, origin_y;       /* window of the frame held by this process           */
  uint32_t width, height;            /* window extent (== full on one GPU)                 */
  uint32_t tiled;                    /* 1: SSR reads the gathered whole-frame images       */
  void*    stream;                   /* HIP stream all passes are recorded on              */
} vkrh_config;

/* views / projection as 16 floats, column-major (glm layout) */
typedef struct vkrh_camera {
  float view[16], prev_view[16], projection[16];
  float fovy, aspect, znear, zfar;
} vkrh_camera;

enum {
  VKRH_STAGE_LUT        = 1u << 0,  /* ssr.preintegrate_pdf (main.cpp:269)                              */
  VKRH_STAGE_GBUFFER    = 1u << 1,  /* synthetic G-buffer for the current camera (replaces main.cpp:345) */
  VKRH_STAGE_PREV_DEPTH = 1u << 2,  /* prev_depth mip 0 from the previous camera + its Hi-Z mips        */
  VKRH_STAGE_DOWNSAMPLE = 1u << 3,  /* downsample_pass.run (main.cpp:347)                               */
  VKRH_STAGE_HIZ_TAIL   = 1u << 4,  /* tiled only: coarse mips of the gathered whole-frame pyramid       */
  VKRH_STAGE_SSR        = 1u << 5,  /* ssr.run: trace, filter, blur (main.cpp:375)                       */
  VKRH_STAGE_GTAO       = 1u << 6,  /* gtao main, filter, accumulate (main.cpp:384-388)                  */
  VKRH_STAGE_TAA        = 1u << 7,  /* taa_pass.run (main.cpp:391)                                       */
  VKRH_STAGE_SHADING    = 1u << 8,  /* shading_pass.draw -> color_out_tex, which TAA then resolves (main.cpp:390) */
  VKRH_STAGE_BRDF_LUT   = 1u << 9,  /* ssr.preintegrate_brdf (main.cpp:270)                             */
  VKRH_STAGE_GTAO_MAIN_ONLY = 1u << 10, /* gtao.add_main_pass alone (BASELINE configs[0])                 */
  /* passes the reference ships but never records                           */
  VKRH_STAGE_GTAO_GRAPHICS      = 1u << 11, /* gtao.add_main_pass_graphics, add_filter_pass, add_reprojection_pass */
  VKRH_STAGE_GTAO_DEINTERLEAVED = 1u << 12, /* gtao.deinterleave_depth, add_main_pass_deinterleaved                */
  VKRH_STAGE_SCREEN_TRACE       = 1u << 13, /* ScreenSpaceTrace main, filter, accumulate                           */
  VKRH_STAGE_SSR_CLASSIFIED     = 1u << 14, /* ssr.run with tile classification + indirect trace (advanced_ssr.cpp:547-550) */
  VKRH_STAGE_SSR_TRACE          = 1u << 15, /* first half of ssr.run: the trace (needs the Hi-Z pyramid)                    */
  VKRH_STAGE_SSR_RESOLVE        = 1u << 16, /* second half of ssr.run: filter + blur (needs albedo at the hit positions)      */
  VKRH_STAGE_RASTER             = 1u << 17, /* scene_renderer.draw_taa on the loaded scene (main.cpp:345) instead of the generator */
  /* tiled, hit normals by request: the trace as two stages around the arrival of the gathered pyramid — the head marches on the
   * window's own levels 1..gathered_mips and parks what needs more, the resume finishes the parked rays on the whole-frame
   * pyramid (after VKRH_STAGE_HIZ_TAIL).  HEAD + RESUME leave what VKRH_STAGE_SSR_TRACE leaves.                          */
  VKRH_STAGE_SSR_TRACE_HEAD     = 1u << 18,
  VKRH_STAGE_SSR_TRACE_RESUME   = 1u << 19,
  VKRH_STAGE_DOWNSAMPLE_NEXT    = 1u << 20,  /* the downsample of the NEXT frame into the G-buffer's second set (pipelined tiled frame) */
  /* main.cpp:379-388, the use_rt_ao branch: gtao.add_main_rt_pass against the loaded scene's acceleration structure (built by
   * vkrh_load_scene), add_filter_pass, add_accumulate_pass.  One GPU only (not on a tiled frame), not together with
   * VKRH_STAGE_GTAO (both write GTAO's images), and only after vkrh_load_scene.                                           */
  VKRH_STAGE_GTAO_RT            = 1u << 21,
  /* ProbeTracePass::run on the G-buffer's depth and normal through the probe grid of the last vkrh_bake_probes -> image
   * "probe_trace" (RGBA8_UNORM, full resolution).  One GPU only (not on a tiled frame), and only after a bake.            */
  VKRH_STAGE_PROBE_TRACE        = 1u << 22,
  /* main.cpp:346: scene_renderer.render_shadow for every configured light (vkrh_set_shadow_lights; by default the one light of
   * main.cpp:295 on layer 0) into the layers of image "shadows" (main.cpp:279-287: 1024^2, 4 layers, D24S8; vkrh_image_layer),
   * recorded after the raster stage and before the downsample.  Once it has run, VKRH_STAGE_SHADING binds layer 0 of "shadows" at
   * binding 5 instead of its 16x16 dummy (the shader never reads it: color_out does not change).  One GPU only (not on a tiled
   * frame), and only after vkrh_load_scene.                                                                              */
  VKRH_STAGE_SHADOW             = 1u << 23,
  /* main.cpp:306: clear_depth(graph, gbuffer.prev_depth) — every mip of prev_depth to depth 1, stencil 0 (the word 0x00FFFFFF) —
   * recorded before every other stage of the run.  One GPU only (not on a tiled frame: transfers take whole images).           */
  VKRH_STAGE_CLEAR_PREV_DEPTH   = 1u << 24,
  /* SSAOPass::draw (ssao.cpp:54-97; the reference ships the pass, its frame loop never records it): gbuffer.depth (mip 0 only)
   * -> image "ssao" (R8_UNORM at the frame's extent, created on first use; vkrh_image) with the frame camera's projection and
   * fovy, aspect, znear, zfar.  Recorded after the G-buffer, raster and shadow stages and before the downsample.  The samples
   * are the constructor's rand() draws in the reference's packing until vkrh_set_ssao_samples pins them.  Nothing reads
   * "ssao": the shading pass keeps GTAO's accumulated image at its occlusion binding.  One GPU only (not on a tiled frame: a
   * sample's reach is unbounded near the eye).                                                                             */
  VKRH_STAGE_SSAO               = 1u << 25,
  /* AdvancedSSR::run_tile_regression_pass (advanced_ssr.cpp:497-538; the reference ships the pass, its run() has it commented
   * out): gbuffer.depth mip 1 -> image "tile_planes" (RGBA32_SFLOAT, (W / 16, H / 16), created on first use; vkrh_image): per
   * 8 x 8 tile of the half-resolution depth the fitted plane and its mean squared residual, with camera_to_world =
   * transpose(normal matrix) of the frame's camera.  Recorded after the downsample of the same run (it reads mip 1) and before
   * the SSR stages, which do not read it.  Not part of VKRH_STAGE_CHAIN.  One GPU only (not on a tiled frame: halved strip
   * bounds are no multiples of 8, tiles would straddle owners).                                                              */
  VKRH_STAGE_TILE_REGRESSION    = 1u << 26,
  /* add_backbuffer_subpass + add_present_subpass (main.cpp:398-401; backbuffer_subpass2.cpp): the source image (default: the
   * TAA output of this run) drawn by program "texdraw" onto image "backbuffer" (RGBA8_SRGB; default: the frame's extent;
   * vkrh_image, vkrh_capture and the read-backs address it), all channels or the one vkrh_set_backbuffer selected.  Recorded
   * last, after TAA.  Nothing reads "backbuffer".  Not part of VKRH_STAGE_CHAIN.  One GPU only (not on a tiled frame: the uv
   * of a pixel spans the whole source).                                                                                    */
  VKRH_STAGE_BACKBUFFER         = 1u << 27,
  /* ShadowMaskPass::run (no reference counterpart: the reference renders its shadow maps and never samples them): gbuffer.depth
   * (mip 0) and one layer of "shadows" per configured light -> image "shadow_mask" (RGBA8_UNORM at the frame's extent, created on
   * first use; vkrh_image): channel l = the visibility of light l under the bias and radius of vkrh_set_shadow_mask, 255 in the
   * channels of lights that are not configured.  Recorded after the G-buffer, raster and shadow stages and before
   * VKRH_STAGE_SHADING, which reads it only when vkrh_set_shadow_mask asked for it.  Needs the maps: VKRH_STAGE_SHADOW in this
   * run or an earlier one since the lights were last set.  Not part of VKRH_STAGE_CHAIN.  One GPU only (not on a tiled frame:
   * the shadow maps are rendered on one GPU).                                                                               */
  VKRH_STAGE_SHADOW_MASK        = 1u << 28,
  /* ShadowMaskPass::run_rt (no reference counterpart): gbuffer.depth (mip 0), gbuffer.normal and the loaded scene's acceleration
   * structure (built by vkrh_load_scene, as for VKRH_STAGE_GTAO_RT) -> image "shadow_mask", the image and the place in the frame
   * order of VKRH_STAGE_SHADOW_MASK: channel l = 255 where the ray from the surface to light l of vkrh_set_shadow_rays meets no
   * triangle, 0 where it does or where the surface faces away; 255 in the channels of lights that are not configured.  With
   * `apply` of vkrh_set_shadow_mask, VKRH_STAGE_SHADING of the same run consumes the mask as it consumes the looked-up one.
   * An error, before anything is recorded: together with VKRH_STAGE_SHADOW_MASK (both write the image), without a loaded scene,
   * on a tiled frame (the rays reach anywhere: one GPU only).  Not part of VKRH_STAGE_CHAIN.                                 */
  VKRH_STAGE_SHADOW_MASK_RT     = 1u << 29,
  /* AdvancedSSR::run_rt (no reference counterpart): the images "reflections" and "blurred" of VKRH_STAGE_SSR from rays traced through
   * the loaded scene's acceleration structure, in the place of the SSR stages in the frame order.  Default mode (all): task
   * ReflectionsRT (depth mip 1, the half-resolution normals, the structure, its attribute table, the scene's textures ->
   * reflections: the albedo at the closest hit of the mirror ray, 0 at a miss) -> SSSR_blur.  No screen-space trace runs, so
   * gtao.raw ("raw") is NOT written: VKRH_STAGE_GTAO with MIS then reads what an earlier frame left there; the companions are
   * VKRH_STAGE_GTAO_RT or use_mis = 0.  fill_misses of vkrh_set_reflection_rays: SSSR_trace -> SSSR_filter -> ReflectionsRT (in
   * place on reflections: only texels whose screen-space ray is invalid are traced, the others keep the filter's value) ->
   * SSSR_blur; everything the trace writes for GTAO is as under VKRH_STAGE_SSR.  An error, before anything is recorded: on a tiled
   * frame (the rays reach anywhere: one GPU only), without a loaded scene, together with VKRH_STAGE_SSR, _SSR_CLASSIFIED,
   * _SSR_RESOLVE or any _SSR_TRACE* (all of them write reflections / blurred).  Not part of VKRH_STAGE_CHAIN.                 */
  VKRH_STAGE_REFLECTIONS_RT     = 1u << 30,
  VKRH_STAGE_CHAIN    = (1u << 3) | (1u << 5) | (1u << 6) | (1u << 7)
};

typedef void* (*vkrh_alloc_fn)(uint64_t bytes, void* user);
typedef void (*vkrh_free_fn)(void* ptr, void* user);

/* replace the device allocator used for every graph image (call before vkrh_create) */
void vkrh_set_allocator(vkrh_alloc_fn alloc, vkrh_free_fn free_fn, void* user);

void* vkrh_create(const vkrh_config* cfg);
void  vkrh_destroy(void* frame);
const char* vkrh_last_error(void);

int vkrh_set_camera(void* frame, const vkrh_camera* cam);
/* pin the host-side randoms of the reference (gtao.cpp:109-111 rand(), advanced_ssr.cpp:168-171 counter) */
int vkrh_pin_randoms(void* frame, float gtao_angle_jitter, uint32_t gtao_frame_count, uint32_t ssr_counter);
/* Scene for VKRH_STAGE_RASTER (replaces scene::load_tinygltf_scene, main.cpp:250): draw i renders
 * indices [index_offset, +index_count) with base vertex vertex_offset under `transform` (16 floats,
 * glm layout); texture index 0xFFFFFFFF = none.  Textures: RGBA8 mip chains, level 0 first. */
typedef struct vkrh_scene_draw {
  float    transform[16];
  uint32_t vertex_offset, index_offset, index_count;
  uint32_t albedo_tex_index, metalic_roughness_index, clip_alpha;
} vkrh_scene_draw;
typedef struct vkrh_scene_texture {
  uint32_t width, height, mip_levels, flags;  /* flags: VKRH_TEXTURE_* (0: every level comes from the host, as before) */
  const uint8_t* levels[16];
} vkrh_scene_texture;
/* images.cpp:93-160: the mip chain is built on the device.  Only levels[0] is read (mip_levels is ignored); the texture gets
 * floor(log2(max(w, h))) + 1 levels, level 0 is uploaded and vkr_gen_mipmaps builds the others — byte for byte what
 * vk-renderer_amd/scene.py build_mips makes on the host.  Not on a tiled frame.                                            */
#define VKRH_TEXTURE_GEN_MIPS 1u
int vkrh_load_scene(void* frame, const vkr_raster_vertex* vertices, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                    const vkrh_scene_draw* draws, uint32_t draw_count, const vkrh_scene_texture* textures, uint32_t texture_count);
/* descriptor (every level) of texture `index` of the loaded scene.  Not on a tiled frame. */
int vkrh_scene_texture_image(void* frame, uint32_t index, vkr_img* out);
/* Bakes a grid_size x grid_size grid of octahedral probes (probe_size^2, from cube_size^2 cube faces) from the scene of
 * vkrh_load_scene through ProbeRenderer::render_probe_grid: probes in x and z between min and max, at min.y; array layer
 * y * grid_size + x.  The grid stays in the frame until the next bake: images "probe_color", "probe_depth" (vkrh_image_layer, all
 * mips), and the cube of the last probe "cubemap_color", "cubemap_distance".  Refused: no scene, grid_size < 2, probe_size or
 * cube_size 0 or not a multiple of 8. */
int vkrh_bake_probes(void* frame, const float min[3], const float max[3], uint32_t grid_size, uint32_t probe_size, uint32_t cube_size);
/* The lights of VKRH_STAGE_SHADOW: `count` (1..4) light matrices of 16 floats (column-major, glm layout), light l renders into
 * layer l of "shadows"; `size` is the edge of the map, 0 keeps 1024 (at most 8192).  Replaces the default light; a change of size
 * reallocates the image at the next VKRH_STAGE_SHADOW.  vkrh_shadow_lights returns the matrices in use (room for 4 x 16 floats). */
int vkrh_set_shadow_lights(void* frame, const float* mvps, uint32_t count, uint32_t size);
int vkrh_shadow_lights(void* frame, float* out, uint32_t* count);
/* The lookup of VKRH_STAGE_SHADOW_MASK: `bias` in D24 codes, added to the map's side of the compare; `radius` 0, 1 or 2 (a box of
 * 1, 9 or 25 taps; anything else is an error); `apply` != 0: a VKRH_STAGE_SHADING of a vkrh_run that also produced the mask
 * records DeferedShadingPass::draw_shadowed (program "defered_shading_shadowed": light 0's channel multiplies the direct term)
 * instead of draw.  Defaults: bias 0, radius 1, apply 0, under which VKRH_STAGE_SHADING records what it always recorded.
 * Not on a tiled frame. */
int vkrh_set_shadow_mask(void* frame, uint32_t bias, uint32_t radius, uint32_t apply);
/* The rays of VKRH_STAGE_SHADOW_MASK_RT: `count` (1..4) lights of 4 floats (xyz, w: w == 1 a point light at xyz, w == 0 a
 * directional light whose xyz is the vector from the surface towards the light and whose length is the reach of the ray; any
 * other w is an error), the ray's origin is the surface point moved by normal_offset along the normal, the segment is
 * t in [tmin, 1] (tmin NaN is an error).  Defaults: one point light at the shading pass's LIGHT_POS, normal_offset 1e-3, tmin 0
 * (measured: DESIGN.md 7.8).  Not on a tiled frame. */
int vkrh_set_shadow_rays(void* frame, const float* lights, uint32_t count, float normal_offset, float tmin);
/* Area lights in VKRH_STAGE_SHADOW_MASK_RT: radii[l] is the radius in world units of the disk that light l of
 * vkrh_set_shadow_rays becomes (for a directional light at the tip of its xyz), sample_count (1..64) the rays per pixel and such
 * light, pattern_side (1, 2 or 4) the side of the tile of sample patterns from vkr_shadow_disk_samples.  With any radius above 0 the
 * stage records vkr_shadow_mask_rt_soft (with vkrh_set_ray_cutouts: vkr_shadow_mask_rt_soft_cutout) under the task name
 * ShadowMaskRTSoft, and a channel holds 255 * visible / sample_count rounded half up; a light with radius 0 stays hard.  An error:
 * `count` different from the number of lights set, sample_count or pattern_side outside those values, a radius that is negative,
 * NaN or infinite.  Default: every radius 0, under which the stage records what it always recorded.  A vkrh_set_shadow_rays with
 * another number of lights sets every radius back to 0.  No new stage bit.  Not on a tiled frame. */
int vkrh_set_shadow_area_lights(void* frame, const float* radii, uint32_t count, uint32_t sample_count, uint32_t pattern_side);
/* The edge-aware filter of the shadow mask (vkr_shadow_mask_filter): with reach 1..4 a VKRH_STAGE_SHADOW_MASK or
 * VKRH_STAGE_SHADOW_MASK_RT records, right after the mask, the task ShadowMaskFilter from image "shadow_mask" (which stays the
 * unfiltered mask) into image "shadow_mask_filtered" (RGBA8_UNORM at the frame's extent; exists only after such a run), and the
 * shadowed shading of vkrh_set_shadow_mask(apply) reads the filtered image.  reach is the side of the tent, the pattern_side of the
 * area lights it reconstructs; a tap counts when dot(n, n_tap) >= normal_min_dot and its distance from the pixel's tangent plane
 * is at most plane_tolerance times the pixel's view depth.  An error: reach above 4, a NaN threshold.  Default: reach 0, off, under
 * which every stage records what it always recorded.  No new stage bit.  Not on a tiled frame. */
int vkrh_set_shadow_mask_filter(void* frame, uint32_t reach, float normal_min_dot, float plane_tolerance);
/* The temporal accumulation of the shadow mask (vkr_shadow_mask_accumulate): with max_count 1..255 a
 * VKRH_STAGE_SHADOW_MASK or VKRH_STAGE_SHADOW_MASK_RT records, right after the mask and before the filter, the task
 * ShadowMaskAccumulate: image "shadow_mask" (which stays this frame's mask), the G-buffer's depth, normal and velocity, "prev_depth"
 * and the histories "shadow_history" (RGBA16_UNORM) / "shadow_history_count" (R8_UNORM) -> "shadow_history_out",
 * "shadow_history_count_out" and "shadow_mask_accumulated" (RGBA8_UNORM); the five images exist only after such a run, the first
 * of which also records four Clear_color tasks.  The filter, if on, reads "shadow_mask_accumulated", and the shadowed shading reads
 * the last image of the chain.  vkrh_end_frame after such a run swaps the two history pairs.  The history weighs at most
 * max_count - 1 frames; prev_inverse_camera is the inverse of the camera's prev_view.  With pattern_frames T > 1 a traced soft mask
 * takes the sample table vkr_shadow_disk_samples_frame(S, P, k mod T, T) in the k-th run that records the pass.
 * The pass runs with reset = 1 (no pixel has a history) in the first such run; after vkrh_set_shadow_rays,
 * vkrh_set_shadow_area_lights, vkrh_set_shadow_lights, vkrh_set_draw_transforms, vkrh_set_ray_cutouts or vkrh_load_scene; and
 * whenever "prev_depth" is not the depth of the previous accumulated run: unless the last vkrh_end_frame had swap_depth != 0 and
 * followed that run with no other vkrh_end_frame between, and no run since has had VKRH_STAGE_PREV_DEPTH,
 * VKRH_STAGE_CLEAR_PREV_DEPTH or a mask stage without the accumulation.
 * An error: max_count above 255, pattern_frames outside 1..64, a NaN tolerance.  Default: max_count 0, off, under which every
 * stage records what it always recorded.  No new stage bit.  Not on a tiled frame. */
int vkrh_set_shadow_mask_accumulate(void* frame, uint32_t max_count, float plane_tolerance, uint32_t pattern_frames);
/* The rays of VKRH_STAGE_REFLECTIONS_RT: fill_misses != 0 traces only the pixels whose screen-space ray is invalid, after the
 * screen-space trace and filter; the ray's origin is the surface point moved by normal_offset along the normal, the ray runs
 * t in [tmin, max_distance] along the unit mirror direction (tmin or max_distance NaN is an error), a hit samples mip level
 * texture_lod of its albedo texture (clamped to the chain).  Defaults: fill_misses 0, normal_offset 1e-3 and tmin 0 (those of
 * vkrh_set_shadow_rays), max_distance = the camera's zfar (also what max_distance <= 0 selects), texture_lod 0.  Not on a tiled frame. */
int vkrh_set_reflection_rays(void* frame, uint32_t fill_misses, float normal_offset, float tmin, float max_distance, uint32_t texture_lod);
/* Lit hits in VKRH_STAGE_REFLECTIONS_RT: after this call the stage records vkr_reflections_rt_lit (with
 * vkrh_set_ray_cutouts: vkr_reflections_rt_lit_cutout) under the task name "ReflectionsRTLit" where "ReflectionsRT" stood: the hit of
 * the mirror ray is lit by `count` (0..4) lights — lights: count x 4 floats in the convention of vkrh_set_shadow_rays, colours: count x 3
 * floats — shadowed by one ray per light from the hit (its origin moved by shadow_offset along the hit's normal, t in [shadow_tmin, 1])
 * and stored as albedo x (ambient (3 floats) + the sum).  count 1 with lights, colours and ambient all NULL selects the default light:
 * the direct diffuse term of defered_shading (its light position, colour 10 / pi, ambient 0.6).  The normal table comes from the
 * loaded scene and follows vkrh_set_draw_transforms.  Off until called: no stage bit, and a frame that never calls it records the
 * tasks and bytes it always did.  Composes with vkrh_set_reflection_rays (both modes) and vkrh_set_ray_cutouts.  An error: more than 4
 * lights, a NULL array otherwise, a light whose w is neither 0 nor 1, a NaN anywhere.  Not on a tiled frame.                        */
int vkrh_set_reflection_lights(void* frame, uint32_t count, const float* lights, const float* colours, const float* ambient, float shadow_offset,
                               float shadow_tmin);
/* For tests and tools: the normal table of the loaded scene as it is on the device now (one vkr_hit_normal per triangle of the
 * ray-query structure, in its order; after vkrh_set_draw_transforms the moved one).  *count: the number of records; out may be NULL to
 * ask for it alone.  Synchronises the frame's stream.                                                                               */
int vkrh_scene_hit_normals(void* frame, vkr_hit_normal* out, uint32_t capacity, uint32_t* count);
/* Alpha cutouts in the rays of VKRH_STAGE_SHADOW_MASK_RT and VKRH_STAGE_REFLECTIONS_RT: with enable != 0 the two
 * stages record vkr_shadow_mask_rt_cutout / vkr_reflections_rt_cutout, whose rays pass through a triangle where the alpha of its albedo
 * texture at the hit (level alpha_lod, clamped to the chain) is exactly 0, as the rasteriser discards such a fragment; textures
 * without an alpha-0 texel are masked opaque from the scene's images.  Default: off, and a frame that never calls this or calls it
 * with enable == 0 records the opaque entries.  VKRH_STAGE_GTAO_RT stays opaque (rt_main.frag is).  Not on a tiled frame.          */
int vkrh_set_ray_cutouts(void* frame, uint32_t enable, uint32_t alpha_lod);
/* Moves the draws of the loaded scene: transforms is count x 16 floats, one model matrix per draw of vkrh_load_scene in its order
 * and layout (glm: column-major); count must be that draw count.  Writes the node transforms, then SceneRenderer::update_scene()
 * (the table the raster, shadow-map and cube stages read) and SceneAccelerationStructure::refit() on the frame's stream
 * (vkr_scene_triangles + vkr_accel_refit: no host build, no upload, no synchronisation).  From the next vkrh_run the raster,
 * shadow-map and cube stages and every ray-traced stage see the same pose; images are those of a frame that loaded the scene
 * already in that pose, byte for byte.  `velocity` stays camera-only; baked probes and rendered shadow maps stay as they are until
 * they are rendered again.  Off unless called: no stage bit, no task in any frame.  Refused: without a loaded scene, with another
 * count, on a tiled frame (the ray-traced stages run on one GPU).                                                              */
int vkrh_set_draw_transforms(void* frame, const float* transforms, uint32_t count);
/* Pins the 16 samples of VKRH_STAGE_SSAO (xyz: 16 x 3 floats) and their packing in the uniform block: std140 = 0 the reference's
 * (vec3 at a 12-byte stride in 272 bytes: the shader's sample i is floats [4i, 4i + 1, 4i + 2] of the flat array for i <= 11 and
 * zero for i = 12..15), std140 != 0 one 16-byte slot per sample in 336 bytes (SSAOPass::std140_samples).  Not on a tiled frame. */
int vkrh_set_ssao_samples(void* frame, const float* xyz, uint32_t std140);
/* SSAOPass::draw recorded for pinned samples s[k] = (3k, 3k + 1, 3k + 2) and NOT submitted (no kernel is launched; images come
 * from the installed allocator): depth is image 0 (64 x 36, 7 mips), the target image 1.  Writes the task line in the format of
 * vkrh_selftest_transfers ("SSAO: R0.0 W1.0"), then for the reference's packing and for std140 one line "packing <bytes>:"
 * followed by the 84 floats (%.9g) of the vkr_ssao_params the program "ssao" would hand to vkr_ssao for the recorded block. */
int vkrh_selftest_ssao(char* buf, uint32_t buf_size);
/* AdvancedSSR::run_tile_regression_pass recorded on a 64 x 48 G-buffer for the normal matrix m[c][r] = 4c + r + 1 (column-major
 * 1..16, not symmetric) and fovy, aspect, znear, zfar = 1, 1.5, 0.05, 80, and NOT submitted (no kernel is launched; images come
 * from the installed allocator).  Writes "images: depth <i> tile_planes <j>" (graph indices), "tile_planes: <w>x<h> format <VkFormat>",
 * the task line in the format of vkrh_selftest_transfers ("SSSR_Tile_Regression: R<i>.1 W<j>.0") and "push 80:" followed by the
 * 20 floats (%.9g) of the push constants the task records for the program "tile_regression". */
int vkrh_selftest_tile_regression(char* buf, uint32_t buf_size);
/* What VKRH_STAGE_BACKBUFFER draws: `source_image` a name vkrh_image knows (NULL or "": the TAA output, "taa_target"), looked
 * up when the stage is recorded; `flags` the DrawTex bits (VKR_TEXDRAW_SHOW_*: 0 all channels, else the last set bit of R, G,
 * B, A wins); width / height the backbuffer's extent, 0 and 0 the frame's.  An unknown image name, a depth image (D24_UNORM_S8),
 * "backbuffer" itself, one extent 0 and the other not, or an extent above 65535 is an error.  Not on a tiled frame.        */
int vkrh_set_backbuffer(void* frame, const char* source_image, uint32_t flags, uint32_t width, uint32_t height);
/* add_backbuffer_subpass(graph, image, sampler, DrawTex::ShowR) + add_present_subpass(graph) recorded on a graph whose
 * backbuffer is 64 x 36 for a 128 x 72 RGBA16_SFLOAT source with 3 mips, and NOT submitted (no kernel is launched; images come
 * from the installed allocator).  Writes "images: source <i> backbuffer <j>" (graph indices), "backbuffer: <w>x<h> format
 * <VkFormat>", the task lines in the format of vkrh_selftest_transfers ("BackbufSubpass: W<j>.0 R<i>.0", "presentPrepare:
 * R<j>.0"), "program: texdraw <0|1>" (registered?) and "push 4: <flags>", the push constants the task records. */
int vkrh_selftest_texdraw(char* buf, uint32_t buf_size);
/* GTAORTParams the frame hands to VKRH_STAGE_GTAO_RT for the current camera: camera_to_world = inverse(view) (main.cpp:369-371) */
int vkrh_gtao_rt_params(void* frame, vkr_gtao_rt_params* out);
/* The camera matrices the frame holds after vkrh_set_camera, 3 x 16 floats in glm layout: projection * view and projection *
 * prev_view as stored in the block its passes read, and the inverse(view) of vkrh_gtao_rt_params.  No GPU is touched. */
int vkrh_camera_matrices(void* frame, float* out48);
/* the first `count` random directions of GTAO's ray-query pass (gtao.cpp:415-443), 4 floats each; no GPU is touched */
int vkrh_gtao_directions(float* out, uint32_t count);
/* the ray-query cases of the host mirror's error paths (no kernel is launched; writes "case: message" lines into buf) */
int vkrh_selftest_ray_query(char* buf, uint32_t buf_size);
/* pin ScreenSpaceTrace's per-frame randoms (screen_trace.cpp:49-53) */
int vkrh_pin_screen_trace(void* frame, float angle_jitter, float random_offset, uint32_t frame_count);
/* 1 when the program table of the host layer knows `name` (a name of src/shaders/config.json or one of this path's own) */
int vkrh_has_program(const char* name);
int vkrh_set_gtao_mode(void* frame, uint32_t use_mis, uint32_t two_directions);
/* material mode of the synthetic G-buffer (VKRH_STAGE_GBUFFER): 0, or VKR_SYNTH_TEXTURED_ROUGHNESS (include/vkr_postfx.h) */
int vkrh_set_synth_flags(void* frame, uint32_t flags);
/* tiled frames: whole-frame Hi-Z view mips 0..mips-1 (image mips 1..mips) arrive by all-gather (default 4; tiles whose
 * extent is only divisible by 8, like the 15360x1080 strips of config 4, gather 3); VKRH_STAGE_HIZ_TAIL rebuilds the rest */
int vkrh_set_gathered_mips(void* frame, uint32_t mips);
/* record the stages in `mask` (canonical order) and submit them on the stream */
int vkrh_run(void* frame, uint32_t stage_mask);
/* end-of-frame remaps (main.cpp:416-420); swap_depth = 0 keeps a static G-buffer */
int vkrh_end_frame(void* frame, uint32_t swap_depth);
/* current descriptor of a named image ("depth", "taa_target", ...) */
int vkrh_image(void* frame, const char* name, uint32_t base_mip, uint32_t mip_count, vkr_img* out);
/* copies a named device buffer ("reflective_tiles", "glossy_tiles", "reflective_indirect",
 * "glossy_indirect") to host memory after synchronising the stream; returns its size in *bytes */
int vkrh_read_buffer(void* frame, const char* name, void* dst, uint64_t capacity, uint64_t* bytes);
/* one layer (all its mips) of a named array image ("deinterleaved_depth", "probe_color", "probe_depth", "cubemap_color", "shadows", ...) */
int vkrh_image_layer(void* frame, const char* name, uint32_t layer, vkr_img* out);
/* Reads `name` (mip) back through ReadBackSystem and writes it with the reference's capture writers
 * (main.cpp:118-176): kind 0 = depth CSV (24-bit hex), 1 = depth PNG, 2 = RGBA8 PNG (alpha 255).
 * kind 3 = the final frame (main.cpp:392-396): blit_image(`name`, normally "taa_target" -> "readback") converts the image to
 * RGBA8_SRGB on the device, then "readback" goes through the read-back and the RGBA PNG writer of kind 2.  "readback" is
 * RGBA8_SRGB of the frame's extent, created on first use and visible through vkrh_image afterwards; mip must be 0.  Not on a
 * tiled frame. */
int vkrh_capture(void* frame, const char* name, uint32_t mip, uint32_t kind, const char* path);
/* CPU-only check of the capture writers: writes <dir>/depth.csv, depth.png, color.png from a
 * width x height pattern depth = (x * 65537 + y * 257 + 0xAB000000) (top byte = stencil, must be
 * masked), rgba = (x, y, x ^ y, 7).  No GPU is touched. */
int vkrh_selftest_writers(const char* dir, uint32_t width, uint32_t height);
/* per-task device timing with HIP events on the frame's stream */
int vkrh_enable_task_timing(void* frame, uint32_t on);
/* time only the task of that name (two event records per frame instead of two per pass) */
int vkrh_enable_task_timing_only(void* frame, const char* task);
/* synchronises and returns "name total_ms launches\n" lines accumulated since the last call */
const char* vkrh_collect_task_times(void* frame);
/* Exercises the rendergraph / pass error paths the reference signals with exceptions (no kernel is
 * launched; images come from the installed allocator).  Writes "case: message" lines into buf. */
int vkrh_selftest_errors(char* buf, uint32_t buf_size);
/* Every registered program launched on an empty descriptor set, with no attachments and no push constants (no kernel is
 * launched: each program refuses first).  Writes one line "program: message" per program, sorted by name; a program that
 * does not refuse is reported as "program: no error". */
int vkrh_selftest_programs(char* buf, uint32_t buf_size);
/* The transfer helpers of util_passes.hpp on images of the frame's graph, for launchers written against the rendergraph API.
 * vkrh_create_image adds an image of the caller's own (format: a vkr_format; never a window of the frame) that vkrh_image /
 * vkrh_image_layer then find under `name`; a name of the frame's own images or one already taken is refused.  vkrh_transfer records
 * one helper and submits it on the frame's stream: GEN_MIPMAPS gen_mipmaps(image), CLEAR_DEPTH clear_depth(image, value[0]) (value
 * NULL: 1.0), CLEAR_COLOR clear_color(image, value[0..3]), BLIT blit_image(image, dst).  Not on a tiled frame.                   */
enum { VKRH_TRANSFER_GEN_MIPMAPS = 0, VKRH_TRANSFER_CLEAR_DEPTH = 1, VKRH_TRANSFER_CLEAR_COLOR = 2, VKRH_TRANSFER_BLIT = 3 };
int vkrh_create_image(void* frame, const char* name, uint32_t format, uint32_t width, uint32_t height, uint32_t mip_levels, uint32_t array_layers);
int vkrh_transfer(void* frame, uint32_t op, const char* image, const char* dst, const float* value);
/* The transfer helpers of util_passes.hpp, recorded and NOT submitted (no kernel is launched; images come from the installed
 * allocator): gen_mipmaps on a 40 x 24 image of 6 levels, clear_depth on a D24S8 image of 3 levels and 2 layers, clear_color on an
 * RGBA8 image of 2 levels, blit_image between two images.  Writes one line per recorded task into buf:
 * "name: R<image>.<mip> ... W<image>.<mip> ..." — the declared transfer reads and writes, images numbered in creation order. */
int vkrh_selftest_transfers(char* buf, uint32_t buf_size);
/* names of the tasks executed by the last vkrh_run, '\n'-separated */
const char* vkrh_last_tasks(void* frame);
/* the stream lane (0 = the frame's stream) each of those tasks was recorded on, space separated */
const char* vkrh_last_lanes(void* frame);
/* 0 (default): every task on the frame's stream; 1: independent tasks of one vkrh_run spread over up to three streams */
int vkrh_set_async(void* frame, uint32_t on);

/* ---- the tiled frame: one process per GPU, horizontal strips, RCCL over xGMI -----------------
 * Rank r of `world` owns rows [r * H / world, (r + 1) * H / world) of the full_width x full_height frame and holds
 * them plus `halo` rows above / below (clipped to the frame).  One vkrh_tiled_step() is one frame:
 *
 *   downsample | all-gather(depth mips 1..k) starts on the exchange stream; own albedo / normal rows go into the frame images
 *   TAA (needs neither)            | its halo refresh starts
 *   Hi-Z tail + SSR trace          (after the gather; rays that end on another rank's rows stay pending) | the requests are
 *                                    counted, the counts all-gathered, and — from the second frame on — the whole request /
 *                                    reply round for hit colours + hit normals and the deferred hit-normal test
 *                                    (vkr_sssr_validate) are enqueued on the exchange stream at once
 *   GTAO main, filter, accumulate  | its halo refresh starts
 *   SSR filter + blur              (after the replies are in place) | its halo refresh starts; history remaps
 *
 * Hit colours: the filter reads the albedo at the hit position of every valid ray, anywhere in the frame.  Each rank asks
 * the owners for the footprint rows outside its window (vkr_hit_requests / _reply / _scatter, 4-byte requests and 16-byte
 * replies moved with vkr_halo_exchange) instead of receiving the albedo of the whole frame.  The message sizes of a frame
 * come from the PREVIOUS frame's counts (segments of fixed room, identical on every rank), so the host is not in the path:
 * it looks at this frame's counts before it queues the filter and repeats the round exactly if a segment overflowed; only
 * the first frame waits for its counts (with GTAO queued).  albedo_by_gather = 1 restores the all-gather.
 *
 * Every exchange is one grouped RCCL launch (vkr_all_gather / vkr_halo_exchange) on the frame's own exchange stream,
 * ordered against the compute stream with events only: the host never blocks, and a halo refresh issued after the
 * pass that produces a surface is awaited right before the pass that consumes it in the NEXT frame.
 * comm == NULL builds the same object without a wire: a test harness then advances it phase by phase
 * (vkrh_tiled_phase) and moves the bytes between in-process ranks itself (vkrh_tiled_gather_parts / _halo_peers). */
typedef struct vkrh_tiled_config {
  uint32_t full_width, full_height;
  uint32_t rank, world;
  uint32_t halo;            /* full-res pixels, even, a multiple of 2^gathered_mips                          */
  uint32_t gathered_mips;   /* depth image-mips 1..k travel by all-gather (the tile extent must divide by 2^k) */
  uint32_t force_tiled;     /* world == 1: still run the gathers and the staged frame (rehearsal)              */
  uint32_t albedo_by_gather;/* 0 (default): hit colours AND hit normals by request / reply; 1: all-gather the albedo and the
                             * downsampled normals of the whole frame (round 2); 2: albedo by request, normals gathered      */
  void*    stream;          /* compute stream                                                                */
  vkr_comm* comm;           /* RCCL communicator of include/vkr_postfx.h, or NULL (no wire: lockstep harness) */
  /* NULL: world strips of full_height / world rows.  Otherwise world + 1 increasing row numbers, [0] = 0 and [world] =
   * full_height, identical on every rank: strip r is rows [row_bounds[r], row_bounds[r + 1]).  Every bound is a
   * multiple of 2^gathered_mips and of 2, every strip at least `halo` rows high.  Strips of different heights balance
   * ranks whose rows differ in cost (vkrh_balance_rows); their shares travel with vkr_all_gather_v.                  */
  const uint32_t* row_bounds;
} vkrh_tiled_config;
enum { VKRH_TILED_PHASES = 5, VKRH_TILED_PHASES_SHADED = 6, VKRH_TILED_SHADING_MIN_HALO = 4, VKRH_GATHER_HIZ = 0, VKRH_GATHER_ALBEDO = 1, VKRH_HALO_TAA = 0, VKRH_HALO_AO = 1, VKRH_HALO_SSR = 2 };
void* vkrh_tiled_create(const vkrh_tiled_config* cfg);
void  vkrh_tiled_destroy(void* tiled);
void* vkrh_tiled_frame(void* tiled);                 /* the frame inside: every vkrh_* call above works on it       */
int   vkrh_tiled_step(void* tiled);                  /* one frame, exchanges included (comm != NULL or world == 1)  */
int   vkrh_tiled_flush(void* tiled);                 /* completes the halo refreshes the last frame left in flight  */
/* Deferred shading in the tiled frame (main.cpp:390-391: shading_pass.draw -> color_out_tex, which the TAA resolves).  Off by
 * default, and off is the frame above.  On, the TAA leaves its early place and the frame gets a tail behind the SSR resolve:
 *
 *   ... SSR filter + blur | its halo refresh starts
 *   the AO, SSR and TAA halo refreshes are awaited and unpacked — the AO and SSR rows in the SAME frame, into the images they were
 *   packed from: the shading of a strip's first / last rows reads its neighbours' current accumulated AO and blurred reflections
 *   shading + TAA (one vkrh_run: the TAA resolves color_out) | the TAA halo refresh starts; history remaps
 *
 * Reach: color_out is computed on the strip and one row either side (the TAA reads its four neighbours); for those rows the 3 x 3
 * half-res footprint of sample_ocllusion_ssr (shader.frag:103-130) spans 1 half-res row above the strip's first and 2 below its
 * last, so the halo must hold 2 half-res rows: halo >= VKRH_TILED_SHADING_MIN_HALO.  In the harness the tail is phase 5
 * (VKRH_TILED_PHASES_SHADED phases; halo 1 moves after phase 3, halo 2 after phase 4, halo 0 after phase 5).  One untiled rank
 * runs VKRH_STAGE_CHAIN | VKRH_STAGE_SHADING.  vkrh_tiled_set_shading is refused (vkrh_last_error): a NULL handle; while a halo
 * refresh is in flight (allowed before the first frame and right after vkrh_tiled_flush); world > 1 with a halo below the
 * reach; when VKRH_STAGE_BRDF_LUT has never run on the frame inside.  vkrh_tiled_shading: 1 / 0, or -1 for a NULL handle.   */
int   vkrh_tiled_set_shading(void* tiled, uint32_t on);
int   vkrh_tiled_shading(void* tiled);
/* lockstep harness: phase p of the frame without the wire; what must cross ranks between phases is exposed below */
int   vkrh_tiled_phase(void* tiled, uint32_t phase);
int   vkrh_tiled_gather_parts(void* tiled, uint32_t which, vkr_gather_part* out, uint32_t capacity, uint32_t* count);
int   vkrh_tiled_halo_peers(void* tiled, uint32_t surface, vkr_halo_peer* out, uint32_t capacity, uint32_t* count);
/* The hit-colour request / reply (albedo_by_gather == 0), step by step for the lockstep harness — between phase 3 and phase 4
 * of every rank, the harness moving the bytes of each peer list exactly as vkr_halo_exchange would:
 *   vkrh_tiled_hit_counts    row[o] = the requests this rank has for owner o (counted on the device at the end of phase 2)
 *   vkrh_tiled_hit_requests  matrix[r * world + o] = rank r's count for owner o, identical on every rank: writes the
 *                            requests and returns who gets / sends which bytes
 *   vkrh_tiled_hit_replies   answers the requests that arrived and returns the peer list of the way back
 *   vkrh_tiled_hit_finish    writes the replies that arrived into the whole-frame albedo image                          */
int   vkrh_tiled_hit_counts(void* tiled, uint32_t* row);
int   vkrh_tiled_hit_requests(void* tiled, const uint32_t* matrix, vkr_halo_peer* peers, uint32_t capacity, uint32_t* count);
int   vkrh_tiled_hit_replies(void* tiled, vkr_halo_peer* peers, uint32_t capacity, uint32_t* count);
int   vkrh_tiled_hit_finish(void* tiled);
/* bytes this rank received over the wire for the hit colours in the last frame (requests in + replies in)              */
int   vkrh_tiled_hit_bytes(void* tiled, uint64_t* bytes);
/* native wire: how the hit-colour rounds of the frames so far went — [0] enqueued on the previous frame's capacities (no host
 * round trip), [1] exact rounds after the host had the counts (first frame), [2] rounds repeated because a segment overflowed */
int   vkrh_tiled_hit_rounds(void* tiled, uint64_t* rounds3);
/* The room of every rank-to-owner segment of the NEXT frame's hit round, from this frame's world x world counts (what every
 * rank derives for itself): count * percent / 100 + 64 in steps of 64; adjacent strips always keep a segment, a distant pair that
 * asked for nothing keeps none.                                                                                          */
int   vkrh_hit_capacities(const uint32_t* counts, uint32_t world, uint32_t percent, uint32_t* capacities);
/* Measurement (tools/wire_emulation.py): a frame of several ranks that the in-process harness has driven so far (comm NULL) —
 * its receive buffers hold what real peers send, the hit segments laid out by vkrh_hit_capacities(counts) — continues natively
 * (vkrh_tiled_step) on `comm`, made by vkr_comm_create_emulated: every exchange holds the exchange stream for its wire time and
 * delivers what is already there.  With a static scene that is what the peers would send again.  A second call swaps the
 * communicator (another link rate; counts ignored).                                                                          */
int   vkrh_tiled_emulate_wire(void* tiled, void* comm, const uint32_t* counts);
/* 1: two frames in flight (VKR_TILED_PIPELINE=1): vkrh_tiled_step downsamples the NEXT frame and starts its depth all-gather
 * right after this frame's trace; the TAA runs behind GTAO (host/frame.cpp: pipelined_step)                                 */
int   vkrh_tiled_pipelined(void* tiled);
/* 1: the trace runs in two stages around the depth all-gather (VKRH_STAGE_SSR_TRACE_HEAD / _RESUME) and the TAA after GTAO */
int   vkrh_tiled_local_first(void* tiled);
/* requests of the last frame that this rank could not answer from its window (0 unless the ranks' strips disagree); synchronises */
int   vkrh_tiled_hit_errors(void* tiled, uint32_t* errors);
/* Diagnostics: how long the compute stream stood still for each exchange.  vkrh_tiled_time_waits(on) brackets every wait
 * with an event pair (≈7 us of queue time per frame: for a calibration run, not for the timed one);
 * vkrh_tiled_wait_times returns the totals since the last call in ms — [0] Hi-Z gather, [1] albedo gather, [2] TAA halo,
 * [3] AO halo, [4] SSR halo — and synchronises the compute stream.                                                    */
int   vkrh_tiled_time_waits(void* tiled, uint32_t on);
int   vkrh_tiled_wait_times(void* tiled, float* ms5);
/* New strip bounds from the compute time every rank measured with the current ones (ms[r] over rows
 * [bounds_in[r], bounds_in[r + 1]); cost taken as uniform inside a strip): cuts the frame where the cumulative cost
 * reaches r / world of the total, rounded to `align` rows, no strip below `min_rows`.  Pure host arithmetic.        */
int   vkrh_balance_rows(const float* ms, const uint32_t* bounds_in, uint32_t world, uint32_t align, uint32_t min_rows, uint32_t* bounds_out);

#ifdef __cplusplus
}
#endif
#endif
