// frame.cpp — see frame.hpp.  C++ exceptions thrown by the pass / graph code (the reference's
// only error channel, gpu/common.cpp:6-12) are turned into status codes at this C boundary.
#include "frame.hpp"
#include "gpu_transfer.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "advanced_ssr.hpp"
#include "backbuffer_subpass2.hpp"
#include "defered_shading.hpp"
#include "downsample_pass.hpp"
#include "gtao.hpp"
#include "image_readback.hpp"
#include "probe_renderer.hpp"
#include "scene/scene_as.hpp"
#include "scene_renderer.hpp"
#include "screen_trace.hpp"
#include "shadow_mask.hpp"
#include "synthetic_gbuffer.hpp"
#include "taa.hpp"
#include "util_passes.hpp"

namespace {

thread_local std::string g_error;

struct GraphInit {  // orders construction: the frame window must be set before any pass creates images
  GraphInit(rendergraph::RenderGraph& g, const vkrh_config& c) {
    g.set_frame_window(c.full_width, c.full_height, c.origin_x, c.origin_y, c.width, c.height);
  }
};

// main.cpp:295: perspective(radians(90), 1, 0.05, 80) * lookAt((-1.85867, 5.81832, -0.247114), (0, 2, 1), (0, -1, 0)), the light
// the shading pass calls LIGHT_POS.  Evaluated under the rule of vk-renderer_amd/camera.py (shadow_mvp): the inputs are floats,
// each factor is evaluated in double — plain scalar arithmetic in one fixed order — and rounded to float, the product is
// accumulated in double and rounded once.  Python and C++ hand the kernels the same 16 words.
glm::mat4 default_shadow_mvp() {
  const double e[3] = {(double)-1.85867f, (double)5.81832f, (double)-0.247114f}, c[3] = {0.0, 2.0, 1.0}, up[3] = {0.0, -1.0, 0.0};
  auto dot = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
  auto cross = [](const double* a, const double* b, double* o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; };
  auto unit = [&](double* a) { const double n = std::sqrt(dot(a, a)); a[0] = a[0] / n; a[1] = a[1] / n; a[2] = a[2] / n; };
  double f[3] = {c[0] - e[0], c[1] - e[1], c[2] - e[2]}, s[3], t[3];
  unit(f);
  cross(f, up, s);
  unit(s);
  cross(s, f, t);
  glm::mat4 v{1.f}, p{0.f};  // m[column][row]
  for (int k = 0; k < 3; k++) { v[k][0] = (float)s[k]; v[k][1] = (float)t[k]; v[k][2] = (float)-f[k]; }
  v[3][0] = (float)-dot(s, e); v[3][1] = (float)-dot(t, e); v[3][2] = (float)dot(f, e);
  const double fovy = (double)(90.f * 0.01745329251994329576923690768489f), znear = (double)0.05f, zfar = 80.0;
  const double tg = std::tan(fovy / 2.0);
  p[0][0] = (float)(1.0 / (1.0 * tg));
  p[1][1] = (float)(1.0 / tg);
  p[2][2] = (float)(zfar / (znear - zfar));
  p[2][3] = -1.f;
  p[3][2] = (float)(-(zfar * znear) / (zfar - znear));
  glm::mat4 out{0.f};
  for (int col = 0; col < 4; col++)
    for (int row = 0; row < 4; row++) {
      double acc = 0.0;
      for (int k = 0; k < 4; k++) acc += (double)p[k][row] * (double)v[col][k];
      out[col][row] = (float)acc;
    }
  return out;
}

// What vkrh_run refuses before it records anything.  One rule per stage, in the order the checks are made: a mask that breaks
// several rules is refused with the message of the first.  Per rule, in this order: why the stage does not run on a tiled frame;
// the stages it cannot share a run with (they write the same images); what it needs from earlier calls.
enum class Needs { Nothing, Scene, Tlas, TlasAndScene, Probes };
struct StageRule {
  uint32_t stage; const char* name;
  const char* tiled;                                               // "<name> on a tiled frame (<tiled>)", or nullptr: the stage runs on one
  uint32_t rivals = 0; const char* rivals_tail = nullptr;          // "<name> together with <rivals_tail>"
  Needs needs = Needs::Nothing; const char* needs_tail = nullptr;  // "<name> without <needs_tail>"
};
constexpr uint32_t SSR_STAGES = VKRH_STAGE_SSR | VKRH_STAGE_SSR_CLASSIFIED | VKRH_STAGE_SSR_RESOLVE | VKRH_STAGE_SSR_TRACE |
                                VKRH_STAGE_SSR_TRACE_HEAD | VKRH_STAGE_SSR_TRACE_RESUME;
constexpr StageRule STAGE_RULES[] = {
    {VKRH_STAGE_CLEAR_PREV_DEPTH, "VKRH_STAGE_CLEAR_PREV_DEPTH", "transfers take whole images"},
    {VKRH_STAGE_SSAO, "VKRH_STAGE_SSAO", "a sample's reach is unbounded near the eye: SSAO runs on one GPU"},
    {VKRH_STAGE_TILE_REGRESSION, "VKRH_STAGE_TILE_REGRESSION", "halved strip bounds are no multiples of 8: tiles would straddle owners"},
    {VKRH_STAGE_BACKBUFFER, "VKRH_STAGE_BACKBUFFER", "the uv of a pixel spans the whole source: the backbuffer is drawn on one GPU"},  // + its source
    {VKRH_STAGE_SHADOW_MASK_RT, "VKRH_STAGE_SHADOW_MASK_RT", "the rays reach anywhere: ray-traced shadows run on one GPU",
     VKRH_STAGE_SHADOW_MASK, "VKRH_STAGE_SHADOW_MASK (both write the image shadow_mask)",
     Needs::Tlas, "a loaded scene (vkrh_load_scene builds its acceleration structure)"},
    {VKRH_STAGE_REFLECTIONS_RT, "VKRH_STAGE_REFLECTIONS_RT", "the rays reach anywhere: ray-traced reflections run on one GPU",
     SSR_STAGES, "an SSR stage (VKRH_STAGE_SSR, _SSR_CLASSIFIED, _SSR_RESOLVE, _SSR_TRACE*: all write the images reflections / blurred)",
     Needs::TlasAndScene, "a loaded scene (vkrh_load_scene builds its acceleration structure and attribute table)"},
    {VKRH_STAGE_SHADOW_MASK, "VKRH_STAGE_SHADOW_MASK", "the shadow maps are rendered on one GPU"},  // + shadow maps, of this run or an earlier one
    {VKRH_STAGE_SHADOW, "VKRH_STAGE_SHADOW", "the shadow maps are rendered on one GPU", 0, nullptr, Needs::Scene, "a loaded scene (vkrh_load_scene)"},
    {VKRH_STAGE_GTAO_RT, "VKRH_STAGE_GTAO_RT", "ray-traced AO runs on one GPU", VKRH_STAGE_GTAO,
     "VKRH_STAGE_GTAO (both write GTAO's raw, filtered and accumulated images)", Needs::Tlas, "a loaded scene (vkrh_load_scene builds its acceleration structure)"},
    {VKRH_STAGE_PROBE_TRACE, "VKRH_STAGE_PROBE_TRACE", "probes are traced on one GPU", 0, nullptr, Needs::Probes, "baked probes (vkrh_bake_probes)"},
};

struct PostFxFrame {
  vkrh_config cfg;
  rendergraph::RenderGraph graph;
  GraphInit init;
  struct TransferInit { explicit TransferInit(rendergraph::RenderGraph& g) { gpu_transfer::init(g); } };  // main.cpp: before the passes
  TransferInit transfer_init;
  Gbuffer gbuffer;
  DownsamplePass downsample_pass;
  GTAO gtao;
  AdvancedSSR ssr;
  TAA taa_pass;
  DeferedShadingPass shading_pass;
  rendergraph::ImageResourceId color_out_tex;
  rendergraph::ImageResourceId shadow_map;  // main.cpp passes its shadow map to the shading pass (binding 5; the shader never reads it)
  SyntheticGbuffer synth;
  ScreenSpaceTrace screen_trace;
  ReadBackSystem readback;
  std::unique_ptr<scene::CompiledScene> loaded_scene;
  std::unique_ptr<SceneRenderer> scene_renderer;
  std::unique_ptr<scene::SceneAccelerationStructure> scene_as;  // main.cpp:257-258, built by vkrh_load_scene

  // the probe grid of the last vkrh_bake_probes
  std::unique_ptr<ProbeRenderer> probe_renderer;
  std::unique_ptr<OctahedralProbeGrid> probe_grid;
  ProbeTracePass probe_trace_pass;
  rendergraph::ImageResourceId probe_trace_out;
  bool has_probe_trace_out = false;

  // the shadow maps of VKRH_STAGE_SHADOW: main.cpp:279-287 (1024^2, 4 layers, D24S8), one layer per configured light
  rendergraph::ImageResourceId shadows;
  bool has_shadows = false, shadows_rendered = false;
  uint32_t shadow_size = 1024;
  std::vector<glm::mat4> shadow_lights{default_shadow_mvp()};

  // what runs on one GPU only: "<who>: on a tiled frame (<why>)"
  void refuse_tiled(const char* who, const char* why) const {
    if (cfg.tiled) throw std::runtime_error{std::string{who} + ": on a tiled frame (" + why + ")"};
  }
  // what vkrh_last_tasks (and, after a run, vkrh_last_lanes) report: the submission that just ended
  void record_submitted(bool lanes) {
    task_names.clear();
    for (const auto& n : graph.last_submitted_tasks()) { task_names += n; task_names += '\n'; }
    if (!lanes) return;
    task_lanes.clear();
    for (uint32_t l : graph.last_submitted_lanes()) { task_lanes += std::to_string(l); task_lanes += ' '; }
  }

  // VKRH_STAGE_SSAO: the pass and its target, created on first use (the constructor draws from rand(): a frame that never runs
  // the stage leaves the sequence of the other passes' draws alone)
  std::unique_ptr<SSAOPass> ssao_pass;
  rendergraph::ImageResourceId ssao_tex;
  SSAOPass& ensure_ssao() {
    if (!ssao_pass) {
      ssao_tex = create_ssao_texture(graph, cfg.width, cfg.height);
      ssao_pass.reset(new SSAOPass(graph, ssao_tex));
    }
    return *ssao_pass;
  }
  void set_ssao_samples(const float* xyz, uint32_t std140) {
    if (!xyz) throw std::runtime_error{"vkrh_set_ssao_samples: NULL argument"};
    refuse_tiled("vkrh_set_ssao_samples", "VKRH_STAGE_SSAO runs on one GPU");
    SSAOPass& pass = ensure_ssao();
    for (uint32_t i = 0; i < 16; i++) pass.sphere_samples[i] = glm::vec3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    pass.std140_samples = std140 != 0;
  }

  // VKRH_STAGE_SHADOW_MASK: the pass and its target, created on first use; the lookup's settings (vkrh_set_shadow_mask).
  // shadow_maps_current: VKRH_STAGE_SHADOW has rendered a layer for every light configured now.
  std::unique_ptr<ShadowMaskPass> shadow_mask_pass;
  rendergraph::ImageResourceId shadow_mask_tex;
  uint32_t shadow_mask_bias = 0, shadow_mask_radius = 1;
  bool shadow_mask_apply = false, shadow_maps_current = false;
  ShadowMaskPass& ensure_shadow_mask() {
    if (!shadow_mask_pass) {
      shadow_mask_tex = create_shadow_mask_texture(graph, cfg.width, cfg.height);
      shadow_mask_pass.reset(new ShadowMaskPass());
    }
    return *shadow_mask_pass;
  }
  void set_shadow_mask(uint32_t bias, uint32_t radius, uint32_t apply) {
    refuse_tiled("vkrh_set_shadow_mask", "VKRH_STAGE_SHADOW_MASK runs on one GPU");
    if (radius > 2) throw std::runtime_error{"vkrh_set_shadow_mask: radius " + std::to_string(radius) + ", needs 0..2 (a box of 1, 9 or 25 taps)"};
    shadow_mask_bias = bias; shadow_mask_radius = radius; shadow_mask_apply = apply != 0;
  }

  // The edge-aware filter of the mask (vkrh_set_shadow_mask_filter), right after either mask stage into a second image, created
  // on the first run with the filter on.  Default: reach 0, off.
  uint32_t shadow_filter_reach = 0;
  float shadow_filter_normal_min_dot = 0.9f, shadow_filter_plane_tolerance = 0.01f;
  bool has_shadow_mask_filtered = false;
  rendergraph::ImageResourceId shadow_mask_filtered_tex;
  void set_shadow_mask_filter(uint32_t reach, float normal_min_dot, float plane_tolerance) {
    refuse_tiled("vkrh_set_shadow_mask_filter", "the taps cross strip borders: the filter runs on one GPU");
    if (reach > 4) throw std::runtime_error{"vkrh_set_shadow_mask_filter: reach " + std::to_string(reach) + ", needs 0 (off) or 1..4"};
    if (std::isnan(normal_min_dot) || std::isnan(plane_tolerance)) throw std::runtime_error{"vkrh_set_shadow_mask_filter: a threshold is NaN"};
    shadow_filter_reach = reach; shadow_filter_normal_min_dot = normal_min_dot; shadow_filter_plane_tolerance = plane_tolerance;
  }
  // after the mask stage of this run has been recorded
  void record_shadow_mask_filter(ShadowMaskPass& pass) {
    const rendergraph::ImageResourceId source = record_shadow_mask_accumulate(pass);  // before the filter, which then reads its image
    if (shadow_filter_reach == 0) return;
    if (!has_shadow_mask_filtered) {
      shadow_mask_filtered_tex = create_shadow_mask_texture(graph, cfg.width, cfg.height);
      has_shadow_mask_filtered = true;
    }
    pass.update_filter(shadow_filter_reach, shadow_filter_normal_min_dot, shadow_filter_plane_tolerance);
    pass.run_filter(graph, gbuffer.depth, gbuffer.normal, source, shadow_mask_filtered_tex);
  }

  // The temporal accumulation of the mask (vkrh_set_shadow_mask_accumulate), right after either mask stage and before the filter.
  // Default: max_count 0, off.  The five images are created on the first run with it on.
  uint32_t shadow_accum_max_count = 0, shadow_accum_pattern_frames = 1;
  float shadow_accum_plane_tolerance = 0.01f;
  bool has_shadow_history = false;
  ShadowHistoryTextures shadow_history;
  // The histories hold last frame's visibilities of this frame's lights and geometry, and prev_depth is last frame's depth, only
  // when all of this holds; otherwise the pass runs with reset = 1:
  bool shadow_accum_invalid = true;   // a call since the last accumulated run changed what a visibility means (or there was no such run)
  bool shadow_accum_chained = false;  // the last vkrh_end_frame swapped the depths and followed an accumulated run directly
  bool shadow_accum_pending = false;  // an accumulated run that no vkrh_end_frame has followed yet
  uint32_t shadow_accum_frame = 0;    // the runs that recorded the pass: the index into the cycle of sample tables
  void set_shadow_mask_accumulate(uint32_t max_count, float plane_tolerance, uint32_t pattern_frames) {
    refuse_tiled("vkrh_set_shadow_mask_accumulate", "the reprojection reaches across strips: the accumulation runs on one GPU");
    if (max_count > 255) throw std::runtime_error{"vkrh_set_shadow_mask_accumulate: max_count " + std::to_string(max_count) + ", needs 0 (off) or 1..255"};
    if (pattern_frames < 1 || pattern_frames > 64)
      throw std::runtime_error{"vkrh_set_shadow_mask_accumulate: pattern_frames " + std::to_string(pattern_frames) + ", needs 1..64"};
    if (std::isnan(plane_tolerance)) throw std::runtime_error{"vkrh_set_shadow_mask_accumulate: plane_tolerance is NaN"};
    shadow_accum_max_count = max_count; shadow_accum_plane_tolerance = plane_tolerance; shadow_accum_pattern_frames = pattern_frames;
  }
  // the sample tables of this run's traced soft mask: before run_rt
  void select_shadow_sample_tables(ShadowMaskPass& pass) {
    if (shadow_accum_max_count && shadow_accum_pattern_frames > 1) pass.update_rt_soft_frame(shadow_accum_frame % shadow_accum_pattern_frames, shadow_accum_pattern_frames);
  }
  // after the mask stage of this run has been recorded -> the image the next stage of the shadow pipeline reads
  rendergraph::ImageResourceId record_shadow_mask_accumulate(ShadowMaskPass& pass) {
    if (shadow_accum_max_count == 0) {
      shadow_accum_chained = false;  // a mask the histories never saw
      return shadow_mask_tex;
    }
    if (!has_shadow_history) {
      shadow_history = create_shadow_history_textures(graph, cfg.width, cfg.height);
      has_shadow_history = true;
      for (rendergraph::ImageResourceId id : {shadow_history.history, shadow_history.out_history, shadow_history.count, shadow_history.out_count})
        clear_color(graph, id, VkClearColorValue{{0.f, 0.f, 0.f, 0.f}});
    }
    pass.update_accumulate(shadow_accum_max_count, shadow_accum_plane_tolerance, prev_view, shadow_accum_invalid || !shadow_accum_chained);
    pass.run_accumulate(graph, gbuffer.depth, gbuffer.normal, gbuffer.velocity_vectors, gbuffer.prev_depth, shadow_mask_tex, shadow_history.history,
                        shadow_history.count, shadow_history.out_history, shadow_history.out_count, shadow_history.accumulated);
    shadow_accum_invalid = false; shadow_accum_chained = false; shadow_accum_pending = true;
    shadow_accum_frame++;
    return shadow_history.accumulated;
  }
  // the last image of the shadow pipeline, for the shadowed shading
  rendergraph::ImageResourceId shadow_mask_final() const {
    return shadow_filter_reach ? shadow_mask_filtered_tex : shadow_accum_max_count ? shadow_history.accumulated : shadow_mask_tex;
  }

  // VKRH_STAGE_SHADOW_MASK_RT: the lights and offsets of the rays (vkrh_set_shadow_rays).  Default: one point light at the shading
  // pass's LIGHT_POS; normal_offset and tmin as measured on the plane-only scene.
  std::vector<float> shadow_rays{-1.85867f, 5.81832f, -0.247114f, 1.0f};
  float shadow_rays_offset = 1e-3f, shadow_rays_tmin = 0.0f;
  void set_shadow_rays(const float* lights, uint32_t count, float normal_offset, float tmin) {
    if (!lights) throw std::runtime_error{"vkrh_set_shadow_rays: NULL argument"};
    refuse_tiled("vkrh_set_shadow_rays", "VKRH_STAGE_SHADOW_MASK_RT runs on one GPU");
    if (count < 1 || count > 4) throw std::runtime_error{"vkrh_set_shadow_rays: count " + std::to_string(count) + ", needs 1..4 (the channels of the mask)"};
    for (uint32_t l = 0; l < count; l++)
      if (!(lights[4 * l + 3] == 0.0f || lights[4 * l + 3] == 1.0f))
        throw std::runtime_error{"vkrh_set_shadow_rays: light " + std::to_string(l) + ": w must be 1 (a point light) or 0 (a directional light)"};
    if (std::isnan(tmin)) throw std::runtime_error{"vkrh_set_shadow_rays: tmin is NaN"};
    if (4 * count != shadow_rays.size()) shadow_area_radii.assign(count, 0.0f);  // the radii belong to the lights they were set for
    shadow_rays.assign(lights, lights + 4 * count);
    shadow_rays_offset = normal_offset; shadow_rays_tmin = tmin;
    shadow_accum_invalid = true;
  }

  // VKRH_STAGE_SHADOW_MASK_RT: the sizes of its lights (vkrh_set_shadow_area_lights).  Default: every radius 0, the hard pass.
  std::vector<float> shadow_area_radii{0.0f};
  uint32_t shadow_area_samples = 16, shadow_area_pattern = 4;
  void set_shadow_area_lights(const float* radii, uint32_t count, uint32_t sample_count, uint32_t pattern_side) {
    if (!radii) throw std::runtime_error{"vkrh_set_shadow_area_lights: NULL argument"};
    refuse_tiled("vkrh_set_shadow_area_lights", "VKRH_STAGE_SHADOW_MASK_RT runs on one GPU");
    if (4 * (size_t)count != shadow_rays.size())
      throw std::runtime_error{"vkrh_set_shadow_area_lights: count " + std::to_string(count) + ", but " + std::to_string(shadow_rays.size() / 4) +
                               " lights are set (vkrh_set_shadow_rays)"};
    if (sample_count < 1 || sample_count > 64)
      throw std::runtime_error{"vkrh_set_shadow_area_lights: sample_count " + std::to_string(sample_count) + ", needs 1..64"};
    if (pattern_side != 1 && pattern_side != 2 && pattern_side != 4)
      throw std::runtime_error{"vkrh_set_shadow_area_lights: pattern_side " + std::to_string(pattern_side) + ", needs 1, 2 or 4"};
    for (uint32_t l = 0; l < count; l++)
      if (!(radii[l] >= 0.0f) || std::isinf(radii[l]))
        throw std::runtime_error{"vkrh_set_shadow_area_lights: light " + std::to_string(l) + ": the radius must be finite and >= 0"};
    shadow_area_radii.assign(radii, radii + count);
    shadow_area_samples = sample_count; shadow_area_pattern = pattern_side;
    shadow_accum_invalid = true;
  }

  // VKRH_STAGE_REFLECTIONS_RT: the mode and the rays (vkrh_set_reflection_rays).  Defaults: every pixel traced, the offsets of the
  // shadow rays, max_distance 0 = the camera's zfar at the time of the run, level 0 of the hit's texture.
  AdvancedSSR::RtSettings reflection_rays {};
  void set_reflection_rays(uint32_t fill_misses, float normal_offset, float tmin, float max_distance, uint32_t texture_lod) {
    refuse_tiled("vkrh_set_reflection_rays", "VKRH_STAGE_REFLECTIONS_RT runs on one GPU");
    if (std::isnan(tmin)) throw std::runtime_error{"vkrh_set_reflection_rays: tmin is NaN"};
    if (std::isnan(max_distance)) throw std::runtime_error{"vkrh_set_reflection_rays: max_distance is NaN"};
    reflection_rays.fill_misses = fill_misses != 0; reflection_rays.normal_offset = normal_offset; reflection_rays.tmin = tmin;
    reflection_rays.max_distance = max_distance > 0.f ? max_distance : 0.f; reflection_rays.texture_lod = texture_lod;
  }

  // VKRH_STAGE_REFLECTIONS_RT: whether the hit of the mirror ray is lit and shadowed (vkrh_set_reflection_lights).  Default: off, the
  // unlit albedo.  The default light is the direct diffuse term of defered_shading: its hard-coded light position, colour 10 / pi
  // (with min(1 / ld2, 1) that kernel's rad / pi) and its ambient 0.6.
  AdvancedSSR::RtLights reflection_lights {};
  void set_reflection_lights(uint32_t count, const float* lights, const float* colours, const float* ambient, float shadow_offset, float shadow_tmin) {
    refuse_tiled("vkrh_set_reflection_lights", "VKRH_STAGE_REFLECTIONS_RT runs on one GPU");
    if (count > 4) throw std::runtime_error{"vkrh_set_reflection_lights: " + std::to_string(count) + " lights, at most 4"};
    if (std::isnan(shadow_offset)) throw std::runtime_error{"vkrh_set_reflection_lights: shadow_offset is NaN"};
    if (std::isnan(shadow_tmin)) throw std::runtime_error{"vkrh_set_reflection_lights: shadow_tmin is NaN"};
    vkr_reflect_lights b {};
    if (count == 1 && !lights && !colours && !ambient) {
      const float pos[4] = {-1.85867f, 5.81832f, -0.247114f, 1.0f};
      for (int k = 0; k < 4; k++) b.lights[0][k] = pos[k];
      for (int k = 0; k < 3; k++) { b.colour[0][k] = 10.0f / 3.1415926535897932384626433832795f; b.ambient[k] = 0.6f; }
    } else {
      if ((count && (!lights || !colours)) || !ambient) throw std::runtime_error{"vkrh_set_reflection_lights: NULL argument (only count 1 with no array at all selects the default light)"};
      for (uint32_t l = 0; l < count; l++) {
        const float w = lights[4 * l + 3];
        if (!(w == 0.0f || w == 1.0f))
          throw std::runtime_error{"vkrh_set_reflection_lights: light " + std::to_string(l) + " has w = " + std::to_string(w) + ", expected 1 (a point light) or 0 (a directional light)"};
        for (int k = 0; k < 4; k++) b.lights[l][k] = lights[4 * l + k];
        for (int k = 0; k < 3; k++) {
          if (std::isnan(colours[3 * l + k])) throw std::runtime_error{"vkrh_set_reflection_lights: colour " + std::to_string(l) + " is NaN"};
          b.colour[l][k] = colours[3 * l + k];
        }
      }
      for (int k = 0; k < 3; k++) {
        if (std::isnan(ambient[k])) throw std::runtime_error{"vkrh_set_reflection_lights: ambient is NaN"};
        b.ambient[k] = ambient[k];
      }
    }
    b.light_count = count; b.shadow_offset = shadow_offset; b.shadow_tmin = shadow_tmin;
    reflection_lights.enable = true; reflection_lights.block = b;
  }

  // VKRH_STAGE_SHADOW_MASK_RT and VKRH_STAGE_REFLECTIONS_RT: whether their rays see alpha cutouts (vkrh_set_ray_cutouts).  Default:
  // off, the opaque query.  VKRH_STAGE_GTAO_RT stays opaque, as the reference's rt_main.frag is.
  RtCutouts ray_cutouts {};
  void set_ray_cutouts(uint32_t enable, uint32_t alpha_lod) {
    refuse_tiled("vkrh_set_ray_cutouts", "the ray-traced stages run on one GPU");
    ray_cutouts.enable = enable != 0; ray_cutouts.alpha_lod = alpha_lod;
    shadow_accum_invalid = true;
  }

  // VKRH_STAGE_TILE_REGRESSION: AdvancedSSR allocates tile_planes when the pass is first recorded
  bool has_tile_planes = false;

  // VKRH_STAGE_BACKBUFFER (main.cpp:398-401): what is drawn, how and at which extent (vkrh_set_backbuffer)
  std::string backbuffer_source;  // empty: the TAA output
  uint32_t backbuffer_flags = 0, backbuffer_w = 0, backbuffer_h = 0;  // extent 0: the frame's
  bool backbuffer_drawn = false;
  VkSampler backbuffer_sampler = gpu::create_sampler(gpu::DEFAULT_SAMPLER);
  rendergraph::ImageResourceId backbuffer_source_id() { return backbuffer_source.empty() ? taa_pass.get_output() : lookup(backbuffer_source); }
  void set_backbuffer(const char* source_image, uint32_t flags, uint32_t width, uint32_t height) {
    refuse_tiled("vkrh_set_backbuffer", "VKRH_STAGE_BACKBUFFER runs on one GPU");
    if ((width == 0) != (height == 0) || width > 65535 || height > 65535)
      throw std::runtime_error{"vkrh_set_backbuffer: extent " + std::to_string(width) + "x" + std::to_string(height) + " (0 x 0: the frame's; at most 65535 a side)"};
    const std::string name = source_image ? source_image : "";
    if (name == "backbuffer") throw std::runtime_error{"vkrh_set_backbuffer: the backbuffer cannot be its own source"};
    if (!name.empty()) {  // an unknown name throws here; the image is looked up again when the stage is recorded
      const auto info = graph.get_descriptor(lookup(name));
      if (info.format == VK_FORMAT_D24_UNORM_S8_UINT) throw std::runtime_error{"vkrh_set_backbuffer: '" + name + "' is a depth image (texdraw samples colour formats)"};
    }
    backbuffer_source = name; backbuffer_flags = flags; backbuffer_w = width; backbuffer_h = height;
  }

  // main.cpp:392-396: the RGBA8_SRGB image the final frame is blitted into before it is read back (capture kind 3)
  rendergraph::ImageResourceId readback_image;
  bool has_readback_image = false;
  rendergraph::ImageResourceId ensure_readback_image() {
    if (!has_readback_image) {
      readback_image = graph.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R8G8B8A8_SRGB, VK_IMAGE_ASPECT_COLOR_BIT, cfg.width, cfg.height},
                                          VK_IMAGE_TILING_OPTIMAL, VK_IMAGE_USAGE_TRANSFER_DST_BIT | VK_IMAGE_USAGE_TRANSFER_SRC_BIT);
      has_readback_image = true;
    }
    return readback_image;
  }

  DrawTAAParams draw_params{};
  glm::mat4 projection, view, prev_view;
  bool has_camera = false;
  bool brdf_lut_ran = false;  // VKRH_STAGE_BRDF_LUT has filled the LUT the shading pass samples (vkrh_tiled_set_shading asks)
  std::string task_names, task_lanes;

  explicit PostFxFrame(const vkrh_config& c)
      : cfg{c}, graph{c.stream, gpu::DeviceConfig{true}}, init{graph, c}, transfer_init{graph},  // main.cpp:73: a ray-query device
        gbuffer{graph, c.width, c.height},
        gtao{graph, c.width, c.height, true, true},  // main.cpp:265 with USE_RAY_QUERY = 1: (graph, W, H, true, half_res = 1)
        ssr{graph, c.width, c.height},
        taa_pass{graph, c.width, c.height},
        shading_pass{graph, nullptr},
        screen_trace{graph, c.width, c.height} {
    if (c.tiled) gbuffer.enable_tiling(graph, c.full_width, c.full_height);
    shadow_map = graph.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_D24_UNORM_S8_UINT, VK_IMAGE_ASPECT_DEPTH_BIT, 16, 16},
                                    VK_IMAGE_TILING_OPTIMAL, VK_IMAGE_USAGE_DEPTH_STENCIL_ATTACHMENT_BIT | VK_IMAGE_USAGE_SAMPLED_BIT);
    // main.cpp:289-291
    color_out_tex = graph.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R8G8B8A8_SRGB, VK_IMAGE_ASPECT_COLOR_BIT, c.width, c.height},
                                       VK_IMAGE_TILING_OPTIMAL, VK_IMAGE_USAGE_COLOR_ATTACHMENT_BIT | VK_IMAGE_USAGE_SAMPLED_BIT);
  }

  void set_camera(const vkrh_camera& cam) {
    std::memcpy(&view, cam.view, 64);
    std::memcpy(&prev_view, cam.prev_view, 64);
    std::memcpy(&projection, cam.projection, 64);
    // main.cpp:334-339
    draw_params.prev_mvp = projection * prev_view;
    draw_params.mvp = projection * view;
    draw_params.prev_camera = prev_view;
    draw_params.camera = view;
    draw_params.fovy_aspect_znear_zfar = glm::vec4{cam.fovy, cam.aspect, cam.znear, cam.zfar};
    draw_params.jitter = glm::vec4{0.f, 0.f, 0.f, 0.f};
    has_camera = true;
  }

  // main.cpp:369-371
  GTAORTParams gtao_rt_params() const {
    const glm::vec4 fazz = draw_params.fovy_aspect_znear_zfar;
    return GTAORTParams{glm::inverse(view), fazz.x, fazz.y, fazz.z, fazz.w};
  }

  void bake_probes(const float* mn, const float* mx, uint32_t grid_size, uint32_t probe_size, uint32_t cube_size) {
    // refused before anything is recorded
    if (!mn || !mx) throw std::runtime_error{"vkrh_bake_probes: NULL argument"};
    refuse_tiled("vkrh_bake_probes", "probes are baked on one GPU");
    if (grid_size < 2 || grid_size > 64) throw std::runtime_error{"vkrh_bake_probes: grid_size " + std::to_string(grid_size) + ", needs 2..64"};
    if (probe_size == 0 || probe_size % 8 || probe_size > 4096) throw std::runtime_error{"vkrh_bake_probes: probe_size must be a multiple of 8 in 8..4096"};
    if (cube_size == 0 || cube_size % 8 || cube_size > 4096) throw std::runtime_error{"vkrh_bake_probes: cube_size must be a multiple of 8 in 8..4096"};
    if (!scene_renderer) throw std::runtime_error{"vkrh_bake_probes: without a loaded scene (vkrh_load_scene)"};
    probe_grid.reset();
    probe_renderer.reset(new ProbeRenderer(graph, cube_size));
    probe_grid.reset(new OctahedralProbeGrid(graph, grid_size, probe_size));
    probe_renderer->render_probe_grid(graph, *scene_renderer, glm::vec3{mn[0], mn[1], mn[2]}, glm::vec3{mx[0], mx[1], mx[2]}, *probe_grid);
    graph.submit();
    record_submitted(false);
  }

  void set_shadow_lights(const float* mvps, uint32_t count, uint32_t size) {
    if (!mvps) throw std::runtime_error{"vkrh_set_shadow_lights: NULL argument"};
    if (count < 1 || count > 4) throw std::runtime_error{"vkrh_set_shadow_lights: count " + std::to_string(count) + ", needs 1..4 (the layers of the shadow image)"};
    if (size > 8192) throw std::runtime_error{"vkrh_set_shadow_lights: size " + std::to_string(size) + ", at most 8192"};
    shadow_lights.resize(count);
    for (uint32_t i = 0; i < count; i++) std::memcpy((void*)&shadow_lights[i], mvps + 16 * i, 64);
    shadow_size = size ? size : 1024;
    shadow_maps_current = false;  // VKRH_STAGE_SHADOW_MASK waits for the next VKRH_STAGE_SHADOW
    shadow_accum_invalid = true;
  }

  // the `shadows` image, created on first use (main.cpp:279-287) and again when the size changes
  void ensure_shadows() {
    if (has_shadows && graph.get_descriptor(shadows).width == shadow_size) return;
    const gpu::ImageInfo info{VK_FORMAT_D24_UNORM_S8_UINT, VK_IMAGE_ASPECT_DEPTH_BIT | VK_IMAGE_ASPECT_STENCIL_BIT, shadow_size, shadow_size, 1, 1, 4};
    if (has_shadows) {
      // the graph's resource table only grows: the new image takes the old one's place, so that its memory is returned
      if (hipStreamSynchronize((hipStream_t)cfg.stream) != hipSuccess) throw std::runtime_error{"shadow map: stream synchronisation failed"};
      graph.get_image(shadows) = std::make_shared<gpu::Image>(info, gpu::FrameWindow{});
    } else {
      shadows = graph.create_frame_image(info);  // never a window of the frame, whatever the frame's extent
      has_shadows = true;
    }
    shadows_rendered = false;
  }

  bool has(Needs needs) const {
    const bool tlas = scene_as && scene_as->tlas;
    return needs == Needs::Scene ? scene_renderer != nullptr : needs == Needs::Tlas ? tlas : needs == Needs::TlasAndScene ? tlas && scene_renderer
           : needs == Needs::Probes ? probe_grid != nullptr : true;
  }
  void check_stage_rules(uint32_t mask) {
    for (const StageRule& rule : STAGE_RULES) {
      if (!(mask & rule.stage)) continue;
      const auto refuse = [&](const char* how, const char* tail, const char* end) {
        throw std::runtime_error{std::string{"vkrh_run: "} + rule.name + how + tail + end};
      };
      if (cfg.tiled && rule.tiled) refuse(" on a tiled frame (", rule.tiled, ")");
      if (mask & rule.rivals) refuse(" together with ", rule.rivals_tail, "");
      if (!has(rule.needs)) refuse(" without ", rule.needs_tail, "");
      // the two rules that are no table entries, at their stage's place in the order
      if (rule.stage == VKRH_STAGE_BACKBUFFER) (void)backbuffer_source_id();  // a source that does not exist (yet) throws
      if (rule.stage == VKRH_STAGE_SHADOW_MASK && !(mask & VKRH_STAGE_SHADOW) && !shadow_maps_current)
        refuse(" without ", "rendered shadow maps (VKRH_STAGE_SHADOW for the lights in use)", "");
    }
  }

  void run(uint32_t mask) {
    if (!has_camera && (mask & ~uint32_t(VKRH_STAGE_LUT))) throw std::runtime_error{"vkrh_run: camera not set"};
    check_stage_rules(mask);  // refused before anything is recorded
    const glm::vec4 fazz = draw_params.fovy_aspect_znear_zfar;
    if (mask & (VKRH_STAGE_CLEAR_PREV_DEPTH | VKRH_STAGE_PREV_DEPTH)) shadow_accum_chained = false;  // prev_depth is no longer last frame's depth
    if (mask & VKRH_STAGE_CLEAR_PREV_DEPTH) clear_depth(graph, gbuffer.prev_depth);  // main.cpp:306
    if (mask & VKRH_STAGE_LUT) ssr.preintegrate_pdf(graph);
    if (mask & VKRH_STAGE_BRDF_LUT) { ssr.preintegrate_brdf(graph); brdf_lut_ran = true; }
    if (mask & VKRH_STAGE_PREV_DEPTH) {
      // what the previous frame left behind: its depth in `prev_depth`, including the Hi-Z mips
      synth.draw_depth(graph, gbuffer.prev_depth, prev_view, draw_params.prev_mvp, fazz);
      downsample_pass.run(graph, gbuffer.normal, gbuffer.velocity_vectors, gbuffer.prev_depth, gbuffer.downsampled_normals,
                          gbuffer.downsampled_velocity_vectors);
    }
    if (mask & VKRH_STAGE_GBUFFER) synth.draw_taa(graph, gbuffer, draw_params);
    if (mask & VKRH_STAGE_RASTER) {  // main.cpp:345
      if (!scene_renderer) throw std::runtime_error{"vkrh_run: VKRH_STAGE_RASTER without a loaded scene"};
      scene_renderer->draw_taa(graph, gbuffer, draw_params);
    }
    if (mask & VKRH_STAGE_SHADOW) {  // main.cpp:346, for every configured light
      ensure_shadows();
      for (uint32_t l = 0; l < shadow_lights.size(); l++) scene_renderer->render_shadow(graph, shadow_lights[l], shadows, l);
      shadows_rendered = true;
      shadow_maps_current = true;
    }
    if (mask & VKRH_STAGE_SHADOW_MASK) {  // reads depth mip 0 and the layers just rendered
      ShadowMaskPass& pass = ensure_shadow_mask();
      pass.update_params(view, shadow_lights.data(), (uint32_t)shadow_lights.size(), fazz.x, fazz.y, fazz.z, fazz.w, shadow_mask_radius, shadow_mask_bias);
      pass.run(graph, gbuffer.depth, shadows, (uint32_t)shadow_lights.size(), shadow_mask_tex);
      record_shadow_mask_filter(pass);
    }
    if (mask & VKRH_STAGE_SHADOW_MASK_RT) {  // reads depth mip 0 and the normal of this run's G-buffer; the slot of the looked-up mask
      ShadowMaskPass& pass = ensure_shadow_mask();
      pass.update_rt_params(view, shadow_rays.data(), (uint32_t)(shadow_rays.size() / 4), fazz.x, fazz.y, fazz.z, fazz.w, shadow_rays_offset, shadow_rays_tmin);
      float radii[4] = {0.f, 0.f, 0.f, 0.f};
      std::copy(shadow_area_radii.begin(), shadow_area_radii.end(), radii);
      pass.update_rt_soft(radii, shadow_area_samples, shadow_area_pattern);
      select_shadow_sample_tables(pass);
      if (ray_cutouts.enable && scene_renderer)
        pass.run_rt(graph, gbuffer.depth, gbuffer.normal, AdvancedSSR::RtScene{scene_as->tlas, scene_as->hit_attributes, scene_renderer->get_images(), nullptr},
                    ray_cutouts, shadow_mask_tex);
      else
        pass.run_rt(graph, gbuffer.depth, gbuffer.normal, scene_as->tlas, shadow_mask_tex);
      record_shadow_mask_filter(pass);
    }
    if (mask & VKRH_STAGE_SSAO) {  // reads depth mip 0 only: before the downsample writes the other mips
      SSAOPass& pass = ensure_ssao();
      pass.draw(graph, gbuffer.depth, ssao_tex, SSAOInParams{projection, fazz.x, fazz.y, fazz.z, fazz.w});
    }
    if (mask & VKRH_STAGE_DOWNSAMPLE)  // main.cpp:347
      downsample_pass.run(graph, gbuffer.normal, gbuffer.velocity_vectors, gbuffer.depth, gbuffer.downsampled_normals,
                          gbuffer.downsampled_velocity_vectors);
    if (mask & VKRH_STAGE_DOWNSAMPLE_NEXT) {
      if (!gbuffer.pipelined) throw std::runtime_error{"vkrh_run: VKRH_STAGE_DOWNSAMPLE_NEXT without the G-buffer's second set"};
      downsample_pass.run(graph, gbuffer.normal, gbuffer.velocity_vectors, gbuffer.depth_next, gbuffer.downsampled_normals_next,
                          gbuffer.downsampled_velocity_vectors_next);
    }
    if ((mask & VKRH_STAGE_HIZ_TAIL) && gbuffer.tiled) {
      // the launcher gathered whole-frame mips 0..k of frame_hiz; finish the chain locally
      downsample_pass.run_downsample_depth(graph, gbuffer.frame_hiz, hiz_gathered_mips - 1);
    }
    // main.cpp:368-373
    const glm::mat4 normal_mat = glm::transpose(glm::inverse(view));
    const GTAOParams gtao_params{normal_mat, fazz.x, fazz.y, fazz.z, fazz.w};
    const AdvancedSSRParams assr_params{normal_mat, fazz.x, fazz.y, fazz.z, fazz.w};
    if (mask & VKRH_STAGE_TILE_REGRESSION) {  // reads depth mip 1: after the downsample of this run; independent of the SSR stages
      ssr.run_tile_regression_pass(graph, assr_params, gbuffer);
      has_tile_planes = true;
    }
    if (mask & (VKRH_STAGE_SSR | VKRH_STAGE_SSR_CLASSIFIED)) {                               // main.cpp:375
      ssr.get_settings().use_tile_classification = (mask & VKRH_STAGE_SSR_CLASSIFIED) != 0;
      ssr.run(graph, assr_params, draw_params, gbuffer, gtao.raw);
    }
    if (mask & VKRH_STAGE_SSR_TRACE_HEAD) ssr.run_trace_head(graph, assr_params, gbuffer, gtao.raw, hiz_gathered_mips);
    if (mask & VKRH_STAGE_SSR_TRACE_RESUME) ssr.run_trace_resume(graph, gbuffer, gtao.raw);
    if (mask & VKRH_STAGE_SSR_TRACE) ssr.run_trace(graph, assr_params, gbuffer, gtao.raw);
    if (mask & VKRH_STAGE_SSR_RESOLVE) ssr.run_resolve(graph, assr_params, draw_params, gbuffer);
    if (mask & VKRH_STAGE_REFLECTIONS_RT) {  // the place of the SSR stages: reads depth mip 1 and the half-resolution normals of the downsample
      AdvancedSSR::RtSettings rt = reflection_rays;
      if (!(rt.max_distance > 0.f)) rt.max_distance = fazz.w;
      const bool classified = ssr.get_settings().use_tile_classification;  // fill mode traces with the plain trace; the setting is the SSR stages'
      ssr.get_settings().use_tile_classification = false;
      ssr.run_rt(graph, assr_params, draw_params, gbuffer, gtao.raw,
                 AdvancedSSR::RtScene{scene_as->tlas, scene_as->hit_attributes, scene_renderer->get_images(), scene_as->hit_normals}, rt, ray_cutouts,
                 reflection_lights);
      ssr.get_settings().use_tile_classification = classified;
    }
    if (mask & VKRH_STAGE_GTAO_MAIN_ONLY)
      gtao.add_main_pass(graph, gtao_params, gbuffer.depth, gbuffer.normal, gbuffer.material, ssr.get_preintegrated_pdf());
    if (mask & VKRH_STAGE_GTAO) {                                                           // main.cpp:384-388
      gtao.add_main_pass(graph, gtao_params, gbuffer.depth, gbuffer.normal, gbuffer.material, ssr.get_preintegrated_pdf());
      gtao.add_filter_pass(graph, gtao_params, gbuffer.depth);
      gtao.add_accumulate_pass(graph, draw_params, gbuffer);
    }
    if (mask & VKRH_STAGE_GTAO_RT) {                                                        // main.cpp:379-388 (use_rt_ao)
      gtao.add_main_rt_pass(graph, gtao_rt_params(), scene_as->tlas, gbuffer.depth, gbuffer.normal);
      gtao.add_filter_pass(graph, gtao_params, gbuffer.depth);
      gtao.add_accumulate_pass(graph, draw_params, gbuffer);
    }
    // ---- passes the reference ships but never records ----
    if (mask & VKRH_STAGE_PROBE_TRACE) {
      if (!has_probe_trace_out) {
        probe_trace_out = graph.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R8G8B8A8_UNORM, VK_IMAGE_ASPECT_COLOR_BIT, cfg.width, cfg.height},
                                             VK_IMAGE_TILING_OPTIMAL, VK_IMAGE_USAGE_STORAGE_BIT | VK_IMAGE_USAGE_SAMPLED_BIT);
        has_probe_trace_out = true;
      }
      const glm::vec4 fazz = draw_params.fovy_aspect_znear_zfar;
      probe_trace_pass.run(graph, *probe_grid, gbuffer.depth, gbuffer.normal, probe_trace_out, ProbeTraceParams{glm::inverse(view), fazz.x, fazz.y, fazz.z, fazz.w});
    }
    if (mask & VKRH_STAGE_GTAO_GRAPHICS) {
      gtao.add_main_pass_graphics(graph, gtao_params, gbuffer.depth, gbuffer.normal);
      gtao.add_filter_pass(graph, gtao_params, gbuffer.depth);
      const GTAOReprojection reprojection{prev_view * glm::inverse(view), fazz.x, fazz.y, fazz.z, fazz.w};
      gtao.add_reprojection_pass(graph, reprojection, gbuffer.depth, gbuffer.prev_depth);
    }
    if (mask & VKRH_STAGE_GTAO_DEINTERLEAVED) {
      gtao.deinterleave_depth(graph, gbuffer.depth);
      gtao.add_main_pass_deinterleaved(graph, gtao_params, gbuffer.normal);
    }
    if (mask & VKRH_STAGE_SCREEN_TRACE) {
      const ScreenTraceParams st_params{normal_mat, fazz.x, fazz.y, fazz.z, fazz.w};
      screen_trace.add_main_pass(graph, st_params, gbuffer.depth, gbuffer.normal, gbuffer.albedo, gbuffer.material);
      screen_trace.add_filter_pass(graph, st_params, gbuffer.depth);
      screen_trace.add_accumulate_pass(graph, st_params, gbuffer.depth, gbuffer.prev_depth);
    }
    // main.cpp:343,390-391: shading composes albedo / AO / reflections into color_out_tex, which TAA
    // resolves.  Without the shading stage TAA resolves the albedo attachment (the headline
    // composite of BASELINE.json is the nine passes without shading).
    if (mask & VKRH_STAGE_SHADING) {
      // main.cpp:339,390: once VKRH_STAGE_SHADOW has filled it, layer 0 of `shadows` and its matrix; until then the dummy
      const bool lit = has_shadows && shadows_rendered;
      shading_pass.update_params(view, lit ? shadow_lights[0] : glm::mat4{1.f}, fazz.x, fazz.y, fazz.z, fazz.w);
      if (shadow_mask_apply && (mask & (VKRH_STAGE_SHADOW_MASK | VKRH_STAGE_SHADOW_MASK_RT)))  // vkrh_set_shadow_mask(apply) and the mask of this run
        shading_pass.draw_shadowed(graph, gbuffer, lit ? shadows : shadow_map, gtao.accumulated_ao, ssr.get_preintegrated_brdf(), ssr.get_blurred(),
                                   shadow_mask_final(), color_out_tex);  // the filtered mask when the filter is on, else the accumulated one
      else
        shading_pass.draw(graph, gbuffer, lit ? shadows : shadow_map, gtao.accumulated_ao, ssr.get_preintegrated_brdf(), ssr.get_blurred(), color_out_tex);
    }
    if (mask & VKRH_STAGE_TAA) taa_pass.run(graph, gbuffer, (mask & VKRH_STAGE_SHADING) ? color_out_tex : gbuffer.albedo, draw_params);
    if (mask & VKRH_STAGE_BACKBUFFER) {  // main.cpp:398-401
      graph.set_backbuffer_extent(backbuffer_w ? backbuffer_w : cfg.width, backbuffer_h ? backbuffer_h : cfg.height);
      add_backbuffer_subpass(graph, backbuffer_source_id(), backbuffer_sampler, DrawTex(backbuffer_flags));
      add_present_subpass(graph);
      backbuffer_drawn = true;
    }
    graph.submit();
    if ((mask & (VKRH_STAGE_GBUFFER | VKRH_STAGE_RASTER)) && gbuffer.pipelined) copy_depth_to_next_set();
    record_submitted(true);
  }

  // pipelined: the G-buffer's depth (mip 0 of the depth image) also into the second set — the G-buffer of the benchmark is one
  // static frame; a renderer with two frames in flight draws every frame's depth into the set that frame will use
  void copy_depth_to_next_set() {
    const vkr_img a = graph.get_image(gbuffer.depth)->describe(0, 1), b = graph.get_image(gbuffer.depth_next)->describe(0, 1);
    if (hipMemcpy2DAsync(b.base, b.pitch_bytes[0], a.base, a.pitch_bytes[0], size_t(a.width) * 4, a.height, hipMemcpyDeviceToDevice, (hipStream_t)cfg.stream) != hipSuccess)
      throw std::runtime_error{"pipelined frame: copy of the depth into the second set failed"};
  }

  // TraceParams as run() hands them to the SSR passes (main.cpp:368-373), for the tiled frame's deferred hit-normal test
  vkr_trace_params trace_params() const {
    vkr_trace_params t {};
    const glm::mat4 normal_mat = glm::transpose(glm::inverse(view));
    std::memcpy(t.normal_mat.m, &normal_mat, sizeof(t.normal_mat.m));
    const glm::vec4 fazz = draw_params.fovy_aspect_znear_zfar;
    t.fovy = fazz.x; t.aspect = fazz.y; t.znear = fazz.z; t.zfar = fazz.w;
    return t;
  }

  void end_frame(bool swap_depth) {  // main.cpp:416-420
    if (swap_depth) graph.remap(gbuffer.depth, gbuffer.prev_depth);
    if (shadow_accum_pending) {  // what the accumulation wrote is what it reads next
      graph.remap(shadow_history.history, shadow_history.out_history);
      graph.remap(shadow_history.count, shadow_history.out_count);
    }
    shadow_accum_chained = shadow_accum_pending && swap_depth;
    shadow_accum_pending = false;
    graph.remap(gtao.output, gtao.prev_frame);  // main.cpp:417: the reprojection variant's history (gtao.cpp:241-284)
    taa_pass.remap_targets(graph);
    ssr.remap_images(graph);
    gtao.remap(graph);
  }

  uint32_t hiz_gathered_mips = 4;  // tiled: view mips 0..3 of frame_hiz (image mips 1..4) arrive by all-gather

  std::map<std::string, rendergraph::ImageResourceId> user_images;  // vkrh_create_image

  static VkFormat vk_format(uint32_t format) {  // the inverse of gpu::to_vkr_format
    for (VkFormat f : {VK_FORMAT_D24_UNORM_S8_UINT, VK_FORMAT_R16G16_UNORM, VK_FORMAT_R16G16_SFLOAT, VK_FORMAT_R8G8B8A8_SRGB, VK_FORMAT_R8G8B8A8_UNORM,
                       VK_FORMAT_R16G16B16A16_UNORM, VK_FORMAT_R16G16B16A16_SFLOAT, VK_FORMAT_R16_SFLOAT, VK_FORMAT_R32_SFLOAT, VK_FORMAT_R8_UNORM,
                       VK_FORMAT_R32G32B32A32_SFLOAT, VK_FORMAT_R16_UNORM})
      if (gpu::to_vkr_format(f) == format) return f;
    throw std::runtime_error{"vkrh_create_image: unknown format " + std::to_string(format)};
  }
  void create_user_image(const char* name, uint32_t format, uint32_t w, uint32_t h, uint32_t mips, uint32_t layers) {
    if (!name || !*name) throw std::runtime_error{"vkrh_create_image: NULL name"};
    refuse_tiled("vkrh_create_image", "transfers take whole images");
    if (user_images.count(name) || named_image(name)) throw std::runtime_error{std::string{"vkrh_create_image: the name '"} + name + "' is taken"};
    const VkFormat fmt = vk_format(format);
    if (!w || !h || !mips || mips > VKR_MAX_MIPS || !layers) throw std::runtime_error{"vkrh_create_image: bad extent, mip or layer count"};
    const VkImageAspectFlags aspect = format == VKR_FMT_D24_UNORM_S8 ? VK_IMAGE_ASPECT_DEPTH_BIT | VK_IMAGE_ASPECT_STENCIL_BIT : VK_IMAGE_ASPECT_COLOR_BIT;
    user_images[name] = graph.create_frame_image(gpu::ImageInfo{fmt, aspect, w, h, 1, mips, layers});
  }
  void transfer(uint32_t op, const char* image, const char* dst, const float* value) {
    refuse_tiled("vkrh_transfer", "transfers take whole images");
    if (!image) throw std::runtime_error{"vkrh_transfer: NULL image name"};
    const rendergraph::ImageResourceId id = lookup(image);
    switch (op) {
      case VKRH_TRANSFER_GEN_MIPMAPS: gen_mipmaps(graph, id); break;
      case VKRH_TRANSFER_CLEAR_DEPTH: clear_depth(graph, id, value ? value[0] : 1.0f); break;
      case VKRH_TRANSFER_CLEAR_COLOR: {
        if (!value) throw std::runtime_error{"vkrh_transfer: clear_color needs a value"};
        VkClearColorValue v{};
        std::memcpy(v.float32, value, sizeof(v.float32));
        clear_color(graph, id, v);
        break;
      }
      case VKRH_TRANSFER_BLIT: {
        if (!dst) throw std::runtime_error{"vkrh_transfer: blit_image needs a destination"};
        const rendergraph::ImageResourceId to = lookup(dst);
        if (to == id) throw std::runtime_error{"vkrh_transfer: blit_image onto the source"};
        blit_image(graph, id, to);
        break;
      }
      default: throw std::runtime_error{"vkrh_transfer: unknown operation " + std::to_string(op)};
    }
    graph.submit();
    record_submitted(false);
  }

  // The names vkrh_image and its kin know besides the user's own: what each stands for and, for an image that is created on
  // demand, when it exists ("vkrh_image: '<name>' <absent>" until then).  A new image is one line here.
  struct NamedImage {
    const char* name;
    rendergraph::ImageResourceId (*image)(PostFxFrame&);
    bool (*exists)(const PostFxFrame&) = nullptr;  // nullptr: always
    const char* absent = nullptr;
  };
  static const NamedImage* named_image(const std::string& name) {
    using F = PostFxFrame;
    static constexpr const char* BAKED = "only exists after vkrh_bake_probes";
    static constexpr const char* SHADOW_HISTORY_ONLY = "only exists after a mask stage with vkrh_set_shadow_mask_accumulate on";
    static const NamedImage table[] = {
        {"depth", [](F& f) { return f.gbuffer.depth; }}, {"prev_depth", [](F& f) { return f.gbuffer.prev_depth; }}, {"normal", [](F& f) { return f.gbuffer.normal; }},
        {"albedo", [](F& f) { return f.gbuffer.albedo; }}, {"material", [](F& f) { return f.gbuffer.material; }}, {"velocity", [](F& f) { return f.gbuffer.velocity_vectors; }},
        {"dn", [](F& f) { return f.gbuffer.downsampled_normals; }}, {"dv", [](F& f) { return f.gbuffer.downsampled_velocity_vectors; }}, {"raw", [](F& f) { return f.gtao.raw; }},
        {"filtered", [](F& f) { return f.gtao.filtered; }}, {"acc_ao", [](F& f) { return f.gtao.accumulated_ao; }}, {"acc_hist", [](F& f) { return f.gtao.accumulated_history; }},
        {"rays", [](F& f) { return f.ssr.get_rays(); }}, {"reflections", [](F& f) { return f.ssr.get_ouput(); }}, {"blurred", [](F& f) { return f.ssr.get_blurred(); }},
        {"blurred_hist", [](F& f) { return f.ssr.get_blurred_history(); }}, {"pdf", [](F& f) { return f.ssr.get_preintegrated_pdf(); }}, {"taa_hist", [](F& f) { return f.taa_pass.get_history(); }},
        {"taa_target", [](F& f) { return f.taa_pass.get_output(); }}, {"frame_hiz", [](F& f) { return f.gbuffer.frame_hiz; }}, {"frame_normals", [](F& f) { return f.gbuffer.frame_normals; }},
        {"frame_albedo", [](F& f) { return f.gbuffer.frame_albedo; }}, {"color_out", [](F& f) { return f.color_out_tex; }}, {"brdf", [](F& f) { return f.ssr.get_preintegrated_brdf(); }},
        {"ao_prev_frame", [](F& f) { return f.gtao.prev_frame; }}, {"ao_output", [](F& f) { return f.gtao.output; }}, {"deinterleaved_depth", [](F& f) { return f.gtao.deinterleaved_depth; }},
        {"st_raw", [](F& f) { return f.screen_trace.raw; }}, {"st_filtered", [](F& f) { return f.screen_trace.filtered; }}, {"st_accumulated", [](F& f) { return f.screen_trace.accumulated; }},
        {"pend_mask", [](F& f) { return f.gbuffer.pend_mask; }, [](const F& f) { return f.gbuffer.normals_by_request; }, "only exists with hit normals by request"},
        {"probe_trace", [](F& f) { return f.probe_trace_out; }, [](const F& f) { return f.has_probe_trace_out; }, "only exists after VKRH_STAGE_PROBE_TRACE"},
        {"probe_color", [](F& f) { return f.probe_grid->color_array; }, [](const F& f) { return f.probe_grid != nullptr; }, BAKED},
        {"probe_depth", [](F& f) { return f.probe_grid->depth_array; }, [](const F& f) { return f.probe_grid != nullptr; }, BAKED},
        {"cubemap_color", [](F& f) { return f.probe_renderer->get_cubemap_color(); }, [](const F& f) { return f.probe_grid != nullptr; }, BAKED},
        {"cubemap_distance", [](F& f) { return f.probe_renderer->get_cubemap_distance(); }, [](const F& f) { return f.probe_grid != nullptr; }, BAKED},
        {"shadows", [](F& f) { return f.shadows; }, [](const F& f) { return f.has_shadows; }, "only exists after VKRH_STAGE_SHADOW"},
        {"readback", [](F& f) { return f.readback_image; }, [](const F& f) { return f.has_readback_image; },
         "only exists after a final-frame capture (vkrh_capture kind 3)"},
        {"ssao", [](F& f) { return f.ssao_tex; }, [](const F& f) { return f.ssao_pass != nullptr; }, "only exists after VKRH_STAGE_SSAO or vkrh_set_ssao_samples"},
        {"tile_planes", [](F& f) { return f.ssr.get_tile_planes(); }, [](const F& f) { return f.has_tile_planes; }, "only exists after VKRH_STAGE_TILE_REGRESSION"},
        {"backbuffer", [](F& f) { return f.graph.get_backbuffer(); }, [](const F& f) { return f.backbuffer_drawn; }, "only exists after VKRH_STAGE_BACKBUFFER"},
        {"shadow_mask", [](F& f) { return f.shadow_mask_tex; }, [](const F& f) { return f.shadow_mask_pass != nullptr; },
         "only exists after VKRH_STAGE_SHADOW_MASK or VKRH_STAGE_SHADOW_MASK_RT"},
        {"shadow_mask_filtered", [](F& f) { return f.shadow_mask_filtered_tex; }, [](const F& f) { return f.has_shadow_mask_filtered; },
         "only exists after a mask stage with vkrh_set_shadow_mask_filter on"},
        {"shadow_mask_accumulated", [](F& f) { return f.shadow_history.accumulated; }, [](const F& f) { return f.has_shadow_history; }, SHADOW_HISTORY_ONLY},
        {"shadow_history", [](F& f) { return f.shadow_history.history; }, [](const F& f) { return f.has_shadow_history; }, SHADOW_HISTORY_ONLY},
        {"shadow_history_out", [](F& f) { return f.shadow_history.out_history; }, [](const F& f) { return f.has_shadow_history; }, SHADOW_HISTORY_ONLY},
        {"shadow_history_count", [](F& f) { return f.shadow_history.count; }, [](const F& f) { return f.has_shadow_history; }, SHADOW_HISTORY_ONLY},
        {"shadow_history_count_out", [](F& f) { return f.shadow_history.out_count; }, [](const F& f) { return f.has_shadow_history; }, SHADOW_HISTORY_ONLY},
    };
    for (const NamedImage& e : table)
      if (name == e.name) return &e;
    return nullptr;
  }
  rendergraph::ImageResourceId lookup(const std::string& name) {
    const auto user = user_images.find(name);
    if (user != user_images.end()) return user->second;
    const NamedImage* e = named_image(name);
    if (!e) throw std::runtime_error{"vkrh_image: unknown image '" + name + "'"};
    if (e->exists && !e->exists(*this)) throw std::runtime_error{"vkrh_image: '" + name + "' " + e->absent};
    return e->image(*this);
  }
};


// ---- the tiled frame: strips + RCCL (frame.hpp) ----------------------------------------------------------------------
struct TiledFrame {
  vkrh_tiled_config cfg;
  uint32_t W, H, th, y0, wy0, wh;  // tile rows [y0, y0 + th), window rows [wy0, wy0 + wh)
  bool tiled;
  std::unique_ptr<PostFxFrame> frame;
  hipStream_t compute = nullptr, xchg = nullptr;
  hipEvent_t ev_ready[5] {}, ev_done[5] {};  // 0 hiz, 1 albedo, 2 taa, 3 ao, 4 ssr
  bool halo_in_flight[3] {false, false, false};
  struct HaloBuf { void* send = nullptr; void* recv = nullptr; uint64_t bytes = 0; };
  HaloBuf halo[3][2];  // [surface][0: neighbour above, 1: neighbour below]

  static void check(hipError_t e, const char* what) { if (e != hipSuccess) throw std::runtime_error {std::string {what} + ": " + hipGetErrorString(e)}; }

  std::vector<uint32_t> bounds;   // world + 1 strip boundaries (rows)
  bool uniform = true;             // equal strips: ncclAllGather; otherwise vkr_all_gather_v
  std::vector<std::vector<uint64_t>> gather_offsets[2];  // [which][part][world + 1]: byte offsets of the ranks' shares

  explicit TiledFrame(const vkrh_tiled_config& c) : cfg {c} {
    W = c.full_width; H = c.full_height;
    if (c.world == 0 || c.rank >= c.world) throw std::runtime_error {"vkrh_tiled_create: rank outside the world"};
    tiled = c.world > 1 || c.force_tiled;
    const uint32_t k = c.gathered_mips;
    bounds.resize(c.world + 1);
    if (c.row_bounds) {
      for (uint32_t r = 0; r <= c.world; r++) bounds[r] = c.row_bounds[r];
      if (bounds[0] != 0 || bounds[c.world] != H) throw std::runtime_error {"vkrh_tiled_create: row_bounds must run from 0 to the frame height"};
      for (uint32_t r = 0; r < c.world; r++) {
        if (bounds[r + 1] <= bounds[r]) throw std::runtime_error {"vkrh_tiled_create: row_bounds must increase"};
        if (bounds[r + 1] - bounds[r] != H / c.world || H % c.world) uniform = false;
      }
    } else {
      if (H % c.world) throw std::runtime_error {"vkrh_tiled_create: the frame height must divide by the number of ranks"};
      for (uint32_t r = 0; r <= c.world; r++) bounds[r] = r * (H / c.world);
    }
    if (getenv("VKR_TILED_FORCE_GATHER_V")) uniform = false;  // tests: the broadcast-based gather also for equal strips
    cfg.row_bounds = nullptr;  // the caller's array need not outlive the call
    th = bounds[c.rank + 1] - bounds[c.rank]; y0 = bounds[c.rank];
    if (tiled && (k < 1 || k > 4 || W % (1u << k) || (c.world > 1 && c.halo % (1u << k))))
      throw std::runtime_error {"vkrh_tiled_create: tile extent and halo must be multiples of 2^gathered_mips (1..4)"};
    for (uint32_t r = 0; tiled && r <= c.world; r++)
      if (bounds[r] % (1u << k) || (bounds[r] & 1u)) throw std::runtime_error {"vkrh_tiled_create: strip bounds must be multiples of 2^gathered_mips (1..4)"};
    for (uint32_t r = 0; c.world > 1 && r < c.world; r++)
      if (c.halo > bounds[r + 1] - bounds[r] || (c.halo & 1u)) throw std::runtime_error {"vkrh_tiled_create: halo must be even and no larger than a strip"};
    const uint32_t halo_px = c.world > 1 ? c.halo : 0;
    wy0 = y0 >= halo_px ? y0 - halo_px : 0;
    const uint32_t wy1 = std::min(H, y0 + th + halo_px);
    wh = wy1 - wy0;
    compute = (hipStream_t)c.stream;
    vkrh_config fc {W, H, 0, (int32_t)wy0, W, wh, tiled ? 1u : 0u, c.stream};
    frame.reset(new PostFxFrame(fc));
    frame->hiz_gathered_mips = tiled ? k : 4;
    if (normals_by_request()) frame->gbuffer.enable_normal_requests(frame->graph, wy0 / 2, (wy0 + wh) / 2);
    if (tiled && c.world > 1 && !env_set("VKR_TILED_WHOLE_WINDOW")) clip_outputs();
    // Two frames in flight (VKR_TILED_PIPELINE=1, native wire, hit colours by request): the next frame's downsample and depth
    // all-gather start right after this frame's trace and travel while its GTAO, TAA, resolve and blur run (pipelined_step).
    pipeline_enabled = tiled && c.world > 1 && by_request() && env_set("VKR_TILED_PIPELINE");
    if (pipeline_enabled) frame->gbuffer.enable_pipelining(frame->graph);
    if (tiled) {
      // the exchanges' kernels (a few workgroups each) must not queue behind a frame's worth of compute waves
      int prio_low = 0, prio_high = 0;
      check(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high), "stream priority range");
      check(hipStreamCreateWithPriority(&xchg, hipStreamNonBlocking, prio_high), "exchange stream");
      for (auto& e : ev_ready) check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "event");
      for (auto& e : ev_done) check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "event");
      if (by_request()) hit_init();
      for (int s = 0; s < 3; s++)
        for (int n = 0; n < 2; n++) {
          if (!neighbour(n, nullptr)) continue;
          const vkr_img d = surface(s);
          halo[s][n].bytes = uint64_t(halo_px >> halo_dv(s)) * d.width * vkr_format_bytes(d.format);
          halo[s][n].send = gpu::device_alloc(halo[s][n].bytes);
          halo[s][n].recv = gpu::device_alloc(halo[s][n].bytes);
        }
    }
  }
  bool pipeline_enabled = false, primed = false;
  static bool env_set(const char* name) { const char* v = getenv(name); return v && *v && *v != '0'; }
  // Which rows of its window a rank has to COMPUTE (gpu::Image::set_store_rows; VKR_TILED_WHOLE_WINDOW=1 keeps round 3's "every
  // pass on the whole window").  The three history surfaces and the filtered AO: the strip itself — the halo rows of a history
  // arrive from the neighbours before the next frame reads them (copy_halo overwrote what the pass had computed there anyway),
  // and the accumulation reads the filtered AO at its own pixel only.  The resolved reflections: the strip and the blur's apron
  // (blur.comp: taps up to 11 texels away; ssr.hip BLUR_R).  The rays — with their pending mask / data and the (occlusion, pdf)
  // image the trace shares with GTAO main — two rows more: the resolve reads its four neighbours (filter.comp:112-134), GTAO's
  // filter taps reach two rows (filter.comp:17-51); the request / reply round and the deferred normal test walk the same rows
  // (rays_img() etc. describe the store rows).  The downsample stays whole-window: everything above reads its halo.
  // With shading on, color_out: the strip and one row either side — the TAA reads its four neighbours (resolve.comp) — clamped
  // to the frame (the window ends there).
  bool clipped = false;
  void store_rows(rendergraph::ImageResourceId id, uint32_t shift, uint32_t apron) {
    gpu::Image& img = *frame->graph.get_image(id);
    const uint32_t top = y0 - wy0;  // rows of halo above the strip inside the window
    const uint32_t first = top >> shift, last = (top + th) >> shift, h = img.get_info().height;
    const uint32_t lo = first > apron ? first - apron : 0, hi = std::min(h, last + apron);
    img.set_store_rows(lo, hi - lo);
  }
  void clip_outputs() {
    clipped = true;
    const auto rows = [&](rendergraph::ImageResourceId id, uint32_t shift, uint32_t apron) { store_rows(id, shift, apron); };
    rows(frame->taa_pass.get_output(), 0, 0); rows(frame->taa_pass.get_history(), 0, 0);
    rows(frame->gtao.accumulated_ao, 1, 0); rows(frame->gtao.accumulated_history, 1, 0); rows(frame->gtao.filtered, 1, 0);
    rows(frame->ssr.get_blurred(), 1, 0); rows(frame->ssr.get_blurred_history(), 1, 0);
    rows(frame->ssr.get_ouput(), 1, 12);
    rows(frame->ssr.get_rays(), 1, 14); rows(frame->gtao.raw, 1, 14);
    if (normals_by_request()) { rows(frame->gbuffer.pend_mask, 1, 14); rows(frame->gbuffer.pend_data, 1, 14); }
  }
  void drop_wait_marks() {
    for (auto& v : wait_marks) { for (auto& m : v) { (void)hipEventDestroy(m.first); (void)hipEventDestroy(m.second); } v.clear(); }
  }
  ~TiledFrame() {
    if (compute) (void)hipStreamSynchronize(compute);
    drop_wait_marks();
    if (xchg) { (void)hipStreamSynchronize(xchg); (void)hipStreamDestroy(xchg); }
    for (auto e : ev_ready) if (e) (void)hipEventDestroy(e);
    for (auto e : ev_done) if (e) (void)hipEventDestroy(e);
    for (auto& s : halo) for (auto& b : s) { gpu::device_free(b.send); gpu::device_free(b.recv); }
    hit_release();
  }

  // ---- geometry -------------------------------------------------------------------------------------------------
  bool neighbour(int n, int* rank) const {  // 0: the strip above, 1: the strip below
    if (cfg.world < 2) return false;
    if (n == 0 ? cfg.rank == 0 : cfg.rank + 1 == cfg.world) return false;
    if (rank) *rank = n == 0 ? int(cfg.rank) - 1 : int(cfg.rank) + 1;
    return true;
  }
  static uint32_t halo_dv(int s) { return s == VKRH_HALO_TAA ? 0u : 1u; }
  // the pass OUTPUT of each history surface (it becomes the history at the end-of-frame remap)
  vkr_img surface(int s) {
    const auto id = s == VKRH_HALO_TAA ? frame->taa_pass.get_output() : s == VKRH_HALO_AO ? frame->gtao.accumulated_ao : frame->ssr.get_blurred();
    return frame->graph.get_image(id)->describe(0, 1);
  }
  // pack (to_buffers) / unpack the halo rows of surface s: one vkr_copy_rects launch on the compute stream.  A refresh is
  // packed right after the pass that wrote the surface and unpacked in the NEXT frame (or in flush()), i.e. after
  // end_frame() has swapped output and history: by then the output id names the old history image, which the pass is
  // about to overwrite.  The rows belong into the very image they were packed from — now the history the pass reads —
  // so the descriptor is taken at pack time and kept for the unpack.
  vkr_img packed_from[3] {};
  void copy_halo(int s, bool to_buffers) {
    gpu::TraceRange range {to_buffers ? "halo pack" : "halo unpack"};
    if (to_buffers) packed_from[s] = surface(s);
    const vkr_img d = packed_from[s];
    const uint32_t dv = halo_dv(s), bpp = vkr_format_bytes(d.format), rows = cfg.halo >> dv, row_bytes = d.width * bpp;
    const uint32_t ty0 = (y0 >> dv) - uint32_t(d.origin_y), tth = th >> dv;  // the tile's first row inside the window image
    vkr_rect_copy rc[2];
    uint32_t n = 0;
    for (int nb = 0; nb < 2; nb++) {
      if (!neighbour(nb, nullptr)) continue;
      // send: my first / last `rows` tile rows (they lie in that neighbour's halo); receive: the rows just outside my tile
      const uint32_t send_row = nb == 0 ? ty0 : ty0 + tth - rows, recv_row = nb == 0 ? ty0 - rows : ty0 + tth;
      const uint64_t img = (uint64_t)(uintptr_t)d.base;
      if (to_buffers) rc[n++] = vkr_rect_copy {img + uint64_t(send_row) * d.pitch_bytes[0], (uint64_t)(uintptr_t)halo[s][nb].send, d.pitch_bytes[0], row_bytes, row_bytes, rows};
      else rc[n++] = vkr_rect_copy {(uint64_t)(uintptr_t)halo[s][nb].recv, img + uint64_t(recv_row) * d.pitch_bytes[0], row_bytes, d.pitch_bytes[0], row_bytes, rows};
    }
    if (n && vkr_copy_rects(rc, n, compute) != 0) throw std::runtime_error {std::string {"copy_rects: "} + vkr_last_error()};
  }
  uint32_t halo_peers(int s, vkr_halo_peer* out) {
    uint32_t n = 0;
    for (int nb = 0; nb < 2; nb++) {
      int peer;
      if (!neighbour(nb, &peer)) continue;
      out[n++] = vkr_halo_peer {peer, 0u, halo[s][nb].send, halo[s][nb].bytes, halo[s][nb].recv, halo[s][nb].bytes};
    }
    return n;
  }
  // A strip's rows of a whole-frame surface are contiguous in the window image AND in the frame image (same width, same
  // pitch), so every surface is gathered in place: send = the tile's rows where they lie, recv = the frame image.
  uint32_t gather_parts(int which, vkr_gather_part* out, bool next_set = false) {
    auto& offs = gather_offsets[which];
    offs.clear();
    auto part = [&](rendergraph::ImageResourceId src, uint32_t src_mip, rendergraph::ImageResourceId dst, uint32_t dst_mip, uint32_t dv) {
      const vkr_img s = frame->graph.get_image(src)->describe(src_mip, 1), d = frame->graph.get_image(dst)->describe(dst_mip, 1);
      const uint32_t rows = th >> dv;
      if (s.pitch_bytes[0] != d.pitch_bytes[0] || d.height != (H >> dv) || s.width != d.width || d.origin_y != 0)
        throw std::runtime_error {"tiled frame: window and whole-frame images must share width and row pitch"};
      const uint32_t ly = (y0 >> dv) - uint32_t(s.origin_y);
      std::vector<uint64_t> o(cfg.world + 1);
      for (uint32_t r = 0; r <= cfg.world; r++) o[r] = uint64_t(bounds[r] >> dv) * s.pitch_bytes[0];
      offs.push_back(std::move(o));
      return vkr_gather_part {(const uint8_t*)s.base + uint64_t(ly) * s.pitch_bytes[0], d.base, uint64_t(rows) * s.pitch_bytes[0]};
    };
    uint32_t n = 0;
    auto& g = frame->gbuffer;
    if (which == VKRH_GATHER_HIZ) {  // (next_set: what the pipelined frame has just downsampled for the frame after this one)
      for (uint32_t m = 1; m <= cfg.gathered_mips; m++) out[n++] = part(next_set ? g.depth_next : g.depth, m, g.frame_hiz, m - 1, m);
      if (!normals_by_request()) out[n++] = part(next_set ? g.downsampled_normals_next : g.downsampled_normals, 0, g.frame_normals, 0, 1);
    } else {
      out[n++] = part(g.albedo, 0, g.frame_albedo, 0, 0);
    }
    return n;
  }

  // ---- ordering between the compute and the exchange stream ----------------------------------------------------------
  void start(int slot, const std::function<int()>& issue) {
    if (!cfg.comm) return;  // harness mode: the caller moves the bytes between phases
    check(hipEventRecord(ev_ready[slot], compute), "event record");
    check(hipStreamWaitEvent(xchg, ev_ready[slot], 0), "stream wait");
    if (issue() != 0) throw std::runtime_error {std::string {"exchange: "} + vkr_last_error()};
    check(hipEventRecord(ev_done[slot], xchg), "event record");
  }
  // Exposed waiting (diagnostics, vkrh_tiled_wait_times): with wait timing on, an event pair on the compute stream brackets
  // every wait for an exchange — the second event cannot complete before the exchange has, so the pair measures how long
  // the compute stream actually stood still for it (0 when the bytes had already arrived).
  bool time_waits = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> wait_marks[5];
  void wait(int slot) {
    if (!cfg.comm) return;
    hipEvent_t before = nullptr, after = nullptr;
    if (time_waits) {
      check(hipEventCreate(&before), "event"); check(hipEventCreate(&after), "event");
      check(hipEventRecord(before, compute), "event record");
    }
    check(hipStreamWaitEvent(compute, ev_done[slot], 0), "stream wait");
    if (time_waits) {
      check(hipEventRecord(after, compute), "event record");
      wait_marks[slot].emplace_back(before, after);
    }
  }
  // total exposed wait per exchange since the last call, ms: [hiz, albedo, taa halo, ao halo, ssr halo]; synchronises
  void collect_waits(float out[5]) {
    check(hipStreamSynchronize(compute), "synchronize");
    for (int s = 0; s < 5; s++) {
      out[s] = 0.0f;
      for (auto& m : wait_marks[s]) {
        float ms = 0.0f;
        check(hipEventElapsedTime(&ms, m.first, m.second), "event elapsed");
        out[s] += ms;
        (void)hipEventDestroy(m.first); (void)hipEventDestroy(m.second);
      }
      wait_marks[s].clear();
    }
  }
  void start_gather(int which, bool next_set = false) {
    gpu::TraceRange range {which == VKRH_GATHER_HIZ ? "all-gather Hi-Z" : "all-gather albedo"};
    start(which, [&] {
      vkr_gather_part p[8];
      const uint32_t n = gather_parts(which, p, next_set);
      if (uniform) return vkr_all_gather(cfg.comm, p, n, xchg);
      vkr_gather_v_part v[8];  // strips of different heights: every share at its own offset of the frame image
      for (uint32_t i = 0; i < n; i++) v[i] = vkr_gather_v_part {p[i].send, p[i].recv, gather_offsets[which][i].data()};
      return vkr_all_gather_v(cfg.comm, v, n, xchg);
    });
  }
  void start_halo(int s) {
    gpu::TraceRange range {"halo exchange"};
    halo_in_flight[s] = true;
    start(2 + s, [&] { vkr_halo_peer p[2]; const uint32_t n = halo_peers(s, p); return vkr_halo_exchange(cfg.comm, p, n, xchg); });
  }
  void finish_halo(int s) {  // the refresh of surface s started in the previous frame: wait for it, then scatter it into the ring
    if (!halo_in_flight[s]) return;
    wait(2 + s);
    copy_halo(s, false);
    halo_in_flight[s] = false;
  }

  // ---- hit colours by request / reply (frame.hpp; csrc/hit_exchange.hip) ------------------------------------------------
  struct HitState {
    // device, every part 64-byte aligned (RCCL moves the counts): counts @0, reply errors @HIT_ERRORS,
    // the gathered world x world matrix @HIT_MATRIX
    uint32_t* counts = nullptr;
    uint32_t* workspace = nullptr;  // VKR_HIT_WORKSPACE_WORDS: what pass 1 of vkr_hit_requests leaves for pass 2
    uint32_t* host_counts = nullptr;  // pinned: world * world + 1
    vkr_hit_request* req_out = nullptr; uint8_t* reply_in = nullptr; uint64_t cap_out = 0;   // what I ask / get back
    vkr_hit_request* req_in = nullptr; uint8_t* reply_out = nullptr; uint64_t cap_in = 0;    // what I am asked / answer
    std::vector<uint32_t> out_seg, in_seg;  // [world + 1]: my requests for owner o / the requests of rank r for me, as runs
    uint64_t wire_bytes = 0;
    bool counted = false;
    // Native wire without a host round trip: the room of every rank-to-owner segment THIS frame, derived on every rank from
    // LAST frame's world x world counts (identical everywhere: the counts are all-gathered).  With it the whole round — requests,
    // both exchanges, replies, scatter — is enqueued behind the trace at once; the host only looks at this frame's counts
    // afterwards (phase 4) and repeats the round exactly if a segment was too small.  Empty: no previous frame yet.
    std::vector<uint32_t> cap_matrix;
    std::vector<uint32_t> caps_out;     // [world]: row `rank` of cap_matrix (what vkr_hit_requests_bounded takes)
    hipEvent_t ev_counts = nullptr;     // this frame's counts (and last frame's reply errors) have reached host_counts
    bool speculative = false;           // this frame's round went out on capacities
    uint32_t cap_percent = 125;         // room = this share of last frame's count (+ 64, rounded up to 64); VKR_HIT_CAP_PERCENT
    uint64_t rounds_speculative = 0, rounds_exact = 0, rounds_repeated = 0;
  } hit;
  // The trace in two stages around the gather (needs the pending-ray images of the request / reply mode): VKR_TILED_LOCAL_FIRST=1.
  // OFF by default: measured on a 15360 x 1080 strip of config 4 (tools/trace_local_probe.py) the head parks 70 - 76 % of the
  // rays — a march climbs past the gathered levels after four skipped tiles — so the resume launch repeats most of the work
  // through 80-byte records: head 0.42 + resume 0.67 ms against 0.70 ms for the one launch, more than the 0.16 - 0.28 ms of
  // exposed gather it can hide.
  bool local_first() const { return normals_by_request() && local_first_enabled; }
  bool local_first_enabled = getenv("VKR_TILED_LOCAL_FIRST") != nullptr && std::string {getenv("VKR_TILED_LOCAL_FIRST")} == "1";
  bool by_request() const { return tiled && cfg.world > 1 && cfg.albedo_by_gather != 1; }          // hit colours
  bool normals_by_request() const { return tiled && cfg.world > 1 && cfg.albedo_by_gather == 0; }   // ... and hit normals
  vkr_img dn_img() { return frame->graph.get_image(frame->gbuffer.downsampled_normals)->describe(0, 1); }
  vkr_img frame_normals_img() { return frame->graph.get_image(frame->gbuffer.frame_normals)->describe(0, 1); }
  vkr_img pend_mask_img() { return frame->graph.get_image(frame->gbuffer.pend_mask)->describe_store(0, 1); }
  vkr_img pend_data_img() { return frame->graph.get_image(frame->gbuffer.pend_data)->describe_store(0, 1); }
  // what vkr_hit_requests walks: the rays for the albedo rows, the pending rays of the windowed trace for the normal rows
  struct HitSources { vkr_img rays, mask, data; vkr_hit_sources src; };
  void hit_sources(HitSources& h) {
    h.rays = rays_img();
    h.src = vkr_hit_sources {&h.rays, W, H, wy0, wy0 + wh, nullptr, nullptr, 0, 0, 0, 0};
    if (normals_by_request()) {
      h.mask = pend_mask_img(); h.data = pend_data_img();
      h.src.pending_mask = &h.mask; h.src.pending_data = &h.data;
      h.src.normal_width = W / 2; h.src.normal_height = H / 2; h.src.normal_row0 = wy0 / 2; h.src.normal_row1 = (wy0 + wh) / 2;
    }
  }
  vkr_img rays_img() { return frame->graph.get_image(frame->ssr.get_rays())->describe_store(0, 1); }
  vkr_img albedo_img() { return frame->graph.get_image(frame->gbuffer.albedo)->describe(0, 1); }
  vkr_img frame_albedo_img() { return frame->graph.get_image(frame->gbuffer.frame_albedo)->describe(0, 1); }
  void hit_init() {
    const uint32_t w = cfg.world;
    if (w > 16) throw std::runtime_error {"tiled frame: the request / reply exchange is laid out for at most 16 ranks"};
    hit.counts = (uint32_t*)gpu::device_alloc(sizeof(uint32_t) * HIT_WORDS);
    check(hipMemset(hit.counts, 0, sizeof(uint32_t) * HIT_WORDS), "memset");  // (the error word is read before the first count clears it)
    hit.workspace = (uint32_t*)gpu::device_alloc(sizeof(uint32_t) * VKR_HIT_WORKSPACE_WORDS);
    check(hipHostMalloc((void**)&hit.host_counts, sizeof(uint32_t) * (w * w + 4), hipHostMallocDefault), "pinned counts");
    hit.out_seg.assign(w + 1, 0); hit.in_seg.assign(w + 1, 0);
    // room for what this rank can ask for — every ray of its window ending on another strip — and the same for what it
    // may be asked (anything beyond grows, see grow())
    // (the worst case — every ray of the window ending on another strip, (4 + 16) B x 2 directions x 2 surfaces — was
    // 370 MB per rank at c4 for an exchange that moves 10 - 30 MB; a quarter of the rays is still 4x what the frames ask, and grow() covers the rest)
    const uint64_t worst = ((normals_by_request() ? 2ull : 1ull) * (W / 2) * (wh / 2)) / 4 + 4096;
    uint64_t cap = 0;
    grow((void**)&hit.req_out, &cap, worst, sizeof(vkr_hit_request));
    grow((void**)&hit.reply_in, &hit.cap_out, worst, VKR_HIT_REPLY_BYTES);
    cap = 0;
    grow((void**)&hit.req_in, &cap, worst, sizeof(vkr_hit_request));
    grow((void**)&hit.reply_out, &hit.cap_in, worst, VKR_HIT_REPLY_BYTES);
    grew = false;  // before the first frame: the caller synchronises after set-up (prepare), nothing is in flight
    check(hipEventCreateWithFlags(&hit.ev_counts, hipEventDisableTiming), "event");
    if (const char* e = getenv("VKR_HIT_CAP_PERCENT")) hit.cap_percent = (uint32_t)std::max(1, atoi(e));
  }
  void hit_release() {
    gpu::device_free(hit.counts);
    gpu::device_free(hit.workspace);
    if (hit.host_counts) (void)hipHostFree(hit.host_counts);
    if (hit.ev_counts) (void)hipEventDestroy(hit.ev_counts);
    gpu::device_free(hit.req_out); gpu::device_free(hit.reply_in); gpu::device_free(hit.req_in); gpu::device_free(hit.reply_out);
  }
  // own rows of the whole-frame albedo: the window's rows are copied where the all-gather would have put the tile's
  void hit_local_rows(hipStream_t s) {
    const vkr_img a = albedo_img(), f = frame_albedo_img();
    if (a.pitch_bytes[0] != f.pitch_bytes[0] || a.width != f.width) throw std::runtime_error {"tiled frame: window and whole-frame albedo must share width and row pitch"};
    check(hipMemcpyAsync((uint8_t*)f.base + uint64_t(a.origin_y) * f.pitch_bytes[0], a.base, uint64_t(a.height) * a.pitch_bytes[0], hipMemcpyDeviceToDevice, s), "albedo rows");
    if (normals_by_request()) {
      const vkr_img n = dn_img(), fn = frame_normals_img();
      if (n.pitch_bytes[0] != fn.pitch_bytes[0] || n.width != fn.width) throw std::runtime_error {"tiled frame: window and whole-frame normals must share width and row pitch"};
      check(hipMemcpyAsync((uint8_t*)fn.base + uint64_t(n.origin_y) * fn.pitch_bytes[0], n.base, uint64_t(n.height) * n.pitch_bytes[0], hipMemcpyDeviceToDevice, s), "normal rows");
    }
  }
  // pass 1, behind the trace on stream s (the harness: the compute stream; with a communicator: the exchange stream, so that
  // GTAO starts right after the trace and the count runs beside it)
  void hit_count(hipStream_t s) {
    const uint32_t w = cfg.world;
    check(hipMemsetAsync(hit.counts, 0, sizeof(uint32_t) * HIT_MATRIX, s), "memset");
    HitSources h;
    hit_sources(h);
    if (vkr_hit_requests(&h.src, bounds.data(), w, hit.counts, hit.workspace, nullptr, nullptr, s) != 0)
      throw std::runtime_error {std::string {"hit_requests: "} + vkr_last_error()};
    hit.counted = true;
  }
  // An allocator may initialise what it hands out asynchronously on the COMPUTE stream (the torch-backed one zero-fills
  // there).  Buffers the exchange stream writes are therefore allocated before the first frame, for the worst case of
  // this rank's own requests; should a rank ever be asked for more than that, the exchange stream is ordered behind the
  // compute stream once, so that a late fill cannot wipe what the exchange has already landed (found by the 4-process
  // wire test under load: replies zeroed in the frame that allocated them).
  bool grew = false;
  void grow(void** p, uint64_t* cap, uint64_t need, uint64_t elem) {
    if (need <= *cap) return;
    // a round that went out on capacities may still be in flight on the exchange stream (the host no longer waits for it): what
    // it reads and writes must not go back to the allocator under it.  Rare: a buffer grows by a quarter more than it needs.
    if (*p && xchg) check(hipStreamSynchronize(xchg), "synchronize");
    gpu::device_free(*p);
    *cap = need + need / 4 + 1024;
    *p = gpu::device_alloc(*cap * elem);
    grew = true;
  }
  void order_exchange_behind_allocations(hipStream_t s) {
    if (!grew || s == compute) { grew = false; return; }
    grew = false;
    check(hipEventRecord(ev_ready[VKRH_GATHER_ALBEDO], compute), "event record");
    check(hipStreamWaitEvent(s, ev_ready[VKRH_GATHER_ALBEDO], 0), "stream wait");
  }
  // pass 2 on stream s, given everybody's counts — or, bounded, everybody's segment capacities: fills req_out and returns the
  // peer list of the request exchange
  uint32_t hit_write(const uint32_t* matrix, hipStream_t s, vkr_halo_peer* peers, bool bounded = false) {
    const uint32_t w = cfg.world, me = cfg.rank;
    for (uint32_t o = 0; o < w; o++) hit.out_seg[o + 1] = hit.out_seg[o] + matrix[me * w + o];
    for (uint32_t r = 0; r < w; r++) hit.in_seg[r + 1] = hit.in_seg[r] + matrix[r * w + me];
    if (matrix[me * w + me]) throw std::runtime_error {"tiled frame: a rank requested hit colours from itself"};
    uint64_t cap = hit.cap_out;
    grow((void**)&hit.req_out, &cap, hit.out_seg[w], sizeof(vkr_hit_request));
    grow((void**)&hit.reply_in, &hit.cap_out, hit.out_seg[w], VKR_HIT_REPLY_BYTES);
    cap = hit.cap_in;
    grow((void**)&hit.req_in, &cap, hit.in_seg[w], sizeof(vkr_hit_request));
    grow((void**)&hit.reply_out, &hit.cap_in, hit.in_seg[w], VKR_HIT_REPLY_BYTES);
    order_exchange_behind_allocations(s);
    if (hit.out_seg[w]) {
      HitSources h;
      hit_sources(h);
      int rc;
      // Every slot starts as "no request".  Bounded segments have unused room by construction; an exact round that REPEATS a
      // bounded one may write fewer requests than it counted, because the deferred normal test of the first round has
      // meanwhile turned some provisional hits into misses (their albedo texels are no longer asked for).
      check(hipMemsetAsync(hit.req_out, 0xFF, uint64_t(hit.out_seg[w]) * sizeof(vkr_hit_request), s), "memset");
      if (bounded) {
        hit.caps_out.assign(matrix + me * w, matrix + me * w + w);
        rc = vkr_hit_requests_bounded(&h.src, bounds.data(), w, hit.workspace, hit.out_seg.data(), hit.caps_out.data(), hit.req_out, hit.counts + HIT_DROPPED, s);
      } else {
        rc = vkr_hit_requests(&h.src, bounds.data(), w, hit.counts, hit.workspace, hit.out_seg.data(), hit.req_out, s);
      }
      if (rc != 0) throw std::runtime_error {std::string {"hit_requests: "} + vkr_last_error()};
    }
    uint32_t n = 0;
    hit.wire_bytes = 0;
    for (uint32_t p = 0; p < w; p++) {
      const uint64_t so = hit.out_seg[p + 1] - hit.out_seg[p], ri = hit.in_seg[p + 1] - hit.in_seg[p];
      if (p == me || (so == 0 && ri == 0)) continue;
      peers[n++] = vkr_halo_peer {int32_t(p), 0u, hit.req_out + hit.out_seg[p], so * sizeof(vkr_hit_request), hit.req_in + hit.in_seg[p], ri * sizeof(vkr_hit_request)};
      hit.wire_bytes += ri * sizeof(vkr_hit_request) + so * VKR_HIT_REPLY_BYTES;  // requests in now, replies to my requests later
    }
    return n;
  }
  // answers on stream s; returns the peer list of the way back
  uint32_t hit_reply(hipStream_t s, vkr_halo_peer* peers) {
    const uint32_t w = cfg.world, me = cfg.rank;
    const vkr_img a = albedo_img(), dn = dn_img();
    if (vkr_hit_reply(&a, normals_by_request() ? &dn : nullptr, hit.req_in, hit.in_seg[w], hit.reply_out, hit.counts + HIT_ERRORS, s) != 0)
      throw std::runtime_error {std::string {"hit_reply: "} + vkr_last_error()};
    uint32_t n = 0;
    for (uint32_t p = 0; p < w; p++) {
      const uint64_t so = hit.in_seg[p + 1] - hit.in_seg[p], ri = hit.out_seg[p + 1] - hit.out_seg[p];
      if (p == me || (so == 0 && ri == 0)) continue;
      peers[n++] = vkr_halo_peer {int32_t(p), 0u, hit.reply_out + uint64_t(hit.in_seg[p]) * VKR_HIT_REPLY_BYTES, so * VKR_HIT_REPLY_BYTES,
                                  hit.reply_in + uint64_t(hit.out_seg[p]) * VKR_HIT_REPLY_BYTES, ri * VKR_HIT_REPLY_BYTES};
    }
    return n;
  }
  void hit_scatter(hipStream_t s, bool bounded = false) {
    const vkr_img f = frame_albedo_img(), fn = frame_normals_img();
    if (vkr_hit_scatter(&f, normals_by_request() ? &fn : nullptr, hit.req_out, hit.reply_in, hit.out_seg[cfg.world], s) != 0)
      throw std::runtime_error {std::string {"hit_scatter: "} + vkr_last_error()};
    if (normals_by_request()) {  // the hit-normal test the windowed trace deferred: the footprints are complete now
      const vkr_img r = rays_img(), m = pend_mask_img(), d = pend_data_img();
      const vkr_trace_params tp = frame->trace_params();
      // (a bounded round that dropped requests of THIS rank has not brought every hit normal: the test waits for the exact round)
      if (vkr_sssr_validate_unless(&r, &m, &d, &fn, &tp, bounded ? hit.counts + HIT_DROPPED : nullptr, s) != 0) throw std::runtime_error {std::string {"sssr_validate: "} + vkr_last_error()};
    }
    hit.counted = false;
  }
  // The native exchange.  Behind the trace, on the exchange stream: count, all-gather of the counts, their copy to the host
  // (with the reply errors of the previous frame) and an event.  With capacities from the previous frame the whole round
  // follows at once (hit_round: requests into fixed-room segments, the two point-to-point exchanges at those sizes, replies,
  // scatter, the deferred normal test) and ends in ev_done[VKRH_GATHER_ALBEDO], which the filter waits for: no host round trip
  // between the trace and the filter.  hit_exchange_complete() is where the host looks at the counts: in the first frame it
  // is the round trip (called with GTAO queued, before anything else goes on the exchange stream: ADVICE r03 — the old
  // whole-stream synchronise also waited for GTAO and its halo exchange); later it only checks that no segment overflowed
  // and otherwise repeats the round exactly (every rank sees the same matrix and takes the same branch).
  void hit_exchange_native() {
    const uint32_t w = cfg.world;
    check(hipEventRecord(ev_ready[VKRH_GATHER_ALBEDO], compute), "event record");  // the trace (and its pending images) are complete
    check(hipStreamWaitEvent(xchg, ev_ready[VKRH_GATHER_ALBEDO], 0), "stream wait");
    // the error word of the previous frame's replies, before the memset of hit_count() clears it
    check(hipMemcpyAsync(hit.host_counts + w * w, hit.counts + HIT_ERRORS, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, xchg), "errors to host");
    hit_count(xchg);
    const vkr_gather_part part {hit.counts, hit.counts + HIT_MATRIX, uint64_t(w) * sizeof(uint32_t)};
    if (vkr_all_gather(cfg.comm, &part, 1, xchg) != 0) throw std::runtime_error {std::string {"exchange: "} + vkr_last_error()};
    check(hipMemcpyAsync(hit.host_counts, hit.counts + HIT_MATRIX, sizeof(uint32_t) * w * w, hipMemcpyDeviceToHost, xchg), "counts to host");
    check(hipEventRecord(hit.ev_counts, xchg), "event record");
    hit_pending = true;
    hit.speculative = !hit.cap_matrix.empty();
    if (hit.speculative) { hit_round(hit.cap_matrix.data(), true); hit.rounds_speculative++; }
  }
  // requests -> exchange -> replies -> exchange -> scatter (+ deferred normal test), all on the exchange stream
  void hit_round(const uint32_t* matrix, bool bounded) {
    vkr_halo_peer peers[HIT_PEERS];
    uint32_t n = hit_write(matrix, xchg, peers, bounded);
    if (vkr_halo_exchange(cfg.comm, peers, n, xchg) != 0) throw std::runtime_error {std::string {"exchange: "} + vkr_last_error()};
    n = hit_reply(xchg, peers);
    if (vkr_halo_exchange(cfg.comm, peers, n, xchg) != 0) throw std::runtime_error {std::string {"exchange: "} + vkr_last_error()};
    hit_scatter(xchg, bounded);
    check(hipEventRecord(ev_done[VKRH_GATHER_ALBEDO], xchg), "event record");
  }
  bool hit_pending = false;
  void hit_exchange_complete() {  // host-blocking on the counts only
    if (!hit_pending) return;
    gpu::TraceRange range {hit.speculative ? "hit colours: check the counts" : "hit colours: counts -> requests -> replies -> scatter"};
    hit_pending = false;
    const uint32_t w = cfg.world;
    check(hipEventSynchronize(hit.ev_counts), "event synchronize");
    if (hit.host_counts[w * w] != 0)
      throw std::runtime_error {"tiled frame: " + std::to_string(hit.host_counts[w * w]) + " hit-colour requests of the previous frame named texels their owner does not hold (the ranks' strips disagree); one of them: request " +
                                std::to_string(hit.host_counts[w * w + 1]) + " in slot " + std::to_string(hit.host_counts[w * w + 2]) + " of " + std::to_string(hit.in_seg[w])};
    bool overflow = false;
    for (uint32_t i = 0; hit.speculative && i < w * w; i++) overflow = overflow || hit.host_counts[i] > hit.cap_matrix[i];
    if (!hit.speculative || overflow) {
      hit_round(hit.host_counts, false);
      (overflow ? hit.rounds_repeated : hit.rounds_exact)++;
    }
    hit.cap_matrix.resize(w * w);
    hit_capacities(hit.host_counts, w, hit.cap_percent, hit.cap_matrix.data());
    hit.speculative = false;
  }
  // room for the next frame: last count + a quarter, in steps of 64; neighbours always keep a segment, a pair that asked for
  // nothing and is not adjacent keeps none (if it ever asks, that frame repeats its round)
  static void hit_capacities(const uint32_t* counts, uint32_t w, uint32_t percent, uint32_t* caps) {
    for (uint32_t r = 0; r < w; r++)
      for (uint32_t o = 0; o < w; o++) {
        const uint32_t c = counts[r * w + o];
        const bool adjacent = r + 1 == o || o + 1 == r;
        caps[r * w + o] = (r == o || (c == 0 && !adjacent)) ? 0u : uint32_t((uint64_t(c) * percent / 100 + 63) / 64 * 64 + 64);
      }
  }
  // Measurement (tools/wire_emulation.py): a frame that has so far been driven phase by phase by the in-process harness —
  // which left in its receive buffers exactly what real peers send, in segments laid out by hit_capacities(counts) — goes on
  // natively (vkrh_tiled_step) on `comm`, an emulated communicator (vkr_comm_create_emulated): the exchanges take their
  // time on the exchange stream and deliver what is already there.  `counts` is the world x world matrix of that last frame.
  void emulate_wire(void* comm, const uint32_t* counts) {
    if (!tiled || cfg.world < 2 || !comm) throw std::runtime_error {"vkrh_tiled_emulate_wire: needs a harness-driven frame of several ranks and a communicator"};
    check(hipStreamSynchronize(compute), "synchronize");
    if (xchg) check(hipStreamSynchronize(xchg), "synchronize");
    const bool again = cfg.comm != nullptr;  // a second call only swaps the communicator (another link rate): the frame's state stays
    cfg.comm = (vkr_comm*)comm;
    if (again) { flush(); check(hipStreamSynchronize(compute), "synchronize"); return; }
    if (by_request()) {
      if (!counts) throw std::runtime_error {"vkrh_tiled_emulate_wire: the counts of the last frame are needed (hit colours by request)"};
      const uint32_t w = cfg.world;
      check(hipMemcpy(hit.counts + HIT_MATRIX, counts, sizeof(uint32_t) * w * w, hipMemcpyHostToDevice), "counts");
      hit.cap_matrix.resize(w * w);
      hit_capacities(counts, w, hit.cap_percent, hit.cap_matrix.data());
      hit.speculative = false; hit_pending = false; hit.counted = false;
    }
  }
  static constexpr uint32_t HIT_PEERS = 16;
  static constexpr uint32_t HIT_ERRORS = 32, HIT_DROPPED = 40, HIT_MATRIX = 64, HIT_WORDS = 64 + 256;  // world <= 16; [0, HIT_MATRIX) is cleared by every count

  // ---- the frame, in phases (an exchange may only start / must be complete at a phase boundary) ------------------------
  void phase(uint32_t p) {
    if (!tiled) throw std::runtime_error {"vkrh_tiled_phase: this frame is not tiled (one rank without force_tiled has no phases: use vkrh_tiled_step)"};
    PostFxFrame& f = *frame;
    static const char* const names[VKRH_TILED_PHASES_SHADED] = {"tiled: downsample | start gathers", "tiled: TAA | halo", "tiled: Hi-Z tail + trace",
                                                               "tiled: GTAO | halo | hit colours", "tiled: SSR filter + blur | halo", "tiled: halos | shading + TAA | halo"};
    gpu::TraceRange range {p < VKRH_TILED_PHASES_SHADED ? names[p] : "tiled: ?"};
    switch (p) {
      case 0:
        f.run(VKRH_STAGE_DOWNSAMPLE);
        start_gather(VKRH_GATHER_HIZ);
        if (!by_request()) start_gather(VKRH_GATHER_ALBEDO);
        else hit_local_rows(compute);
        break;
      case 1:
        if (local_first()) {
          // local rows first: prologue, pinned steps and as much of every march as this rank's own pyramid rows allow run while
          // the depth all-gather is still on the wire; a ray that needs more is parked (csrc/ssr.hip, k_sssr_trace<.., LOCAL>).
          // The TAA, which used to be what ran ahead of the gather, moves behind GTAO: there it covers the hit-colour round.
          f.run(VKRH_STAGE_SSR_TRACE_HEAD);
          break;
        }
        if (!shading) taa_and_halo();  // shaded: the TAA resolves color_out, at the end of the frame (phase 5)
        break;
      case 2:
        wait(VKRH_GATHER_HIZ);
        f.run(VKRH_STAGE_HIZ_TAIL | (local_first() ? VKRH_STAGE_SSR_TRACE_RESUME : VKRH_STAGE_SSR_TRACE));
        if (by_request()) {
          if (cfg.comm) hit_exchange_native();  // count -> all-gather of the counts -> host copy, all on the exchange stream
          else hit_count(compute);
        }
        break;
      case 3:  // GTAO needs the trace's (occlusion, pdf) but not the albedo: it runs ahead of the reference's order to hide the second gather
        finish_halo(VKRH_HALO_AO);
        f.run(VKRH_STAGE_GTAO);
        // first frame (no capacities yet): the host waits for the counts here — GTAO is queued on the device, nothing else yet on the exchange stream
        if (by_request() && cfg.comm && !hit.speculative) hit_exchange_complete();
        copy_halo(VKRH_HALO_AO, true);
        start_halo(VKRH_HALO_AO);
        if (local_first() && !shading) taa_and_halo();
        break;
      case 4:
        if (by_request() && !cfg.comm && hit.counted) throw std::runtime_error {"vkrh_tiled_phase: the harness must complete the hit-colour exchange before phase 4"};
        if (by_request() && cfg.comm) hit_exchange_complete();  // the round went out on capacities: the counts arrived long ago, look at them
        wait(VKRH_GATHER_ALBEDO);
        finish_halo(VKRH_HALO_SSR);
        f.run(VKRH_STAGE_SSR_RESOLVE);
        copy_halo(VKRH_HALO_SSR, true);
        start_halo(VKRH_HALO_SSR);
        if (!shading) f.end_frame(false);
        break;
      case 5:
        if (!shading) throw std::runtime_error {"vkrh_tiled_phase: phases are 0..4"};
        shaded_tail();
        break;
      default: throw std::runtime_error {shading ? "vkrh_tiled_phase: phases are 0..5" : "vkrh_tiled_phase: phases are 0..4"};
    }
  }
  void taa_and_halo() {
    finish_halo(VKRH_HALO_TAA);
    frame->run(VKRH_STAGE_TAA);
    copy_halo(VKRH_HALO_TAA, true);
    start_halo(VKRH_HALO_TAA);
  }
  // Two frames in flight.  The depth pyramid is the one surface every rank needs whole, its all-gather the longest exchange of
  // the frame, and in the plain order only the TAA runs between the downsample that produces it and the trace that needs it.
  // Here the downsample of frame f + 1 (into the G-buffer's second set) and its all-gather start right after the trace of
  // frame f — the last reader of the whole-frame pyramid — and travel while GTAO, TAA, resolve and blur of frame f run; the TAA
  // moves behind GTAO, where it covers the hit-colour round.  Every step still runs every pass once.  Needs the next frame's
  // G-buffer to be resident when this frame's trace has run (the benchmark's is static; a renderer double-buffers it).
  void pipelined_step() {
    PostFxFrame& f = *frame;
    if (!primed) {  // the first frame's own downsample and gather
      f.run(VKRH_STAGE_DOWNSAMPLE_NEXT);
      start_gather(VKRH_GATHER_HIZ, true);
      f.gbuffer.swap_sets(f.graph);
      hit_local_rows(compute);
      primed = true;
    }
    wait(VKRH_GATHER_HIZ);
    f.run(VKRH_STAGE_HIZ_TAIL | VKRH_STAGE_SSR_TRACE);
    hit_exchange_native();
    f.run(VKRH_STAGE_DOWNSAMPLE_NEXT);          // frame f + 1
    start_gather(VKRH_GATHER_HIZ, true);
    finish_halo(VKRH_HALO_AO);
    f.run(VKRH_STAGE_GTAO);
    if (!hit.speculative) hit_exchange_complete();  // first frame: the host round trip, with GTAO queued
    copy_halo(VKRH_HALO_AO, true);
    start_halo(VKRH_HALO_AO);
    if (!shading) taa_and_halo();
    hit_exchange_complete();
    wait(VKRH_GATHER_ALBEDO);
    finish_halo(VKRH_HALO_SSR);
    f.run(VKRH_STAGE_SSR_RESOLVE);
    copy_halo(VKRH_HALO_SSR, true);
    start_halo(VKRH_HALO_SSR);
    if (shading) shaded_tail();
    else f.end_frame(false);
    f.gbuffer.swap_sets(f.graph);               // what was downsampled for frame f + 1 becomes the current set
    hit_local_rows(compute);                    // its own rows of the whole-frame albedo / normals (after this frame's resolve has read them)
  }
  void step() {
    if (!tiled) { frame->run(VKRH_STAGE_CHAIN | (shading ? VKRH_STAGE_SHADING : 0u)); frame->end_frame(false); return; }
    if (!cfg.comm && cfg.world > 1) throw std::runtime_error {"vkrh_tiled_step: no communicator (drive vkrh_tiled_phase from a harness instead)"};
    if (pipeline_enabled && cfg.comm) { pipelined_step(); return; }
    const uint32_t phases = shading ? VKRH_TILED_PHASES_SHADED : VKRH_TILED_PHASES;
    if (!cfg.comm) {  // one rank, no wire: the gathers degenerate to copies of the tile into the frame images
      for (uint32_t p = 0; p < phases; p++) {
        if (p == 2) local_gather(VKRH_GATHER_HIZ);
        if (p == 4) local_gather(VKRH_GATHER_ALBEDO);
        phase(p);
      }
      return;
    }
    for (uint32_t p = 0; p < phases; p++) phase(p);
  }
  void local_gather(int which) {
    vkr_gather_part p[8];
    const uint32_t n = gather_parts(which, p);
    for (uint32_t i = 0; i < n; i++)
      check(hipMemcpyAsync((uint8_t*)p[i].recv + gather_offsets[which][i][cfg.rank], p[i].send, p[i].bytes, hipMemcpyDeviceToDevice, compute), "local gather");
  }
  void flush() { for (int s = 0; s < 3; s++) finish_halo(s); }

  // ---- deferred shading (frame.hpp) --------------------------------------------------------------------------------------
  bool shading = false;
  void set_shading(bool on) {
    // a refresh packed under one order would be unpacked under the other: the TAA rows at the wrong end of the frame
    for (int s = 0; s < 3; s++)
      if (halo_in_flight[s]) throw std::runtime_error {"vkrh_tiled_set_shading: a halo refresh is in flight (before the first frame, or right after vkrh_tiled_flush)"};
    if (on && cfg.world > 1 && cfg.halo < VKRH_TILED_SHADING_MIN_HALO)
      throw std::runtime_error {"vkrh_tiled_set_shading: halo " + std::to_string(cfg.halo) + ", the shading of a strip's last rows reads 2 half-res rows of its neighbour (halo >= " +
                                std::to_string(VKRH_TILED_SHADING_MIN_HALO) + ")"};
    if (on && !frame->brdf_lut_ran) throw std::runtime_error {"vkrh_tiled_set_shading: VKRH_STAGE_BRDF_LUT has not run on this frame (the shading pass samples the LUT)"};
    shading = on;
    if (clipped) {
      if (on) store_rows(frame->color_out_tex, 0, 1);
      else frame->graph.get_image(frame->color_out_tex)->set_store_rows(0, 0);
    }
  }
  // The end of the shaded frame.  The AO and SSR refreshes started in THIS frame: awaited and unpacked here, into the images they
  // were packed from (copy_halo), their rows are the neighbours' current interiors — what the one-GPU shading reads there.  The
  // TAA refresh is last frame's.  One run() for both stages, so that the TAA resolves color_out.
  void shaded_tail() {
    finish_halo(VKRH_HALO_AO);
    finish_halo(VKRH_HALO_SSR);
    finish_halo(VKRH_HALO_TAA);
    frame->run(VKRH_STAGE_SHADING | VKRH_STAGE_TAA);
    copy_halo(VKRH_HALO_TAA, true);
    start_halo(VKRH_HALO_TAA);
    frame->end_frame(false);
  }
};

template <typename F> int guarded(F&& f) {
  try { f(); return 0; }
  catch (const std::exception& e) { g_error = e.what(); return 1; }
  catch (...) { g_error = "unknown exception"; return 2; }
}

// the frame behind a vkrh_* handle; a NULL handle is an error message, not a crash
PostFxFrame& frame_ref(void* frame) {
  if (!frame) throw std::runtime_error{"NULL frame"};
  return *(PostFxFrame*)frame;
}

// ---- what the selftests share: they write lines into `out` and hand them to the caller's buffer ----
void expect(std::string& out, const char* name, const std::function<void()>& f) {  // "case: no error" or "case: <what()>"
  try { f(); out += std::string{name} + ": no error\n"; }
  catch (const std::exception& e) { out += std::string{name} + ": " + e.what() + "\n"; }
}
// one line per task recorded since the last submit: "name: R<image>.<mip> ... W<image>.<mip> ...", the declared reads and writes
void dump_pending_tasks(const rendergraph::RenderGraph& graph, std::string& out) {
  for (const auto& t : graph.pending_tasks()) {
    out += t.name + ":";
    for (const auto& a : t.accesses) out += std::string{a.write ? " W" : " R"} + std::to_string(a.key >> 8) + "." + std::to_string(a.key & 0xFF);
    out += "\n";
  }
}
// a struct of 32-bit words as floats (%.9g) and the end of the line
template <typename T> void append_words(std::string& out, const T& value) {
  float words[sizeof(T) / 4];
  std::memcpy(words, &value, sizeof(T));
  for (float w : words) { char num[32]; std::snprintf(num, sizeof num, " %.9g", w); out += num; }
  out += "\n";
}
int copy_out(char* buf, uint32_t buf_size, const std::string& out) {
  if (buf && buf_size) std::snprintf(buf, buf_size, "%s", out.c_str());
  return 0;
}

}  // namespace

extern "C" {

void vkrh_set_allocator(vkrh_alloc_fn alloc, vkrh_free_fn free_fn, void* user) {
  gpu::set_device_allocator((gpu::AllocFn)alloc, (gpu::FreeFn)free_fn, user);
}

void* vkrh_create(const vkrh_config* cfg) {
  PostFxFrame* f = nullptr;
  int rc = guarded([&] {
    if (!cfg) throw std::runtime_error{"vkrh_create: NULL config"};
    if ((cfg->width | cfg->height | (uint32_t)cfg->origin_x | (uint32_t)cfg->origin_y) & 1u)
      throw std::runtime_error{"vkrh_create: window origin and extent must be even"};
    f = new PostFxFrame(*cfg);
  });
  return rc == 0 ? f : nullptr;
}
void vkrh_destroy(void* frame) { delete (PostFxFrame*)frame; }
const char* vkrh_last_error(void) { return g_error.c_str(); }
int vkrh_has_program(const char* name) {
  gpu::register_hot_path_programs();
  return name && gpu::has_program(name) ? 1 : 0;
}

int vkrh_set_camera(void* frame, const vkrh_camera* cam) {
  return guarded([&] { if (!frame || !cam) throw std::runtime_error{"NULL argument"}; frame_ref(frame).set_camera(*cam); });
}
int vkrh_pin_randoms(void* frame, float jitter, uint32_t gtao_frame_count, uint32_t ssr_counter) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    f->gtao.pin_angle_jitter(jitter);
    f->gtao.set_frame_count(gtao_frame_count);
    f->ssr.set_counter(ssr_counter);
  });
}
int vkrh_load_scene(void* frame, const vkr_raster_vertex* vertices, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                    const vkrh_scene_draw* draws, uint32_t draw_count, const vkrh_scene_texture* textures, uint32_t texture_count) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    if (!f || !vertices || !indices || (!draws && draw_count) || (!textures && texture_count)) throw std::runtime_error{"NULL argument"};
    std::vector<scene::FlatDraw> flat(draw_count);
    for (uint32_t i = 0; i < draw_count; i++) {
      std::memcpy(&flat[i].transform, draws[i].transform, 64);
      flat[i].vertex_offset = draws[i].vertex_offset; flat[i].index_offset = draws[i].index_offset; flat[i].index_count = draws[i].index_count;
      flat[i].albedo_tex_index = draws[i].albedo_tex_index; flat[i].metalic_roughness_index = draws[i].metalic_roughness_index;
      flat[i].clip_alpha = draws[i].clip_alpha != 0;
    }
    std::vector<scene::TextureData> tex(texture_count);
    for (uint32_t i = 0; i < texture_count; i++) {  // refused before anything is uploaded
      if (textures[i].flags & ~uint32_t(VKRH_TEXTURE_GEN_MIPS)) throw std::runtime_error{"vkrh_load_scene: unknown texture flag"};
      tex[i].gen_mips = (textures[i].flags & VKRH_TEXTURE_GEN_MIPS) != 0;
      if (tex[i].gen_mips && f->cfg.tiled) throw std::runtime_error{"vkrh_load_scene: VKRH_TEXTURE_GEN_MIPS on a tiled frame (texture mips are built on one GPU)"};
      if (tex[i].gen_mips && (textures[i].width == 0 || textures[i].height == 0 || !textures[i].levels[0])) throw std::runtime_error{"vkrh_load_scene: VKRH_TEXTURE_GEN_MIPS needs level 0"};
      if (!tex[i].gen_mips && (textures[i].mip_levels == 0 || textures[i].mip_levels > VKR_MAX_MIPS)) throw std::runtime_error{"vkrh_load_scene: bad mip count"};
      tex[i].width = textures[i].width; tex[i].height = textures[i].height; tex[i].mip_levels = tex[i].gen_mips ? 1u : textures[i].mip_levels;
      for (uint32_t m = 0; m < tex[i].mip_levels; m++) tex[i].levels[m] = textures[i].levels[m];
    }
    f->scene_renderer.reset();
    f->scene_as.reset();
    f->loaded_scene.reset(new scene::CompiledScene(scene::make_scene((const scene::Vertex*)vertices, vertex_count, indices, index_count,
                                                                     flat.data(), draw_count, tex.data(), texture_count, f->graph.get_stream())));
    f->scene_renderer.reset(new SceneRenderer(*f->loaded_scene));
    f->scene_renderer->init_pipeline(f->graph, f->gbuffer);  // main.cpp:256-259
    f->scene_renderer->update_scene();
    gpu::TransferCmdPool transfer_pool{f->graph.get_stream()};  // main.cpp:257-258
    f->scene_as.reset(new scene::SceneAccelerationStructure);
    f->scene_as->build(transfer_pool, *f->loaded_scene);
    f->shadow_accum_invalid = true;
  });
}
int vkrh_scene_texture_image(void* frame, uint32_t index, vkr_img* out) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    if (!out) throw std::runtime_error{"vkrh_scene_texture_image: NULL argument"};
    f->refuse_tiled("vkrh_scene_texture_image", "scene textures live on one GPU");
    if (!f->loaded_scene) throw std::runtime_error{"vkrh_scene_texture_image: without a loaded scene (vkrh_load_scene)"};
    if (index >= f->loaded_scene->images.size()) throw std::runtime_error{"vkrh_scene_texture_image: texture " + std::to_string(index) + " of " + std::to_string(f->loaded_scene->images.size())};
    const auto& img = f->loaded_scene->images[index];
    *out = img->describe(0, img->get_mip_levels());
  });
}
int vkrh_bake_probes(void* frame, const float min[3], const float max[3], uint32_t grid_size, uint32_t probe_size, uint32_t cube_size) {
  return guarded([&] { frame_ref(frame).bake_probes(min, max, grid_size, probe_size, cube_size); });
}
int vkrh_set_shadow_lights(void* frame, const float* mvps, uint32_t count, uint32_t size) {
  return guarded([&] { frame_ref(frame).set_shadow_lights(mvps, count, size); });
}
int vkrh_shadow_lights(void* frame, float* out, uint32_t* count) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    if (!out || !count) throw std::runtime_error{"vkrh_shadow_lights: NULL argument"};
    *count = (uint32_t)f->shadow_lights.size();
    std::memcpy(out, f->shadow_lights.data(), 64 * f->shadow_lights.size());
  });
}
int vkrh_set_shadow_mask(void* frame, uint32_t bias, uint32_t radius, uint32_t apply) { return guarded([&] { frame_ref(frame).set_shadow_mask(bias, radius, apply); }); }
int vkrh_set_shadow_mask_filter(void* frame, uint32_t reach, float normal_min_dot, float plane_tolerance) {
  return guarded([&] { frame_ref(frame).set_shadow_mask_filter(reach, normal_min_dot, plane_tolerance); });
}
int vkrh_set_shadow_mask_accumulate(void* frame, uint32_t max_count, float plane_tolerance, uint32_t pattern_frames) {
  return guarded([&] { frame_ref(frame).set_shadow_mask_accumulate(max_count, plane_tolerance, pattern_frames); });
}
int vkrh_set_ssao_samples(void* frame, const float* xyz, uint32_t std140) { return guarded([&] { frame_ref(frame).set_ssao_samples(xyz, std140); }); }
int vkrh_set_backbuffer(void* frame, const char* source_image, uint32_t flags, uint32_t width, uint32_t height) {
  return guarded([&] { frame_ref(frame).set_backbuffer(source_image, flags, width, height); });
}
int vkrh_set_shadow_rays(void* frame, const float* lights, uint32_t count, float normal_offset, float tmin) {
  return guarded([&] { frame_ref(frame).set_shadow_rays(lights, count, normal_offset, tmin); });
}
int vkrh_set_reflection_rays(void* frame, uint32_t fill_misses, float normal_offset, float tmin, float max_distance, uint32_t texture_lod) {
  return guarded([&] { frame_ref(frame).set_reflection_rays(fill_misses, normal_offset, tmin, max_distance, texture_lod); });
}
int vkrh_set_shadow_area_lights(void* frame, const float* radii, uint32_t count, uint32_t sample_count, uint32_t pattern_side) {
  return guarded([&] { frame_ref(frame).set_shadow_area_lights(radii, count, sample_count, pattern_side); });
}
int vkrh_set_reflection_lights(void* frame, uint32_t count, const float* lights, const float* colours, const float* ambient, float shadow_offset,
                               float shadow_tmin) {
  return guarded([&] { frame_ref(frame).set_reflection_lights(count, lights, colours, ambient, shadow_offset, shadow_tmin); });
}
int vkrh_scene_hit_normals(void* frame, vkr_hit_normal* out, uint32_t capacity, uint32_t* count) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    if (!count) throw std::runtime_error{"vkrh_scene_hit_normals: NULL argument"};
    if (!f->scene_as) throw std::runtime_error{"vkrh_scene_hit_normals: without a loaded scene (vkrh_load_scene)"};
    const std::vector<vkr_hit_normal> table = f->scene_as->download_hit_normals(f->graph.get_stream());
    *count = (uint32_t)table.size();
    if (!out) return;  // the size alone
    if (table.size() > capacity) throw std::runtime_error{"vkrh_scene_hit_normals: " + std::to_string(table.size()) + " records do not fit into " + std::to_string(capacity)};
    if (!table.empty()) std::memcpy(out, table.data(), sizeof(vkr_hit_normal) * table.size());
  });
}
int vkrh_set_ray_cutouts(void* frame, uint32_t enable, uint32_t alpha_lod) { return guarded([&] { frame_ref(frame).set_ray_cutouts(enable, alpha_lod); }); }
int vkrh_set_draw_transforms(void* frame, const float* transforms, uint32_t count) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    f->refuse_tiled("vkrh_set_draw_transforms", "the ray-traced stages run on one GPU");
    if (!f->loaded_scene || !f->scene_renderer || !f->scene_as) throw std::runtime_error{"vkrh_set_draw_transforms: without a loaded scene (vkrh_load_scene)"};
    auto& nodes = f->loaded_scene->base_nodes;  // one per draw of vkrh_load_scene, in its order (scene::make_scene)
    if (count != nodes.size())
      throw std::runtime_error{"vkrh_set_draw_transforms: " + std::to_string(count) + " transforms for the " + std::to_string(nodes.size()) + " draws of vkrh_load_scene"};
    if (!transforms && count) throw std::runtime_error{"vkrh_set_draw_transforms: NULL argument"};
    for (uint32_t i = 0; i < count; i++) std::memcpy((void*)&nodes[i].transform, transforms + 16 * size_t(i), 64);
    f->scene_renderer->update_scene();
    f->scene_as->refit(*f->loaded_scene, f->graph.get_stream());
    f->shadow_accum_invalid = true;
  });
}

int vkrh_gtao_rt_params(void* frame, vkr_gtao_rt_params* out) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    if (!f || !out) throw std::runtime_error{"NULL argument"};
    if (!f->has_camera) throw std::runtime_error{"vkrh_gtao_rt_params: camera not set"};
    const GTAORTParams p = f->gtao_rt_params();
    std::memcpy(out, &p, sizeof(*out));
  });
}
int vkrh_camera_matrices(void* frame, float* out48) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    if (!f || !out48) throw std::runtime_error{"NULL argument"};
    if (!f->has_camera) throw std::runtime_error{"vkrh_camera_matrices: camera not set"};
    // nothing is evaluated here that the frame does not hand on: the two products are set_camera's, stored in the block every
    // pass reads; the inverse is the one gtao_rt_params() gives the ray-traced stages
    const glm::mat4 held[3] = {f->draw_params.mvp, f->draw_params.prev_mvp, f->gtao_rt_params().camera_to_world};
    std::memcpy(out48, held, sizeof(held));
  });
}
int vkrh_gtao_directions(float* out, uint32_t count) {
  return guarded([&] {
    if (!out && count) throw std::runtime_error{"NULL argument"};
    const auto dirs = gtao_random_directions(count);
    std::memcpy(out, dirs.data(), sizeof(glm::vec4) * dirs.size());
  });
}
int vkrh_pin_screen_trace(void* frame, float angle_jitter, float random_offset, uint32_t frame_count) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    f->screen_trace.pin_randoms(angle_jitter, random_offset);
    f->screen_trace.set_frame_count(frame_count);
  });
}
int vkrh_set_gtao_mode(void* frame, uint32_t use_mis, uint32_t two_directions) {
  return guarded([&] { auto* f = &frame_ref(frame); f->gtao.set_mis(use_mis != 0); f->gtao.set_two_directions(two_directions != 0); });
}
int vkrh_set_synth_flags(void* frame, uint32_t flags) {
  return guarded([&] {
    if (!frame) throw std::runtime_error{"NULL argument"};
    if (flags & ~uint32_t(VKR_SYNTH_TEXTURED_ROUGHNESS)) throw std::runtime_error{"vkrh_set_synth_flags: unknown flag"};
    frame_ref(frame).synth.set_material_flags(flags);
  });
}
int vkrh_set_gathered_mips(void* frame, uint32_t mips) {
  return guarded([&] {
    if (mips < 1 || mips > 4) throw std::runtime_error{"vkrh_set_gathered_mips: 1..4"};
    frame_ref(frame).hiz_gathered_mips = mips;
  });
}
int vkrh_run(void* frame, uint32_t stage_mask) { return guarded([&] { frame_ref(frame).run(stage_mask); }); }
int vkrh_end_frame(void* frame, uint32_t swap_depth) { return guarded([&] { frame_ref(frame).end_frame(swap_depth != 0); }); }
int vkrh_image(void* frame, const char* name, uint32_t base_mip, uint32_t mip_count, vkr_img* out) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    if (!f || !name || !out) throw std::runtime_error{"NULL argument"};
    auto& img = f->graph.get_image(f->lookup(name));
    if (mip_count == 0) mip_count = img->get_mip_levels() - base_mip;
    *out = img->describe(base_mip, mip_count);
  });
}
int vkrh_read_buffer(void* frame, const char* name, void* dst, uint64_t capacity, uint64_t* bytes) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    if (!f || !name || !dst) throw std::runtime_error{"NULL argument"};
    const std::string n{name};
    rendergraph::BufferResourceId id;
    if (n == "reflective_tiles") id = f->ssr.get_reflective_tiles();
    else if (n == "glossy_tiles") id = f->ssr.get_glossy_tiles();
    else if (n == "reflective_indirect") id = f->ssr.get_reflective_indirect();
    else if (n == "glossy_indirect") id = f->ssr.get_glossy_indirect();
    else throw std::runtime_error{"vkrh_read_buffer: unknown buffer '" + n + "'"};
    auto& buf = f->graph.get_buffer(id);
    const uint64_t size = buf->get_size();
    if (bytes) *bytes = size;
    if (capacity < size) throw std::runtime_error{"vkrh_read_buffer: destination too small"};
    void* stream = f->graph.get_stream();
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy(dst, buf->device_ptr(stream), size, hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error{"vkrh_read_buffer: copy failed"};
  });
}
int vkrh_image_layer(void* frame, const char* name, uint32_t layer, vkr_img* out) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    if (!f || !name || !out) throw std::runtime_error{"NULL argument"};
    auto& img = f->graph.get_image(f->lookup(name));
    *out = img->describe_layer(layer, 0, img->get_mip_levels());
  });
}
int vkrh_capture(void* frame, const char* name, uint32_t mip, uint32_t kind, const char* path) {
  return guarded([&] {
    auto* f = &frame_ref(frame);
    if (!f || !name || !path) throw std::runtime_error{"NULL argument"};
    rendergraph::ImageResourceId source = f->lookup(name);
    if (kind == 3) {  // main.cpp:392-396: the final frame through an RGBA8_SRGB image
      if (f->cfg.tiled) throw std::runtime_error{"vkrh_capture: the final-frame capture on a tiled frame (transfers take whole images)"};
      if (mip != 0) throw std::runtime_error{"vkrh_capture: the final-frame capture blits mip 0"};
      const rendergraph::ImageResourceId dst = f->ensure_readback_image();
      if (source == dst) throw std::runtime_error{"vkrh_capture: 'readback' is the destination of the final-frame capture"};
      blit_image(f->graph, source, dst);
      source = dst;
    }
    const ReadBackID id = f->readback.read_image(f->graph, source, 0, mip, 0);
    // the request matures frames_count + 1 submits later, like the reference's fenced frames
    for (uint32_t i = 0; i <= f->graph.get_frames_count() + 1 && !f->readback.is_data_available(id); i++) {
      f->graph.submit();
      f->readback.after_submit(f->graph);
    }
    if (!f->readback.is_data_available(id)) throw std::runtime_error{"readback did not mature"};
    ReadBackData data = f->readback.get_data(id);
    bool ok = true;
    if (kind == 0) {
      if (data.texel_fmt != VK_FORMAT_D24_UNORM_S8_UINT) throw std::runtime_error{"depth CSV capture needs a D24S8 image"};
      write_depth_csv(data, path);
    } else if (kind == 1) {
      if (data.texel_size != 4) throw std::runtime_error{"depth PNG capture needs 4-byte texels"};
      ok = write_depth_png(data, path);
    } else if (kind == 2 || kind == 3) {
      if (data.texel_size != 4) throw std::runtime_error{"RGBA PNG capture needs 4-byte texels"};
      ok = write_rgba_png(data, path);
    } else {
      throw std::runtime_error{"unknown capture kind"};
    }
    if (!ok) throw std::runtime_error{std::string{"cannot write "} + path};
  });
}
int vkrh_selftest_writers(const char* dir, uint32_t width, uint32_t height) {
  return guarded([&] {
    if (!dir || !width || !height) throw std::runtime_error{"bad arguments"};
    auto make = [&](VkFormat fmt) {
      ReadBackData d;
      d.width = width; d.height = height; d.texel_fmt = fmt; d.texel_size = 4;
      d.bytes.reset(new uint8_t[size_t(width) * height * 4]);
      return d;
    };
    ReadBackData depth = make(VK_FORMAT_D24_UNORM_S8_UINT), color = make(VK_FORMAT_R8G8B8A8_SRGB);
    for (uint32_t y = 0; y < height; y++)
      for (uint32_t x = 0; x < width; x++) {
        const size_t i = size_t(y) * width + x;
        reinterpret_cast<uint32_t*>(depth.bytes.get())[i] = x * 65537u + y * 257u + 0xAB000000u;
        uint8_t* c = color.bytes.get() + 4 * i;
        c[0] = uint8_t(x); c[1] = uint8_t(y); c[2] = uint8_t(x ^ y); c[3] = 7;
      }
    const std::string base{dir};
    write_depth_csv(depth, base + "/depth.csv");
    if (!write_depth_png(depth, base + "/depth.png") || !write_rgba_png(color, base + "/color.png"))
      throw std::runtime_error{"cannot write PNG files under " + base};
  });
}
int vkrh_enable_task_timing(void* frame, uint32_t on) { return guarded([&] { frame_ref(frame).graph.enable_task_timing(on != 0); }); }
int vkrh_enable_task_timing_only(void* frame, const char* task) { return guarded([&] { frame_ref(frame).graph.enable_task_timing(true, task ? task : ""); }); }
const char* vkrh_collect_task_times(void* frame) {
  if (!frame) { g_error = "NULL frame"; return nullptr; }
  auto* f = (PostFxFrame*)frame;
  f->task_names.clear();
  int rc = guarded([&] {
    for (auto& t : f->graph.collect_task_times())
      f->task_names += t.name + " " + std::to_string(t.total_ms) + " " + std::to_string(t.launches) + "\n";
  });
  return rc == 0 ? f->task_names.c_str() : nullptr;
}
int vkrh_selftest_errors(char* buf, uint32_t buf_size) {
  std::string out;
  expect(out, "unknown_program", [] { gpu::create_compute_pipeline("no_such_program"); });
  expect(out, "known_program", [] { gpu::create_compute_pipeline("gtao_compute_main"); });
  const auto downsample = [](uint32_t depth_mips, uint32_t normals_width) {  // DownsamplePass::run on a 16 x 16 G-buffer
    rendergraph::RenderGraph g;
    const auto u = VK_IMAGE_USAGE_SAMPLED_BIT;
    auto d = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_D24_UNORM_S8_UINT, VK_IMAGE_ASPECT_DEPTH_BIT, 16, 16, 1, depth_mips, 1}, VK_IMAGE_TILING_OPTIMAL, u);
    auto n = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R16G16_UNORM, VK_IMAGE_ASPECT_COLOR_BIT, 16, 16}, VK_IMAGE_TILING_OPTIMAL, u);
    auto v = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R16G16_SFLOAT, VK_IMAGE_ASPECT_COLOR_BIT, 16, 16}, VK_IMAGE_TILING_OPTIMAL, u);
    auto on = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R16G16_UNORM, VK_IMAGE_ASPECT_COLOR_BIT, normals_width, 8}, VK_IMAGE_TILING_OPTIMAL, u);
    auto ov = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R16G16_SFLOAT, VK_IMAGE_ASPECT_COLOR_BIT, 8, 8}, VK_IMAGE_TILING_OPTIMAL, u);
    DownsamplePass pass;
    pass.run(g, n, v, d, on, ov);
  };
  expect(out, "single_mip_depth", [&] { downsample(1, 8); });
  expect(out, "mismatched_outputs", [&] { downsample(5, 4); });
  expect(out, "incompatible_usage", [] {
    rendergraph::RenderGraph g;
    auto img = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R16_SFLOAT, VK_IMAGE_ASPECT_COLOR_BIT, 8, 8}, VK_IMAGE_TILING_OPTIMAL, VK_IMAGE_USAGE_STORAGE_BIT);
    struct D { rendergraph::ImageViewId a, b; };
    g.add_task<D>("bad",
      [&](D& d, rendergraph::RenderGraphBuilder& b) { d.a = b.sample_image(img, VK_SHADER_STAGE_COMPUTE_BIT); d.b = b.use_storage_image(img, VK_SHADER_STAGE_COMPUTE_BIT, 0, 0); },
      [](D&, rendergraph::RenderResources&, gpu::CmdContext&) {});
  });
  expect(out, "read_then_write_in_separate_tasks", [] {
    rendergraph::RenderGraph g;
    auto img = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R16_SFLOAT, VK_IMAGE_ASPECT_COLOR_BIT, 8, 8}, VK_IMAGE_TILING_OPTIMAL, VK_IMAGE_USAGE_STORAGE_BIT);
    struct D { rendergraph::ImageViewId a; };
    g.add_task<D>("r", [&](D& d, rendergraph::RenderGraphBuilder& b) { d.a = b.sample_image(img, VK_SHADER_STAGE_COMPUTE_BIT); }, [](D&, rendergraph::RenderResources&, gpu::CmdContext&) {});
    g.add_task<D>("w", [&](D& d, rendergraph::RenderGraphBuilder& b) { d.a = b.use_storage_image(img, VK_SHADER_STAGE_COMPUTE_BIT, 0, 0); }, [](D&, rendergraph::RenderResources&, gpu::CmdContext&) {});
  });
  expect(out, "remap_keeps_ids_valid", [&] {
    rendergraph::RenderGraph g;
    auto a = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R16_SFLOAT, VK_IMAGE_ASPECT_COLOR_BIT, 8, 8}, VK_IMAGE_TILING_OPTIMAL, VK_IMAGE_USAGE_STORAGE_BIT);
    auto b = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R16_SFLOAT, VK_IMAGE_ASPECT_COLOR_BIT, 16, 8}, VK_IMAGE_TILING_OPTIMAL, VK_IMAGE_USAGE_STORAGE_BIT);
    void* pa = g.get_image(a)->device_ptr();
    void* pb = g.get_image(b)->device_ptr();
    g.remap(a, b);
    if (g.get_image(a)->device_ptr() != pb || g.get_image(b)->device_ptr() != pa || g.get_descriptor(a).width != 16)
      throw std::runtime_error{"remap did not swap the table entries"};
  });
  expect(out, "tasks_run_in_submission_order", [&] {
    rendergraph::RenderGraph g;
    std::string order;
    struct D {};
    for (const char* n : {"a", "b", "c"})
      g.add_task<D>(n, [](D&, rendergraph::RenderGraphBuilder&) {}, [&order, n](D&, rendergraph::RenderResources&, gpu::CmdContext&) { order += n; });
    if (!order.empty()) throw std::runtime_error{"run callback executed before submit"};
    g.submit();
    if (order != "abc") throw std::runtime_error{"tasks reordered: " + order};
  });
  expect(out, "ray_query_gtao", [] { rendergraph::RenderGraph g; GTAO gtao{g, 64, 64, true}; });
  expect(out, "ubo_ring_overflow", [] {
    gpu::UniformBufferPool pool;
    struct Big { char b[6000]; };
    pool.allocate_ubo<Big>(); pool.allocate_ubo<Big>(); pool.allocate_ubo<Big>();
  });
  return copy_out(buf, buf_size, out);
}

int vkrh_selftest_programs(char* buf, uint32_t buf_size) {
  std::string out;
  gpu::register_hot_path_programs();
  for (const std::string& name : gpu::program_names())
    expect(out, name.c_str(), [&] {
      gpu::CmdContext cmd;
      cmd.bind_pipeline(gpu::create_compute_pipeline(name.c_str()));
      cmd.bind_descriptors_compute(0, {cmd.allocate_set()});
      cmd.dispatch(1, 1, 1);
    });
  return copy_out(buf, buf_size, out);
}

int vkrh_create_image(void* frame, const char* name, uint32_t format, uint32_t width, uint32_t height, uint32_t mip_levels, uint32_t array_layers) {
  return guarded([&] { frame_ref(frame).create_user_image(name, format, width, height, mip_levels, array_layers); });
}
int vkrh_transfer(void* frame, uint32_t op, const char* image, const char* dst, const float* value) {
  return guarded([&] { frame_ref(frame).transfer(op, image, dst, value); });
}
int vkrh_selftest_transfers(char* buf, uint32_t buf_size) {
  std::string out;
  const int rc = guarded([&] {
    rendergraph::RenderGraph g;
    const auto u = VK_IMAGE_USAGE_TRANSFER_SRC_BIT | VK_IMAGE_USAGE_TRANSFER_DST_BIT;
    auto tex = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R8G8B8A8_SRGB, VK_IMAGE_ASPECT_COLOR_BIT, 40, 24, 1, 6, 1}, VK_IMAGE_TILING_OPTIMAL, u);
    auto depth = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_D24_UNORM_S8_UINT, VK_IMAGE_ASPECT_DEPTH_BIT, 16, 16, 1, 3, 2}, VK_IMAGE_TILING_OPTIMAL, u);
    auto color = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R8G8B8A8_UNORM, VK_IMAGE_ASPECT_COLOR_BIT, 16, 8, 1, 2, 1}, VK_IMAGE_TILING_OPTIMAL, u);
    auto src = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R16G16B16A16_SFLOAT, VK_IMAGE_ASPECT_COLOR_BIT, 32, 16}, VK_IMAGE_TILING_OPTIMAL, u);
    auto dst = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R8G8B8A8_SRGB, VK_IMAGE_ASPECT_COLOR_BIT, 32, 16}, VK_IMAGE_TILING_OPTIMAL, u);
    gen_mipmaps(g, tex);
    clear_depth(g, depth);
    VkClearColorValue red{};
    red.float32[0] = 1.f;
    clear_color(g, color, red);
    blit_image(g, src, dst);
    dump_pending_tasks(g, out);
  });
  return rc != 0 ? rc : copy_out(buf, buf_size, out);
}

int vkrh_selftest_ssao(char* buf, uint32_t buf_size) {
  std::string out;
  const int rc = guarded([&] {
    rendergraph::RenderGraph g;
    auto depth = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_D24_UNORM_S8_UINT, VK_IMAGE_ASPECT_DEPTH_BIT | VK_IMAGE_ASPECT_STENCIL_BIT, 64, 36, 1, 7, 1},
                                VK_IMAGE_TILING_OPTIMAL, VK_IMAGE_USAGE_DEPTH_STENCIL_ATTACHMENT_BIT | VK_IMAGE_USAGE_SAMPLED_BIT);
    auto target = create_ssao_texture(g, 64, 36);
    SSAOPass pass{g, target};
    for (uint32_t k = 0; k < 16; k++) pass.sphere_samples[k] = glm::vec3{float(3 * k), float(3 * k + 1), float(3 * k + 2)};
    const SSAOInParams params{glm::mat4{1.f}, 1.0f, 1.5f, 0.05f, 80.f};
    pass.draw(g, depth, target, params);
    dump_pending_tasks(g, out);
    for (const bool std140 : {false, true}) {
      pass.std140_samples = std140;
      const std::vector<uint8_t> block = pass.uniform_block(params);
      const vkr_ssao_params p = gpu::ssao_params_from_block(block.data(), block.size());
      out += "packing " + std::to_string(block.size()) + ":";
      append_words(out, p);
    }
  });
  return rc != 0 ? rc : copy_out(buf, buf_size, out);
}

int vkrh_selftest_tile_regression(char* buf, uint32_t buf_size) {
  std::string out;
  const int rc = guarded([&] {
    rendergraph::RenderGraph g;
    Gbuffer gbuffer{g, 64, 48};
    AdvancedSSR pass{g, 64, 48};
    glm::mat4 normal_mat{0.f};
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 4; r++) normal_mat[c][r] = float(4 * c + r + 1);
    const AdvancedSSRParams params{normal_mat, 1.0f, 1.5f, 0.05f, 80.f};
    pass.run_tile_regression_pass(g, params, gbuffer);
    const uint32_t depth = gbuffer.depth.get_index(), planes = pass.get_tile_planes().get_index();
    out += "images: depth " + std::to_string(depth) + " tile_planes " + std::to_string(planes) + "\n";
    const auto ext = g.get_descriptor(pass.get_tile_planes());
    out += "tile_planes: " + std::to_string(ext.width) + "x" + std::to_string(ext.height) + " format " + std::to_string(int(ext.format)) + "\n";
    dump_pending_tasks(g, out);
    const vkr_tile_regression_push pc = AdvancedSSR::tile_regression_push(params);
    out += "push " + std::to_string(sizeof(pc)) + ":";
    append_words(out, pc);
  });
  return rc != 0 ? rc : copy_out(buf, buf_size, out);
}

int vkrh_selftest_texdraw(char* buf, uint32_t buf_size) {
  std::string out;
  const int rc = guarded([&] {
    rendergraph::RenderGraph g;
    g.set_backbuffer_extent(64, 36);
    auto source = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R16G16B16A16_SFLOAT, VK_IMAGE_ASPECT_COLOR_BIT, 128, 72, 1, 3, 1},
                                 VK_IMAGE_TILING_OPTIMAL, VK_IMAGE_USAGE_STORAGE_BIT | VK_IMAGE_USAGE_SAMPLED_BIT);
    add_backbuffer_subpass(g, source, gpu::create_sampler(gpu::DEFAULT_SAMPLER), DrawTex::ShowR);
    add_present_subpass(g);
    const auto backbuffer = g.get_backbuffer();
    out += "images: source " + std::to_string(source.get_index()) + " backbuffer " + std::to_string(backbuffer.get_index()) + "\n";
    const auto ext = g.get_descriptor(backbuffer);
    out += "backbuffer: " + std::to_string(ext.width) + "x" + std::to_string(ext.height) + " format " + std::to_string(int(ext.format)) + "\n";
    dump_pending_tasks(g, out);
    out += std::string{"program: texdraw "} + (gpu::has_program("texdraw") ? "1" : "0") + "\n";
    const vkr_texdraw_push pc = texdraw_push(DrawTex::ShowR);
    out += "push " + std::to_string(sizeof(pc)) + ": " + std::to_string(pc.flags) + "\n";
  });
  return rc != 0 ? rc : copy_out(buf, buf_size, out);
}

int vkrh_selftest_ray_query(char* buf, uint32_t buf_size) {
  std::string out;
  const GTAORTParams params{glm::mat4{1.f}, 1.0f, 1.0f, 0.05f, 80.f};
  auto images = [](rendergraph::RenderGraph& g, rendergraph::ImageResourceId& depth, rendergraph::ImageResourceId& normal) {
    const auto u = VK_IMAGE_USAGE_SAMPLED_BIT;
    depth = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_D24_UNORM_S8_UINT, VK_IMAGE_ASPECT_DEPTH_BIT, 64, 64, 1, 7, 1}, VK_IMAGE_TILING_OPTIMAL, u);
    normal = g.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo{VK_FORMAT_R16G16_UNORM, VK_IMAGE_ASPECT_COLOR_BIT, 64, 64}, VK_IMAGE_TILING_OPTIMAL, u);
  };
  expect(out, "default_graph", [] { rendergraph::RenderGraph g; GTAO gtao{g, 64, 64, true}; });
  expect(out, "ray_query_graph", [] { rendergraph::RenderGraph g{nullptr, gpu::DeviceConfig{true}}; GTAO gtao{g, 64, 64, true}; });
  expect(out, "device_config", [] {
    rendergraph::RenderGraph a, b{nullptr, gpu::DeviceConfig{true}};
    if (a.get_device_config().use_ray_query || !b.get_device_config().use_ray_query) throw std::runtime_error{"device config not kept per graph"};
  });
  const auto rt_pass = [&](bool ray_query, bool with_tlas) {  // add_main_rt_pass of a GTAO built with / without ray query
    rendergraph::RenderGraph g{nullptr, gpu::DeviceConfig{true}};
    GTAO gtao{g, 64, 64, ray_query};
    rendergraph::ImageResourceId depth, normal;
    images(g, depth, normal);
    gtao.add_main_rt_pass(g, params, with_tlas ? (VkAccelerationStructureKHR)&gtao : nullptr, depth, normal);
  };
  expect(out, "null_tlas", [&] { rt_pass(true, false); });
  expect(out, "rt_pass_without_ray_query", [&] { rt_pass(false, true); });
  expect(out, "null_accel_binding", [] {
    gpu::CmdContext cmd;
    gpu::write_set(cmd.allocate_set(), gpu::AccelerationStructBinding{3, nullptr});
  });
  return copy_out(buf, buf_size, out);
}

// ---- tiled frame ----------------------------------------------------------------------------------------------------
void* vkrh_tiled_create(const vkrh_tiled_config* cfg) {
  TiledFrame* t = nullptr;
  int rc = guarded([&] {
    if (!cfg) throw std::runtime_error{"vkrh_tiled_create: NULL config"};
    t = new TiledFrame(*cfg);
  });
  return rc == 0 ? t : nullptr;
}
void vkrh_tiled_destroy(void* tiled) { delete (TiledFrame*)tiled; }
void* vkrh_tiled_frame(void* tiled) { return tiled ? ((TiledFrame*)tiled)->frame.get() : nullptr; }
// (a NULL handle is an error message, not a crash: the Python harness keeps None for frames that are not native)
static TiledFrame& tiled_ref(void* tiled, const char* what) {
  if (!tiled) throw std::runtime_error{std::string{what} + ": NULL tiled frame"};
  return *(TiledFrame*)tiled;
}
int vkrh_tiled_step(void* tiled) { return guarded([&] { tiled_ref(tiled, "vkrh_tiled_step").step(); }); }
int vkrh_tiled_flush(void* tiled) { return guarded([&] { tiled_ref(tiled, "vkrh_tiled_flush").flush(); }); }
int vkrh_tiled_phase(void* tiled, uint32_t phase) { return guarded([&] { tiled_ref(tiled, "vkrh_tiled_phase").phase(phase); }); }
int vkrh_tiled_gather_parts(void* tiled, uint32_t which, vkr_gather_part* out, uint32_t capacity, uint32_t* count) {
  return guarded([&] {
    if (!tiled || !out || !count || capacity < 8 || which > 1) throw std::runtime_error{"vkrh_tiled_gather_parts: bad arguments (capacity >= 8)"};
    *count = ((TiledFrame*)tiled)->gather_parts((int)which, out);
  });
}
int vkrh_tiled_halo_peers(void* tiled, uint32_t surface, vkr_halo_peer* out, uint32_t capacity, uint32_t* count) {
  return guarded([&] {
    if (!tiled || !out || !count || capacity < 2 || surface > 2) throw std::runtime_error{"vkrh_tiled_halo_peers: bad arguments (capacity >= 2)"};
    *count = ((TiledFrame*)tiled)->halo_peers((int)surface, out);
  });
}
int vkrh_tiled_hit_counts(void* tiled, uint32_t* row) {
  return guarded([&] {
    auto* t = (TiledFrame*)tiled;
    if (!t || !row || !t->by_request()) throw std::runtime_error{"vkrh_tiled_hit_counts: not a tiled frame with hit-colour requests"};
    TiledFrame::check(hipMemcpyAsync(row, t->hit.counts, sizeof(uint32_t) * t->cfg.world, hipMemcpyDeviceToHost, t->compute), "counts");
    TiledFrame::check(hipStreamSynchronize(t->compute), "synchronize");
  });
}
int vkrh_tiled_hit_requests(void* tiled, const uint32_t* matrix, vkr_halo_peer* peers, uint32_t capacity, uint32_t* count) {
  return guarded([&] {
    auto* t = (TiledFrame*)tiled;
    if (!t || !matrix || !peers || !count || capacity < TiledFrame::HIT_PEERS || !t->by_request()) throw std::runtime_error{"vkrh_tiled_hit_requests: bad arguments (capacity >= 16)"};
    *count = t->hit_write(matrix, t->compute, peers);
  });
}
int vkrh_tiled_hit_replies(void* tiled, vkr_halo_peer* peers, uint32_t capacity, uint32_t* count) {
  return guarded([&] {
    auto* t = (TiledFrame*)tiled;
    if (!t || !peers || !count || capacity < TiledFrame::HIT_PEERS || !t->by_request()) throw std::runtime_error{"vkrh_tiled_hit_replies: bad arguments (capacity >= 16)"};
    *count = t->hit_reply(t->compute, peers);
  });
}
int vkrh_tiled_hit_finish(void* tiled) {
  return guarded([&] {
    auto* t = (TiledFrame*)tiled;
    if (!t || !t->by_request()) throw std::runtime_error{"vkrh_tiled_hit_finish: not a tiled frame with hit-colour requests"};
    t->hit_scatter(t->compute);
  });
}
int vkrh_tiled_hit_errors(void* tiled, uint32_t* errors) {
  return guarded([&] {
    auto* t = (TiledFrame*)tiled;
    if (!t || !errors || !t->by_request()) throw std::runtime_error{"vkrh_tiled_hit_errors: not a tiled frame with hit-colour requests"};
    TiledFrame::check(hipDeviceSynchronize(), "synchronize");
    TiledFrame::check(hipMemcpy(errors, t->hit.counts + TiledFrame::HIT_ERRORS, sizeof(uint32_t), hipMemcpyDeviceToHost), "errors");
  });
}
int vkrh_tiled_hit_bytes(void* tiled, uint64_t* bytes) {
  return guarded([&] {
    if (!tiled || !bytes) throw std::runtime_error{"vkrh_tiled_hit_bytes: NULL argument"};
    *bytes = ((TiledFrame*)tiled)->hit.wire_bytes;
  });
}
int vkrh_tiled_hit_rounds(void* tiled, uint64_t* rounds3) {
  return guarded([&] {
    if (!tiled || !rounds3) throw std::runtime_error{"vkrh_tiled_hit_rounds: NULL argument"};
    const auto& h = ((TiledFrame*)tiled)->hit;
    rounds3[0] = h.rounds_speculative; rounds3[1] = h.rounds_exact; rounds3[2] = h.rounds_repeated;
  });
}
int vkrh_hit_capacities(const uint32_t* counts, uint32_t world, uint32_t percent, uint32_t* capacities) {
  return guarded([&] {
    if (!counts || !capacities || world == 0 || world > 16 || percent == 0) throw std::runtime_error{"vkrh_hit_capacities: bad arguments"};
    TiledFrame::hit_capacities(counts, world, percent, capacities);
  });
}
int vkrh_tiled_emulate_wire(void* tiled, void* comm, const uint32_t* counts) {
  return guarded([&] { tiled_ref(tiled, "vkrh_tiled_emulate_wire").emulate_wire(comm, counts); });
}
int vkrh_tiled_pipelined(void* tiled) { return tiled && ((TiledFrame*)tiled)->pipeline_enabled ? 1 : 0; }
int vkrh_tiled_local_first(void* tiled) { return tiled && ((TiledFrame*)tiled)->local_first() ? 1 : 0; }
int vkrh_tiled_set_shading(void* tiled, uint32_t on) { return guarded([&] { tiled_ref(tiled, "vkrh_tiled_set_shading").set_shading(on != 0); }); }
int vkrh_tiled_shading(void* tiled) {
  int on = -1;
  (void)guarded([&] { on = tiled_ref(tiled, "vkrh_tiled_shading").shading ? 1 : 0; });
  return on;
}
int vkrh_tiled_time_waits(void* tiled, uint32_t on) {
  return guarded([&] {
    auto* t = &tiled_ref(tiled, "vkrh_tiled_time_waits");
    t->time_waits = on != 0;
    if (!on) {  // marks nobody collected: their events must not pile up
      TiledFrame::check(hipStreamSynchronize(t->compute), "synchronize");
      t->drop_wait_marks();
    }
  });
}
int vkrh_tiled_wait_times(void* tiled, float* ms5) {
  return guarded([&] {
    if (!tiled || !ms5) throw std::runtime_error{"vkrh_tiled_wait_times: NULL argument"};
    ((TiledFrame*)tiled)->collect_waits(ms5);
  });
}
int vkrh_balance_rows(const float* ms, const uint32_t* bounds_in, uint32_t world, uint32_t align, uint32_t min_rows, uint32_t* bounds_out) {
  return guarded([&] {
    if (!ms || !bounds_in || !bounds_out || world == 0 || align == 0) throw std::runtime_error{"vkrh_balance_rows: bad arguments"};
    const uint32_t H = bounds_in[world];
    min_rows = std::max((min_rows + align - 1) / align * align, align);
    if (bounds_in[0] != 0 || H % align || uint64_t(min_rows) * world > H) throw std::runtime_error{"vkrh_balance_rows: the frame does not hold `world` strips of min_rows"};
    double total = 0.0;
    for (uint32_t r = 0; r < world; r++) {
      if (bounds_in[r + 1] <= bounds_in[r] || !(ms[r] > 0.0f)) throw std::runtime_error{"vkrh_balance_rows: bounds must increase and times be positive"};
      total += ms[r];
    }
    // row y of the frame where the cumulative cost (piecewise linear: uniform inside a measured strip) reaches `target`
    auto row_at = [&](double target) {
      double acc = 0.0;
      for (uint32_t r = 0; r < world; r++) {
        if (acc + ms[r] >= target || r + 1 == world)
          return bounds_in[r] + (target - acc) / ms[r] * double(bounds_in[r + 1] - bounds_in[r]);
        acc += ms[r];
      }
      return double(H);
    };
    bounds_out[0] = 0; bounds_out[world] = H;
    for (uint32_t r = 1; r < world; r++) {
      const double y = row_at(total * r / world);
      uint32_t b = uint32_t(y / align + 0.5) * align;
      // keep every strip, the ones still to come included, at least min_rows high
      b = std::max(b, bounds_out[r - 1] + min_rows);
      b = std::min(b, H - (world - r) * min_rows);
      bounds_out[r] = b;
    }
  });
}
const char* vkrh_last_tasks(void* frame) { return frame ? ((PostFxFrame*)frame)->task_names.c_str() : ""; }
const char* vkrh_last_lanes(void* frame) { return frame ? ((PostFxFrame*)frame)->task_lanes.c_str() : ""; }
int vkrh_set_async(void* frame, uint32_t on) { return guarded([&] { frame_ref(frame).graph.set_async(on != 0); }); }

}  // extern "C"
