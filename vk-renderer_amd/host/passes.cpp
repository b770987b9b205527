// passes.cpp — the pass structs of passes.hpp.  Each method packs the constants the matching reference pass
// uploads (file:line given per method), lists its bindings in the shader's binding order and hands them to
// pass_recorder.hpp; the bound program (gpu/gpu.cpp program table) turns that into one C-ABI call.
#include "passes.hpp"
#include "imgui_pass.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>

#include <hip/hip_runtime_api.h>

#include "pass_recorder.hpp"
#include "probe_renderer.hpp"
#include "scene/scene_as.hpp"
#include "util_passes.hpp"
#include "backbuffer_subpass2.hpp"

using rendergraph::ImageResourceId;
using rendergraph::RenderGraph;

namespace {

constexpr VkImageAspectFlags DEPTH = VK_IMAGE_ASPECT_DEPTH_BIT;
constexpr VkImageAspectFlags COLOR = VK_IMAGE_ASPECT_COLOR_BIT;

ImageResourceId make_image(RenderGraph &graph, VkFormat format, uint32_t w, uint32_t h, VkImageUsageFlags usage,
                           VkImageAspectFlags aspect = COLOR, uint32_t mips = 1, uint32_t layers = 1)
{
  return graph.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo {format, aspect, w, h, 1, mips, layers}, VK_IMAGE_TILING_OPTIMAL, usage);
}

VkSampler default_sampler() { return gpu::create_sampler(gpu::DEFAULT_SAMPLER); }

gpu::GraphicsPipeline fullscreen_pipeline(const char *program, const gpu::Registers &regs = {}) {
  auto p = gpu::create_graphics_pipeline();
  p.set_program(program);
  p.set_registers(regs);
  p.set_vertex_input({});
  return p;
}

void copy_mat(vkr_mat4 &dst, const glm::mat4 &src) { std::memcpy(dst.m, &src, sizeof(dst.m)); }

// {inverse(camera), inverse(prev_camera), fovy_aspect_znear_zfar}: TAAParams (taa.cpp:24-30), the blur's
// Params (advanced_ssr.cpp:388-401)
vkr_reproject_params reproject_params(const DrawTAAParams &p) {
  vkr_reproject_params r;
  copy_mat(r.inverse_camera, glm::inverse(p.camera));
  copy_mat(r.prev_inverse_camera, glm::inverse(p.prev_camera));
  std::memcpy(r.fovy_aspect_znear_zfar, &p.fovy_aspect_znear_zfar, sizeof(r.fovy_aspect_znear_zfar));
  return r;
}

constexpr uint32_t HALTON_SEQ_SIZE = 128;
enum : uint32_t { NORMALIZE_REFLECTIONS = 1, ACCUMULATE_REFLECTIONS = 2, BILATERAL_FILTER = 4 };  // advanced_ssr.cpp:304-306

}  // namespace

// ==== Gbuffer (scene_renderer.cpp:8-44) ================================================================
Gbuffer::Gbuffer(RenderGraph &graph, uint32_t width, uint32_t height) : w {width}, h {height} {
  const auto color_usage = VK_IMAGE_USAGE_COLOR_ATTACHMENT_BIT|VK_IMAGE_USAGE_SAMPLED_BIT|VK_IMAGE_USAGE_TRANSFER_SRC_BIT;
  const auto depth_usage = VK_IMAGE_USAGE_DEPTH_STENCIL_ATTACHMENT_BIT|VK_IMAGE_USAGE_SAMPLED_BIT|VK_IMAGE_USAGE_TRANSFER_SRC_BIT;
  albedo = make_image(graph, VK_FORMAT_R8G8B8A8_SRGB, width, height, color_usage);
  normal = make_image(graph, VK_FORMAT_R16G16_UNORM, width, height, color_usage);
  velocity_vectors = make_image(graph, VK_FORMAT_R16G16_SFLOAT, width, height, color_usage);
  downsampled_normals = make_image(graph, VK_FORMAT_R16G16_UNORM, width/2, height/2, color_usage);
  downsampled_velocity_vectors = make_image(graph, VK_FORMAT_R16G16_SFLOAT, width/2, height/2, color_usage);
  material = make_image(graph, VK_FORMAT_R8G8B8A8_SRGB, width, height, color_usage);
  const uint32_t depth_mips = uint32_t(std::floor(std::log2(std::max(width, height)))) + 1;  // :13
  const auto ds = DEPTH|VK_IMAGE_ASPECT_STENCIL_BIT;
  depth = make_image(graph, VK_FORMAT_D24_UNORM_S8_UINT, width, height, depth_usage, ds, depth_mips);
  prev_depth = make_image(graph, VK_FORMAT_D24_UNORM_S8_UINT, width, height, depth_usage|VK_IMAGE_USAGE_TRANSFER_DST_BIT, ds, depth_mips);
  frame_hiz = depth;
  frame_normals = downsampled_normals;
  frame_albedo = albedo;
}

void Gbuffer::enable_tiling(RenderGraph &graph, uint32_t full_width, uint32_t full_height) {
  tiled = true;
  const uint32_t frame_mips = uint32_t(std::floor(std::log2(std::max(full_width, full_height)))) + 1;
  frame_hiz = graph.create_frame_image(gpu::ImageInfo {VK_FORMAT_D24_UNORM_S8_UINT, DEPTH, full_width/2, full_height/2, 1, frame_mips - 1, 1});
  frame_normals = graph.create_frame_image(gpu::ImageInfo {VK_FORMAT_R16G16_UNORM, COLOR, full_width/2, full_height/2});
  frame_albedo = graph.create_frame_image(gpu::ImageInfo {VK_FORMAT_R8G8B8A8_SRGB, COLOR, full_width, full_height});
}

void Gbuffer::enable_normal_requests(RenderGraph &graph, uint32_t row0, uint32_t row1) {
  if (!tiled) throw std::runtime_error {"Gbuffer::enable_normal_requests: the G-buffer is not tiled"};
  normals_by_request = true;
  normal_row0 = row0; normal_row1 = row1;
  const auto usage = VK_IMAGE_USAGE_STORAGE_BIT|VK_IMAGE_USAGE_SAMPLED_BIT;
  pend_mask = graph.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo {VK_FORMAT_R8_UNORM, COLOR, w/2, h/2}, VK_IMAGE_TILING_OPTIMAL, usage);
  pend_data = graph.create_image(VK_IMAGE_TYPE_2D, gpu::ImageInfo {VK_FORMAT_R32G32B32A32_SFLOAT, COLOR, 2 * (w/2), h/2}, VK_IMAGE_TILING_OPTIMAL, usage);
}

void Gbuffer::enable_pipelining(RenderGraph &graph) {
  if (pipelined) return;
  const auto color_usage = VK_IMAGE_USAGE_COLOR_ATTACHMENT_BIT|VK_IMAGE_USAGE_SAMPLED_BIT|VK_IMAGE_USAGE_TRANSFER_SRC_BIT;
  const auto depth_usage = VK_IMAGE_USAGE_DEPTH_STENCIL_ATTACHMENT_BIT|VK_IMAGE_USAGE_SAMPLED_BIT|VK_IMAGE_USAGE_TRANSFER_SRC_BIT;
  const uint32_t depth_mips = uint32_t(std::floor(std::log2(std::max(w, h)))) + 1;
  depth_next = make_image(graph, VK_FORMAT_D24_UNORM_S8_UINT, w, h, depth_usage|VK_IMAGE_USAGE_TRANSFER_DST_BIT, DEPTH|VK_IMAGE_ASPECT_STENCIL_BIT, depth_mips);
  downsampled_normals_next = make_image(graph, VK_FORMAT_R16G16_UNORM, w/2, h/2, color_usage);
  downsampled_velocity_vectors_next = make_image(graph, VK_FORMAT_R16G16_SFLOAT, w/2, h/2, color_usage);
  pipelined = true;
}

void Gbuffer::swap_sets(RenderGraph &graph) {
  if (!pipelined) throw std::runtime_error {"Gbuffer::swap_sets: pipelining is not enabled"};
  graph.remap(depth, depth_next);  // (untiled, frame_hiz / frame_normals ARE these ids and follow the swap)
  graph.remap(downsampled_normals, downsampled_normals_next);
  graph.remap(downsampled_velocity_vectors, downsampled_velocity_vectors_next);
}

// ==== DownsamplePass (downsample_pass.cpp) ================================================================
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
DownsamplePass::DownsamplePass() : sampler {default_sampler()} {
  gpu::Registers always_write {};  // :6-9: depth test ALWAYS + depth write
  always_write.depth_stencil.depthTestEnable = VK_TRUE;
  always_write.depth_stencil.depthCompareOp = VK_COMPARE_OP_ALWAYS;
  always_write.depth_stencil.depthWriteEnable = VK_TRUE;
  downsample_gbuffer = fullscreen_pipeline("downsample_gbuffer", always_write);
  downsample_depth = fullscreen_pipeline("depth_mips", always_write);
}
#endif

// :25-92.  Size checks and their messages :37-50.
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void DownsamplePass::run_downsample_gbuff(RenderGraph &graph, ImageResourceId src_normals, ImageResourceId src_velocity, ImageResourceId depth,
  ImageResourceId out_normal, ImageResourceId out_velocity)
{
  const auto d = graph.get_descriptor(depth), n = graph.get_descriptor(out_normal), v = graph.get_descriptor(out_velocity);
  if (d.mip_levels < 2)
    throw std::runtime_error {"Can't downsample depth texture with 1 mip level"};
  const uint32_t half_w = std::max(1u, d.width/2), half_h = std::max(1u, d.height/2);
  if (half_w != n.width || half_h != n.height || v.width != n.width || v.height != n.height)
    throw std::runtime_error {"Output textures have different sizes"};
  downsample_gbuffer.set_rendersubpass({true, {n.format, v.format, d.format}});
  rec::fullscreen(graph, "DownsampleGbuffer", downsample_gbuffer,
    {rec::sampled_mips(0, depth, sampler, DEPTH, 0, 1), rec::sampled_mips(1, src_normals, sampler, COLOR, 0, 1),
     rec::sampled_mips(2, src_velocity, sampler, COLOR, 0, 1),
     rec::color_target(out_normal), rec::color_target(out_velocity), rec::depth_target(depth, 1)},
    rec::no_push(), half_w, half_h);
}
#endif

// :94-131 records one "DownsampleDepth" draw per mip (L-2 dependent passes).  MI355X-first: one task whose
// attachments are all remaining mips; the bound program reduces five levels per workgroup through LDS.
// Each mip is still the 2x2 min of its parent with extent max(1, W >> i) (:118-120).
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void DownsamplePass::run_downsample_depth(RenderGraph &graph, ImageResourceId depth, uint32_t src_mip) {
  const auto desc = graph.get_descriptor(depth);
  if (src_mip + 1 >= desc.mip_levels) return;
  downsample_depth.set_rendersubpass({true, {desc.format}});
  std::vector<rec::Binding> binds {rec::sampled_mips(0, depth, sampler, DEPTH, src_mip, 1)};
  for (uint32_t mip = src_mip + 1; mip < desc.mip_levels; mip++) binds.push_back(rec::depth_target(depth, mip));
  rec::fullscreen(graph, "DownsampleDepth", downsample_depth, binds, rec::no_push(),
                  std::max(desc.width >> (src_mip + 1), 1u), std::max(desc.height >> (src_mip + 1), 1u));
}
#endif

#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void DownsamplePass::run(RenderGraph &graph, ImageResourceId src_normals, ImageResourceId src_velocity, ImageResourceId depth,
  ImageResourceId out_normals, ImageResourceId out_velocity)
{
  run_downsample_gbuff(graph, src_normals, src_velocity, depth, out_normals, out_velocity);  // :133-143
  run_downsample_depth(graph, depth, 1);
}
#endif

// ==== GTAO (gtao.cpp) ================================================================================
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
ImageResourceId create_gtao_texture(RenderGraph &graph, uint32_t width, uint32_t height) {  // :10-13
  return make_image(graph, VK_FORMAT_R8_UNORM, width, height, VK_IMAGE_USAGE_COLOR_ATTACHMENT_BIT|VK_IMAGE_USAGE_SAMPLED_BIT);
}
#endif

// resources :17-47, pipelines :49-81
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
GTAO::GTAO(RenderGraph &graph, uint32_t width, uint32_t height, bool use_ray_query, bool half_res, int pattern_n)
  : deinterleave_n {pattern_n}, pinned_jitter {std::numeric_limits<float>::quiet_NaN()}
{
  if (use_ray_query && !graph.get_device_config().use_ray_query)
    throw std::runtime_error {"GTAO: ray-query AO needs a device with ray query (construct the graph with gpu::DeviceConfig {.use_ray_query = true})"};
  if (half_res) {
    width /= 2;
    height /= 2;
    depth_lod = 1;
  }
  const auto usage = VK_IMAGE_USAGE_STORAGE_BIT|VK_IMAGE_USAGE_SAMPLED_BIT;
  raw = make_image(graph, VK_FORMAT_R16G16B16A16_SFLOAT, width, height, usage|VK_IMAGE_USAGE_COLOR_ATTACHMENT_BIT);
  filtered = make_image(graph, VK_FORMAT_R16_SFLOAT, width, height, usage);
  prev_frame = make_image(graph, VK_FORMAT_R16_SFLOAT, width, height, usage);
  output = make_image(graph, VK_FORMAT_R16_SFLOAT, width, height, usage);
  accumulated_ao = make_image(graph, VK_FORMAT_R16G16_SFLOAT, width, height, usage);
  accumulated_history = make_image(graph, VK_FORMAT_R16G16_SFLOAT, width, height, usage);
  const uint32_t pattern_step = 1u << uint32_t(pattern_n);
  // (an image cannot be empty: below pattern_step texels a side — a 2 x 2 frame — a layer is one texel, and the variant's floored
  // 8 x 4 dispatch over it is no group at all)
  deinterleaved_depth = make_image(graph, VK_FORMAT_R32_SFLOAT, std::max(1u, width/pattern_step), std::max(1u, height/pattern_step), usage, COLOR, 1,
                                   pattern_step * pattern_step);

  main_pipeline = gpu::create_compute_pipeline("gtao_compute_main");
  filter_pipeline = gpu::create_compute_pipeline("gtao_filter");
  accumulate_pipeline = gpu::create_compute_pipeline("gtao_accumulate");
  reproject_pipeline = gpu::create_compute_pipeline("gtao_reproject");
  deinterleave_pipeline = gpu::create_compute_pipeline("deinterleave_depth");
  main_deinterleaved_pipeline = gpu::create_compute_pipeline("main_deinterleaved");
  main_pipeline_gfx = fullscreen_pipeline("gtao_main");
  main_pipeline_gfx.set_rendersubpass({false, {graph.get_descriptor(raw).format}});
  if (use_ray_query) {  // :57-63, :35
    rt_main_pipeline = fullscreen_pipeline("gtao_rt_main");
    rt_main_pipeline.set_rendersubpass({false, {graph.get_descriptor(raw).format}});
    const auto dirs = gtao_random_directions(64);
    random_vectors = gpu::create_buffer(VMA_MEMORY_USAGE_CPU_TO_GPU, sizeof(glm::vec4) * dirs.size(), VK_BUFFER_USAGE_UNIFORM_BUFFER_BIT);
    std::memcpy(random_vectors->get_mapped_ptr(), dirs.data(), sizeof(glm::vec4) * dirs.size());
  }
  sampler = default_sampler();
}
#endif

std::vector<glm::vec4> gtao_random_directions(uint32_t count) {
  std::minstd_rand0 engine;  // what std::default_random_engine is in libstdc++; default seed 1
  std::uniform_real_distribution<float> unit {0.0f, 1.0f};
  std::vector<glm::vec4> out;
  out.reserve(count);
  while (out.size() < count) {
    const float x = float(double(unit(engine)) * 2.0 - 1.0);
    const float y = float(double(unit(engine)) * 2.0 - 1.0);
    const float z = unit(engine);
    const float len = std::sqrt((x * x + y * y) + z * z);  // glm::length of (x, y, z, 0)
    if (double(len) <= 0.00001 || len > 1.0f) continue;
    out.push_back(glm::vec4 {x / len, y / len, z / len, 0.0f});
  }
  return out;
}

// the 12-entry angle table + jitter every main-pass flavour uses (:109-111, :362-364, :487-489)
float GTAO::next_base_angle() {
  static const float table[12] {60.f, 300.f, 180.f, 240.f, 120.f, 0.f, 300.f, 60.f, 180.f, 120.f, 240.f, 0.f};
  const float jitter = std::isnan(pinned_jitter)? (rand()/float(RAND_MAX) - 0.5f) : pinned_jitter;
  return table[frame_count++ % 12]/360.f + jitter;
}

// :84-148; PushConsts :101-113; floor dispatch :145
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void GTAO::add_main_pass(RenderGraph &graph, const GTAOParams &params, ImageResourceId depth, ImageResourceId normal,
  ImageResourceId material, ImageResourceId preintegrated_pdf)
{
  static_assert(sizeof(GTAOParams) == sizeof(vkr_gtao_params), "GTAOParams must match the C-ABI");
  const vkr_gtao_push pc {next_base_angle(), weight_ratio, mis_gtao? 1u : 0u, two_directions? 255u : 0u, only_reflections? 255u : 0u};
  rec::compute(graph, "GTAO_main", main_pipeline,
    {rec::sampled_mips(0, depth, sampler, DEPTH, depth_lod, 1), rec::uniform(1, params), rec::sampled(2, normal, sampler),
     rec::sampled(3, material, sampler), rec::sampled(4, preintegrated_pdf, sampler), rec::storage(5, raw)},
    rec::push(pc), rec::Grid {raw, 8, 4, rec::Floor});
}
#endif

// :198-239
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void GTAO::add_filter_pass(RenderGraph &graph, const GTAOParams &params, ImageResourceId depth) {
  const vkr_gtao_filter_push pc {params.znear, params.zfar};
  rec::compute(graph, "GTAO_filter", filter_pipeline,
    {rec::sampled_mips(0, depth, sampler, DEPTH, depth_lod, 1), rec::sampled(1, raw, sampler), rec::storage(2, filtered)},
    rec::push(pc), rec::Grid {filtered, 8, 4, rec::Floor});
}
#endif

// :286-347; AccumConstants :300-305; clear_history is consumed once :313-315; ceil dispatch :345
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void GTAO::add_accumulate_pass(RenderGraph &graph, const DrawTAAParams &params, const Gbuffer &gbuffer) {
  vkr_gtao_accum_params consts;
  copy_mat(consts.inverse_camera, glm::inverse(params.camera));
  copy_mat(consts.prev_inverse_camera, glm::inverse(params.prev_camera));
  copy_mat(consts.mvp, params.mvp);
  std::memcpy(consts.fovy_aspect_znear_zfar, &params.fovy_aspect_znear_zfar, sizeof(consts.fovy_aspect_znear_zfar));
  const vkr_gtao_accum_push pc {clear_history? 1u : 0u};
  clear_history = false;
  rec::compute(graph, "GTAO_accumulate", accumulate_pipeline,
    {rec::sampled_mips(0, gbuffer.depth, sampler, DEPTH, depth_lod, 1), rec::sampled_mips(1, gbuffer.prev_depth, sampler, DEPTH, depth_lod, 1),
     rec::sampled(2, filtered, sampler), rec::storage(3, accumulated_ao), rec::sampled(4, gbuffer.downsampled_velocity_vectors, sampler),
     rec::sampled(5, accumulated_history, sampler), rec::uniform(6, consts)},
    rec::push(pc), rec::Grid {accumulated_ao, 8, 4, rec::Ceil});
}
#endif

// ---- the variants the reference's frame loop never records ----
// :349-413: full-screen triangle into `raw`
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void GTAO::add_main_pass_graphics(RenderGraph &graph, const GTAOParams &params, ImageResourceId depth, ImageResourceId normal) {
  const vkr_gtao_gfx_push pc {next_base_angle()};
  const auto ext = graph.get_descriptor(raw);
  rec::fullscreen(graph, "GTAO", main_pipeline_gfx,
    {rec::sampled_mips(0, depth, sampler, DEPTH, depth_lod, 1), rec::uniform(1, params), rec::sampled(2, normal, sampler), rec::color_target(raw)},
    rec::push(pc), ext.width, ext.height);
}
#endif

// :150-196: full-screen triangle into `raw`; bindings 0 GTAORTParams, 1 depth (view mip depth_lod), 2 normal, 3 the scene's
// acceleration structure, 4 RandomVectors; push constant: the rotation (:162)
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void GTAO::add_main_rt_pass(RenderGraph &graph, const GTAORTParams &params, VkAccelerationStructureKHR tlas, ImageResourceId depth,
  ImageResourceId normal)
{
  static_assert(sizeof(GTAORTParams) == sizeof(vkr_gtao_rt_params), "GTAORTParams must match the C-ABI");
  if (!rt_main_pipeline.has_program())
    throw std::runtime_error {"GTAO::add_main_rt_pass: this GTAO was constructed without use_ray_query"};
  if (!tlas)
    throw std::runtime_error {"GTAO::add_main_rt_pass: null acceleration structure (tlas): build scene::SceneAccelerationStructure first"};
  const float rotation = std::isnan(pinned_jitter)? (rand()/float(RAND_MAX) - 0.5f) : pinned_jitter;
  const vkr_gtao_rt_push pc {rotation};
  const auto ext = graph.get_descriptor(raw);
  rec::fullscreen(graph, "GTAO_rt_main", rt_main_pipeline,
    {rec::uniform(0, params), rec::sampled_mips(1, depth, sampler, DEPTH, depth_lod, 1), rec::sampled(2, normal, sampler),
     rec::accel(3, tlas), rec::uniform_buffer(4, random_vectors), rec::color_target(raw)},
    rec::push(pc), ext.width, ext.height);
}
#endif

// :528-536, the panel as the reference draws it; the ImGui names are inert in this headless build (imgui_pass.hpp)
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void GTAO::draw_ui() {
  ImGui::Begin("GTAO");
  ImGui::Checkbox("Enable MIS", &mis_gtao);
  ImGui::Checkbox("Use 2 directions", &two_directions);
  ImGui::Checkbox("Only reflections ao", &only_reflections);
  ImGui::SliderFloat("Weight ratio", &weight_ratio, 1.0, 5.0);
  clear_history = ImGui::Button("Clear history") || clear_history;  // a headless request_clear_history() stays pending
  ImGui::End();
}
#endif

// :241-284: filtered + prev_frame -> output
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void GTAO::add_reprojection_pass(RenderGraph &graph, const GTAOReprojection &params, ImageResourceId depth, ImageResourceId prev_depth) {
  static_assert(sizeof(GTAOReprojection) == sizeof(vkr_gtao_reprojection), "GTAOReprojection must match the C-ABI");
  rec::compute(graph, "GTAO_reproject", reproject_pipeline,
    {rec::uniform(0, params), rec::sampled_mips(1, depth, sampler, DEPTH, depth_lod, 1), rec::sampled_mips(2, prev_depth, sampler, DEPTH, depth_lod, 1),
     rec::sampled(3, filtered, sampler), rec::sampled(4, prev_frame, sampler), rec::storage(5, output)},
    rec::no_push(), rec::Grid {output, 8, 4, rec::Floor});
}
#endif

// :445-470: the dispatch is sized by the *array* extent, as the reference records it (:468)
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void GTAO::deinterleave_depth(RenderGraph &graph, ImageResourceId depth) {
  const vkr_deinterleave_push pc {deinterleave_n};
  rec::compute(graph, "GTAO_deinterleave", deinterleave_pipeline,
    {rec::sampled_mips(0, depth, sampler, DEPTH, depth_lod, 1), rec::storage_array(1, deinterleaved_depth)},
    rec::push(pc), rec::Grid {deinterleaved_depth, 8, 4, rec::Floor});
}
#endif

// :472-526: one dispatch per array layer of the *output* image (raw has one), exactly as the reference loops
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void GTAO::add_main_pass_deinterleaved(RenderGraph &graph, const GTAOParams &params, ImageResourceId normal) {
  const float base_angle = next_base_angle();
  const uint32_t layers = graph.get_descriptor(raw).array_layers? graph.get_descriptor(raw).array_layers : 1;
  for (uint32_t layer = 0; layer < layers; layer++) {
    const vkr_gtao_deinterleaved_push pc {deinterleave_n, layer, base_angle};
    rec::compute(graph, "GTAO_deinterleaved", main_deinterleaved_pipeline,
      {rec::sampled(0, deinterleaved_depth, sampler), rec::uniform(1, params), rec::sampled(2, normal, sampler), rec::storage(3, raw)},
      rec::push(pc), rec::Grid {raw, 8, 4, rec::Floor});
  }
}
#endif

// ==== AdvancedSSR (advanced_ssr.cpp) ========================================================================
// radical inverse with the reference's float-floor division (:8-20) kept as is
static float halton_elem(uint32_t index, uint32_t base) {
  float scale = 1.f, result = 0.f;
  for (uint32_t current = index;;) {
    scale = scale / float(base);
    result = result + scale * float(current % base);
    current = uint32_t(std::floor(float(current) / float(base)));
    if (current == 0) break;
  }
  return result;
}

#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
std::vector<glm::vec4> halton23_seq(uint32_t count) {  // :22-34
  std::vector<glm::vec4> seq(count);
  for (uint32_t i = 0; i < count; i++)
    seq[i] = glm::vec4 {halton_elem(i + 1, 2), halton_elem(i + 1, 3), 0.f, 0.f};
  return seq;
}
#endif

// :36-93
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
AdvancedSSR::AdvancedSSR(RenderGraph &graph, uint32_t w, uint32_t h) {
  trace_pass = gpu::create_compute_pipeline("sssr_trace");
  filter_pass = gpu::create_compute_pipeline("sssr_filter");
  blur_pass = gpu::create_compute_pipeline("sssr_blur");
  preintegrate_pass = gpu::create_compute_pipeline("pdf_preintegrate");
  preintegrate_brdf_pass = gpu::create_compute_pipeline("brdf_preintegrate");
  classification_pass = gpu::create_compute_pipeline("sssr_classification");
  trace_indirect_pass = gpu::create_compute_pipeline("sssr_trace_indirect");

  // xy: the reference's table; zw: cos / sin of 2 PI y evaluated on the host for the HIP trace kernel
  // (vkr_halton23_fill, include/vkr_postfx.h) — zero in the reference
  auto halton_samples = halton23_seq(HALTON_SEQ_SIZE);
  std::vector<float> filled(4 * HALTON_SEQ_SIZE);
  vkr_halton23_fill(filled.data(), HALTON_SEQ_SIZE);
  for (uint32_t i = 0; i < HALTON_SEQ_SIZE; i++) {
    if (filled[4 * i] != halton_samples[i].x || filled[4 * i + 1] != halton_samples[i].y)
      throw std::runtime_error {"Halton table mismatch between host pass and C-ABI helper"};
    halton_samples[i].z = filled[4 * i + 2];
    halton_samples[i].w = filled[4 * i + 3];
  }
  const uint64_t bytes = sizeof(halton_samples[0]) * HALTON_SEQ_SIZE;
  halton_buffer = gpu::create_buffer(VMA_MEMORY_USAGE_CPU_TO_GPU, bytes, VK_BUFFER_USAGE_UNIFORM_BUFFER_BIT);
  std::memcpy(halton_buffer->get_mapped_ptr(), halton_samples.data(), bytes);

  const auto usage = VK_IMAGE_USAGE_SAMPLED_BIT|VK_IMAGE_USAGE_STORAGE_BIT;
  rays = make_image(graph, VK_FORMAT_R16G16B16A16_UNORM, w/2, h/2, usage);
  rays_occlusion = make_image(graph, VK_FORMAT_R16_SFLOAT, w/2, h/2, usage);
  reflections = make_image(graph, VK_FORMAT_R8G8B8A8_UNORM, w/2, h/2, usage);
  blurred_reflection = make_image(graph, VK_FORMAT_R8G8B8A8_UNORM, w/2, h/2, usage);
  blurred_reflection_history = make_image(graph, VK_FORMAT_R8G8B8A8_UNORM, w/2, h/2, usage);
  preintegrated_pdf = make_image(graph, VK_FORMAT_R32_SFLOAT, 1024, 1024, usage);
  preintegrated_brdf = make_image(graph, VK_FORMAT_R16G16_SFLOAT, 1024, 1024, usage);
  sampler = default_sampler();

  // :77-83: indirect arguments and one tile-index slot per 8x8 block of the full-res frame
  const auto indirect_usage = VK_BUFFER_USAGE_STORAGE_BUFFER_BIT|VK_BUFFER_USAGE_INDIRECT_BUFFER_BIT|VK_BUFFER_USAGE_TRANSFER_DST_BIT;
  reflective_indirect = graph.create_buffer(VMA_MEMORY_USAGE_GPU_ONLY, sizeof(VkDispatchIndirectCommand), indirect_usage);
  glossy_indirect = graph.create_buffer(VMA_MEMORY_USAGE_GPU_ONLY, sizeof(VkDispatchIndirectCommand), indirect_usage);
  const uint64_t tile_bytes = sizeof(int) * std::max<uint64_t>(1, uint64_t(w) * h/64);
  reflective_tiles = graph.create_buffer(VMA_MEMORY_USAGE_GPU_ONLY, tile_bytes, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT);
  glossy_tiles = graph.create_buffer(VMA_MEMORY_USAGE_GPU_ONLY, tile_bytes, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT);
}
#endif

#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void AdvancedSSR::preintegrate_pdf(RenderGraph &graph) {  // :95-114
  rec::compute(graph, "SSR_preintegrate", preintegrate_pass, {rec::storage(0, preintegrated_pdf)}, rec::no_push(),
               rec::Grid {preintegrated_pdf, 8, 4, rec::Ceil});
}
#endif

#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void AdvancedSSR::preintegrate_brdf(RenderGraph &graph) {  // :116-136
  rec::compute(graph, "BRDF_preintegrate", preintegrate_brdf_pass,
               {rec::uniform_buffer(0, halton_buffer), rec::storage(1, preintegrated_brdf)}, rec::no_push(),
               rec::Grid {preintegrated_brdf, 8, 4, rec::Ceil});
}
#endif

// TraceParams (:138-145) with the frame counter, which cycles modulo max_accumulated_rays (:168-171)
static vkr_trace_params trace_params(const AdvancedSSRParams &p, uint32_t counter) {
  vkr_trace_params t;
  copy_mat(t.normal_mat, p.normal_mat);
  t.frame_random = counter;
  t.fovy = p.fovy; t.aspect = p.aspect; t.znear = p.znear; t.zfar = p.zfar;
  return t;
}

void AdvancedSSR::advance_counter() {
  if (settings.update_random) counter = (counter + 1) % uint32_t(settings.max_accumulated_rays);
}

// :147-214.  Single GPU: the march reads image mips 1..L-1 of gbuff.depth (:186); tiled: the gathered
// whole-frame pyramid and normals.
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void AdvancedSSR::run_trace_pass(RenderGraph &graph, const AdvancedSSRParams &params, const Gbuffer &gbuff, ImageResourceId ssr_occlusion) {
  const vkr_trace_params config = trace_params(params, counter);
  const vkr_trace_push pc {settings.max_rougness};
  advance_counter();
  const auto hiz = gbuff.tiled? gbuff.frame_hiz : gbuff.depth;
  const uint32_t mips = graph.get_descriptor(hiz).mip_levels;
  if (gbuff.tiled && gbuff.normals_by_request) {  // multi-GPU: the hit-normal test of rays that end on another rank's rows is deferred
    if (!trace_windowed_pass.has_program()) trace_windowed_pass = gpu::create_compute_pipeline("sssr_trace_windowed");
    const vkr_trace_window_push wpc {settings.max_rougness, gbuff.normal_row0, gbuff.normal_row1};
    rec::compute(graph, "SSSR_trace", trace_windowed_pass,
      {rec::sampled_mips(0, hiz, sampler, DEPTH, 0, mips), rec::sampled(1, gbuff.frame_normals, sampler), rec::sampled(2, gbuff.material, sampler),
       rec::uniform(3, config), rec::uniform_buffer(4, halton_buffer), rec::storage(5, rays), rec::storage(6, ssr_occlusion),
       rec::sampled(7, preintegrated_pdf, sampler), rec::storage(8, gbuff.pend_mask), rec::storage(9, gbuff.pend_data)},
      rec::push(wpc), rec::Grid {rays, 8, 8, rec::Ceil});
    return;
  }
  rec::compute(graph, "SSSR_trace", trace_pass,
    {gbuff.tiled? rec::sampled_mips(0, hiz, sampler, DEPTH, 0, mips) : rec::sampled_mips(0, hiz, sampler, DEPTH, 1, mips - 1),
     rec::sampled(1, gbuff.tiled? gbuff.frame_normals : gbuff.downsampled_normals, sampler), rec::sampled(2, gbuff.material, sampler),
     rec::uniform(3, config), rec::uniform_buffer(4, halton_buffer), rec::storage(5, rays), rec::storage(6, ssr_occlusion),
     rec::sampled(7, preintegrated_pdf, sampler)},
    rec::push(pc), rec::Grid {rays, 8, 8, rec::Ceil});
}
#endif

// :308-369; flags :331-338; depth view = mips 0..9 (:342); tiled: the hit colour comes from the whole-frame albedo
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void AdvancedSSR::run_filter_pass(RenderGraph &graph, const AdvancedSSRParams &params, const Gbuffer &gbuff) {
  const vkr_trace_params config = trace_params(params, counter);
  vkr_filter_push pc {0u};
  if (settings.normalize_reflections) pc.render_flags |= NORMALIZE_REFLECTIONS;
  if (settings.accumulate_reflections) pc.render_flags |= ACCUMULATE_REFLECTIONS;
  if (settings.bilateral_filter) pc.render_flags |= BILATERAL_FILTER;
  const uint32_t depth_mips = std::min(10u, graph.get_descriptor(gbuff.depth).mip_levels);
  rec::compute(graph, "SSSR_filter", filter_pass,
    {rec::sampled(0, rays, sampler), rec::sampled_mips(1, gbuff.depth, sampler, DEPTH, 0, depth_mips),
     rec::sampled(2, gbuff.tiled? gbuff.frame_albedo : gbuff.albedo, sampler), rec::sampled(3, gbuff.normal, sampler),
     rec::sampled(4, gbuff.material, sampler), rec::storage(5, reflections), rec::uniform(6, config)},
    rec::push(pc), rec::Grid {reflections, 8, 8, rec::Ceil});
}
#endif

// :371-438
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void AdvancedSSR::run_blur_pass(RenderGraph &graph, const AdvancedSSRParams &, const DrawTAAParams &taa_params, const Gbuffer &gbuff) {
  const vkr_blur_push pc {settings.max_rougness, settings.accumulate_reflections? 1u : 0u, settings.use_blur? 0u : 1u};
  const uint32_t depth_mips = std::min(10u, graph.get_descriptor(gbuff.depth).mip_levels);
  rec::compute(graph, "SSSR_blur", blur_pass,
    {rec::sampled_mips(0, gbuff.depth, sampler, DEPTH, 0, depth_mips), rec::sampled(1, gbuff.normal, sampler), rec::sampled(2, reflections, sampler),
     rec::sampled(3, gbuff.material, sampler), rec::sampled(4, blurred_reflection_history, sampler),
     rec::sampled(5, gbuff.downsampled_velocity_vectors, sampler), rec::sampled_mips(6, gbuff.prev_depth, sampler, DEPTH, 0, depth_mips),
     rec::storage(7, blurred_reflection), rec::uniform(8, reproject_params(taa_params))},
    rec::push(pc), rec::Grid {blurred_reflection, 8, 8, rec::Ceil});
}
#endif

// :440-452: VkDispatchIndirectCommand{0, 1, 1} into both argument buffers
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void AdvancedSSR::clear_indirect_params(RenderGraph &graph) {
  struct Nothing {};
  const auto a = reflective_indirect, b = glossy_indirect;
  graph.add_task<Nothing>("SSSR_Clear",
    [&](Nothing &, rendergraph::RenderGraphBuilder &builder) {
      builder.transfer_write(a);
      builder.transfer_write(b);
    },
    [=](Nothing &, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) {
      const VkDispatchIndirectCommand none {0, 1, 1};
      cmd.update_buffer(resources.get_buffer(a)->api_buffer(), 0, none);
      cmd.update_buffer(resources.get_buffer(b)->api_buffer(), 0, none);
    });
}
#endif

// :454-495
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void AdvancedSSR::run_classification_pass(RenderGraph &graph, const AdvancedSSRParams &, const Gbuffer &gbuff) {
  const auto extent = graph.get_descriptor(rays).extent2D();
  const vkr_classification_push pc {int(extent.width), int(extent.height), settings.max_rougness, settings.glossy_roughness_value};
  rec::compute(graph, "SSSR_Classification", classification_pass,
    {rec::sampled(0, gbuff.material, sampler), rec::storage_buffer(1, reflective_tiles, false), rec::storage_buffer(2, glossy_tiles, false),
     rec::storage_buffer(3, reflective_indirect, false), rec::storage_buffer(4, glossy_indirect, false)},
    rec::push(pc), rec::Grid {rays, 8, 8, rec::Ceil});
}
#endif

// :216-302: two indirect dispatches of one program, mirror tiles (reflection_type 0) then glossy tiles (1)
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void AdvancedSSR::run_trace_indirect_pass(RenderGraph &graph, const AdvancedSSRParams &params, const Gbuffer &gbuff) {
  const vkr_trace_params config = trace_params(params, counter);
  const float max_roughness = settings.max_rougness;
  advance_counter();
  const auto hiz = gbuff.tiled? gbuff.frame_hiz : gbuff.depth;
  const uint32_t mips = graph.get_descriptor(hiz).mip_levels;
  const std::vector<rec::Binding> common {
    gbuff.tiled? rec::sampled_mips(0, hiz, sampler, DEPTH, 0, mips) : rec::sampled_mips(0, hiz, sampler, DEPTH, 1, mips - 1),
    rec::sampled(1, gbuff.tiled? gbuff.frame_normals : gbuff.downsampled_normals, sampler), rec::sampled(2, gbuff.material, sampler),
    rec::uniform(3, config), rec::uniform_buffer(4, halton_buffer), rec::storage(5, rays)};
  const rendergraph::BufferResourceId lists[2] {reflective_tiles, glossy_tiles}, arguments[2] {reflective_indirect, glossy_indirect};
  const auto pipeline = trace_indirect_pass;

  struct Data { std::vector<rec::Bound> bound; };
  graph.add_task<Data>("SSSR_trace",
    [&](Data &d, rendergraph::RenderGraphBuilder &builder) {
      d.bound = rec::declare(common, builder, VK_SHADER_STAGE_COMPUTE_BIT);
      for (int k = 0; k < 2; k++) {
        builder.use_indirect_buffer(arguments[k]);
        builder.use_storage_buffer(lists[k], VK_SHADER_STAGE_COMPUTE_BIT);
      }
    },
    [=](Data &d, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) {
      cmd.bind_pipeline(pipeline);
      for (uint32_t kind = 0; kind < 2; kind++) {
        VkDescriptorSet set = rec::write(d.bound, resources, cmd);
        gpu::write_set(set, gpu::SSBOBinding {6, resources.get_buffer(lists[kind])});
        const vkr_trace_indirect_push pc {kind, max_roughness};
        cmd.bind_descriptors_compute(0, {set});
        cmd.push_constants_compute(0, sizeof(pc), &pc);
        cmd.dispatch_indirect(resources.get_buffer(arguments[kind])->api_buffer());
      }
    });
}
#endif

void AdvancedSSR::run_trace(RenderGraph &graph, const AdvancedSSRParams &params, const Gbuffer &gbuff, ImageResourceId ssr_occlusion) {
  if (settings.use_tile_classification) {  // the path advanced_ssr.cpp:547-550 keeps commented out
    clear_indirect_params(graph);
    run_classification_pass(graph, params, gbuff);
    run_trace_indirect_pass(graph, params, gbuff);
  } else {
    run_trace_pass(graph, params, gbuff, ssr_occlusion);
  }
}

void AdvancedSSR::run_trace_head(RenderGraph &graph, const AdvancedSSRParams &params, const Gbuffer &gbuff, ImageResourceId ssr_occlusion, uint32_t local_levels) {
  if (!gbuff.tiled || !gbuff.normals_by_request) throw std::runtime_error {"run_trace_head: only the tiled frame with hit normals by request traces in two tasks"};
  if (settings.use_tile_classification) throw std::runtime_error {"run_trace_head: not with tile classification"};
  head_config = trace_params(params, counter);
  advance_counter();
  if (!trace_head_pass.has_program()) trace_head_pass = gpu::create_compute_pipeline("sssr_trace_windowed_head");
  const uint32_t mips = graph.get_descriptor(gbuff.frame_hiz).mip_levels;
  const vkr_trace_window_push wpc {settings.max_rougness, gbuff.normal_row0, gbuff.normal_row1};
  rec::compute(graph, "SSSR_trace", trace_head_pass,
    {rec::sampled_mips(0, gbuff.depth, sampler, DEPTH, 1, local_levels), rec::sampled(1, gbuff.frame_normals, sampler), rec::sampled(2, gbuff.material, sampler),
     rec::uniform(3, head_config), rec::uniform_buffer(4, halton_buffer), rec::storage(5, rays), rec::storage(6, ssr_occlusion),
     rec::sampled(7, preintegrated_pdf, sampler), rec::storage(8, gbuff.pend_mask), rec::storage(9, gbuff.pend_data),
     rec::sampled_mips(10, gbuff.frame_hiz, sampler, DEPTH, 0, mips)},  // extents and level count only: its rows are still arriving
    rec::push(wpc), rec::Grid {rays, 8, 8, rec::Ceil});
}

void AdvancedSSR::run_trace_resume(RenderGraph &graph, const Gbuffer &gbuff, ImageResourceId ssr_occlusion) {
  if (!trace_resume_pass.has_program()) trace_resume_pass = gpu::create_compute_pipeline("sssr_trace_windowed_resume");
  const uint32_t mips = graph.get_descriptor(gbuff.frame_hiz).mip_levels;
  const vkr_trace_window_push wpc {settings.max_rougness, gbuff.normal_row0, gbuff.normal_row1};
  rec::compute(graph, "SSSR_trace_resume", trace_resume_pass,
    {rec::sampled_mips(0, gbuff.frame_hiz, sampler, DEPTH, 0, mips), rec::sampled(1, gbuff.frame_normals, sampler), rec::sampled(2, gbuff.material, sampler),
     rec::uniform(3, head_config), rec::uniform_buffer(4, halton_buffer), rec::storage(5, rays), rec::storage(6, ssr_occlusion),
     rec::sampled(7, preintegrated_pdf, sampler), rec::storage(8, gbuff.pend_mask), rec::storage(9, gbuff.pend_data)},
    rec::push(wpc), rec::Grid {rays, 8, 8, rec::Ceil});
}

void AdvancedSSR::run_resolve(RenderGraph &graph, const AdvancedSSRParams &params, const DrawTAAParams &taa_params, const Gbuffer &gbuff) {
  run_filter_pass(graph, params, gbuff);
  run_blur_pass(graph, params, taa_params, gbuff);
}

#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void AdvancedSSR::run(RenderGraph &graph, const AdvancedSSRParams &params, const DrawTAAParams &taa_params, const Gbuffer &gbuff,
  ImageResourceId ssr_occlusion)
{
  run_trace(graph, params, gbuff, ssr_occlusion);  // :540-554
  run_resolve(graph, params, taa_params, gbuff);
}
#endif

// ==== TAA (taa.cpp) ========================================================================================
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
TAA::TAA(RenderGraph &graph, uint32_t w, uint32_t h) {  // :3-12
  pipeline = gpu::create_compute_pipeline("taa_resolve");
  const auto usage = VK_IMAGE_USAGE_SAMPLED_BIT|VK_IMAGE_USAGE_STORAGE_BIT|VK_IMAGE_USAGE_TRANSFER_SRC_BIT;
  history = make_image(graph, VK_FORMAT_R16G16B16A16_SFLOAT, w, h, usage);
  target = make_image(graph, VK_FORMAT_R16G16B16A16_SFLOAT, w, h, usage);
  sampler = default_sampler();
}
#endif

#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void TAA::run(RenderGraph &graph, const Gbuffer &gbuffer, ImageResourceId color, const DrawTAAParams &params) {  // :19-63
  rec::compute(graph, "TAA", pipeline,
    {rec::sampled(0, history, sampler), rec::sampled(1, gbuffer.prev_depth, sampler, DEPTH), rec::sampled(2, gbuffer.depth, sampler, DEPTH),
     rec::sampled(3, gbuffer.velocity_vectors, sampler), rec::sampled(4, color, sampler), rec::storage(5, target),
     rec::uniform(6, reproject_params(params))},
    rec::no_push(), rec::Grid {target, 8, 8, rec::Ceil});
}
#endif

#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void TAA::remap_targets(RenderGraph &graph) { graph.remap(history, target); }  // :65-67

// ==== simple SSR (ssr.cpp) =====================================================================================
ImageResourceId create_ssr_tex(RenderGraph &graph, uint32_t w, uint32_t h) {  // :5-8
  return make_image(graph, VK_FORMAT_R8G8B8A8_UNORM, w, h, VK_IMAGE_USAGE_COLOR_ATTACHMENT_BIT|VK_IMAGE_USAGE_SAMPLED_BIT|VK_IMAGE_USAGE_STORAGE_BIT);
}
#endif

// :10-73.  Depth is read through a NEAREST sampler with U / W clamp-to-border (:21-28).
void add_ssr_pass(RenderGraph &graph, ImageResourceId depth, ImageResourceId normal, ImageResourceId color, ImageResourceId material,
  ImageResourceId out, const SSRParams &params)
{
  static_assert(sizeof(SSRParams) == sizeof(vkr_ssr_params), "SSRParams must match the C-ABI");
  auto nearest = gpu::DEFAULT_SAMPLER;
  nearest.minFilter = nearest.magFilter = VK_FILTER_NEAREST;
  nearest.mipmapMode = VK_SAMPLER_MIPMAP_MODE_NEAREST;
  nearest.addressModeU = nearest.addressModeW = VK_SAMPLER_ADDRESS_MODE_CLAMP_TO_BORDER;
  const auto sampler = default_sampler();
  auto pipeline = fullscreen_pipeline("ssr");
  pipeline.set_rendersubpass({false, {graph.get_descriptor(out).format}});
  const auto ext = graph.get_descriptor(out);
  rec::fullscreen(graph, "SSR", pipeline,
    {rec::sampled(0, normal, sampler), rec::sampled(1, depth, gpu::create_sampler(nearest), DEPTH), rec::sampled(2, color, sampler),
     rec::uniform(3, params), rec::sampled(4, material, sampler), rec::color_target(out)},
    rec::no_push(), ext.width, ext.height);
}

// ==== ScreenSpaceTrace (screen_trace.cpp) ========================================================================
ScreenSpaceTrace::ScreenSpaceTrace(RenderGraph &graph, uint32_t width, uint32_t height) {  // :3-21
  const auto usage = VK_IMAGE_USAGE_STORAGE_BIT|VK_IMAGE_USAGE_SAMPLED_BIT;
  raw = make_image(graph, VK_FORMAT_R16G16B16A16_SFLOAT, width, height, usage);
  filtered = make_image(graph, VK_FORMAT_R16G16B16A16_SFLOAT, width, height, usage);
  accumulated = make_image(graph, VK_FORMAT_R16G16B16A16_SFLOAT, width, height, usage);
  trace_pipeline = gpu::create_compute_pipeline("screen_trace_main");
  filter_pipeline = gpu::create_compute_pipeline("screen_trace_filter");
  accum_pipeline = gpu::create_compute_pipeline("screen_trace_accumulate");
  sampler = default_sampler();
}

// :23-95; angle table + jitter and random_offset drawn per frame, always in this order (:47-53); dispatch w/8 x h/8
void ScreenSpaceTrace::add_main_pass(RenderGraph &graph, const ScreenTraceParams &params, ImageResourceId depth, ImageResourceId normal,
  ImageResourceId color, ImageResourceId material)
{
  static const float table[12] {60.f, 300.f, 180.f, 240.f, 120.f, 0.f, 300.f, 60.f, 180.f, 120.f, 240.f, 0.f};
  const float drawn_jitter = random_floats(generator) - 0.5f;
  const float drawn_offset = random_floats(generator);
  vkr_screen_trace_params ubo {};
  copy_mat(ubo.normal_mat, params.normal_mat);
  ubo.angle_offset = table[frame_count++ % 12]/360.f + (std::isnan(pinned_jitter)? drawn_jitter : pinned_jitter);
  ubo.random_offset = std::isnan(pinned_offset)? drawn_offset : pinned_offset;
  ubo.fovy = params.fovy; ubo.aspect = params.aspect; ubo.znear = params.znear; ubo.zfar = params.zfar;
  rec::compute(graph, "ScreenTrace", trace_pipeline,
    {rec::sampled_mips(0, depth, sampler, DEPTH, 0, 1), rec::sampled(1, normal, sampler), rec::sampled(2, color, sampler),
     rec::sampled(3, material, sampler), rec::storage(4, raw), rec::uniform(5, ubo)},
    rec::no_push(), rec::Grid {raw, 8, 8, rec::Floor});
}

void ScreenSpaceTrace::add_filter_pass(RenderGraph &graph, const ScreenTraceParams &params, ImageResourceId depth) {  // :97-140
  const vkr_screen_trace_filter_push pc {params.znear, params.zfar};
  rec::compute(graph, "ScreenTraceFilter", filter_pipeline,
    {rec::sampled(0, raw, sampler), rec::sampled_mips(1, depth, sampler, DEPTH, 0, 1), rec::storage(2, filtered)},
    rec::push(pc), rec::Grid {filtered, 8, 4, rec::Floor});
}

void ScreenSpaceTrace::add_accumulate_pass(RenderGraph &graph, const ScreenTraceParams &params, ImageResourceId depth, ImageResourceId prev_depth) {  // :142-181
  const vkr_screen_trace_accum_push pc {params.fovy, params.aspect, params.znear, params.zfar};
  rec::compute(graph, "ScreenTraceAccumulate", accum_pipeline,
    {rec::sampled_mips(0, depth, sampler, DEPTH, 0, 1), rec::sampled_mips(1, prev_depth, sampler, DEPTH, 0, 1), rec::sampled(2, filtered, sampler),
     rec::storage(3, accumulated)},
    rec::push(pc), rec::Grid {accumulated, 8, 4, rec::Floor});
}

// ==== DeferedShadingPass (defered_shading.cpp) ======================================================================
// advanced_ssr.cpp:508-519: the push constants of "tile_regression"
vkr_tile_regression_push AdvancedSSR::tile_regression_push(const AdvancedSSRParams &params) {
  vkr_tile_regression_push pc;
  copy_mat(pc.camera_to_world, glm::transpose(params.normal_mat));
  pc.fovy = params.fovy; pc.aspect = params.aspect; pc.znear = params.znear; pc.zfar = params.zfar;
  return pc;
}

// advanced_ssr.cpp:497-538: task "SSSR_Tile_Regression"; depth mip 1 sampled, tile_planes stored, ceil((w/2)/8) x ceil((h/2)/8)
// groups (rays has the half-resolution extent the reference divides out of the depth's).  tile_planes is (w/16, h/16) RGBA32F
// (:85-86), allocated here on first use instead of in the constructor: frames that never run the pass keep their allocations.
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void AdvancedSSR::run_tile_regression_pass(RenderGraph &graph, const AdvancedSSRParams &params, const Gbuffer &gbuff) {
  if (tile_planes == ImageResourceId {}) {
    const auto full = graph.get_descriptor(gbuff.depth).extent2D();
    if (full.width < 16 || full.height < 16)
      throw std::runtime_error {"AdvancedSSR::run_tile_regression_pass: a " + std::to_string(full.width) + "x" + std::to_string(full.height) +
                                " frame has no (w/16, h/16) tile image"};
    tile_planes = make_image(graph, VK_FORMAT_R32G32B32A32_SFLOAT, full.width/16, full.height/16, VK_IMAGE_USAGE_SAMPLED_BIT|VK_IMAGE_USAGE_STORAGE_BIT);
  }
  if (!tile_regression.has_program()) tile_regression = gpu::create_compute_pipeline("tile_regression");
  rec::compute(graph, "SSSR_Tile_Regression", tile_regression,
    {rec::sampled_mips(0, gbuff.depth, sampler, DEPTH, 1, 1), rec::storage(1, tile_planes)},
    rec::push(tile_regression_push(params)), rec::Grid {rays, 8, 8, rec::Ceil});
}
#endif

// ---- ray-traced reflections (no reference counterpart) ----
vkr_reflect_rt_params AdvancedSSR::reflect_rt_params(const AdvancedSSRParams &params, const RtSettings &rt) {
  vkr_reflect_rt_params p {};
  copy_mat(p.inverse_camera, glm::transpose(params.normal_mat));  // normal_mat = transpose(inverse(view))
  p.fovy = params.fovy; p.aspect = params.aspect; p.znear = params.znear; p.zfar = params.zfar;
  p.normal_offset = rt.normal_offset; p.tmin = rt.tmin; p.max_distance = rt.max_distance; p.texture_lod = rt.texture_lod;
  p.flags = rt.fill_misses? VKR_REFLECT_RT_FILL_MISSES : 0u;
  return p;
}

// task "ReflectionsRT": set {0 depth (mip 1 of the image: mip 0 of the view), 1 the half-resolution normals, 2 rays (only with
// fill_misses), 3 the acceleration structure, 4 its attribute table, 5 the block, 6 reflections (storage), 7 the scene's textures[]},
// one 16 x 16 group (four waves of 8 x 8 pixels) per 16 x 16 pixels of reflections.  Written out instead of rec::compute because of
// the array of images, which is no graph resource (as in ProbeRenderer's cube pass).  Task "ReflectionsRTLit" (lights.enable): the
// same set, 9 the normal table and 10 the lights: on that set the two programs record the lit entries (gpu/gpu.cpp)
void AdvancedSSR::run_reflections_rt_pass(RenderGraph &graph, const AdvancedSSRParams &params, const Gbuffer &gbuff, const RtScene &scene,
  const RtSettings &rt, const RtCutouts &cutouts, const RtLights &lights)
{
  if (!scene.tlas)
    throw std::runtime_error {"AdvancedSSR::run_reflections_rt_pass: null acceleration structure (tlas): build scene::SceneAccelerationStructure first"};
  if (!scene.hit_attributes)
    throw std::runtime_error {"AdvancedSSR::run_reflections_rt_pass: no attribute table: build scene::SceneAccelerationStructure first"};
  if (gbuff.tiled)
    throw std::runtime_error {"AdvancedSSR::run_reflections_rt_pass: on a window of the frame (the rays reach anywhere: a single-GPU pass)"};
  if (lights.enable && !scene.hit_normals)
    throw std::runtime_error {"AdvancedSSR::run_reflections_rt_pass: no normal table: build scene::SceneAccelerationStructure first"};
  if (!reflections_rt_pass.has_program()) reflections_rt_pass = gpu::create_compute_pipeline("reflections_rt");
  std::vector<rec::Binding> bindings {rec::sampled_mips(0, gbuff.depth, sampler, DEPTH, 1, 1), rec::sampled(1, gbuff.downsampled_normals, sampler)};
  if (rt.fill_misses) bindings.push_back(rec::sampled(2, rays, sampler));
  bindings.insert(bindings.end(), {rec::accel(3, scene.tlas), rec::uniform_buffer(4, scene.hit_attributes), rec::uniform(5, reflect_rt_params(params, rt)),
                                   rec::storage(6, reflections)});
  if (cutouts.enable) {  // the same set and the cutout block; the program adds the mask of the textures that cannot make a hole
    if (!reflections_rt_cutout_pass.has_program()) reflections_rt_cutout_pass = gpu::create_compute_pipeline("reflections_rt_cutout");
    bindings.push_back(rec::uniform(8, vkr_ray_cutout {cutouts.alpha_lod, 0u}));
  }
  if (lights.enable) bindings.insert(bindings.end(), {rec::uniform_buffer(9, scene.hit_normals), rec::uniform(10, lights.block)});
  struct Data { std::vector<rec::Bound> bound; };
  const auto pipeline = cutouts.enable ? reflections_rt_cutout_pass : reflections_rt_pass;
  const auto textures = scene.textures;
  const auto sized_by = reflections;
  graph.add_task<Data>(lights.enable ? "ReflectionsRTLit" : "ReflectionsRT",
    [&](Data &d, rendergraph::RenderGraphBuilder &builder) { d.bound = rec::declare(bindings, builder, VK_SHADER_STAGE_COMPUTE_BIT); },
    [=](Data &d, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) {
      VkDescriptorSet set = rec::write(d.bound, resources, cmd);
      gpu::write_set(set, gpu::ArrayOfImagesBinding {7, textures});
      cmd.bind_pipeline(pipeline);
      cmd.bind_descriptors_compute(0, {set});
      const auto extent = resources.get_image(sized_by)->get_extent();
      cmd.dispatch((extent.width + 15)/16, (extent.height + 15)/16, 1);
    });
}

void AdvancedSSR::run_rt(RenderGraph &graph, const AdvancedSSRParams &params, const DrawTAAParams &taa_params, const Gbuffer &gbuff,
  ImageResourceId ssr_occlusion, const RtScene &scene, const RtSettings &rt, const RtCutouts &cutouts, const RtLights &lights)
{
  if (rt.fill_misses) {
    run_trace(graph, params, gbuff, ssr_occlusion);
    run_filter_pass(graph, params, gbuff);
  }
  run_reflections_rt_pass(graph, params, gbuff, scene, rt, cutouts, lights);
  run_blur_pass(graph, params, taa_params, gbuff);
}

// advanced_ssr.cpp:556-567
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void AdvancedSSR::render_ui() {
  ImGui::Begin("SSSR");
  ImGui::SliderFloat("Max Roughness", &settings.max_rougness, 0.f, 1.f);
  ImGui::SliderFloat("Min glossy roughness", &settings.glossy_roughness_value, 0.f, 1.f);
  ImGui::SliderInt("Temporal rays", &settings.max_accumulated_rays, 1, 128);
  ImGui::Checkbox("Enable normalization", &settings.normalize_reflections);
  ImGui::Checkbox("Enable accumulation", &settings.accumulate_reflections);
  ImGui::Checkbox("Enable random rays", &settings.update_random);
  ImGui::Checkbox("Enable blur", &settings.use_blur);
  ImGui::Checkbox("Enable bilateral filter", &settings.bilateral_filter);
  ImGui::End();
}
#endif

// defered_shading.cpp:120-126
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void DeferedShadingPass::draw_ui() {
  ImGui::Begin("DeferedShading");
  ImGui::SliderFloat("Max Roughness", &min_max_roughness.y, min_max_roughness.x, 1.f);
  ImGui::SliderFloat("Min Roughness", &min_max_roughness.x, 0.f, min_max_roughness.y);
  ImGui::Checkbox("Show AO only", &only_ao);
  ImGui::End();
}
#endif

#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
DeferedShadingPass::DeferedShadingPass(RenderGraph &graph, SDL_Window *) {  // :14-31
  pipeline = fullscreen_pipeline("defered_shading");
  sampler = default_sampler();
  ubo_consts = graph.create_buffer(VMA_MEMORY_USAGE_GPU_ONLY, sizeof(vkr_shading_params), VK_BUFFER_USAGE_TRANSFER_DST_BIT|VK_BUFFER_USAGE_UNIFORM_BUFFER_BIT);
  graph_ref = &graph;
}
#endif

// :33-45: ShaderConstants {inverse(camera), camera, shadow_mvp, fovy, aspect, znear, zfar} written into the constant
// buffer (gpu_transfer::write_buffer in the reference; here the buffer keeps a host shadow the program reads)
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void DeferedShadingPass::update_params(const glm::mat4 &camera, const glm::mat4 &shadow, float fovy, float aspect, float znear, float zfar) {
  vkr_shading_params consts;
  copy_mat(consts.inverse_camera, glm::inverse(camera));
  copy_mat(consts.camera, camera);
  copy_mat(consts.shadow_mvp, shadow);
  consts.fovy = fovy; consts.aspect = aspect; consts.znear = znear; consts.zfar = zfar;
  std::memcpy(graph_ref->get_buffer(ubo_consts)->get_mapped_ptr(), &consts, sizeof(consts));
}
#endif

// :47-118.  Bindings 0-8 (:93-102); the shadow map (binding 5) is bound by the reference but never read by the
// shader, so it may be left out; push constants {vec2 min_max_roughness, uint show_ao} (:68-72).
#ifndef VKR_REFERENCE_PASSES  // defined by the reference's own source in the drop-in build (Makefile: refpasses)
void DeferedShadingPass::draw(RenderGraph &graph, const Gbuffer &gbuffer, ImageResourceId shadow, ImageResourceId ssao, ImageResourceId brdf_tex,
  ImageResourceId reflections, ImageResourceId out_image)
{
  vkr_shading_push pc {{min_max_roughness.x, min_max_roughness.y}, only_ao? 1u : 0u};
  pipeline.set_rendersubpass({false, {graph.get_descriptor(out_image).format}});
  std::vector<rec::Binding> binds {
    rec::sampled(0, gbuffer.albedo, sampler), rec::sampled(1, gbuffer.normal, sampler), rec::sampled(2, gbuffer.material, sampler),
    rec::sampled(3, gbuffer.depth, sampler, DEPTH), rec::uniform_buffer(4, ubo_consts), rec::sampled(6, ssao, sampler),
    rec::sampled(7, brdf_tex, sampler), rec::sampled(8, reflections, sampler), rec::color_target(out_image)};
  if (shadow.get_index() != ~0u) binds.push_back(rec::sampled_mips(5, shadow, sampler, DEPTH, 0, 1));
  const auto ext = graph.get_descriptor(out_image);
  rec::fullscreen(graph, "DeferedShading", pipeline, binds, rec::push(pc), ext.width, ext.height);
}
#endif

// draw() with the shadow mask at binding 9, through program "defered_shading_shadowed" (no reference counterpart, so it is part
// of both builds of the mirror)
void DeferedShadingPass::draw_shadowed(RenderGraph &graph, const Gbuffer &gbuffer, ImageResourceId shadow, ImageResourceId ssao, ImageResourceId brdf_tex,
  ImageResourceId reflections, ImageResourceId mask, ImageResourceId out_image)
{
  if (!shadowed_pipeline.has_program()) shadowed_pipeline = fullscreen_pipeline("defered_shading_shadowed");
  vkr_shading_push pc {{min_max_roughness.x, min_max_roughness.y}, only_ao? 1u : 0u};
  shadowed_pipeline.set_rendersubpass({false, {graph.get_descriptor(out_image).format}});
  std::vector<rec::Binding> binds {
    rec::sampled(0, gbuffer.albedo, sampler), rec::sampled(1, gbuffer.normal, sampler), rec::sampled(2, gbuffer.material, sampler),
    rec::sampled(3, gbuffer.depth, sampler, DEPTH), rec::uniform_buffer(4, ubo_consts), rec::sampled(6, ssao, sampler),
    rec::sampled(7, brdf_tex, sampler), rec::sampled(8, reflections, sampler), rec::sampled(9, mask, sampler), rec::color_target(out_image)};
  if (shadow.get_index() != ~0u) binds.push_back(rec::sampled_mips(5, shadow, sampler, DEPTH, 0, 1));
  const auto ext = graph.get_descriptor(out_image);
  rec::fullscreen(graph, "DeferedShading", shadowed_pipeline, binds, rec::push(pc), ext.width, ext.height);
}

// ==== ShadowMaskPass (shadow_mask.hpp) ===============================================================================
ImageResourceId create_shadow_mask_texture(RenderGraph &graph, uint32_t width, uint32_t height) {
  return make_image(graph, VK_FORMAT_R8G8B8A8_UNORM, width, height, VK_IMAGE_USAGE_STORAGE_BIT|VK_IMAGE_USAGE_SAMPLED_BIT);
}

ShadowHistoryTextures create_shadow_history_textures(RenderGraph &graph, uint32_t width, uint32_t height) {
  const VkImageUsageFlags usage = VK_IMAGE_USAGE_STORAGE_BIT|VK_IMAGE_USAGE_SAMPLED_BIT|VK_IMAGE_USAGE_TRANSFER_DST_BIT;
  ShadowHistoryTextures t;
  t.history = make_image(graph, VK_FORMAT_R16G16B16A16_UNORM, width, height, usage);
  t.out_history = make_image(graph, VK_FORMAT_R16G16B16A16_UNORM, width, height, usage);
  t.count = make_image(graph, VK_FORMAT_R8_UNORM, width, height, usage);
  t.out_count = make_image(graph, VK_FORMAT_R8_UNORM, width, height, usage);
  t.accumulated = create_shadow_mask_texture(graph, width, height);
  return t;
}

ShadowMaskPass::ShadowMaskPass() {
  pipeline = gpu::create_compute_pipeline("shadow_mask");
  sampler = default_sampler();
}

void ShadowMaskPass::update_params(const glm::mat4 &camera, const glm::mat4 *mvps, uint32_t count, float fovy, float aspect, float znear, float zfar,
  uint32_t radius, uint32_t bias)
{
  if (!mvps || count < 1 || count > 4) throw std::runtime_error {"ShadowMaskPass::update_params: " + std::to_string(count) + " lights, needs 1..4"};
  params = vkr_shadow_mask_params {};
  copy_mat(params.inverse_camera, glm::inverse(camera));
  for (uint32_t l = 0; l < count; l++) copy_mat(params.mvps[l], mvps[l]);
  params.fovy = fovy; params.aspect = aspect; params.znear = znear; params.zfar = zfar;
  params.layer_count = count; params.radius = radius; params.bias = bias;
  camera_is_rt = false;
}

// task "ShadowMask": set {0 depth (mip 0), 1 the shadow array (every layer), 2 the block, 3 the mask (storage)}, one 16 x 16 group
// per 16 x 16 pixels
void ShadowMaskPass::run(RenderGraph &graph, ImageResourceId depth, ImageResourceId shadows, uint32_t layer_count, ImageResourceId out) {
  const auto maps = graph.get_descriptor(shadows);
  if (layer_count < 1 || layer_count > 4 || layer_count > std::max(1u, maps.array_layers))
    throw std::runtime_error {"ShadowMaskPass::run: " + std::to_string(layer_count) + " layers of a shadow map with " + std::to_string(std::max(1u, maps.array_layers))};
  if (maps.width != maps.height)
    throw std::runtime_error {"ShadowMaskPass::run: the shadow map is " + std::to_string(maps.width) + "x" + std::to_string(maps.height) + ", it must be square"};
  vkr_shadow_mask_params block = params;
  block.layer_count = layer_count;
  rec::compute(graph, "ShadowMask", pipeline,
    {rec::sampled_mips(0, depth, sampler, DEPTH, 0, 1), rec::sampled(1, shadows, sampler, DEPTH), rec::uniform(2, block), rec::storage(3, out)},
    rec::no_push(), rec::Grid {out, 16, 16, rec::Ceil});
}

void ShadowMaskPass::update_rt_params(const glm::mat4 &camera, const float *lights, uint32_t count, float fovy, float aspect, float znear,
  float zfar, float normal_offset, float tmin)
{
  if (!lights || count < 1 || count > 4) throw std::runtime_error {"ShadowMaskPass::update_rt_params: " + std::to_string(count) + " lights, needs 1..4"};
  rt_params = vkr_shadow_rt_params {};
  copy_mat(rt_params.inverse_camera, glm::inverse(camera));
  rt_params.fovy = fovy; rt_params.aspect = aspect; rt_params.znear = znear; rt_params.zfar = zfar;
  for (uint32_t l = 0; l < count; l++)
    for (int k = 0; k < 4; k++) rt_params.lights[l][k] = lights[4*l + k];
  rt_params.light_count = count; rt_params.normal_offset = normal_offset; rt_params.tmin = tmin;
  camera_is_rt = true;
}

void ShadowMaskPass::update_rt_soft(const float radius[4], uint32_t sample_count, uint32_t pattern_side) {
  if (!radius || sample_count < 1 || sample_count > 64 || (pattern_side != 1 && pattern_side != 2 && pattern_side != 4))
    throw std::runtime_error {"ShadowMaskPass::update_rt_soft: " + std::to_string(sample_count) + " samples in a pattern tile of side " +
                              std::to_string(pattern_side) + ", needs 1..64 and 1, 2 or 4"};
  rt_soft_frame_table = nullptr;  // update_rt_soft_frame chooses again
  for (int l = 0; l < 4; l++) {
    if (!(radius[l] >= 0.f) || std::isinf(radius[l])) throw std::runtime_error {"ShadowMaskPass::update_rt_soft: light " + std::to_string(l) + ": the radius must be finite and >= 0"};
    rt_soft.radius[l] = radius[l];
  }
  if (rt_soft_on() && (!rt_soft_table || rt_soft.sample_count != sample_count || rt_soft.pattern_side != pattern_side)) {
    rt_soft_table = gpu::create_buffer(VMA_MEMORY_USAGE_CPU_TO_GPU, sizeof(float) * 2 * sample_count * pattern_side * pattern_side, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT);
    vkr_shadow_disk_samples(sample_count, pattern_side, (float *)rt_soft_table->get_mapped_ptr());
    rt_soft.sample_count = sample_count; rt_soft.pattern_side = pattern_side;
  }
}

void ShadowMaskPass::update_rt_soft_frame(uint32_t frame, uint32_t frame_count) {
  if (frame_count < 1 || frame_count > 64) throw std::runtime_error {"ShadowMaskPass::update_rt_soft_frame: " + std::to_string(frame_count) + " frames, needs 1..64"};
  if (!rt_soft_on() || !rt_soft_table) return;  // the hard pass has no table
  const uint32_t S = rt_soft.sample_count, P = rt_soft.pattern_side;
  if (rt_soft_frames.size() != frame_count || rt_soft_frames_key[0] != S || rt_soft_frames_key[1] != P || rt_soft_frames_key[2] != frame_count) {
    // fresh buffers, never rewritten: a table an earlier submission may still read stays as it is
    rt_soft_frames.assign(frame_count, nullptr);
    for (uint32_t t = 0; t < frame_count; t++) {
      rt_soft_frames[t] = gpu::create_buffer(VMA_MEMORY_USAGE_CPU_TO_GPU, sizeof(float) * 2 * S * P * P, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT);
      vkr_shadow_disk_samples_frame(S, P, t, frame_count, (float *)rt_soft_frames[t]->get_mapped_ptr());
    }
    rt_soft_frames_key[0] = S; rt_soft_frames_key[1] = P; rt_soft_frames_key[2] = frame_count;
  }
  rt_soft_frame_table = rt_soft_frames[frame % frame_count];
}

// task "ShadowMaskRT": set {0 depth (mip 0), 1 normal, 2 the acceleration structure, 3 the block, 4 the mask (storage)} in the
// C-ABI's order, one 16 x 16 group (four waves of 8 x 8 pixels) per 16 x 16 pixels
void ShadowMaskPass::run_rt(RenderGraph &graph, ImageResourceId depth, ImageResourceId normal, VkAccelerationStructureKHR tlas, ImageResourceId out) {
  if (!tlas)
    throw std::runtime_error {"ShadowMaskPass::run_rt: null acceleration structure (tlas): build scene::SceneAccelerationStructure first"};
  if (rt_soft_on()) {  // set {0..4 as below, 5 the soft block, 6 the sample table}
    if (!rt_soft_pipeline.has_program()) rt_soft_pipeline = gpu::create_compute_pipeline("shadow_mask_rt_soft");
    rec::compute(graph, "ShadowMaskRTSoft", rt_soft_pipeline,
      {rec::sampled_mips(0, depth, sampler, DEPTH, 0, 1), rec::sampled(1, normal, sampler), rec::accel(2, tlas), rec::uniform(3, rt_params),
       rec::storage(4, out), rec::uniform(5, rt_soft), rec::uniform_buffer(6, bound_rt_soft_table())},
      rec::no_push(), rec::Grid {out, 16, 16, rec::Ceil});
    return;
  }
  if (!rt_pipeline.has_program()) rt_pipeline = gpu::create_compute_pipeline("shadow_mask_rt");
  rec::compute(graph, "ShadowMaskRT", rt_pipeline,
    {rec::sampled_mips(0, depth, sampler, DEPTH, 0, 1), rec::sampled(1, normal, sampler), rec::accel(2, tlas), rec::uniform(3, rt_params),
     rec::storage(4, out)},
    rec::no_push(), rec::Grid {out, 16, 16, rec::Ceil});
}

// the same task through program "shadow_mask_rt_cutout": set {0..4 as above, 5 the attribute table, 6 the cutout block, 7 the scene's
// textures[]}.  Written out instead of rec::compute because of the array of images (as AdvancedSSR::run_reflections_rt_pass)
void ShadowMaskPass::run_rt(RenderGraph &graph, ImageResourceId depth, ImageResourceId normal, const AdvancedSSR::RtScene &scene,
  const RtCutouts &cutouts, ImageResourceId out)
{
  if (!cutouts.enable) { run_rt(graph, depth, normal, scene.tlas, out); return; }
  if (!scene.tlas)
    throw std::runtime_error {"ShadowMaskPass::run_rt: null acceleration structure (tlas): build scene::SceneAccelerationStructure first"};
  if (!scene.hit_attributes)
    throw std::runtime_error {"ShadowMaskPass::run_rt: no attribute table: build scene::SceneAccelerationStructure first"};
  const bool soft = rt_soft_on();  // "shadow_mask_rt_soft_cutout": the same set, 8 the soft block, 9 the sample table
  gpu::ComputePipeline &pipeline_used = soft ? rt_soft_cutout_pipeline : rt_cutout_pipeline;
  if (!pipeline_used.has_program()) pipeline_used = gpu::create_compute_pipeline(soft ? "shadow_mask_rt_soft_cutout" : "shadow_mask_rt_cutout");
  std::vector<rec::Binding> bindings {rec::sampled_mips(0, depth, sampler, DEPTH, 0, 1), rec::sampled(1, normal, sampler), rec::accel(2, scene.tlas),
    rec::uniform(3, rt_params), rec::storage(4, out), rec::uniform_buffer(5, scene.hit_attributes),
    rec::uniform(6, vkr_ray_cutout {cutouts.alpha_lod, 0u})};
  if (soft) bindings.insert(bindings.end(), {rec::uniform(8, rt_soft), rec::uniform_buffer(9, bound_rt_soft_table())});
  struct Data { std::vector<rec::Bound> bound; };
  const auto program = pipeline_used;
  const auto textures = scene.textures;
  graph.add_task<Data>(soft ? "ShadowMaskRTSoft" : "ShadowMaskRT",
    [&](Data &d, rendergraph::RenderGraphBuilder &builder) { d.bound = rec::declare(bindings, builder, VK_SHADER_STAGE_COMPUTE_BIT); },
    [=](Data &d, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) {
      VkDescriptorSet set = rec::write(d.bound, resources, cmd);
      gpu::write_set(set, gpu::ArrayOfImagesBinding {7, textures});
      cmd.bind_pipeline(program);
      cmd.bind_descriptors_compute(0, {set});
      const auto extent = resources.get_image(out)->get_extent();
      cmd.dispatch((extent.width + 15)/16, (extent.height + 15)/16, 1);
    });
}

// ==== SyntheticGbuffer ===============================================================================================
SyntheticGbuffer::SyntheticGbuffer(uint32_t s) : seed {s} {
  pipeline = gpu::create_graphics_pipeline();
  pipeline.set_program("synthetic_gbuffer");
  pipeline.set_vertex_input({});
}

static vkr_synth_params synth_params(const glm::mat4 &camera, const glm::mat4 &mvp, const glm::mat4 &prev_mvp, const glm::vec4 &fazz, uint32_t seed, uint32_t flags) {
  vkr_synth_params p {};
  copy_mat(p.camera_to_world, glm::inverse(camera));
  copy_mat(p.prev_mvp, prev_mvp);
  copy_mat(p.mvp, mvp);
  p.fovy = fazz.x; p.aspect = fazz.y; p.znear = fazz.z; p.zfar = fazz.w;
  p.seed = seed;
  p.flags = flags;
  return p;
}

// same attachments, in the same order, as SceneRenderer::draw_taa
void SyntheticGbuffer::draw_taa(RenderGraph &graph, const Gbuffer &gbuffer, const DrawTAAParams &params) {
  rec::fullscreen(graph, "GbufferPass", pipeline,
    {rec::uniform(0, synth_params(params.camera, params.mvp, params.prev_mvp, params.fovy_aspect_znear_zfar, seed, material_flags & VKR_SYNTH_TEXTURED_ROUGHNESS)),
     rec::color_target(gbuffer.albedo), rec::color_target(gbuffer.normal), rec::color_target(gbuffer.material),
     rec::color_target(gbuffer.velocity_vectors), rec::depth_target(gbuffer.depth)},
    rec::no_push(), gbuffer.w, gbuffer.h);
}

void SyntheticGbuffer::draw_depth(RenderGraph &graph, ImageResourceId depth_target, const glm::mat4 &camera, const glm::mat4 &mvp, const glm::vec4 &fazz) {
  const auto desc = graph.get_descriptor(depth_target);
  rec::fullscreen(graph, "GbufferDepthOnly", pipeline,
    {rec::uniform(0, synth_params(camera, mvp, mvp, fazz, seed, VKR_SYNTH_DEPTH_ONLY)), rec::depth_target(depth_target)},
    rec::no_push(), desc.width, desc.height);
}

// ==== util_passes.hpp (reference: src/util_passes.cpp:42-179) — transfers through vkr_gen_mipmaps / vkr_clear_image / vkr_blit_image
namespace {
void transfer_status(int rc, const char *what) {
  if (rc != 0) throw std::runtime_error {std::string {what} + ": " + vkr_last_error()};
}
struct MipRange { ImageResourceId image; uint32_t base_mip, mips, layers; };
// one transfer task: the declarations the reference makes for it, and the C-ABI call on the command context's stream
void add_transfer_task(RenderGraph &graph, const char *name, const std::vector<MipRange> &reads, const std::vector<MipRange> &writes,
                       std::function<void(rendergraph::RenderResources &, void *stream)> run) {
  struct Data {};
  graph.add_task<Data>(name,
    [&](Data &, rendergraph::RenderGraphBuilder &builder) {
      for (const auto &r : reads) builder.transfer_read(r.image, r.base_mip, r.mips, 0, r.layers);
      for (const auto &w : writes) builder.transfer_write(w.image, w.base_mip, w.mips, 0, w.layers);
    },
    [=](Data &, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) { run(resources, cmd.get_stream()); });
}
// every mip of every layer: a layer's descriptor covers the texels of that layer only
void add_clear_task(RenderGraph &graph, const char *name, ImageResourceId image, const vkr_clear_value &value) {
  const auto info = graph.get_descriptor(image);
  add_transfer_task(graph, name, {}, {{image, 0, info.mip_levels, info.array_layers}}, [=](rendergraph::RenderResources &resources, void *stream) {
    const gpu::Image &img = *resources.get_image(image);
    for (uint32_t layer = 0; layer < img.get_array_layers(); layer++) {
      const vkr_img d = img.describe_layer(layer, 0, img.get_mip_levels());
      transfer_status(vkr_clear_image(&d, &value, stream), name);
    }
  });
}
}  // namespace

void gen_mipmaps(RenderGraph &graph, ImageResourceId image) {
  const uint32_t levels = graph.get_descriptor(image).mip_levels;
  for (uint32_t dst_mip = 1; dst_mip < levels; dst_mip++)  // the reference's task list: one blit per level
    add_transfer_task(graph, "Genmips", {{image, dst_mip - 1, 1, 1}}, {{image, dst_mip, 1, 1}}, [=](rendergraph::RenderResources &resources, void *stream) {
      const vkr_img d = resources.get_image(image)->describe(dst_mip - 1, 2);  // the chain of one level
      transfer_status(vkr_gen_mipmaps(&d, stream), "Genmips");
    });
}

void clear_depth(RenderGraph &graph, ImageResourceId image, float val) {
  vkr_clear_value value {};
  value.depth = val;  // stencil 0, as a VkClearDepthStencilValue with only .depth set
  add_clear_task(graph, "Clear_depth", image, value);
}

void clear_color(RenderGraph &graph, ImageResourceId image, VkClearColorValue val) {
  vkr_clear_value value {};
  std::memcpy(value.color, val.float32, sizeof(value.color));  // every format of this path is UNORM / SRGB / SFLOAT: the float member
  add_clear_task(graph, "Clear_color", image, value);
}

void blit_image(RenderGraph &graph, ImageResourceId src, ImageResourceId dst) {
  add_transfer_task(graph, "CopyImage", {{src, 0, 1, 1}}, {{dst, 0, 1, 1}}, [=](rendergraph::RenderResources &resources, void *stream) {
    const vkr_img s = resources.get_image(src)->describe(0, 1), d = resources.get_image(dst)->describe(0, 1);
    transfer_status(vkr_blit_image(&s, &d, VKR_FILTER_LINEAR, stream), "CopyImage");  // the reference blits with VK_FILTER_LINEAR
  });
}

// ==== ShadowMaskPass, the filter (shadow_mask.hpp): here because the task is a direct C-ABI call like the transfers above ==========
void ShadowMaskPass::update_filter(uint32_t reach, float normal_min_dot, float plane_tolerance) {
  if (reach < 1 || reach > 4) throw std::runtime_error {"ShadowMaskPass::update_filter: reach " + std::to_string(reach) + ", needs 1..4"};
  if (std::isnan(normal_min_dot) || std::isnan(plane_tolerance)) throw std::runtime_error {"ShadowMaskPass::update_filter: a threshold is NaN"};
  filter.reach = reach; filter.normal_min_dot = normal_min_dot; filter.plane_tolerance = plane_tolerance;
}

void ShadowMaskPass::run_filter(RenderGraph &graph, ImageResourceId depth, ImageResourceId normal, ImageResourceId mask, ImageResourceId out) {
  if (filter.reach == 0) throw std::runtime_error {"ShadowMaskPass::run_filter: update_filter first"};
  vkr_shadow_filter_params block = filter;
  if (camera_is_rt) {
    block.inverse_camera = rt_params.inverse_camera;
    block.fovy = rt_params.fovy; block.aspect = rt_params.aspect; block.znear = rt_params.znear; block.zfar = rt_params.zfar;
  } else {
    block.inverse_camera = params.inverse_camera;
    block.fovy = params.fovy; block.aspect = params.aspect; block.znear = params.znear; block.zfar = params.zfar;
  }
  add_transfer_task(graph, "ShadowMaskFilter", {{depth, 0, 1, 1}, {normal, 0, 1, 1}, {mask, 0, 1, 1}}, {{out, 0, 1, 1}},
    [=](rendergraph::RenderResources &resources, void *stream) {
      const vkr_img d = resources.get_image(depth)->describe(0, 1), n = resources.get_image(normal)->describe(0, 1);
      const vkr_img m = resources.get_image(mask)->describe(0, 1), o = resources.get_image(out)->describe(0, 1);
      transfer_status(vkr_shadow_mask_filter(&d, &n, &m, &block, &o, stream), "ShadowMaskFilter");
    });
}

// ==== ShadowMaskPass, the temporal accumulation: a direct C-ABI call like the filter ================================================
void ShadowMaskPass::update_accumulate(uint32_t max_count, float plane_tolerance, const glm::mat4 &prev_view, bool reset) {
  if (max_count < 1 || max_count > 255) throw std::runtime_error {"ShadowMaskPass::update_accumulate: max_count " + std::to_string(max_count) + ", needs 1..255"};
  if (std::isnan(plane_tolerance)) throw std::runtime_error {"ShadowMaskPass::update_accumulate: plane_tolerance is NaN"};
  accum = vkr_shadow_accum_params {};
  copy_mat(accum.prev_inverse_camera, glm::inverse(prev_view));
  accum.max_count = max_count; accum.plane_tolerance = plane_tolerance; accum.reset = reset ? 1u : 0u;
}

void ShadowMaskPass::run_accumulate(RenderGraph &graph, ImageResourceId depth, ImageResourceId normal, ImageResourceId velocity, ImageResourceId prev_depth,
  ImageResourceId mask, ImageResourceId history, ImageResourceId history_count, ImageResourceId out_history, ImageResourceId out_count,
  ImageResourceId out_mask)
{
  if (accum.max_count == 0) throw std::runtime_error {"ShadowMaskPass::run_accumulate: update_accumulate first"};
  vkr_shadow_accum_params block = accum;
  if (camera_is_rt) {
    block.inverse_camera = rt_params.inverse_camera;
    block.fovy = rt_params.fovy; block.aspect = rt_params.aspect; block.znear = rt_params.znear; block.zfar = rt_params.zfar;
  } else {
    block.inverse_camera = params.inverse_camera;
    block.fovy = params.fovy; block.aspect = params.aspect; block.znear = params.znear; block.zfar = params.zfar;
  }
  add_transfer_task(graph, "ShadowMaskAccumulate",
    {{depth, 0, 1, 1}, {normal, 0, 1, 1}, {velocity, 0, 1, 1}, {prev_depth, 0, 1, 1}, {mask, 0, 1, 1}, {history, 0, 1, 1}, {history_count, 0, 1, 1}},
    {{out_history, 0, 1, 1}, {out_count, 0, 1, 1}, {out_mask, 0, 1, 1}},
    [=](rendergraph::RenderResources &resources, void *stream) {
      const auto view = [&](ImageResourceId id) { return resources.get_image(id)->describe(0, 1); };
      const vkr_img d = view(depth), n = view(normal), v = view(velocity), pd = view(prev_depth), m = view(mask), h = view(history),
                    c = view(history_count), oh = view(out_history), oc = view(out_count), om = view(out_mask);
      transfer_status(vkr_shadow_mask_accumulate(&d, &n, &v, &pd, &m, &h, &c, &block, &oh, &oc, &om, stream), "ShadowMaskAccumulate");
    });
}

// ==== scene (scene/scene.cpp, scene/images.cpp) and SceneRenderer (scene_renderer.cpp:46-220) ===========================
namespace scene {

CompiledScene make_scene(const Vertex *vertices, uint32_t vertex_count, const uint32_t *indices, uint32_t index_count,
                         const FlatDraw *draws, uint32_t draw_count, const TextureData *textures, uint32_t texture_count, void *stream)
{
  CompiledScene out;
  auto upload = [](const void *src, uint64_t bytes) {  // scene.cpp:285-296: one vertex and one index buffer for the whole file
    auto buf = gpu::create_buffer(VMA_MEMORY_USAGE_CPU_TO_GPU, std::max<uint64_t>(bytes, 4), VK_BUFFER_USAGE_TRANSFER_DST_BIT);
    if (bytes) std::memcpy(buf->get_mapped_ptr(), src, bytes);
    return buf;
  };
  out.vertex_buffer = upload(vertices, sizeof(Vertex) * uint64_t(vertex_count));
  out.index_buffer = upload(indices, sizeof(uint32_t) * uint64_t(index_count));
  auto repeat = gpu::DEFAULT_SAMPLER;  // scene_renderer.cpp:77-81
  repeat.addressModeU = repeat.addressModeV = VK_SAMPLER_ADDRESS_MODE_REPEAT;
  out.samplers.push_back(gpu::create_sampler(repeat));
  for (uint32_t i = 0; i < texture_count; i++) {  // images.cpp:32-49: RGBA8_SRGB with a full mip chain
    const TextureData &t = textures[i];
    // images.cpp:93-160 builds the chain on the GPU; so does gen_mips (level 0 uploaded, the rest by vkr_gen_mipmaps)
    const uint32_t levels = t.gen_mips ? uint32_t(std::floor(std::log2(float(std::max(t.width, t.height))))) + 1u : t.mip_levels;
    auto img = std::make_shared<gpu::Image>(gpu::ImageInfo {VK_FORMAT_R8G8B8A8_SRGB, COLOR, t.width, t.height, 1, levels, 1}, gpu::FrameWindow {});
    bool never_zero = true;
    // gen_mips: only level 0 is in host memory.  It decides for every level: the alpha of a mip texel is rint(255 * average) of
    // four alphas of the level below, and an average of codes >= 1 rounds to a code >= 1
    for (uint32_t m = 0; m < (t.gen_mips ? 1u : levels); m++) {
      img->upload_mip(m, t.levels[m]);
      const size_t texels = size_t(std::max(1u, t.width >> m)) * std::max(1u, t.height >> m);
      for (size_t k = 0; k < texels && never_zero; k++) never_zero = t.levels[m][4 * k + 3] != 0;
    }
    if (t.gen_mips && levels > 1) {  // upload_mip is synchronous: level 0 is in place
      const vkr_img d = img->describe(0, levels);
      transfer_status(vkr_gen_mipmaps(&d, stream), "make_scene: texture mips");
    }
    img->alpha_never_zero = never_zero;
    out.images.push_back(img);
    out.textures.push_back(Texture {i, 0});
  }
  for (uint32_t i = 0; i < draw_count; i++) {
    const FlatDraw &d = draws[i];
    Material mat;
    mat.albedo_tex_index = d.albedo_tex_index;
    mat.metalic_roughness_index = d.metalic_roughness_index;
    mat.clip_alpha = d.clip_alpha;
    out.materials.push_back(mat);
    BaseMesh mesh;
    mesh.primitives.push_back(Primitive {d.vertex_offset, d.index_offset, d.index_count, i});
    out.root_meshes.push_back(mesh);
    out.base_nodes.push_back(BaseNode {d.transform, {}, int(i)});
  }
  return out;
}

// ---- scene/scene_as.hpp: the acceleration structure of the ray-query AO -----------------------------------------------
SceneAccelerationStructure::~SceneAccelerationStructure() {
  if (tlas) vkr_accel_destroy((vkr_accel*)tlas);
}

void SceneAccelerationStructure::build(gpu::TransferCmdPool &transfer_pool, const CompiledScene &source) {  // scene_as.cpp:19-24
  blas_triangles.clear();
  blas_attributes.clear();
  blas_normals.clear();
  for (const auto &mesh : source.root_meshes) build_blas(transfer_pool, mesh, source);
  build_tlas(transfer_pool, source);
}

void SceneAccelerationStructure::build_blas(gpu::TransferCmdPool &, const BaseMesh &mesh, const CompiledScene &source) {
  const auto *vertices = (const Vertex *)source.vertex_buffer->host_data();
  const auto *indices = (const uint32_t *)source.index_buffer->host_data();
  const uint64_t vertex_count = vertices ? source.vertex_buffer->get_size() / sizeof(Vertex) : 0;
  const uint64_t index_count = indices ? source.index_buffer->get_size() / sizeof(uint32_t) : 0;
  std::vector<float> tris, normals;
  std::vector<vkr_hit_attrib> attribs;
  for (const auto &prim : mesh.primitives) {  // scene_as.cpp:60-70: primitiveCount = index_count / 3, firstVertex = vertex_offset
    if (uint64_t(prim.index_offset) + prim.index_count > index_count)
      throw std::runtime_error {"SceneAccelerationStructure: a primitive's indices lie outside the index buffer"};
    const uint32_t albedo = prim.material_index < source.materials.size()? source.materials[prim.material_index].albedo_tex_index : 0xFFFFFFFFu;
    for (uint32_t j = 0; j + 3 <= prim.index_count; j += 3) {
      vkr_hit_attrib a {};
      a.albedo_index = albedo;
      for (uint32_t k = 0; k < 3; k++) {
        const uint64_t v = uint64_t(prim.vertex_offset) + indices[prim.index_offset + j + k];
        if (v >= vertex_count) throw std::runtime_error {"SceneAccelerationStructure: an index names a vertex outside the vertex buffer"};
        tris.insert(tris.end(), {vertices[v].pos.x, vertices[v].pos.y, vertices[v].pos.z});
        normals.insert(normals.end(), {vertices[v].norm.x, vertices[v].norm.y, vertices[v].norm.z});
        a.uv[k][0] = vertices[v].uv.x; a.uv[k][1] = vertices[v].uv.y;
      }
      attribs.push_back(a);
    }
  }
  blas_triangles.push_back(std::move(tris));
  blas_attributes.push_back(std::move(attribs));
  blas_normals.push_back(std::move(normals));
}

namespace {
struct FlatNode { glm::mat4 transform; int mesh; };
void flatten_nodes(std::vector<FlatNode> &out, const BaseNode &node, const glm::mat4 &pre_transform) {  // scene_as.cpp:144-157
  const glm::mat4 transform = pre_transform * node.transform;
  if (node.mesh_index >= 0) out.push_back(FlatNode {transform, node.mesh_index});
  for (const auto &child : node.children) flatten_nodes(out, child, transform);
}
}  // namespace

void SceneAccelerationStructure::build_tlas(gpu::TransferCmdPool &, const CompiledScene &source) {
  std::vector<FlatNode> nodes;
  for (const auto &node : source.base_nodes) flatten_nodes(nodes, node, glm::mat4 {1.f});
  world_triangles.clear();
  world_attributes.clear();
  world_normals.clear();
  for (const auto &n : nodes) {
    if (size_t(n.mesh) >= blas_triangles.size()) throw std::runtime_error {"SceneAccelerationStructure: a node names a mesh without a structure (build_blas first)"};
    const glm::mat4 &m = n.transform;  // m[column][row]
    const auto &obj = blas_triangles[n.mesh];
    if (size_t(n.mesh) < blas_attributes.size())  // one record per instance, in the order of the triangles
      world_attributes.insert(world_attributes.end(), blas_attributes[n.mesh].begin(), blas_attributes[n.mesh].end());
    for (size_t i = 0; i + 3 <= obj.size(); i += 3) {
      const float x = obj[i], y = obj[i + 1], z = obj[i + 2];
      for (int row = 0; row < 3; row++) {
        const float p0 = m[0][row] * x, p1 = m[1][row] * y, p2 = m[2][row] * z;
        const float s01 = p0 + p1, s012 = s01 + p2;
        world_triangles.push_back(s012 + m[3][row]);
      }
    }
    if (size_t(n.mesh) < blas_normals.size()) {  // the normal matrix of SceneRenderer::update_scene, no translation
      const glm::mat4 nm = glm::transpose(glm::inverse(m));
      const auto &nrm = blas_normals[n.mesh];
      for (size_t i = 0; i + 9 <= nrm.size(); i += 9) {
        vkr_hit_normal r {};
        for (int k = 0; k < 3; k++) {
          const float x = nrm[i + 3 * k], y = nrm[i + 3 * k + 1], z = nrm[i + 3 * k + 2];
          for (int row = 0; row < 3; row++) {
            const float p0 = nm[0][row] * x, p1 = nm[1][row] * y, p2 = nm[2][row] * z;
            const float s01 = p0 + p1;
            r.n[k][row] = s01 + p2;
          }
        }
        world_normals.push_back(r);
      }
    }
  }
  if (tlas) vkr_accel_destroy((vkr_accel*)tlas);
  tlas = nullptr;
  vkr_accel *accel = nullptr;
  if (vkr_accel_create(world_triangles.data(), uint32_t(world_triangles.size() / 9), &accel) != 0)
    throw std::runtime_error {std::string {"SceneAccelerationStructure: "} + vkr_last_error()};
  tlas = (VkAccelerationStructureKHR)accel;
  // the attribute table of the closest-hit consumers: uploaded once, when it is first bound
  hit_attributes.reset();
  if (world_attributes.size() != world_triangles.size() / 9)
    throw std::runtime_error {"SceneAccelerationStructure: the attribute table does not match the triangles (build_blas before build_tlas)"};
  const uint64_t bytes = sizeof(vkr_hit_attrib) * world_attributes.size();
  hit_attributes = gpu::create_buffer(VMA_MEMORY_USAGE_CPU_TO_GPU, std::max<uint64_t>(bytes, sizeof(vkr_hit_attrib)), VK_BUFFER_USAGE_STORAGE_BUFFER_BIT);
  std::memset(hit_attributes->get_mapped_ptr(), 0, hit_attributes->get_size());  // an empty scene: one unused record (a buffer has no size 0)
  if (bytes) std::memcpy(hit_attributes->get_mapped_ptr(), world_attributes.data(), bytes);
  // the normal table of the lit consumers, with it
  hit_normals.reset();
  if (world_normals.size() != world_triangles.size() / 9)
    throw std::runtime_error {"SceneAccelerationStructure: the normal table does not match the triangles (build_blas before build_tlas)"};
  const uint64_t normal_bytes = sizeof(vkr_hit_normal) * world_normals.size();
  hit_normals = gpu::create_buffer(VMA_MEMORY_USAGE_CPU_TO_GPU, std::max<uint64_t>(normal_bytes, sizeof(vkr_hit_normal)), VK_BUFFER_USAGE_STORAGE_BUFFER_BIT);
  std::memset(hit_normals->get_mapped_ptr(), 0, hit_normals->get_size());
  if (normal_bytes) std::memcpy(hit_normals->get_mapped_ptr(), world_normals.data(), normal_bytes);
  refit_triangles.reset();  // another structure: the first refit() allocates for it
  refit_scratch.reset();
}

void SceneAccelerationStructure::refit(const CompiledScene &source, void *stream) {
  if (!tlas) throw std::runtime_error {"SceneAccelerationStructure::refit: no structure (build first)"};
  std::vector<FlatNode> nodes;
  for (const auto &node : source.base_nodes) flatten_nodes(nodes, node, glm::mat4 {1.f});
  // the draw list in build_tlas() order, with a model matrix per node
  std::vector<vkr_raster_transform> transforms(nodes.size());
  std::vector<vkr_raster_draw> draws;
  uint64_t triangles = 0;
  for (size_t i = 0; i < nodes.size(); i++) {
    if (size_t(nodes[i].mesh) >= source.root_meshes.size()) throw std::runtime_error {"SceneAccelerationStructure::refit: a node names a mesh the scene does not have"};
    std::memcpy(transforms[i].model.m, &nodes[i].transform, sizeof(transforms[i].model.m));
    const glm::mat4 normal = glm::transpose(glm::inverse(nodes[i].transform));  // as build_tlas(): read by vkr_scene_triangle_normals
    std::memcpy(transforms[i].normal.m, &normal, sizeof(transforms[i].normal.m));
    for (const auto &prim : source.root_meshes[nodes[i].mesh].primitives) {
      vkr_raster_draw d {};
      d.transform_index = uint32_t(i);
      d.albedo_index = d.mr_index = 0xFFFFFFFFu;
      d.index_offset = prim.index_offset; d.index_count = prim.index_count; d.vertex_offset = prim.vertex_offset;
      draws.push_back(d);
      triangles += prim.index_count / 3u;
    }
  }
  if (triangles != world_triangles.size() / 9)
    throw std::runtime_error {"SceneAccelerationStructure::refit: the scene has " + std::to_string(triangles) + " triangles, the structure was built from " +
                              std::to_string(world_triangles.size() / 9) + " (a refit moves triangles; build() again to add or remove some)"};
  if (triangles == 0) return;
  const uint64_t scratch_bytes = vkr_scene_triangles_scratch_bytes(uint32_t(draws.size()));
  if (!refit_triangles) refit_triangles = gpu::create_buffer(VMA_MEMORY_USAGE_GPU_ONLY, sizeof(float) * 9 * triangles, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT);
  if (!refit_scratch || refit_scratch->get_size() < scratch_bytes) {
    // an earlier refit() may still read the old table on the stream
    if (refit_scratch && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) throw std::runtime_error {"SceneAccelerationStructure::refit: the stream is in error"};
    refit_scratch = gpu::create_buffer(VMA_MEMORY_USAGE_GPU_ONLY, scratch_bytes, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT);
  }
  vkr_raster_scene scene {};
  scene.vertices = (const vkr_raster_vertex *)source.vertex_buffer->device_ptr(stream);
  scene.vertex_count = uint32_t(source.vertex_buffer->get_size() / sizeof(vkr_raster_vertex));
  scene.indices = (const uint32_t *)source.index_buffer->device_ptr(stream);
  scene.index_count = uint32_t(source.index_buffer->get_size() / sizeof(uint32_t));
  scene.transforms = transforms.data(); scene.transform_count = uint32_t(transforms.size());
  scene.draws = draws.data(); scene.draw_count = uint32_t(draws.size());
  float *moved = (float *)refit_triangles->device_ptr(stream);
  if (vkr_scene_triangles(&scene, moved, triangles, refit_scratch->device_ptr(stream), scratch_bytes, stream) != 0 ||
      vkr_accel_refit((vkr_accel *)tlas, moved, stream) != 0)
    throw std::runtime_error {std::string {"SceneAccelerationStructure::refit: "} + vkr_last_error()};
  // the normals move with the draws; the two launches read the draw table one after the other on the stream, each after its own
  // upload of it
  if (hit_normals &&
      vkr_scene_triangle_normals(&scene, (vkr_hit_normal *)hit_normals->device_ptr(stream), triangles, refit_scratch->device_ptr(stream), scratch_bytes, stream) != 0)
    throw std::runtime_error {std::string {"SceneAccelerationStructure::refit: "} + vkr_last_error()};
}

std::vector<vkr_hit_normal> SceneAccelerationStructure::download_hit_normals(void *stream) {
  std::vector<vkr_hit_normal> out(world_triangles.size() / 9);
  if (out.empty() || !hit_normals) return out;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
      hipMemcpy(out.data(), hit_normals->device_ptr(stream), sizeof(vkr_hit_normal) * out.size(), hipMemcpyDeviceToHost) != hipSuccess)
    throw std::runtime_error {"SceneAccelerationStructure::download_hit_normals: the copy failed"};
  return out;
}

std::vector<float> SceneAccelerationStructure::download_world_triangles(void *stream) {
  if (!refit_triangles) return world_triangles;
  std::vector<float> out(world_triangles.size());
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
      hipMemcpy(out.data(), refit_triangles->device_ptr(stream), sizeof(float) * out.size(), hipMemcpyDeviceToHost) != hipSuccess)
    throw std::runtime_error {"SceneAccelerationStructure::download_world_triangles: the copy failed"};
  return out;
}

}  // namespace scene

void SceneRenderer::init_pipeline(RenderGraph &graph, const Gbuffer &) {  // :46-103
  owner = &graph;
  gpu::Registers regs {};
  regs.depth_stencil.depthTestEnable = VK_TRUE;
  regs.depth_stencil.depthWriteEnable = VK_TRUE;
  opaque_taa_pipeline = fullscreen_pipeline("gbuf_opaque_taa", regs);
  opaque_taa_pipeline.set_rendersubpass({true, {VK_FORMAT_R8G8B8A8_SRGB, VK_FORMAT_R16G16_UNORM, VK_FORMAT_R8G8B8A8_SRGB, VK_FORMAT_R16G16_SFLOAT}});
  shadow_pipeline = gpu::create_graphics_pipeline();  // :72-75
  shadow_pipeline.set_program("default_shadow");
  shadow_pipeline.set_registers(regs);
  shadow_pipeline.set_vertex_input(scene::get_vertex_input_shadow());
  auto repeat = gpu::DEFAULT_SAMPLER;
  repeat.addressModeU = repeat.addressModeV = VK_SAMPLER_ADDRESS_MODE_REPEAT;
  sampler = gpu::create_sampler(repeat);
  // host-visible here: the raster program premultiplies view_projection * model per draw on the host
  transform_buffer = graph.create_buffer(VMA_MEMORY_USAGE_CPU_TO_GPU, sizeof(glm::mat4) * 1000, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT|VK_BUFFER_USAGE_TRANSFER_DST_BIT);
  for (auto tex : target.textures) {
    auto &img = target.images[tex.image_index];
    texture_views.emplace_back(new gpu::ImageViewObject {img.get(), gpu::ImageViewRange {VK_IMAGE_VIEW_TYPE_2D, COLOR, 0, img->get_mip_levels(), 0, 1}});
    scene_textures.push_back({(VkImageView)texture_views.back().get(), target.samplers[tex.sampler_index]});
  }
  bindless_textures = gpu::allocate_descriptor_set(opaque_taa_pipeline.get_layout(1), {std::max<uint32_t>(1, uint32_t(scene_textures.size()))});
  if (!scene_textures.empty()) gpu::write_set(bindless_textures, gpu::ArrayOfImagesBinding {0, scene_textures});
}

// :105-131: depth-first walk, transforms = [model, transpose(inverse(model))] per drawn node
void SceneRenderer::update_scene() {
  if (!owner) throw std::runtime_error {"SceneRenderer::update_scene before init_pipeline"};
  std::vector<glm::mat4> transforms;
  draw_calls.clear();
  struct Walk {
    std::vector<glm::mat4> &transforms;
    std::vector<DrawCall> &calls;
    void node(const scene::BaseNode &n, const glm::mat4 &acc) {
      const glm::mat4 m = acc * n.transform;
      if (n.mesh_index >= 0) {
        calls.push_back(DrawCall {uint32_t(transforms.size()/2), uint32_t(n.mesh_index)});
        transforms.push_back(m);
        transforms.push_back(glm::transpose(glm::inverse(m)));
      }
      for (const auto &c : n.children) node(c, m);
    }
  } walk {transforms, draw_calls};
  for (const auto &n : target.base_nodes) walk.node(n, glm::mat4 {1.f});
  auto &buf = owner->get_buffer(transform_buffer);
  if (sizeof(glm::mat4) * transforms.size() > buf->get_size()) throw std::runtime_error {"Too many scene transforms"};
  std::memcpy(buf->get_mapped_ptr(), transforms.data(), sizeof(glm::mat4) * transforms.size());
}

// :140-220: clear, bind geometry + transforms + bindless textures, one draw_indexed per primitive with its PushData;
// CmdContext::end_renderpass hands the recorded draws to the raster program as one pass
void SceneRenderer::draw_taa(RenderGraph &graph, const Gbuffer &gbuffer, const DrawTAAParams &params) {
  static_assert(sizeof(vkr_gbuf_const) == 2 * sizeof(glm::mat4) + 2 * sizeof(glm::vec4), "GbufConst must match the C-ABI");
  vkr_gbuf_const consts {};
  copy_mat(consts.view_projection, params.mvp);
  copy_mat(consts.prev_view_projection, params.prev_mvp);
  std::memcpy(consts.jitter, &params.jitter, sizeof(consts.jitter));
  std::memcpy(consts.fovy_aspect_znear_zfar, &params.fovy_aspect_znear_zfar, sizeof(consts.fovy_aspect_znear_zfar));
  const std::vector<rec::Binding> binds {
    rec::uniform(0, consts), rec::storage_buffer(1, transform_buffer),
    rec::color_target(gbuffer.albedo), rec::color_target(gbuffer.normal), rec::color_target(gbuffer.material),
    rec::color_target(gbuffer.velocity_vectors), rec::depth_target(gbuffer.depth)};
  const uint32_t w = gbuffer.w, h = gbuffer.h;

  struct Data { std::vector<rec::Bound> bound; };
  graph.add_task<Data>("GbufferPass",
    [&](Data &d, rendergraph::RenderGraphBuilder &builder) { d.bound = rec::declare(binds, builder, VK_SHADER_STAGE_VERTEX_BIT); builder.use_context_scratch(); },
    [=](Data &d, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) {
      std::vector<gpu::ImageViewObject> targets;
      for (const auto &r : d.bound)
        if (r.b.kind == rec::Binding::Color || r.b.kind == rec::Binding::Depth) targets.push_back(resources.get_image_range(r.view));
      cmd.set_framebuffer(w, h, targets);
      cmd.bind_pipeline(opaque_taa_pipeline);
      cmd.clear_color_attachments(0.f, 0.f, 0.f, 0.f);
      cmd.clear_depth_attachment(1.f);
      cmd.bind_viewport(0.f, 0.f, float(w), float(h), 0.f, 1.f);
      cmd.bind_scissors(0, 0, w, h);
      cmd.bind_vertex_buffers(0, {target.vertex_buffer->api_buffer()}, {0ul});
      cmd.bind_index_buffer(target.index_buffer->api_buffer(), 0, VK_INDEX_TYPE_UINT32);
      cmd.bind_descriptors_graphics(0, {rec::write(d.bound, resources, cmd)});
      cmd.bind_descriptors_graphics(1, {bindless_textures});
      for (const auto &call : draw_calls) {
        for (const auto &prim : target.root_meshes[call.mesh].primitives) {
          const auto &material = target.materials[prim.material_index];
          const uint32_t ntex = uint32_t(scene_textures.size());
          const uint32_t pc[4] {call.transform, material.albedo_tex_index < ntex? material.albedo_tex_index : scene::INVALID_TEXTURE,
                                material.metalic_roughness_index < ntex? material.metalic_roughness_index : scene::INVALID_TEXTURE,
                                material.clip_alpha? 0xffu : 0u};  // PushData :132-137
          cmd.push_constants_graphics(VK_SHADER_STAGE_VERTEX_BIT|VK_SHADER_STAGE_FRAGMENT_BIT, 0, sizeof(pc), pc);
          cmd.draw_indexed(prim.index_count, 1, prim.index_offset, int32_t(prim.vertex_offset), 0);
        }
      }
      cmd.end_renderpass();
    });
}

// :222-274, a commented-out body in the reference (it predates the scene traversal): here it draws, walking draw_calls x
// mesh.primitives as draw_taa does.  Depth attachment (out_tex, mip 0, layer) cleared to 1, UBO mat4, SSBO transforms, a 4-byte
// push constant transform_index, one draw_indexed per primitive.  The reference sizes the framebuffer width x width (:234-235);
// a non-square image is refused instead of rendered wrongly.
void SceneRenderer::render_shadow(RenderGraph &graph, const glm::mat4 &shadow_mvp, rendergraph::ImageResourceId out_tex, uint32_t layer) {
  struct Data {
    rendergraph::ImageViewId depth;
  };
  const auto desc = graph.get_descriptor(out_tex);
  if (desc.width != desc.height)
    throw std::runtime_error {"SceneRenderer::render_shadow: the shadow map is " + std::to_string(desc.width) + "x" + std::to_string(desc.height) + ", it must be square"};
  if (layer >= std::max(1u, desc.array_layers)) throw std::runtime_error {"SceneRenderer::render_shadow: layer outside the shadow map"};
  graph.add_task<Data>("ShadowPass",
    [&](Data &input, rendergraph::RenderGraphBuilder &builder) {
      input.depth = builder.use_depth_attachment(out_tex, 0, layer);
      builder.use_storage_buffer(transform_buffer, VK_SHADER_STAGE_VERTEX_BIT);
      builder.use_context_scratch();
    },
    [=](Data &input, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) {
      const auto &depth_rt = resources.get_image(input.depth);
      const uint32_t w = depth_rt->get_info().width;
      const uint32_t h = depth_rt->get_info().width;

      shadow_pipeline.set_rendersubpass({true, {depth_rt->get_info().format}});

      cmd.set_framebuffer(w, h, {resources.get_image_range(input.depth)});
      cmd.bind_pipeline(shadow_pipeline);
      cmd.clear_color_attachments(0.f, 0.f, 0.f, 0.f);
      cmd.clear_depth_attachment(1.f);
      cmd.bind_viewport(0.f, 0.f, float(w), float(h), 0.f, 1.f);
      cmd.bind_scissors(0, 0, w, h);
      cmd.bind_vertex_buffers(0, {target.vertex_buffer->api_buffer()}, {0ul});
      cmd.bind_index_buffer(target.index_buffer->api_buffer(), 0, VK_INDEX_TYPE_UINT32);

      auto set = resources.allocate_set(shadow_pipeline.get_layout(0));
      auto block = cmd.allocate_ubo<glm::mat4>();
      *block.ptr = shadow_mvp;

      gpu::write_set(set,
        gpu::UBOBinding {0, cmd.get_ubo_pool(), block},
        gpu::SSBOBinding {1, resources.get_buffer(transform_buffer)});

      cmd.bind_descriptors_graphics(0, {set}, {block.offset});

      for (const auto &draw_call : draw_calls) {
        for (const auto &prim : target.root_meshes[draw_call.mesh].primitives) {
          cmd.push_constants_graphics(VK_SHADER_STAGE_VERTEX_BIT, 0, sizeof(uint32_t), &draw_call.transform);
          cmd.draw_indexed(prim.index_count, 1, prim.index_offset, int32_t(prim.vertex_offset), 0);
        }
      }

      cmd.end_renderpass();
    });
}

// ==== SSAOPass (ssao.cpp) ================================================================================
ImageResourceId create_ssao_texture(RenderGraph &graph, uint32_t width, uint32_t height) {  // :8-11
  return make_image(graph, VK_FORMAT_R8_UNORM, width, height, VK_IMAGE_USAGE_COLOR_ATTACHMENT_BIT|VK_IMAGE_USAGE_SAMPLED_BIT);
}

namespace {
constexpr uint32_t SSAO_SAMPLES_COUNT = 16;  // :13
struct SSAOParams {  // :15-22, the host's view of the block: 272 bytes
  glm::mat4 projection;
  float fovy;
  float aspect;
  float znear;
  float zfar;
  glm::vec3 samples[SSAO_SAMPLES_COUNT];
};
static_assert(sizeof(SSAOParams) == 272 && sizeof(vkr_ssao_params) == 336, "SSAOParams: host packing and std140");
}  // namespace

// :24-52: 16 points drawn by rejection inside the unit ball, normalised; nothing is printed
SSAOPass::SSAOPass(RenderGraph &graph, ImageResourceId target) {
  pipeline = fullscreen_pipeline("ssao");
  pipeline.set_rendersubpass({false, {graph.get_descriptor(target).format}});
  sampler = default_sampler();
  for (uint32_t i = 0; i < SSAO_SAMPLES_COUNT; i++) {
    while (true) {
      const float x = 2.f * rand()/float(RAND_MAX) - 1.f;
      const float y = 2.f * rand()/float(RAND_MAX) - 1.f;
      const float z = 2.f * rand()/float(RAND_MAX) - 1.f;
      const float l2 = x*x + y*y + z*z;
      if (l2 < 1.0) {
        const auto len = std::sqrt(l2);
        sphere_samples.push_back(glm::vec3 {x/len, y/len, z/len});
        break;
      }
    }
  }
}

std::vector<uint8_t> SSAOPass::uniform_block(const SSAOInParams &params) const {
  if (sphere_samples.size() != SSAO_SAMPLES_COUNT)
    throw std::runtime_error {"SSAOPass: sphere_samples holds " + std::to_string(sphere_samples.size()) + " samples, the shader reads 16"};
  std::vector<uint8_t> bytes(std140_samples? sizeof(vkr_ssao_params) : sizeof(SSAOParams), 0);
  if (std140_samples) {
    vkr_ssao_params block {};
    copy_mat(block.projection, params.projection);
    block.fovy = params.fovy; block.aspect = params.aspect; block.znear = params.znear; block.zfar = params.zfar;
    for (uint32_t i = 0; i < SSAO_SAMPLES_COUNT; i++)
      for (int c = 0; c < 3; c++) block.samples[i][c] = sphere_samples[i][c];
    std::memcpy(bytes.data(), &block, sizeof(block));
  } else {  // :69-77
    SSAOParams block {};
    block.projection = params.projection;
    block.fovy = params.fovy;
    block.aspect = params.aspect;
    block.znear = params.znear;
    block.zfar = params.zfar;
    for (uint32_t i = 0; i < SSAO_SAMPLES_COUNT; i++) block.samples[i] = sphere_samples[i];
    std::memcpy(bytes.data(), &block, sizeof(block));
  }
  return bytes;
}

// :54-97: task "SSAO"; depth sampled (depth aspect, mip 0, one level), colour attachment `target`, the block from the frame's
// uniform ring, one full-screen triangle at the target's extent
void SSAOPass::draw(RenderGraph &graph, ImageResourceId depth, ImageResourceId target, const SSAOInParams &params) {
  rec::Binding block;
  block.kind = rec::Binding::UniformBlock;
  block.slot = 1;
  block.bytes = uniform_block(params);
  const auto ext = graph.get_descriptor(target);
  rec::fullscreen(graph, "SSAO", pipeline,
    {rec::sampled_mips(0, depth, sampler, DEPTH, 0, 1), block, rec::color_target(target)},
    rec::no_push(), ext.width, ext.height);
}

// ==== probe renderer (probe_renderer.hpp; reference: src/probe_renderer.cpp, whose render_side is a commented-out body: here it draws)
// Every task executes through the programs cubemap_probe, cube2oct, probe_downsample and trace_probe registered in gpu/gpu.cpp.
using rendergraph::ImageViewId;
static uint32_t full_mip_chain(uint32_t size) { return uint32_t(std::floor(std::log2(float(size)))) + 1u; }

ProbeRenderer::ProbeRenderer(RenderGraph &graph, uint32_t cubemap_res) {
  rendergraph::ImageDescriptor desc {};
  desc.type = VK_IMAGE_TYPE_2D;
  desc.width = desc.height = cubemap_res;
  desc.format = VK_FORMAT_R8G8B8A8_SRGB;
  desc.array_layers = 6;
  desc.mip_levels = 1;
  desc.aspect = COLOR;
  desc.tiling = VK_IMAGE_TILING_OPTIMAL;
  desc.usage = VK_IMAGE_USAGE_COLOR_ATTACHMENT_BIT|VK_IMAGE_USAGE_SAMPLED_BIT;
  cubemap_color = graph.create_image(desc, gpu::ImageCreateOptions::Cubemap);
  desc.format = VK_FORMAT_R16_SFLOAT;
  cubemap_distance = graph.create_image(desc, gpu::ImageCreateOptions::Cubemap);

  // the depth attachment of a face: the programs keep their own depth (the visibility buffer), the image is only declared
  rt_depth = graph.create_frame_image(gpu::ImageInfo {VK_FORMAT_D24_UNORM_S8_UINT, VK_IMAGE_ASPECT_DEPTH_BIT|VK_IMAGE_ASPECT_STENCIL_BIT, cubemap_res, cubemap_res, 1, 1, 1});

  gpu::Registers regs {};
  regs.depth_stencil.depthTestEnable = VK_TRUE;
  regs.depth_stencil.depthWriteEnable = VK_TRUE;
  cubemap_pass = gpu::create_graphics_pipeline();
  cubemap_pass.set_program("cubemap_probe");
  cubemap_pass.set_registers(regs);
  cubemap_pass.set_vertex_input({});
  cubemap_pass.set_rendersubpass({true, {VK_FORMAT_R8G8B8A8_SRGB, VK_FORMAT_R16_SFLOAT, VK_FORMAT_D24_UNORM_S8_UINT}});

  octprobe_pass = gpu::create_compute_pipeline();
  octprobe_pass.set_program("cube2oct");

  downsample_pass = gpu::create_graphics_pipeline();
  downsample_pass.set_program("probe_downsample");
  downsample_pass.set_registers({});
  downsample_pass.set_vertex_input({});
  downsample_pass.set_rendersubpass({false, {VK_FORMAT_R16_UNORM}});

  sampler = gpu::create_sampler(gpu::DEFAULT_SAMPLER);
}

// forward / up of the six faces: up is (0, -1, 0) except on the two faces that look along y
static glm::mat4 face_view(uint32_t side, glm::vec3 pos) {
  glm::vec3 fwd {0.f, 0.f, -1.f}, up {0.f, -1.f, 0.f};
  switch (side) {
    case 0: fwd = glm::vec3 {1.f, 0.f, 0.f}; break;
    case 1: fwd = glm::vec3 {-1.f, 0.f, 0.f}; break;
    case 2: fwd = glm::vec3 {0.f, 1.f, 0.f}; up = glm::vec3 {0.f, 0.f, 1.f}; break;
    case 3: fwd = glm::vec3 {0.f, -1.f, 0.f}; up = glm::vec3 {0.f, 0.f, -1.f}; break;
    case 4: fwd = glm::vec3 {0.f, 0.f, 1.f}; break;
    default: break;
  }
  return glm::lookAt(pos, pos + fwd, up);
}

void ProbeRenderer::render_cubemap(RenderGraph &graph, SceneRenderer &scene_renderer, const glm::vec3 pos) {
  for (uint32_t side = 0; side < 6; side++) render_side(graph, scene_renderer, side, face_view(side, pos));
}

void ProbeRenderer::render_side(RenderGraph &graph, SceneRenderer &scene_renderer, uint32_t side, glm::mat4 view) {
  struct Res { ImageViewId color, distance, depth; };
  struct ShaderUbo { glm::mat4 projection, camera; };
  struct PushData { uint32_t transform_index, albedo_index; };

  graph.add_task<Res>("CubemapSide",
    [&](Res &res, rendergraph::RenderGraphBuilder &builder) {
      res.color = builder.use_color_attachment(cubemap_color, 0, side);
      res.distance = builder.use_color_attachment(cubemap_distance, 0, side);
      res.depth = builder.use_depth_attachment(rt_depth, 0, 0);
      builder.use_storage_buffer(scene_renderer.get_scene_transforms(), VK_SHADER_STAGE_VERTEX_BIT);
      builder.use_context_scratch();
    },
    [=, &scene_renderer](Res &res, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) {
      const auto extent = resources.get_image(res.color)->get_info().extent2D();
      auto blk = cmd.allocate_ubo<ShaderUbo>();
      blk.ptr->projection = glm::perspective(glm::radians(90.f), 1.f, 0.05f, 80.f);
      blk.ptr->camera = view;

      cmd.set_framebuffer(extent.width, extent.height, {resources.get_image_range(res.color), resources.get_image_range(res.distance), resources.get_image_range(res.depth)});
      auto &target = scene_renderer.get_target();
      cmd.bind_pipeline(cubemap_pass);
      cmd.clear_depth_attachment(1.f);
      cmd.clear_color_attachments(100.f, 0.f, 0.f, 0.f);
      cmd.bind_viewport(0.f, 0.f, float(extent.width), float(extent.height), 0.f, 1.f);
      cmd.bind_scissors(0, 0, extent.width, extent.height);
      cmd.bind_vertex_buffers(0, {target.vertex_buffer->api_buffer()}, {0ul});
      cmd.bind_index_buffer(target.index_buffer->api_buffer(), 0, VK_INDEX_TYPE_UINT32);

      auto set = resources.allocate_set(cubemap_pass.get_layout(0));
      gpu::write_set(set,
        gpu::UBOBinding {0, cmd.get_ubo_pool(), blk},
        gpu::SSBOBinding {1, resources.get_buffer(scene_renderer.get_scene_transforms())},
        gpu::ArrayOfImagesBinding {2, scene_renderer.get_images()});
      cmd.bind_descriptors_graphics(0, {set}, {blk.offset});

      const uint32_t ntex = uint32_t(scene_renderer.get_images().size());
      for (const auto &draw_call : scene_renderer.get_drawcalls()) {
        for (const auto &prim : target.root_meshes[draw_call.mesh].primitives) {
          const auto &material = target.materials[prim.material_index];
          if (material.albedo_tex_index == scene::INVALID_TEXTURE || material.albedo_tex_index >= ntex) continue;
          const PushData pc {draw_call.transform, material.albedo_tex_index};
          cmd.push_constants_graphics(VK_SHADER_STAGE_VERTEX_BIT|VK_SHADER_STAGE_FRAGMENT_BIT, 0, sizeof(PushData), &pc);
          cmd.draw_indexed(prim.index_count, 1, prim.index_offset, int32_t(prim.vertex_offset), 0);
        }
      }
      cmd.end_renderpass();
    });
}

void ProbeRenderer::render_octahedral(RenderGraph &graph, ImageResourceId probe_color, ImageResourceId probe_depth, uint32_t array_layer) {
  struct Input { ImageViewId cube_color, cube_distance, oct_color, oct_depth; };
  graph.add_task<Input>("Cubemap2Octahedral",
    [&](Input &input, rendergraph::RenderGraphBuilder &builder) {
      input.cube_color = builder.sample_cubemap(cubemap_color, VK_SHADER_STAGE_COMPUTE_BIT);
      input.cube_distance = builder.sample_cubemap(cubemap_distance, VK_SHADER_STAGE_COMPUTE_BIT);
      input.oct_color = builder.use_storage_image(probe_color, VK_SHADER_STAGE_COMPUTE_BIT, 0, array_layer);
      input.oct_depth = builder.use_storage_image(probe_depth, VK_SHADER_STAGE_COMPUTE_BIT, 0, array_layer);
    },
    [=](Input &input, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) {
      const auto desc = resources.get_image(input.oct_color)->get_extent();
      auto set = resources.allocate_set(octprobe_pass, 0);
      gpu::write_set(set,
        gpu::TextureBinding {0, resources.get_view(input.cube_color), sampler},
        gpu::TextureBinding {1, resources.get_view(input.cube_distance), sampler},
        gpu::StorageTextureBinding {2, resources.get_view(input.oct_color)},
        gpu::StorageTextureBinding {3, resources.get_view(input.oct_depth)});
      cmd.bind_pipeline(octprobe_pass);
      cmd.bind_descriptors_compute(0, {set});
      cmd.dispatch(desc.width/8, desc.height/4, 1);
    });
}

void ProbeRenderer::probe_downsample(RenderGraph &graph, ImageResourceId probe_depth, uint32_t array_layer) {
  const auto desc = graph.get_descriptor(probe_depth);
  struct Input { ImageViewId depth_tex, depth_rt; };
  for (uint32_t i = 1; i < desc.mip_levels; i++) {
    graph.add_task<Input>("DownsampleProbe",
      [&](Input &input, rendergraph::RenderGraphBuilder &builder) {
        input.depth_rt = builder.use_color_attachment(probe_depth, i, array_layer);
        input.depth_tex = builder.sample_image(probe_depth, VK_SHADER_STAGE_FRAGMENT_BIT, COLOR, i - 1, 1, array_layer, 1);
      },
      [=](Input &input, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) {
        auto set = resources.allocate_set(downsample_pass, 0);
        gpu::write_set(set, gpu::TextureBinding {0, resources.get_view(input.depth_tex), sampler});
        const uint32_t w = desc.width/(1u << i), h = desc.height/(1u << i);
        cmd.set_framebuffer(w, h, {resources.get_image_range(input.depth_rt)});
        cmd.bind_pipeline(downsample_pass);
        cmd.bind_descriptors_graphics(0, {set});
        cmd.bind_viewport(0.f, 0.f, float(w), float(h), 0.f, 1.f);
        cmd.bind_scissors(0, 0, w, h);
        cmd.draw(3, 1, 0, 0);
        cmd.end_renderpass();
      });
  }
}

void ProbeRenderer::render_probe(RenderGraph &graph, SceneRenderer &scene_renderer, const glm::vec3 pos, OctahedralProbe &probe) {
  render_cubemap(graph, scene_renderer, pos);
  render_octahedral(graph, probe.color, probe.depth);
  probe_downsample(graph, probe.depth);
  probe.pos = pos;
}

void ProbeRenderer::render_probe_grid(RenderGraph &graph, SceneRenderer &scene_renderer, glm::vec3 min, glm::vec3 max, OctahedralProbeGrid &probe_grid) {
  for (int k = 0; k < 3; k++) {
    const float lo = std::min(min[k], max[k]), hi = std::max(min[k], max[k]);
    min[k] = lo; max[k] = hi;
  }
  probe_grid.min = min;
  probe_grid.max = max;
  if (probe_grid.grid_size < 2) throw std::runtime_error {"ProbeRenderer::render_probe_grid: a probe grid needs grid_size >= 2"};

  const float cells = float(probe_grid.grid_size - 1);
  const glm::vec3 step {(max.x - min.x)/cells, (max.y - min.y)/cells, (max.z - min.z)/cells};
  for (uint32_t y = 0; y < probe_grid.grid_size; y++) {
    for (uint32_t x = 0; x < probe_grid.grid_size; x++) {
      const glm::vec3 pos {min.x + step.x * float(x), min.y + step.y * 0.f, min.z + step.z * float(y)};  // probes in x and z, at min.y
      const uint32_t array_layer = y * probe_grid.grid_size + x;
      render_cubemap(graph, scene_renderer, pos);
      render_octahedral(graph, probe_grid.color_array, probe_grid.depth_array, array_layer);
      probe_downsample(graph, probe_grid.depth_array, array_layer);
    }
  }
}

// (probe images are never windows of a tiled frame, whatever their extent: create_frame_image)
OctahedralProbe::OctahedralProbe(RenderGraph &graph, uint32_t size) {
  gpu::ImageInfo desc {VK_FORMAT_R8G8B8A8_UNORM, COLOR, size, size};
  color = graph.create_frame_image(desc);
  desc.mip_levels = full_mip_chain(size);
  desc.format = VK_FORMAT_R16_UNORM;
  depth = graph.create_frame_image(desc);
}

OctahedralProbeGrid::OctahedralProbeGrid(RenderGraph &graph, uint32_t grid_sz, uint32_t size) : grid_size {grid_sz} {
  gpu::ImageInfo desc {VK_FORMAT_R8G8B8A8_UNORM, COLOR, size, size};
  desc.array_layers = grid_sz * grid_sz;
  color_array = graph.create_frame_image(desc);
  desc.mip_levels = full_mip_chain(size);
  desc.format = VK_FORMAT_R16_UNORM;
  depth_array = graph.create_frame_image(desc);
}

ProbeTracePass::ProbeTracePass() {
  trace_pass = gpu::create_compute_pipeline();
  trace_pass.set_program("trace_probe");
  sampler = gpu::create_sampler(gpu::DEFAULT_SAMPLER);
}

void ProbeTracePass::run(RenderGraph &graph, OctahedralProbeGrid &probe, ImageResourceId gbuffer_depth, ImageResourceId gbuffer_norm, ImageResourceId out_image,
                         const ProbeTraceParams &params) {
  struct Input { ImageViewId depth, normal, probe_color, probe_depth, out_tex; };
  static_assert(sizeof(vkr_probe_trace_consts) == sizeof(glm::mat4) + 2 * sizeof(glm::vec4) + 5 * sizeof(uint32_t), "Constants must match the C-ABI");
  vkr_probe_trace_consts consts {};
  std::memcpy(consts.inverse_view.m, &params.inv_view, sizeof(consts.inverse_view.m));
  const glm::vec4 pmin {probe.min.x, probe.min.y, probe.min.z, 1.f}, pmax {probe.max.x, probe.max.y, probe.max.z, 1.f};
  std::memcpy(consts.probe_min, &pmin, sizeof(consts.probe_min));
  std::memcpy(consts.probe_max, &pmax, sizeof(consts.probe_max));
  consts.grid_size = probe.grid_size;
  consts.fovy = params.fovy; consts.aspect = params.aspect; consts.znear = params.znear; consts.zfar = params.zfar;

  graph.add_task<Input>("TraceProbe",
    [&](Input &input, rendergraph::RenderGraphBuilder &builder) {
      input.depth = builder.sample_image(gbuffer_depth, VK_SHADER_STAGE_COMPUTE_BIT, VK_IMAGE_ASPECT_DEPTH_BIT, 0, 1, 0, 1);
      input.normal = builder.sample_image(gbuffer_norm, VK_SHADER_STAGE_COMPUTE_BIT);
      input.probe_color = builder.sample_image(probe.color_array, VK_SHADER_STAGE_COMPUTE_BIT);
      input.probe_depth = builder.sample_image(probe.depth_array, VK_SHADER_STAGE_COMPUTE_BIT);
      input.out_tex = builder.use_storage_image(out_image, VK_SHADER_STAGE_COMPUTE_BIT, 0, 0);
    },
    [=](Input &input, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) {
      const auto desc = resources.get_image(input.out_tex)->get_extent();
      auto blk = cmd.allocate_ubo<vkr_probe_trace_consts>();
      *blk.ptr = consts;
      auto set = resources.allocate_set(trace_pass, 0);
      gpu::write_set(set,
        gpu::TextureBinding {0, resources.get_view(input.depth), sampler},
        gpu::TextureBinding {1, resources.get_view(input.normal), sampler},
        gpu::TextureBinding {2, resources.get_view(input.probe_color), sampler},
        gpu::TextureBinding {3, resources.get_view(input.probe_depth), sampler},
        gpu::UBOBinding {4, cmd.get_ubo_pool(), blk},
        gpu::StorageTextureBinding {5, resources.get_view(input.out_tex)});
      cmd.bind_pipeline(trace_pass);
      cmd.bind_descriptors_compute(0, {set}, {blk.offset});
      cmd.dispatch(desc.width/8, desc.height/4, 1);
    });
}

// ==== backbuffer subpass (backbuffer_subpass2.cpp) =======================================================
vkr_texdraw_push texdraw_push(DrawTex flags) { return vkr_texdraw_push {uint32_t(flags)}; }

namespace {
// :17-20,27-28,38-50: what both overloads share once the texture view exists.  `texture`: the view of a graph image
// (declared by the builder), or none, in which case `image` is bound directly (:74-77).
struct BackbufData {
  rendergraph::ImageViewId backbuff_view;
  rendergraph::ImageViewId texture_view;
  std::shared_ptr<gpu::ImageViewObject> direct_view;  // lives as long as the task: the set only holds a pointer to it
};

void record_backbuffer_subpass(RenderGraph &graph, const ImageResourceId *draw_img, gpu::ImagePtr image, VkSampler sampler, DrawTex flags) {
  gpu::GraphicsPipeline pipeline = fullscreen_pipeline("texdraw");
  pipeline.set_rendersubpass({false, {graph.get_descriptor(graph.get_backbuffer()).format}});
  const vkr_texdraw_push pc = texdraw_push(flags);
  graph.add_task<BackbufData>("BackbufSubpass",
    [&](BackbufData &data, rendergraph::RenderGraphBuilder &builder) {
      data.backbuff_view = builder.use_backbuffer_attachment();
      if (draw_img) data.texture_view = builder.sample_image(*draw_img, VK_SHADER_STAGE_FRAGMENT_BIT, 0, 0, 1, 0, 1);
    },
    [=](BackbufData &data, rendergraph::RenderResources &resources, gpu::CmdContext &cmd) {
      const auto ext = resources.get_image(data.backbuff_view)->get_extent();
      VkImageView texture;
      if (image) {  // :74: a view of every mip of the image; the program samples its base level
        gpu::ImageViewRange range;
        range.aspect = image->get_info().aspect; range.base_mip = 0; range.mips_count = image->get_mip_levels();
        data.direct_view = std::make_shared<gpu::ImageViewObject>(gpu::ImageViewObject {image.get(), range});
        texture = (VkImageView)data.direct_view.get();
      } else {
        texture = resources.get_view(data.texture_view);
      }
      VkDescriptorSet set = resources.allocate_set(pipeline, 0);
      gpu::write_set(set, gpu::TextureBinding {0, texture, sampler});
      cmd.set_framebuffer(ext.width, ext.height, {resources.get_image_range(data.backbuff_view)});
      cmd.bind_pipeline(pipeline);
      cmd.clear_color_attachments(0.f, 0.f, 0.f, 0.f);
      cmd.bind_descriptors_graphics(0, {set}, {});
      cmd.push_constants_graphics(VK_SHADER_STAGE_FRAGMENT_BIT, 0, sizeof(pc), &pc);
      cmd.bind_viewport(0.f, 0.f, float(ext.width), float(ext.height), 0.f, 1.f);
      cmd.bind_scissors(0, 0, ext.width, ext.height);
      cmd.draw(3, 1, 0, 0);
      imgui_draw(nullptr);
      cmd.end_renderpass();
    });
}
}  // namespace

void add_backbuffer_subpass(RenderGraph &graph, ImageResourceId draw_img, VkSampler sampler, DrawTex flags) {
  record_backbuffer_subpass(graph, &draw_img, nullptr, sampler, flags);
}

void add_backbuffer_subpass(RenderGraph &graph, gpu::ImagePtr &image, VkSampler sampler, DrawTex flags) {
  if (!image) throw std::runtime_error {"add_backbuffer_subpass: null image"};
  record_backbuffer_subpass(graph, nullptr, image, sampler, flags);
}

// :95-104: task "presentPrepare" hands the backbuffer over; nothing executes
void add_present_subpass(RenderGraph &graph) {
  struct Nil {};
  graph.add_task<Nil>("presentPrepare",
    [&](Nil &, rendergraph::RenderGraphBuilder &builder) { builder.prepare_backbuffer(); },
    [=](Nil &, rendergraph::RenderResources &, gpu::CmdContext &) {});
}
