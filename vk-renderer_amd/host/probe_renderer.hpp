// probe_renderer.hpp — the probe renderer of the reference (src/probe_renderer.hpp) over the host mirror: a grid of octahedral
// probes baked from the scene (cube faces -> octahedral colour + depth -> min-depth mip chain) and the pass that traces
// reflections through it.  Programs: cubemap_probe, cube2oct, probe_downsample, trace_probe (include/vkr_postfx.h).
// Implementation: passes.cpp, with the other pass classes.
#ifndef VKR_HOST_PROBE_RENDERER_HPP_INCLUDED
#define VKR_HOST_PROBE_RENDERER_HPP_INCLUDED

#include "scene_renderer.hpp"

const uint32_t PROBE_SIZE = 256;
const uint32_t CUBE_SIZE = 128;

struct OctahedralProbe {
  OctahedralProbe(rendergraph::RenderGraph &graph, uint32_t size = PROBE_SIZE);

  glm::vec3 pos {0.f, 0.f, 0.f};
  rendergraph::ImageResourceId color;  // RGBA8_UNORM
  rendergraph::ImageResourceId depth;  // R16_UNORM, floor(log2(size)) + 1 mips
};

struct OctahedralProbeGrid {
  OctahedralProbeGrid(rendergraph::RenderGraph &graph, uint32_t grid_sz = 4, uint32_t size = PROBE_SIZE);

  glm::vec3 min {0.f, 0.f, 0.f};
  glm::vec3 max {0.f, 0.f, 0.f};
  uint32_t grid_size {0};

  rendergraph::ImageResourceId color_array;  // grid_size^2 layers; layer = y * grid_size + x
  rendergraph::ImageResourceId depth_array;  // all mips of every layer, mip-major
};

struct ProbeRenderer {
  ProbeRenderer(rendergraph::RenderGraph &graph, uint32_t cubemap_res = CUBE_SIZE);

  // the six faces (+X, -X, +Y, -Y, +Z, -Z) of the cube at pos into the renderer's cube images
  void render_cubemap(rendergraph::RenderGraph &graph, SceneRenderer &scene_renderer, const glm::vec3 pos);
  void render_probe(rendergraph::RenderGraph &graph, SceneRenderer &scene_renderer, const glm::vec3 pos, OctahedralProbe &probe);
  // probes in x and z at min.y (min / max swapped per axis where needed); throws for grid_size < 2
  void render_probe_grid(rendergraph::RenderGraph &graph, SceneRenderer &scene_renderer, glm::vec3 min, glm::vec3 max, OctahedralProbeGrid &probe_grid);

  // (not in the reference) the cube images of the last bake, for read-back
  rendergraph::ImageResourceId get_cubemap_color() const { return cubemap_color; }
  rendergraph::ImageResourceId get_cubemap_distance() const { return cubemap_distance; }

private:
  rendergraph::ImageResourceId cubemap_color;
  rendergraph::ImageResourceId cubemap_distance;
  rendergraph::ImageResourceId rt_depth;

  gpu::GraphicsPipeline cubemap_pass;
  gpu::ComputePipeline octprobe_pass;
  gpu::GraphicsPipeline downsample_pass;

  VkSampler sampler;

  void render_side(rendergraph::RenderGraph &graph, SceneRenderer &scene_renderer, uint32_t side, glm::mat4 view);
  void render_octahedral(rendergraph::RenderGraph &graph, rendergraph::ImageResourceId probe_color, rendergraph::ImageResourceId probe_depth, uint32_t array_layer = 0);
  void probe_downsample(rendergraph::RenderGraph &graph, rendergraph::ImageResourceId probe_depth, uint32_t array_layer = 0);
};

struct ProbeTraceParams {
  glm::mat4 inv_view;  // camera -> world
  float fovy;
  float aspect;
  float znear;
  float zfar;
};

struct ProbeTracePass {
  ProbeTracePass();

  void run(rendergraph::RenderGraph &graph, OctahedralProbeGrid &probe, rendergraph::ImageResourceId gbuffer_depth, rendergraph::ImageResourceId gbuffer_norm,
           rendergraph::ImageResourceId out_image, const ProbeTraceParams &params);

private:
  gpu::ComputePipeline trace_pass;
  VkSampler sampler;
};

#endif
