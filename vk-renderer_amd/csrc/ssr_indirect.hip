// ssr_indirect.hip — the tile-classified stochastic SSR trace the reference ships but leaves commented
// out of AdvancedSSR::run (advanced_ssr.cpp:548-550): programs
// "sssr_classification" (classification.comp), "sssr_trace_indirect" (trace_indirect.comp) and the
// SSSR_Clear transfer (advanced_ssr.cpp:440-452).
//
// HIP has no dispatch-indirect: the trace is launched over the upper bound of the tile list and
// every workgroup compares its index with the count the classification left in the indirect-args
// buffer (VkDispatchIndirectCommand.x), exiting at once when it is beyond — an empty workgroup costs
// a few cycles, and nothing returns to the host between the two passes.
#include "ssr_sampling.hpp"

namespace vkr {

// advanced_ssr.cpp:447-450: VkDispatchIndirectCommand{0, 1, 1} into both argument buffers
__global__ void k_sssr_clear_indirect(uint32_t* reflective, uint32_t* glossy) {
  if (threadIdx.x < 3) {
    const uint32_t v = threadIdx.x == 0 ? 0u : 1u;
    reflective[threadIdx.x] = v;
    glossy[threadIdx.x] = v;
  }
}

// classification.comp:38-98.  One wave per 8x8 tile; the shared-memory tree (offsets 32,16,...,1,
// element t += element t+offset) is the same pairing as wave shuffles by the same offsets, so lane 0
// ends with the identical fp32 sum.
__global__ __launch_bounds__(64) void k_sssr_classification(Tex material, int32_t* reflective_tiles, int32_t* glossy_tiles,
                                                            uint32_t* reflective_args, uint32_t* glossy_args, int tex_w, int tex_h,
                                                            float max_roughness, float glossy_value) {
  __shared__ float s_lut[VKR_SRGB_LUT_SIZE];
  const int tid = threadIdx.x;
  srgb_lut_stage(s_lut, tid, 64);
  __syncthreads();
  const int px = blockIdx.x * 8 + (tid & 7), py = blockIdx.y * 8 + (tid >> 3);
  float sampled_roughness = 1.0f;
  if (px < tex_w && py < tex_h) {
    const f2 screen_uv = mk2((float)px / (float)tex_w, (float)py / (float)tex_h);
    sampled_roughness = sample_srgb_channel(material, screen_uv, 1, s_lut);
  }
  float v = mixf(0.0f, max_roughness, sampled_roughness);
#pragma unroll
  for (int offset = 32; offset != 0; offset >>= 1) v = v + __shfl_down(v, offset, 64);
  if (tid == 0) {
    const float average_roughness = v / 64.0f;
    const int tiles_x = (tex_w + 7) / 8;
    const int tile_index = blockIdx.y * tiles_x + blockIdx.x;
    if (average_roughness < glossy_value) reflective_tiles[atomicAdd(reflective_args, 1u)] = tile_index;
    else glossy_tiles[atomicAdd(glossy_args, 1u)] = tile_index;
  }
}

struct TraceIndirectArgs {
  Pyramid depth;
  Tex normal, material, out_ray;
  const float4* halton;
  const int32_t* tiles;
  const uint32_t* args;  // VkDispatchIndirectCommand: x = number of tiles
  Mat4 normal_mat;
  Proj pr;
  uint32_t frame_random, reflection_type;
  float max_roughness;
  MarchQuotients mq;  // at most_detailed_mip 0 (mirror tiles) or 1 (glossy)
  float f_over_fn;    // zfar / (zfar - znear) (gbuffer_encode.glsl:77)
};

// trace_indirect.comp:43-135.  One wave per listed tile.
__global__ __launch_bounds__(64) void k_sssr_trace_indirect(TraceIndirectArgs a) {
  if (blockIdx.x >= *a.args) return;  // beyond the indirect count
  __shared__ uint4 s_mip[16];
  __shared__ float s_lut[VKR_SRGB_LUT_SIZE];
  const int tid = threadIdx.x;
  srgb_lut_stage(s_lut, tid, 64);
  stage_mip_table(a.depth, tid, s_mip);
  __syncthreads();
  const int tile_index = a.tiles[blockIdx.x];
  const int tile_width = (a.out_ray.fw + 7) / 8;
  const int gx = 8 * (tile_index % tile_width) + (tid & 7), gy = 8 * (tile_index / tile_width) + (tid >> 3);
  if (gx >= a.out_ray.fw || gy >= a.out_ray.fh) return;
  const f2 tex_size = mk2((float)a.out_ray.fw, (float)a.out_ray.fh);
  const f2 screen_uv = mk2((float)gx / tex_size.x, (float)gy / tex_size.y);  // no +0.5 (trace_indirect.comp:51)
  const Proj pr = a.pr;
  const Tex& depth0 = a.depth.mip[0];

  float roughness = sample_srgb_channel(a.material, screen_uv, 1, s_lut);
  roughness = mixf(0.0f, a.max_roughness, roughness);
  roughness *= roughness;
  const float pixel_depth = sample<FmtD24>(depth0, screen_uv);
  RayConst rc;
  rc.normal = sample_view_normal(a.normal, a.normal_mat, screen_uv);
  rc.view_vec = reconstruct_view_vec(screen_uv, pixel_depth, pr);
  const f3 R = setup_ray(rc, screen_uv, roughness, a.halton, a.frame_random, pr, a.f_over_fn);

  // mirror tiles: hierarchical_raymarch(DEPTH, start, dir, 0, 50); glossy: (.., 1, 25)  (:98-102)
  const int min_mip = a.reflection_type == 0 ? 0 : 1;
  const int max_steps = a.reflection_type == 0 ? 50 : 25;
  const MarchEnv env = march_env(s_mip, a.depth.count, depth0, pr, a.mq, min_mip, 0.0f);
  RayState st;
  st.t = initial_advance(env, rc);
  st.h = 0.0f; st.mip = min_mip; st.i = 0;
  bool more = max_steps > 0;
#pragma unroll 1
  while (more) more = march_step<false, 0>(env, rc, st, max_steps);
  const f3 out_ray = madd(rc.origin, st.t, rc.direction);

  // trace_indirect.comp:104-128; i <= max always (screen_trace.glsl:97); the depth window only for mirror tiles
  bool valid_hit = ray_moved(out_ray, rc.origin, tex_size);
  if (valid_hit && (hit_faces_away(a.normal, a.normal_mat, xy(out_ray), R) || dot(rc.normal, R) < 0.0f)) valid_hit = false;
  if (valid_hit && a.reflection_type == 0) valid_hit = hit_depth_in_window(depth0, out_ray, pr);
  const int lx = gx - a.out_ray.ox, ly = gy - a.out_ray.oy;
  if (lx < 0 || ly < 0 || lx >= a.out_ray.w || ly >= a.out_ray.h) return;
  store_ray(a.out_ray, lx, ly, out_ray, valid_hit, pixel_depth);
}

}  // namespace vkr

using namespace vkr;

extern "C" int vkr_sssr_clear_indirect(uint32_t* reflective_args, uint32_t* glossy_args, void* stream) {
  if (!reflective_args || !glossy_args) { set_error("sssr_clear: NULL argument buffer"); return VKR_ERR_NULL; }
  hipLaunchKernelGGL(k_sssr_clear_indirect, dim3(1), dim3(64), 0, (hipStream_t)stream, reflective_args, glossy_args);
  return launch_status("sssr_clear");
}

extern "C" int vkr_sssr_classification(const vkr_img* material, int32_t* reflective_tiles, int32_t* glossy_tiles,
                                       uint32_t* reflective_args, uint32_t* glossy_args,
                                       const vkr_classification_push* push, void* stream) {
  if (!push || !reflective_tiles || !glossy_tiles || !reflective_args || !glossy_args) { set_error("sssr_classification: NULL argument"); return VKR_ERR_NULL; }
  if (push->width <= 0 || push->height <= 0) { set_error("sssr_classification: empty extent"); return VKR_ERR_EXTENT; }
  Tex m;
  VKR_TRY(make_tex(material, 0, VKR_FMT_RGBA8_SRGB, "sssr_classification.material", &m));
  dim3 grid((push->width + 7) / 8, (push->height + 7) / 8);
  hipLaunchKernelGGL(k_sssr_classification, grid, dim3(64), 0, (hipStream_t)stream, m, reflective_tiles, glossy_tiles, reflective_args,
                     glossy_args, push->width, push->height, push->max_roughness, push->glossy_value);
  return launch_status("sssr_classification");
}

extern "C" int vkr_sssr_trace_indirect(const vkr_img* depth, const vkr_img* normal, const vkr_img* material,
                                       const vkr_trace_params* params, const float* halton_vec4, const vkr_img* out_rays,
                                       const int32_t* tiles, const uint32_t* indirect_args, uint32_t max_tiles,
                                       const vkr_trace_indirect_push* push, void* stream) {
  if (!params || !push || !halton_vec4 || !tiles || !indirect_args || !depth) { set_error("sssr_trace_indirect: NULL argument"); return VKR_ERR_NULL; }
  if (push->reflection_type > 1) { set_error("sssr_trace_indirect: reflection_type %u", push->reflection_type); return VKR_ERR_EXTENT; }
  TraceIndirectArgs a;
  VKR_TRY(bind_depth_pyramid(depth, "sssr_trace_indirect", "depth", &a.depth));
  VKR_TRY(make_tex(normal, 0, VKR_FMT_RG16_UNORM, "sssr_trace_indirect.normal", &a.normal));
  VKR_TRY(make_tex(material, 0, VKR_FMT_RGBA8_SRGB, "sssr_trace_indirect.material", &a.material));
  VKR_TRY(make_tex(out_rays, 0, VKR_FMT_RGBA16_UNORM, "sssr_trace_indirect.rays", &a.out_ray));
  a.halton = (const float4*)halton_vec4;
  a.tiles = tiles;
  a.args = indirect_args;
  load_mat(a.normal_mat, params->normal_mat);
  load_proj(a.pr, params->fovy, params->aspect, params->znear, params->zfar);
  load_march_quotients(a.mq, a.depth.mip[0], push->reflection_type == 0 ? 0 : 1);
  a.f_over_fn = a.pr.zfar / (a.pr.zfar - a.pr.znear);
  a.frame_random = params->frame_random;
  a.reflection_type = push->reflection_type;
  a.max_roughness = push->max_roughness;
  const uint32_t all_tiles = (uint32_t)((a.out_ray.fw + 7) / 8) * (uint32_t)((a.out_ray.fh + 7) / 8);
  const uint32_t bound = max_tiles < all_tiles ? max_tiles : all_tiles;
  if (bound == 0) return VKR_OK;
  hipLaunchKernelGGL(k_sssr_trace_indirect, dim3(bound), dim3(64), 0, (hipStream_t)stream, a);
  return launch_status("sssr_trace_indirect");
}
