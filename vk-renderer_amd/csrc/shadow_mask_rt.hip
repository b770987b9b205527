// shadow_mask_rt.hip — program "shadow_mask_rt".
//
// No reference program.  The producer of the shadow mask that needs no shadow map: per full-resolution pixel one any-hit ray
// per light through the scene's ray-query structure (accel.hip), from the surface point towards the light, into the RGBA8_UNORM
// mask that vkr_shadow_mask writes and vkr_defered_shading_shadowed reads (channel l = light l).  Exact hard shadows for point
// and directional lights: no map, no frustum, no depth bias.  The rule is frozen in DESIGN_NUMERICS.md (Shadow mask, ray traced)
// and restated in tests/shadow_mask_rt_reference.py.
//
// A wave is an 8 x 8 pixel tile: its rays start close together and, for one light, aim at one point or run parallel, so the
// wave-uniform walk visits little more than one ray would.  The rays are long (surface to light), which is what
// wave_any_hit_ray of accel_traverse.hpp is for.  A block is four waves (16 x 16 pixels) with one 64-word stack each in LDS.
// The light loop is wave-uniform; lanes without a ray (outside the image, sky, facing away) follow the walk with live = false
// and never leave ahead of a ballot.  Latency is hidden by resident waves: 8 per SIMD.
#include "vkr_host.hpp"
#include "accel_traverse.hpp"

#include <cmath>

// tools/shadow_mask_rt_timing.py builds this file a second time with the segment-box walk under another entry name, to
// measure the per-ray cull against it; the library is built with the defaults
#ifndef VKR_SHADOW_RT_WALK
#define VKR_SHADOW_RT_WALK wave_any_hit_ray
#endif
#ifndef VKR_SHADOW_RT_ENTRY
#define VKR_SHADOW_RT_ENTRY vkr_shadow_mask_rt
#endif

namespace vkr {

#define SMRT_MAX_LIGHTS 4

// All of it wave-uniform: a kernel argument, read through scalar loads
struct ShadowMaskRtArgs {
  Tex depth, normal, out;
  Mat4 inverse_camera;
  Proj pr;
  AccelView accel;
  float lights[SMRT_MAX_LIGHTS][4];
  uint32_t light_count;  // 1..4
  float normal_offset, tmin;
};

// one lane per pixel of out (== depth's == normal's extent); wave w of the block is the 8 x 8 tile (w & 1, w >> 1) of its 16 x 16
__global__ __launch_bounds__(256) void k_shadow_mask_rt(ShadowMaskRtArgs a) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  const i2 blk = xcd_block<8, 8>();  // chunks of 128 x 128 pixels
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lx = blk.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int ly = blk.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool inside = lx < a.out.w && ly < a.out.h;
  const int cx = inside ? lx : 0, cy = inside ? ly : 0;  // a lane outside the image reads texel (0, 0) and writes nothing
  const float d = d24_to_float(*(const uint32_t*)(a.depth.p + toff(a.depth, cx, cy, 4)));
  const bool geometry = inside && d < 1.0f;
  uint32_t result = 0xFFFFFFFFu;
  if (__ballot(geometry) != 0ull) {  // the whole wave
    const f2 uv = mk2(pixel_centre_uv(cx, (float)a.out.w), pixel_centre_uv(cy, (float)a.out.h));
    const f3 view = reconstruct_view_vec(uv, d, a.pr);
    const f3 world = xyz(mul(a.inverse_camera, mk4(view.x, view.y, view.z, 1.0f)));
    const f3 n = decode_normal(FmtRG16U::load(a.normal, cx, cy));
    const f3 origin = madd(world, a.normal_offset, n);
    for (uint32_t l = 0; l < a.light_count; l++) {  // wave-uniform
      const f3 light = mk3(a.lights[l][0], a.lights[l][1], a.lights[l][2]);
      const f3 dvec = a.lights[l][3] != 0.0f ? light - origin : light;
      const bool cast = geometry && dot(n, dvec) > 0.0f;  // false for a surface facing away, a light at the origin and any NaN
      bool lit = false;
      if (__ballot(cast) != 0ull)  // the whole wave: lanes without a ray follow the walk
        lit = cast && !VKR_SHADOW_RT_WALK(a.accel, origin, dvec, a.tmin, 1.0f, cast, stacks[wave]);
      if (geometry && !lit) result &= ~(0xFFu << (8u * l));
    }
  }
  if (inside) *texel_ptr<uint32_t>(a.out, lx, ly) = result;
}

}  // namespace vkr

using namespace vkr;

extern "C" int VKR_SHADOW_RT_ENTRY(const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel, const vkr_shadow_rt_params* params,
                                   const vkr_img* out_mask, void* stream) {
  static_assert(sizeof(vkr_shadow_rt_params) == 160, "vkr_shadow_rt_params: a matrix, four floats, four lights and four words");
  if (!depth) { set_error("shadow_mask_rt: depth is NULL"); return VKR_ERR_NULL; }
  if (!normal) { set_error("shadow_mask_rt: normal is NULL"); return VKR_ERR_NULL; }
  if (!accel) { set_error("shadow_mask_rt: NULL acceleration structure"); return VKR_ERR_NULL; }
  if (!params) { set_error("shadow_mask_rt: params is NULL"); return VKR_ERR_NULL; }
  if (!out_mask) { set_error("shadow_mask_rt: out_mask is NULL"); return VKR_ERR_NULL; }
  if (params->light_count < 1 || params->light_count > SMRT_MAX_LIGHTS) {
    set_error("shadow_mask_rt: light_count %u, expected 1..%d", params->light_count, SMRT_MAX_LIGHTS);
    return VKR_ERR_EXTENT;
  }
  for (uint32_t l = 0; l < params->light_count; l++)
    if (!(params->lights[l][3] == 0.0f || params->lights[l][3] == 1.0f)) {
      set_error("shadow_mask_rt: light %u has w = %g, expected 1 (a point light) or 0 (a directional light)", l, (double)params->lights[l][3]);
      return VKR_ERR_EXTENT;
    }
  if (params->reserved != 0) { set_error("shadow_mask_rt: reserved is %u, must be 0", params->reserved); return VKR_ERR_EXTENT; }
  if (std::isnan(params->tmin)) { set_error("shadow_mask_rt: tmin is NaN"); return VKR_ERR_EXTENT; }
  ShadowMaskRtArgs a;
  VKR_TRY(make_tex(depth, 0, VKR_FMT_D24_UNORM_S8, "shadow_mask_rt.depth", &a.depth));
  VKR_TRY(make_tex(normal, 0, VKR_FMT_RG16_UNORM, "shadow_mask_rt.normal", &a.normal));
  VKR_TRY(make_tex(out_mask, 0, VKR_FMT_RGBA8_UNORM, "shadow_mask_rt.out_mask", &a.out));
  VKR_TRY(require_whole_frame(a.depth, "shadow_mask_rt: depth", "windows are not supported (the rays reach anywhere: a single-GPU pass)"));
  VKR_TRY(require_whole_frame(a.normal, "shadow_mask_rt: normal", "windows are not supported (the rays reach anywhere: a single-GPU pass)"));
  VKR_TRY(require_whole_frame(a.out, "shadow_mask_rt: out_mask", "windows are not supported (the rays reach anywhere: a single-GPU pass)", 65535));
  if (a.depth.w != a.out.w || a.depth.h != a.out.h || a.normal.w != a.out.w || a.normal.h != a.out.h) {
    set_error("shadow_mask_rt: depth is %dx%d, normal %dx%d, out_mask %dx%d: one extent expected", a.depth.w, a.depth.h, a.normal.w, a.normal.h,
              a.out.w, a.out.h);
    return VKR_ERR_EXTENT;
  }
  load_mat(a.inverse_camera, params->inverse_camera);
  load_proj(a.pr, params->fovy, params->aspect, params->znear, params->zfar);
  a.accel = AccelView{accel->nodes, accel->tris, accel->node_count};
  for (uint32_t l = 0; l < SMRT_MAX_LIGHTS; l++)
    for (int k = 0; k < 4; k++) a.lights[l][k] = l < params->light_count ? params->lights[l][k] : 0.0f;
  a.light_count = params->light_count;
  a.normal_offset = params->normal_offset;
  a.tmin = params->tmin;
  const dim3 tiles(16, 16);
  hipLaunchKernelGGL(k_shadow_mask_rt, grid2d(a.out.w, a.out.h, tiles), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("shadow_mask_rt");
}
