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
#include "rt_surface.hpp"

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
struct ShadowMaskRtArgs : RtSurfaceArgs {
  float lights[SMRT_MAX_LIGHTS][4];
  uint32_t light_count;  // 1..4
  float normal_offset, tmin;
};

__global__ __launch_bounds__(256) void k_shadow_mask_rt(ShadowMaskRtArgs a) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  const RtPixel p = rt_pixel(a);
  uint32_t result = 0xFFFFFFFFu;
  if (__ballot(p.geometry) != 0ull) {  // the whole wave
    const RtSurface s = rt_surface(a, p, a.normal_offset);
    for (uint32_t l = 0; l < a.light_count; l++) {  // wave-uniform
      const f3 light = mk3(a.lights[l][0], a.lights[l][1], a.lights[l][2]);
      const f3 dvec = a.lights[l][3] != 0.0f ? light - s.origin : light;
      const bool cast = p.geometry && dot(s.n, dvec) > 0.0f;  // false for a surface facing away, a light at the origin and any NaN
      bool lit = false;
      if (__ballot(cast) != 0ull)  // the whole wave: lanes without a ray follow the walk
        lit = cast && !VKR_SHADOW_RT_WALK(a.accel, s.origin, dvec, a.tmin, 1.0f, cast, stacks[p.wave]);
      if (p.geometry && !lit) result &= ~(0xFFu << (8u * l));
    }
  }
  if (p.inside) *texel_ptr<uint32_t>(a.out, p.lx, p.ly) = result;
}

}  // namespace vkr

using namespace vkr;

extern "C" int VKR_SHADOW_RT_ENTRY(const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel, const vkr_shadow_rt_params* params,
                                   const vkr_img* out_mask, void* stream) {
  static_assert(sizeof(vkr_shadow_rt_params) == 160, "vkr_shadow_rt_params: a matrix, four floats, four lights and four words");
  VKR_TRY(rt_surface_require("shadow_mask_rt", "out_mask", depth, normal, accel, params, out_mask));
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
  VKR_TRY(rt_surface_bind("shadow_mask_rt", "out_mask", depth, normal, accel, params, out_mask, &a));
  VKR_TRY(rt_surface_one_extent("shadow_mask_rt", "out_mask", a));
  for (uint32_t l = 0; l < SMRT_MAX_LIGHTS; l++)
    for (int k = 0; k < 4; k++) a.lights[l][k] = l < params->light_count ? params->lights[l][k] : 0.0f;
  a.light_count = params->light_count;
  a.normal_offset = params->normal_offset;
  a.tmin = params->tmin;
  const dim3 tiles(16, 16);
  hipLaunchKernelGGL(k_shadow_mask_rt, grid2d(a.out.w, a.out.h, tiles), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("shadow_mask_rt");
}
