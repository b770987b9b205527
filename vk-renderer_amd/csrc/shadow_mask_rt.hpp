// shadow_mask_rt.hpp — program "shadow_mask_rt" but for the walk: the kernel argument, the pass over the pixels of a block with
// the any-hit of a lane's ray handed in, and every gate of the entry.  shadow_mask_rt.hip instantiates it with the opaque walk,
// accel_cutout.hip with the walk that sees alpha cutouts.
#ifndef VKR_SHADOW_MASK_RT_HPP
#define VKR_SHADOW_MASK_RT_HPP

#include "rt_surface.hpp"

#include <cmath>

namespace vkr {

#define SMRT_MAX_LIGHTS 4

// All of it wave-uniform: a kernel argument, read through scalar loads
struct ShadowMaskRtArgs : RtSurfaceArgs {
  float lights[SMRT_MAX_LIGHTS][4];
  uint32_t light_count;  // 1..4
  float normal_offset, tmin;
};

// the pass; `walk(origin, dvec, cast, stack)` is the any-hit of a lane's ray, called by the whole wave
template <class Walk>
VKR_DEV void shadow_mask_rt_pixels(const ShadowMaskRtArgs& a, uint32_t (*stacks)[ACCEL_STACK], const Walk& walk) {
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
        lit = cast && !walk(s.origin, dvec, cast, stacks[p.wave]);
      if (p.geometry && !lit) result &= ~(0xFFu << (8u * l));
    }
  }
  if (p.inside) *texel_ptr<uint32_t>(a.out, p.lx, p.ly) = result;
}

// every gate of the pass and its kernel argument, under `program`'s prefix
inline int shadow_mask_rt_args(const char* program, const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel,
                               const vkr_shadow_rt_params* params, const vkr_img* out_mask, ShadowMaskRtArgs* a) {
  static_assert(sizeof(vkr_shadow_rt_params) == 160, "vkr_shadow_rt_params: a matrix, four floats, four lights and four words");
  VKR_TRY(rt_surface_require(program, "out_mask", depth, normal, accel, params, out_mask));
  if (params->light_count < 1 || params->light_count > SMRT_MAX_LIGHTS) {
    set_error("%s: light_count %u, expected 1..%d", program, params->light_count, SMRT_MAX_LIGHTS);
    return VKR_ERR_EXTENT;
  }
  for (uint32_t l = 0; l < params->light_count; l++)
    if (!(params->lights[l][3] == 0.0f || params->lights[l][3] == 1.0f)) {
      set_error("%s: light %u has w = %g, expected 1 (a point light) or 0 (a directional light)", program, l, (double)params->lights[l][3]);
      return VKR_ERR_EXTENT;
    }
  if (params->reserved != 0) { set_error("%s: reserved is %u, must be 0", program, params->reserved); return VKR_ERR_EXTENT; }
  if (std::isnan(params->tmin)) { set_error("%s: tmin is NaN", program); return VKR_ERR_EXTENT; }
  VKR_TRY(rt_surface_bind(program, "out_mask", depth, normal, accel, params, out_mask, a));
  VKR_TRY(rt_surface_one_extent(program, "out_mask", *a));
  for (uint32_t l = 0; l < SMRT_MAX_LIGHTS; l++)
    for (int k = 0; k < 4; k++) a->lights[l][k] = l < params->light_count ? params->lights[l][k] : 0.0f;
  a->light_count = params->light_count;
  a->normal_offset = params->normal_offset;
  a->tmin = params->tmin;
  return VKR_OK;
}

}  // namespace vkr

#endif
