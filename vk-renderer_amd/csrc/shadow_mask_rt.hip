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
// and never leave ahead of a ballot.  Latency is hidden by resident waves: 8 per SIMD.  The pass itself and the
// entry's gates are shadow_mask_rt.hpp, which accel_cutout.hip instantiates a second time with the walk that sees alpha cutouts.
#include "shadow_mask_rt.hpp"

// tools/shadow_mask_rt_timing.py builds this file a second time with the segment-box walk under another entry name, to
// measure the per-ray cull against it; the library is built with the defaults
#ifndef VKR_SHADOW_RT_WALK
#define VKR_SHADOW_RT_WALK wave_any_hit_ray
#endif
#ifndef VKR_SHADOW_RT_ENTRY
#define VKR_SHADOW_RT_ENTRY vkr_shadow_mask_rt
#endif

namespace vkr {

__global__ __launch_bounds__(256) void k_shadow_mask_rt(ShadowMaskRtArgs a) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  shadow_mask_rt_pixels(a, stacks, [&](f3 o, f3 d, bool cast, uint32_t* stack) { return VKR_SHADOW_RT_WALK(a.accel, o, d, a.tmin, 1.0f, cast, stack); });
}

}  // namespace vkr

using namespace vkr;

extern "C" int VKR_SHADOW_RT_ENTRY(const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel, const vkr_shadow_rt_params* params,
                                   const vkr_img* out_mask, void* stream) {
  ShadowMaskRtArgs a;
  VKR_TRY(shadow_mask_rt_args("shadow_mask_rt", depth, normal, accel, params, out_mask, &a));
  const dim3 tiles(16, 16);
  hipLaunchKernelGGL(k_shadow_mask_rt, grid2d(a.out.w, a.out.h, tiles), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("shadow_mask_rt");
}
