// reflections_rt.hip — program "reflections_rt".
//
// No reference program.  The `reflections` image of AdvancedSSR traced through the scene's ray-query structure (accel.hip)
// instead of marched through the depth pyramid: per pixel the mirror ray of the view direction, its CLOSEST hit
// (wave_closest_hit of accel_traverse.hpp), and the albedo of the hit triangle at the hit's texture coordinates: the "radiance =
// albedo at the hit" of ssr/filter.comp, with alpha 0 as the filter stores it.  Screen-space reflections go black wherever the
// ray leaves the screen or passes behind geometry; this pass has an answer there.  It writes every pixel, or, with
// VKR_REFLECT_RT_FILL_MISSES, only the pixels whose screen-space ray is invalid, in place on the filter's output.  The rule is
// frozen in DESIGN_NUMERICS.md (Reflections, ray traced) and restated in tests/reflections_rt_reference.py.
//
// A wave is an 8 x 8 pixel tile, a block four waves (16 x 16 pixels) with one 64-word stack each and the sRGB decode table in
// LDS, as k_shadow_mask_rt.  Lanes without a ray (outside the image, sky, a kept texel, a surface seen from behind) follow the
// walk with live = false.  The hit is shaded after the walk: the attribute record, the texture table and the four texels are
// not alive while the wave descends.  The pass itself, shade_hit and the entry's gates are reflections_rt.hpp, which
// accel_cutout.hip instantiates a second time with the walk that sees alpha cutouts.
#include "reflections_rt.hpp"

namespace vkr {

__global__ __launch_bounds__(256) void k_reflections_rt(ReflectRtArgs a) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  __shared__ float s_lut[VKR_SRGB_LUT_SIZE];
  reflections_rt_pixels(a, stacks, s_lut, [&](f3 o, f3 d, bool cast, uint32_t* stack, vkr_accel_hit* h) {
    wave_closest_hit(a.accel, o, d, a.tmin, a.max_distance, cast, stack, h);
  });
}

}  // namespace vkr

using namespace vkr;

extern "C" uint64_t vkr_reflections_rt_scratch_bytes(uint32_t texture_count) { return ReflectRtLayout(texture_count).total; }

extern "C" int vkr_reflections_rt(const vkr_img* depth, const vkr_img* normal, const vkr_img* rays, const vkr_accel* accel,
                                  const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                                  const vkr_reflect_rt_params* params, const vkr_img* out_reflections, void* scratch, uint64_t scratch_bytes,
                                  void* stream) {
  ReflectRtArgs a;
  VKR_TRY(reflections_rt_args("reflections_rt", depth, normal, rays, accel, attribs, attrib_count, textures, texture_count, params, false, nullptr,
                              out_reflections, scratch, scratch_bytes, (hipStream_t)stream, &a));
  const dim3 tiles(16, 16);
  hipLaunchKernelGGL(k_reflections_rt, grid2d(a.out.w, a.out.h, tiles), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("reflections_rt");
}
