// reflections_rt_lit.hip — program "reflections_rt_lit" and its twin that sees alpha cutouts.
//
// No reference program.  vkr_reflections_rt whose hit is lit and shadowed before it is stored, so that a reflected object looks
// as the object itself does under defered_shading and the traced shadow mask: per pixel the mirror ray and its CLOSEST hit
// (exactly the unlit pass's), then the hit's position and shading normal (vkr_hit_normal, interpolated and turned towards the
// ray), then per light one shadow ray from the hit through the long-ray ANY-hit walk (wave_any_hit_walk<true>), a diffuse term
// with the falloff of defered_shading's direct light, and the albedo of the hit times ambient plus the sum.  The rule is frozen in
// DESIGN_NUMERICS.md (Reflections, ray traced, lit) and restated in tests/reflections_rt_lit_reference.py.
//
// The kernel has the shape of k_reflections_rt: an 8 x 8 tile per wave, four waves per block, one 64-word stack per wave and the
// sRGB table in LDS.  It is the first kernel of the family that walks twice: after the closest walk the wave's stack is empty and
// serves the shadow walks.  The light loop is wave-uniform; a lane is live in it only when it hit and faces the light, and a wave
// without any hit skips it.  The albedo is fetched after the last shadow walk: the attribute record, the texture table and the
// texels are not alive while the wave descends (reflections_rt_lit.hpp).
#include "reflections_rt_lit.hpp"

namespace vkr {

__global__ __launch_bounds__(256) void k_reflections_rt_lit(ReflectLitArgs a) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  __shared__ float s_lut[VKR_SRGB_LUT_SIZE];
  reflections_rt_pixels(
      a, stacks, s_lut,
      [&](f3 o, f3 d, bool cast, uint32_t* stack, vkr_accel_hit* h) { wave_closest_hit(a.accel, o, d, a.tmin, a.max_distance, cast, stack, h); },
      [&](f3 o, f3 d, bool hit, const vkr_accel_hit& h, uint32_t* stack) {
        return shade_hit_lit(a, o, d, hit, h, s_lut, stack, [&](f3 po, f3 dvec, bool live, uint32_t* st) {
          return wave_any_hit_walk<true>(a.accel, po, dvec, a.shadow_tmin, 1.0f, live, st);
        });
      });
}

// the same with the cutout filter in both walks: the mirror ray and the light pass through holes
__global__ __launch_bounds__(256) void k_reflections_rt_lit_cutout(ReflectLitArgs a, uint32_t alpha_lod, uint32_t opaque_mask) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  __shared__ float s_lut[VKR_SRGB_LUT_SIZE];
  const CutoutFilter f{a.attribs, a.textures, a.texture_count, alpha_lod, opaque_mask};
  reflections_rt_pixels(
      a, stacks, s_lut,
      [&](f3 o, f3 d, bool cast, uint32_t* stack, vkr_accel_hit* h) { wave_closest_hit_walk<false>(a.accel, o, d, a.tmin, a.max_distance, cast, stack, h, f); },
      [&](f3 o, f3 d, bool hit, const vkr_accel_hit& h, uint32_t* stack) {
        return shade_hit_lit(a, o, d, hit, h, s_lut, stack, [&](f3 po, f3 dvec, bool live, uint32_t* st) {
          return wave_any_hit_walk<true>(a.accel, po, dvec, a.shadow_tmin, 1.0f, live, st, f);
        });
      });
}

}  // namespace vkr

using namespace vkr;

extern "C" int vkr_reflections_rt_lit(const vkr_img* depth, const vkr_img* normal, const vkr_img* rays, const vkr_accel* accel,
                                      const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_hit_normal* normals, uint32_t normal_count,
                                      const vkr_img* textures, uint32_t texture_count, const vkr_reflect_rt_params* params,
                                      const vkr_reflect_lights* lights, const vkr_img* out_reflections, void* scratch, uint64_t scratch_bytes,
                                      void* stream) {
  ReflectLitArgs a;
  VKR_TRY(reflections_rt_lit_args("reflections_rt_lit", depth, normal, rays, accel, attribs, attrib_count, normals, normal_count, textures, texture_count,
                                  params, lights, false, nullptr, out_reflections, scratch, scratch_bytes, (hipStream_t)stream, &a));
  const dim3 tiles(16, 16);
  hipLaunchKernelGGL(k_reflections_rt_lit, grid2d(a.out.w, a.out.h, tiles), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("reflections_rt_lit");
}

extern "C" int vkr_reflections_rt_lit_cutout(const vkr_img* depth, const vkr_img* normal, const vkr_img* rays, const vkr_accel* accel,
                                             const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_hit_normal* normals,
                                             uint32_t normal_count, const vkr_img* textures, uint32_t texture_count,
                                             const vkr_reflect_rt_params* params, const vkr_reflect_lights* lights, const vkr_ray_cutout* cutout,
                                             const vkr_img* out_reflections, void* scratch, uint64_t scratch_bytes, void* stream) {
  ReflectLitArgs a;
  VKR_TRY(reflections_rt_lit_args("reflections_rt_lit_cutout", depth, normal, rays, accel, attribs, attrib_count, normals, normal_count, textures,
                                  texture_count, params, lights, true, cutout, out_reflections, scratch, scratch_bytes, (hipStream_t)stream, &a));
  const dim3 tiles(16, 16);
  hipLaunchKernelGGL(k_reflections_rt_lit_cutout, grid2d(a.out.w, a.out.h, tiles), dim3(256), 0, (hipStream_t)stream, a, cutout->alpha_lod,
                     cutout->opaque_texture_mask);
  return launch_status("reflections_rt_lit_cutout");
}
