// accel_cutout.hip — vkr_accel_occluded_cutout and vkr_accel_closest_cutout: the any-hit and the closest hit of arbitrary rays
// that see the holes of alpha-tested triangles (DESIGN_NUMERICS.md, "Ray query, cutouts"), and vkr_accel_cutout_scratch_bytes.
// The kernels are k_accel_occluded's and k_accel_closest's with the cutout filter of ray_cutout.hpp in the walk: a candidate
// whose albedo alpha at the hit is exactly 0 neither retires an any-hit lane nor shrinks the far bound of a closest-hit lane.
// Only alpha is read: no sRGB table in LDS.  And vkr_shadow_mask_rt_cutout and vkr_reflections_rt_cutout: programs
// "shadow_mask_rt" and "reflections_rt" (shadow_mask_rt.hpp, reflections_rt.hpp) with the same filter in their walks: the light
// and the mirror ray pass through holes.
#include "ray_cutout.hpp"
#include "reflections_rt.hpp"
#include "shadow_mask_rt.hpp"

namespace vkr {

__global__ __launch_bounds__(256) void k_accel_occluded_cutout(AccelView a, CutoutFilter f, const float* org, const float* dir, float tmin,
                                                               float tmax, uint32_t n, uint32_t* out) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  const RayLane r = load_ray_lane(org, dir, n, stacks);
  const bool hit = wave_any_hit_walk<true>(a, r.o, r.d, tmin, tmax, r.live, r.stack, f);
  if (r.live) out[r.i] = hit ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_accel_closest_cutout(AccelView a, CutoutFilter f, const float* org, const float* dir, float tmin,
                                                              float tmax, uint32_t n, vkr_accel_hit* out) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  const RayLane r = load_ray_lane(org, dir, n, stacks);
  vkr_accel_hit h;
  wave_closest_hit_walk<false>(a, r.o, r.d, tmin, tmax, r.live, r.stack, &h, f);
  if (r.live) store_u32x4((uint8_t*)(out + r.i), __float_as_uint(h.t), __float_as_uint(h.u), __float_as_uint(h.v), h.index);
}

// k_shadow_mask_rt with the filter in the walk
__global__ __launch_bounds__(256) void k_shadow_mask_rt_cutout(ShadowMaskRtArgs a, CutoutFilter f) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  shadow_mask_rt_pixels(a, stacks, [&](f3 o, f3 d, bool cast, uint32_t* stack) { return wave_any_hit_walk<true>(a.accel, o, d, a.tmin, 1.0f, cast, stack, f); });
}

// k_reflections_rt with the filter in the walk; what the ray hits behind a hole is shaded as any hit (the sRGB table is for that)
__global__ __launch_bounds__(256) void k_reflections_rt_cutout(ReflectRtArgs a, uint32_t alpha_lod, uint32_t opaque_mask) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  __shared__ float s_lut[VKR_SRGB_LUT_SIZE];
  const CutoutFilter f{a.attribs, a.textures, a.texture_count, alpha_lod, opaque_mask};
  reflections_rt_pixels(a, stacks, s_lut, [&](f3 o, f3 d, bool cast, uint32_t* stack, vkr_accel_hit* h) {
    wave_closest_hit_walk<false>(a.accel, o, d, a.tmin, a.max_distance, cast, stack, h, f);
  });
}

}  // namespace vkr

using namespace vkr;

extern "C" uint64_t vkr_accel_cutout_scratch_bytes(uint32_t texture_count) { return CutoutLayout(texture_count).total; }

extern "C" int vkr_accel_occluded_cutout(const vkr_accel* accel, const float* origins, const float* dirs, float tmin, float tmax, uint32_t n,
                                         const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                                         const vkr_ray_cutout* cutout, uint32_t* out_hit, void* scratch, uint64_t scratch_bytes, void* stream) {
  VKR_TRY(check_ray_batch("accel_occluded_cutout", accel, origins, dirs, out_hit, n));
  if (n == 0) return VKR_OK;
  CutoutFilter f;
  VKR_TRY(bind_cutout("accel_occluded_cutout", accel, attribs, attrib_count, textures, texture_count, cutout, scratch, scratch_bytes, (hipStream_t)stream, &f));
  hipLaunchKernelGGL(k_accel_occluded_cutout, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, view_of(accel), f, origins, dirs, tmin, tmax, n,
                     out_hit);
  return launch_status("accel_occluded_cutout");
}

extern "C" int vkr_accel_closest_cutout(const vkr_accel* accel, const float* origins, const float* dirs, float tmin, float tmax, uint32_t n,
                                        const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                                        const vkr_ray_cutout* cutout, vkr_accel_hit* out_hits, void* scratch, uint64_t scratch_bytes, void* stream) {
  VKR_TRY(check_ray_batch("accel_closest_cutout", accel, origins, dirs, out_hits, n));
  if (n == 0) return VKR_OK;
  if (((uintptr_t)out_hits & 15u) != 0) { set_error("accel_closest_cutout: out_hits must be 16-byte aligned"); return VKR_ERR_LAYOUT; }
  CutoutFilter f;
  VKR_TRY(bind_cutout("accel_closest_cutout", accel, attribs, attrib_count, textures, texture_count, cutout, scratch, scratch_bytes, (hipStream_t)stream, &f));
  hipLaunchKernelGGL(k_accel_closest_cutout, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, view_of(accel), f, origins, dirs, tmin, tmax, n,
                     out_hits);
  return launch_status("accel_closest_cutout");
}

extern "C" int vkr_shadow_mask_rt_cutout(const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel, const vkr_hit_attrib* attribs,
                                         uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count, const vkr_shadow_rt_params* params,
                                         const vkr_ray_cutout* cutout, const vkr_img* out_mask, void* scratch, uint64_t scratch_bytes, void* stream) {
  ShadowMaskRtArgs a;
  VKR_TRY(shadow_mask_rt_args("shadow_mask_rt_cutout", depth, normal, accel, params, out_mask, &a));
  CutoutFilter f;
  VKR_TRY(bind_cutout("shadow_mask_rt_cutout", accel, attribs, attrib_count, textures, texture_count, cutout, scratch, scratch_bytes, (hipStream_t)stream, &f));
  const dim3 tiles(16, 16);
  hipLaunchKernelGGL(k_shadow_mask_rt_cutout, grid2d(a.out.w, a.out.h, tiles), dim3(256), 0, (hipStream_t)stream, a, f);
  return launch_status("shadow_mask_rt_cutout");
}

extern "C" int vkr_reflections_rt_cutout(const vkr_img* depth, const vkr_img* normal, const vkr_img* rays, const vkr_accel* accel,
                                         const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                                         const vkr_reflect_rt_params* params, const vkr_ray_cutout* cutout, const vkr_img* out_reflections,
                                         void* scratch, uint64_t scratch_bytes, void* stream) {
  ReflectRtArgs a;
  VKR_TRY(reflections_rt_args("reflections_rt_cutout", depth, normal, rays, accel, attribs, attrib_count, textures, texture_count, params, true, cutout,
                              out_reflections, scratch, scratch_bytes, (hipStream_t)stream, &a));
  const dim3 tiles(16, 16);
  hipLaunchKernelGGL(k_reflections_rt_cutout, grid2d(a.out.w, a.out.h, tiles), dim3(256), 0, (hipStream_t)stream, a, cutout->alpha_lod,
                     cutout->opaque_texture_mask);
  return launch_status("reflections_rt_cutout");
}
