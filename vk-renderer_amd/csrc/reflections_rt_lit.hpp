// reflections_rt_lit.hpp — program "reflections_rt_lit" but for its two walks: the kernel argument, the lighting of a hit with
// the any-hit of a lane's shadow ray handed in, and the gates the entries add to those of reflections_rt.hpp.  The pixel, the
// surface, the mirror ray, the fill mode and the albedo are reflections_rt.hpp's own (reflections_rt_pixels, hit_albedo); what is
// here is DESIGN_NUMERICS.md, "Reflections, ray traced, lit", from the closest hit on.
#ifndef VKR_REFLECTIONS_RT_LIT_HPP
#define VKR_REFLECTIONS_RT_LIT_HPP

#include "reflections_rt.hpp"

namespace vkr {

#define RRTL_MAX_LIGHTS 4

// All of it wave-uniform: a kernel argument, read through scalar loads
struct ReflectLitArgs : ReflectRtArgs {
  const vkr_hit_normal* normals;  // one per input triangle
  float lights[RRTL_MAX_LIGHTS][4];
  float colour[RRTL_MAX_LIGHTS][3];
  float ambient[3];
  uint32_t light_count;  // 0..4
  float shadow_offset, shadow_tmin;
};

// the shading normal of hit h for a ray along dir: the interpolated vertex normals in hit_uv's order, normalised, facing the ray
VKR_DEV f3 hit_normal(const vkr_hit_normal& nr, const vkr_accel_hit& h, f3 dir) {
  const float w = (1.0f - h.u) - h.v;
  const f3 ni = mk3((w * nr.n[0][0] + h.u * nr.n[1][0]) + h.v * nr.n[2][0], (w * nr.n[0][1] + h.u * nr.n[1][1]) + h.v * nr.n[2][1],
                    (w * nr.n[0][2] + h.u * nr.n[1][2]) + h.v * nr.n[2][2]);
  const f3 ns = normalize(ni);
  return dot(ns, dir) > 0.0f ? -ns : ns;  // a NaN stays as it is
}

// The word stored for a lane's ray (origin, dir) with closest hit h, called by the whole wave: `occluded(po, dvec, live, stack)`
// is the any-hit of a lane's shadow ray.  A lane is live in a light's walk only when it hit and faces the light; the others
// follow.  Only po, n, acc and the hit words cross the walks: the albedo is fetched behind them.
template <class Occluded>
VKR_DEV uint32_t shade_hit_lit(const ReflectLitArgs& a, f3 origin, f3 dir, bool hit, const vkr_accel_hit& h, const float* lut, uint32_t* stack,
                               const Occluded& occluded) {
  if (__ballot(hit) == 0ull) return 0u;  // the whole wave: nothing to light
  f3 n = mk3(0.0f, 0.0f, 0.0f), po = n;
  if (hit) {
    n = hit_normal(a.normals[h.index], h, dir);
    po = madd(madd(origin, h.t, dir), a.shadow_offset, n);
  }
  f3 acc = mk3(a.ambient[0], a.ambient[1], a.ambient[2]);
  for (uint32_t l = 0; l < a.light_count; l++) {  // wave-uniform
    const f3 light = mk3(a.lights[l][0], a.lights[l][1], a.lights[l][2]);
    const bool point = a.lights[l][3] != 0.0f;
    const f3 dvec = point ? light - po : light;
    const bool live = hit && dot(n, dvec) > 0.0f;  // false for a surface facing away, a light at the hit and any NaN
    if (__ballot(live) == 0ull) continue;          // the whole wave
    if (!occluded(po, dvec, live, stack) && live) {
      const float ld2 = dot(dvec, dvec);
      float k = dot(n, normalize(dvec));
      if (!(k > 0.0f)) k = 0.0f;
      if (point) {
        const float q = 1.0f / ld2;
        k = k * (q < 1.0f ? q : 1.0f);
      }
      acc = mk3(cfma(k, a.colour[l][0], acc.x), cfma(k, a.colour[l][1], acc.y), cfma(k, a.colour[l][2], acc.z));
    }
  }
  if (!hit) return 0u;
  return reflection_word(hit_albedo(a, h, lut) * acc);
}

// the gates behind reflections_rt_args' own, and the rest of the kernel argument
inline int reflections_rt_lit_gates(const char* program, const vkr_accel* accel, const vkr_hit_normal* normals, uint32_t normal_count,
                                    const vkr_reflect_lights* lights, ReflectLitArgs* a) {
  static_assert(sizeof(vkr_hit_normal) == 48, "vkr_hit_normal: three normals of four floats");
  static_assert(sizeof(vkr_reflect_lights) == 176, "vkr_reflect_lights: nine float4 and eight words");
  if (!lights) { set_error("%s: lights is NULL", program); return VKR_ERR_NULL; }
  if (accel->tri_count && !normals) { set_error("%s: normals is NULL", program); return VKR_ERR_NULL; }
  if (((uintptr_t)normals & 15u) != 0) { set_error("%s: normals must be 16-byte aligned", program); return VKR_ERR_LAYOUT; }
  if (normal_count != accel->tri_count) {
    set_error("%s: %u normal records for a structure of %u triangles (one per input triangle)", program, normal_count, accel->tri_count);
    return VKR_ERR_EXTENT;
  }
  if (lights->light_count > RRTL_MAX_LIGHTS) { set_error("%s: light_count %u, expected 0..%d", program, lights->light_count, RRTL_MAX_LIGHTS); return VKR_ERR_EXTENT; }
  for (uint32_t l = 0; l < lights->light_count; l++)
    if (!(lights->lights[l][3] == 0.0f || lights->lights[l][3] == 1.0f)) {
      set_error("%s: light %u has w = %g, expected 1 (a point light) or 0 (a directional light)", program, l, (double)lights->lights[l][3]);
      return VKR_ERR_EXTENT;
    }
  for (uint32_t l = 0; l < RRTL_MAX_LIGHTS; l++)
    if (!(lights->colour[l][3] == 0.0f)) { set_error("%s: colour %u has w = %g, must be 0", program, l, (double)lights->colour[l][3]); return VKR_ERR_EXTENT; }
  if (!(lights->ambient[3] == 0.0f)) { set_error("%s: ambient has w = %g, must be 0", program, (double)lights->ambient[3]); return VKR_ERR_EXTENT; }
  for (uint32_t r : lights->reserved)
    if (r != 0) { set_error("%s: lights: reserved must be 0", program); return VKR_ERR_EXTENT; }
  if (std::isnan(lights->shadow_offset)) { set_error("%s: shadow_offset is NaN", program); return VKR_ERR_EXTENT; }
  if (std::isnan(lights->shadow_tmin)) { set_error("%s: shadow_tmin is NaN", program); return VKR_ERR_EXTENT; }
  for (int c = 0; c < 3; c++)
    if (std::isnan(lights->ambient[c])) { set_error("%s: ambient is NaN", program); return VKR_ERR_EXTENT; }
  for (uint32_t l = 0; l < lights->light_count; l++)
    for (int c = 0; c < 3; c++)
      if (std::isnan(lights->colour[l][c])) { set_error("%s: colour %u is NaN", program, l); return VKR_ERR_EXTENT; }
  a->normals = normals;
  for (uint32_t l = 0; l < RRTL_MAX_LIGHTS; l++) {
    for (int k = 0; k < 4; k++) a->lights[l][k] = l < lights->light_count ? lights->lights[l][k] : 0.0f;
    for (int k = 0; k < 3; k++) a->colour[l][k] = l < lights->light_count ? lights->colour[l][k] : 0.0f;
  }
  for (int k = 0; k < 3; k++) a->ambient[k] = lights->ambient[k];
  a->light_count = lights->light_count;
  a->shadow_offset = lights->shadow_offset;
  a->shadow_tmin = lights->shadow_tmin;
  return VKR_OK;
}

// both entries: reflections_rt_args with the gates above behind its own
inline int reflections_rt_lit_args(const char* program, const vkr_img* depth, const vkr_img* normal, const vkr_img* rays, const vkr_accel* accel,
                                   const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_hit_normal* normals, uint32_t normal_count,
                                   const vkr_img* textures, uint32_t texture_count, const vkr_reflect_rt_params* params, const vkr_reflect_lights* lights,
                                   bool has_cutout, const vkr_ray_cutout* cutout, const vkr_img* out_reflections, void* scratch, uint64_t scratch_bytes,
                                   hipStream_t stream, ReflectLitArgs* args) {
  return reflections_rt_args(program, depth, normal, rays, accel, attribs, attrib_count, textures, texture_count, params, has_cutout, cutout,
                             out_reflections, scratch, scratch_bytes, stream, args,
                             [&] { return reflections_rt_lit_gates(program, accel, normals, normal_count, lights, args); });
}

}  // namespace vkr

#endif
