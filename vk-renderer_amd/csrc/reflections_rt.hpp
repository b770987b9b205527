// reflections_rt.hpp — program "reflections_rt" but for the walk: the kernel argument, the shading of a hit, the pass over the
// pixels of a block with the closest hit of a lane's ray handed in, the scratch layout, and every gate of the entry up to the
// launch.  reflections_rt.hip instantiates it with the opaque walk, accel_cutout.hip with the walk that sees alpha cutouts, and
// reflections_rt_lit.hip with either walk and a shading of its own (reflections_rt_lit.hpp: the hit lit and shadowed).
#ifndef VKR_REFLECTIONS_RT_HPP
#define VKR_REFLECTIONS_RT_HPP

#include "raster_common.hpp"
#include "rt_surface.hpp"
#include "ray_cutout.hpp"

#include <cmath>

namespace vkr {

// All of it wave-uniform: a kernel argument, read through scalar loads
struct ReflectRtArgs : RtSurfaceArgs {
  Tex rays;                       // read in fill mode only
  const vkr_hit_attrib* attribs;  // one per input triangle
  const Pyramid* textures;        // [texture_count], in scratch
  uint32_t texture_count, texture_lod, fill_misses;
  float normal_offset, tmin, max_distance;
};

// the albedo of triangle h.index at (h.u, h.v)
VKR_DEV f3 hit_albedo(const ReflectRtArgs& a, const vkr_accel_hit& h, const float* lut) {
  const vkr_hit_attrib at = a.attribs[h.index];
  const f2 uv = hit_uv(at, h.u, h.v);
  f3 c = mk3(0.5f, 0.5f, 0.5f);
  if (at.albedo_index < a.texture_count) {  // 0xFFFFFFFF (no texture) fails the same compare
    const Pyramid& p = a.textures[at.albedo_index];
    const uint32_t level = min(a.texture_lod, (uint32_t)(p.count - 1));
    c = xyz(sample_level_repeat(p.mip[level], uv, lut));
  }
  return c;
}
// the RGBA8_UNORM word of a colour, alpha 0
VKR_DEV uint32_t reflection_word(f3 c) { return float_to_unorm8(c.x) | (float_to_unorm8(c.y) << 8) | (float_to_unorm8(c.z) << 16); }
// the RGBA8_UNORM word of a hit: its albedo, alpha 0
VKR_DEV uint32_t shade_hit(const ReflectRtArgs& a, const vkr_accel_hit& h, const float* lut) { return reflection_word(hit_albedo(a, h, lut)); }

// what the pass stores for a lane's ray: the albedo at its hit, 0 without one
struct ShadeAlbedo {
  const ReflectRtArgs& a;
  const float* lut;
  VKR_DEV uint32_t operator()(f3, f3, bool hit, const vkr_accel_hit& h, uint32_t*) const { return hit ? shade_hit(a, h, lut) : 0u; }
};

// the pass; `walk(origin, dir, cast, stack, &hit)` is the closest hit of a lane's ray and `shade(origin, dir, hit, h, stack)` the
// word stored for it (hit: the lane cast a ray and h is its hit), both called by the whole wave
template <class Walk, class Shade>
VKR_DEV void reflections_rt_pixels(const ReflectRtArgs& a, uint32_t (*stacks)[ACCEL_STACK], float* s_lut, const Walk& walk, const Shade& shade) {
  srgb_lut_stage(s_lut, threadIdx.x, 256);
  __syncthreads();
  const RtPixel p = rt_pixel(a);
  bool keep = false;  // fill mode: the screen-space ray of this pixel is a valid hit, the filter's texel stays
  if (a.fill_misses) keep = p.geometry && (texel_ptr<const uint2>(a.rays, p.cx, p.cy)->y >> 16) != 65535u;
  const bool trace = p.geometry && !keep;
  uint32_t result = 0u;
  if (__ballot(trace) != 0ull) {  // the whole wave
    const RtSurface s = rt_surface(a, p, a.normal_offset);
    const f3 eye = mk3(a.inverse_camera.m[12], a.inverse_camera.m[13], a.inverse_camera.m[14]);
    const f3 dir = normalize(reflect(s.world - eye, s.n));
    const bool cast = trace && dot(s.n, dir) > 0.0f;  // false for a surface seen from behind, a grazing zero and any NaN
    if (__ballot(cast) != 0ull) {  // the whole wave: lanes without a ray follow the walk
      vkr_accel_hit h;
      walk(s.origin, dir, cast, stacks[p.wave], &h);
      result = shade(s.origin, dir, cast && h.index != 0xFFFFFFFFu, h, stacks[p.wave]);
    }
  }
  if (p.inside && !keep) *texel_ptr<uint32_t>(a.out, p.lx, p.ly) = result;
}
template <class Walk>
VKR_DEV void reflections_rt_pixels(const ReflectRtArgs& a, uint32_t (*stacks)[ACCEL_STACK], float* s_lut, const Walk& walk) {
  reflections_rt_pixels(a, stacks, s_lut, walk, ShadeAlbedo{a, s_lut});
}

// the scratch: the texture table, one layout for every entry that binds the scene's textures to a ray query
using ReflectRtLayout = CutoutLayout;

// every entry: every gate of the pass, its kernel argument and the upload of the texture table (recorded on the stream: the
// last step before the entry's launch), under `program`'s prefix; has_cutout: the entry takes a vkr_ray_cutout; more(): the
// gates an entry adds behind these, asked before anything is recorded
struct NoMoreGates { int operator()() const { return VKR_OK; } };
template <class More = NoMoreGates>
inline int reflections_rt_args(const char* program, const vkr_img* depth, const vkr_img* normal, const vkr_img* rays, const vkr_accel* accel,
                               const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                               const vkr_reflect_rt_params* params, bool has_cutout, const vkr_ray_cutout* cutout, const vkr_img* out_reflections, void* scratch,
                               uint64_t scratch_bytes, hipStream_t stream, ReflectRtArgs* args, const More& more = More()) {
  static_assert(sizeof(vkr_reflect_rt_params) == 112, "vkr_reflect_rt_params: a matrix, eight floats / words, the flags and three words");
  static_assert(sizeof(vkr_hit_attrib) == 32, "vkr_hit_attrib: three uv pairs and two words");
  const std::string prefix = std::string(program) + ": ", dotted = std::string(program) + ".rays";
  VKR_TRY(rt_surface_require(program, "out_reflections", depth, normal, accel, params, out_reflections));
  if (has_cutout) VKR_TRY(require_cutout(program, cutout));
  if (!scratch) { set_error("%s: scratch is NULL", program); return VKR_ERR_NULL; }
  if (params->flags & ~VKR_REFLECT_RT_FILL_MISSES) { set_error("%s: unknown flag bits 0x%x", program, params->flags & ~VKR_REFLECT_RT_FILL_MISSES); return VKR_ERR_EXTENT; }
  const bool fill = (params->flags & VKR_REFLECT_RT_FILL_MISSES) != 0;
  if (fill && !rays) { set_error("%s: rays is NULL with VKR_REFLECT_RT_FILL_MISSES", program); return VKR_ERR_NULL; }
  if (texture_count && !textures) { set_error("%s: %u textures but a NULL texture array", program, texture_count); return VKR_ERR_NULL; }
  if (texture_count > RASTER_MAX_TEXTURES) { set_error("%s: %u textures, at most %d", program, texture_count, RASTER_MAX_TEXTURES); return VKR_ERR_EXTENT; }
  if (attrib_count != accel->tri_count) {
    set_error("%s: %u attribute records for a structure of %u triangles (one per input triangle)", program, attrib_count, accel->tri_count);
    return VKR_ERR_EXTENT;
  }
  if (attrib_count && !attribs) { set_error("%s: attribs is NULL", program); return VKR_ERR_NULL; }
  if (params->reserved[0] != 0 || params->reserved[1] != 0 || params->reserved[2] != 0) { set_error("%s: reserved must be 0", program); return VKR_ERR_EXTENT; }
  if (std::isnan(params->tmin)) { set_error("%s: tmin is NaN", program); return VKR_ERR_EXTENT; }
  if (std::isnan(params->max_distance)) { set_error("%s: max_distance is NaN", program); return VKR_ERR_EXTENT; }
  ReflectRtArgs& a = *args;
  VKR_TRY(rt_surface_bind(program, "out_reflections", depth, normal, accel, params, out_reflections, &a));
  a.rays = a.out;  // not read without the flag
  if (fill) {
    VKR_TRY(make_tex(rays, 0, VKR_FMT_RGBA16_UNORM, dotted.c_str(), &a.rays));
    VKR_TRY(require_whole_frame(a.rays, (prefix + "rays").c_str(), RT_WHOLE_FRAME));
  }
  VKR_TRY(rt_surface_one_extent(program, "out_reflections", a, fill && (a.rays.w != a.out.w || a.rays.h != a.out.h), fill ? ", rays another" : ""));
  vkr_raster_scene sc {};
  sc.textures = textures; sc.texture_count = texture_count;
  std::vector<Pyramid> pyramids;
  VKR_TRY(make_pyramids(&sc, program, &pyramids));
  for (const Pyramid& p : pyramids)  // REPEAT addresses the whole level
    for (int m = 0; m < p.count; m++) VKR_TRY(require_whole_frame(p.mip[m], (prefix + "texture").c_str(), "a texture is sampled with REPEAT: windows are not supported"));
  const ReflectRtLayout lay(texture_count);
  if (scratch_bytes < lay.total) {
    set_error("%s: scratch too small (%llu bytes, %llu needed)", program, (unsigned long long)scratch_bytes, (unsigned long long)lay.total);
    return VKR_ERR_EXTENT;
  }
  VKR_TRY(more());
  a.attribs = attribs;
  a.textures = (const Pyramid*)((uint8_t*)scratch + lay.textures);
  a.texture_count = texture_count; a.texture_lod = params->texture_lod; a.fill_misses = fill ? 1u : 0u;
  a.normal_offset = params->normal_offset; a.tmin = params->tmin; a.max_distance = params->max_distance;
  store_table<4>(pyramids, a.textures, stream);
  return VKR_OK;
}

}  // namespace vkr

#endif
