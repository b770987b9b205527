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
// not alive while the wave descends.
#include "raster_common.hpp"
#include "rt_surface.hpp"

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

// the RGBA8_UNORM word of a hit: the albedo of triangle h.index at (h.u, h.v), alpha 0
VKR_DEV uint32_t shade_hit(const ReflectRtArgs& a, const vkr_accel_hit& h, const float* lut) {
  const vkr_hit_attrib at = a.attribs[h.index];
  const float w = (1.0f - h.u) - h.v;
  const f2 uv = mk2((w * at.uv[0][0] + h.u * at.uv[1][0]) + h.v * at.uv[2][0], (w * at.uv[0][1] + h.u * at.uv[1][1]) + h.v * at.uv[2][1]);
  f3 c = mk3(0.5f, 0.5f, 0.5f);
  if (at.albedo_index < a.texture_count) {  // 0xFFFFFFFF (no texture) fails the same compare
    const Pyramid& p = a.textures[at.albedo_index];
    const uint32_t level = min(a.texture_lod, (uint32_t)(p.count - 1));
    c = xyz(sample_level_repeat(p.mip[level], uv, lut));
  }
  return float_to_unorm8(c.x) | (float_to_unorm8(c.y) << 8) | (float_to_unorm8(c.z) << 16);
}

__global__ __launch_bounds__(256) void k_reflections_rt(ReflectRtArgs a) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  __shared__ float s_lut[VKR_SRGB_LUT_SIZE];
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
      wave_closest_hit(a.accel, s.origin, dir, a.tmin, a.max_distance, cast, stacks[p.wave], &h);
      if (cast && h.index != 0xFFFFFFFFu) result = shade_hit(a, h, s_lut);
    }
  }
  if (p.inside && !keep) *texel_ptr<uint32_t>(a.out, p.lx, p.ly) = result;
}

// the scratch: the texture table
struct ReflectRtLayout {
  uint64_t textures, total;
  explicit ReflectRtLayout(uint32_t texture_count) {
    ScratchCarver c;
    textures = c.take(sizeof(Pyramid) * (uint64_t)(texture_count ? texture_count : 1u));
    total = c.at;
  }
};

}  // namespace vkr

using namespace vkr;

extern "C" uint64_t vkr_reflections_rt_scratch_bytes(uint32_t texture_count) { return ReflectRtLayout(texture_count).total; }

extern "C" int vkr_reflections_rt(const vkr_img* depth, const vkr_img* normal, const vkr_img* rays, const vkr_accel* accel,
                                  const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                                  const vkr_reflect_rt_params* params, const vkr_img* out_reflections, void* scratch, uint64_t scratch_bytes,
                                  void* stream_) {
  static_assert(sizeof(vkr_reflect_rt_params) == 112, "vkr_reflect_rt_params: a matrix, eight floats / words, the flags and three words");
  static_assert(sizeof(vkr_hit_attrib) == 32, "vkr_hit_attrib: three uv pairs and two words");
  hipStream_t stream = (hipStream_t)stream_;
  VKR_TRY(rt_surface_require("reflections_rt", "out_reflections", depth, normal, accel, params, out_reflections));
  if (!scratch) { set_error("reflections_rt: scratch is NULL"); return VKR_ERR_NULL; }
  if (params->flags & ~VKR_REFLECT_RT_FILL_MISSES) { set_error("reflections_rt: unknown flag bits 0x%x", params->flags & ~VKR_REFLECT_RT_FILL_MISSES); return VKR_ERR_EXTENT; }
  const bool fill = (params->flags & VKR_REFLECT_RT_FILL_MISSES) != 0;
  if (fill && !rays) { set_error("reflections_rt: rays is NULL with VKR_REFLECT_RT_FILL_MISSES"); return VKR_ERR_NULL; }
  if (texture_count && !textures) { set_error("reflections_rt: %u textures but a NULL texture array", texture_count); return VKR_ERR_NULL; }
  if (texture_count > RASTER_MAX_TEXTURES) { set_error("reflections_rt: %u textures, at most %d", texture_count, RASTER_MAX_TEXTURES); return VKR_ERR_EXTENT; }
  if (attrib_count != accel->tri_count) {
    set_error("reflections_rt: %u attribute records for a structure of %u triangles (one per input triangle)", attrib_count, accel->tri_count);
    return VKR_ERR_EXTENT;
  }
  if (attrib_count && !attribs) { set_error("reflections_rt: attribs is NULL"); return VKR_ERR_NULL; }
  if (params->reserved[0] != 0 || params->reserved[1] != 0 || params->reserved[2] != 0) { set_error("reflections_rt: reserved must be 0"); return VKR_ERR_EXTENT; }
  if (std::isnan(params->tmin)) { set_error("reflections_rt: tmin is NaN"); return VKR_ERR_EXTENT; }
  if (std::isnan(params->max_distance)) { set_error("reflections_rt: max_distance is NaN"); return VKR_ERR_EXTENT; }
  ReflectRtArgs a;
  VKR_TRY(rt_surface_bind("reflections_rt", "out_reflections", depth, normal, accel, params, out_reflections, &a));
  a.rays = a.out;  // not read without the flag
  if (fill) {
    VKR_TRY(make_tex(rays, 0, VKR_FMT_RGBA16_UNORM, "reflections_rt.rays", &a.rays));
    VKR_TRY(require_whole_frame(a.rays, "reflections_rt: rays", RT_WHOLE_FRAME));
  }
  VKR_TRY(rt_surface_one_extent("reflections_rt", "out_reflections", a, fill && (a.rays.w != a.out.w || a.rays.h != a.out.h), fill ? ", rays another" : ""));
  vkr_raster_scene sc {};
  sc.textures = textures; sc.texture_count = texture_count;
  std::vector<Pyramid> pyramids;
  VKR_TRY(make_pyramids(&sc, "reflections_rt", &pyramids));
  for (const Pyramid& p : pyramids)  // REPEAT addresses the whole level
    for (int m = 0; m < p.count; m++) VKR_TRY(require_whole_frame(p.mip[m], "reflections_rt: texture", "a texture is sampled with REPEAT: windows are not supported"));
  const ReflectRtLayout lay(texture_count);
  if (scratch_bytes < lay.total) {
    set_error("reflections_rt: scratch too small (%llu bytes, %llu needed)", (unsigned long long)scratch_bytes, (unsigned long long)lay.total);
    return VKR_ERR_EXTENT;
  }
  a.attribs = attribs;
  a.textures = (const Pyramid*)((uint8_t*)scratch + lay.textures);
  a.texture_count = texture_count; a.texture_lod = params->texture_lod; a.fill_misses = fill ? 1u : 0u;
  a.normal_offset = params->normal_offset; a.tmin = params->tmin; a.max_distance = params->max_distance;
  store_table<4>(pyramids, a.textures, stream);
  const dim3 tiles(16, 16);
  hipLaunchKernelGGL(k_reflections_rt, grid2d(a.out.w, a.out.h, tiles), dim3(256), 0, stream, a);
  return launch_status("reflections_rt");
}
