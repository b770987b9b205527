// ray_cutout.hpp — alpha cutouts in the ray query (DESIGN_NUMERICS.md, "Ray query, cutouts"): the texture coordinates of a hit,
// the alpha of a texture level there, the candidate filter that the walks of accel_traverse.hpp ask, and the host's binding of
// "attribute records + textures + scratch" for the entries that take a vkr_ray_cutout (accel_cutout.hip, shadow_mask_rt.hip,
// reflections_rt.hip).
//
// A candidate is transparent when its triangle's albedo texture exists, is not masked opaque, and its alpha at the hit is
// exactly 0: the rasterisers' discard (raster.hip, cubemap.hip), asked of a ray.  Everything but the hit's uv and the four
// alpha taps is wave-uniform (the triangle record of a leaf slot is): the attribute record, the texture and the level come
// through scalar loads, and a masked or absent texture costs a scalar branch and no fetch.
#ifndef VKR_RAY_CUTOUT_HPP
#define VKR_RAY_CUTOUT_HPP

#include "raster_common.hpp"
#include "accel_traverse.hpp"

namespace vkr {

// uv of the hit (u, v) on the triangle of record `at`: w = (1 - u) - v, (w uv0 + u uv1) + v uv2, every operation rounded on its
// own.  What a reflection hit is shaded at and what a cutout is decided at.
VKR_DEV f2 hit_uv(const vkr_hit_attrib& at, float u, float v) {
  const float w = (1.0f - u) - v;
  return mk2((w * at.uv[0][0] + u * at.uv[1][0]) + v * at.uv[2][0], (w * at.uv[0][1] + u * at.uv[1][1]) + v * at.uv[2][1]);
}

// The .w of sample_level_repeat(t, uv, lut): the same addresses, fractions and mix order, of the alpha bytes alone (UNORM8: no
// table).
VKR_DEV float sample_alpha_repeat(const Tex& t, f2 uv) {
  const float x = cfma(uv.x, (float)t.fw, -0.5f), y = cfma(uv.y, (float)t.fh, -0.5f);
  const float x0f = floorf(x), y0f = floorf(y);
  const float fx = x - x0f, fy = y - y0f;
  const int x0 = wrap_repeat(f2i(x0f), t.fw), y0 = wrap_repeat(f2i(y0f), t.fh);
  const int x1 = wrap_repeat(x0 + 1, t.fw), y1 = wrap_repeat(y0 + 1, t.fh);
  auto alpha = [&](int tx, int ty) { return unorm8_to_float((uint32_t)t.p[toff(t, tx, ty, 4) + 3u]); };
  return mixf(mixf(alpha(x0, y0), alpha(x1, y0), fx), mixf(alpha(x0, y1), alpha(x1, y1), fx), fy);
}

// All of it wave-uniform: part of a kernel argument, read through scalar loads
struct CutoutFilter {
  static constexpr bool ALL = false;
  const vkr_hit_attrib* attribs;  // one per input triangle
  const Pyramid* textures;        // [texture_count], in scratch
  uint32_t texture_count;         // at most 32
  uint32_t alpha_lod, opaque_mask;

  // `index` is wave-uniform.  False for a lane without the candidate and for a lane whose candidate is transparent
  VKR_DEV bool keep(uint32_t index, float u, float v, bool cand) const {
    if (__ballot(cand) == 0ull) return false;  // the whole wave: nobody asks
    const vkr_hit_attrib at = attribs[index];
    const uint32_t ti = at.albedo_index;
    if (ti >= texture_count || ((opaque_mask >> ti) & 1u) != 0u) return cand;  // untextured (0xFFFFFFFF too) or masked: opaque
    const Pyramid& p = textures[ti];
    const Tex t = p.mip[min(alpha_lod, (uint32_t)(p.count - 1))];
    if (cand && sample_alpha_repeat(t, hit_uv(at, u, v)) == 0.0f) cand = false;  // a NaN compares false: opaque
    return cand;
  }
};

// ---- host --------------------------------------------------------------------------------------------------------------------
// the scratch of an entry that takes a vkr_ray_cutout: the texture table (the layout of vkr_reflections_rt's)
struct CutoutLayout {
  uint64_t textures, total;
  explicit CutoutLayout(uint32_t texture_count) {
    ScratchCarver c;
    textures = c.take(sizeof(Pyramid) * (uint64_t)(texture_count ? texture_count : 1u));
    total = c.at;
  }
};

inline int require_cutout(const char* program, const vkr_ray_cutout* cutout) {
  if (!cutout) { set_error("%s: cutout is NULL", program); return VKR_ERR_NULL; }
  return VKR_OK;
}

// The gates vkr_reflections_rt has for attributes, textures and scratch, under `program`'s prefix, and the filter they make.
// The last of an entry's gates: it records the upload of the texture table on `stream`.
inline int bind_cutout(const char* program, const vkr_accel* accel, const vkr_hit_attrib* attribs, uint32_t attrib_count, const vkr_img* textures,
                       uint32_t texture_count, const vkr_ray_cutout* cutout, void* scratch, uint64_t scratch_bytes, hipStream_t stream,
                       CutoutFilter* f) {
  static_assert(sizeof(vkr_ray_cutout) == 8, "vkr_ray_cutout: two words");
  static_assert(sizeof(vkr_hit_attrib) == 32, "vkr_hit_attrib: three uv pairs and two words");
  VKR_TRY(require_cutout(program, cutout));
  if (!scratch) { set_error("%s: scratch is NULL", program); return VKR_ERR_NULL; }
  if (texture_count && !textures) { set_error("%s: %u textures but a NULL texture array", program, texture_count); return VKR_ERR_NULL; }
  if (texture_count > RASTER_MAX_TEXTURES) { set_error("%s: %u textures, at most %d", program, texture_count, RASTER_MAX_TEXTURES); return VKR_ERR_EXTENT; }
  if (attrib_count != accel->tri_count) {
    set_error("%s: %u attribute records for a structure of %u triangles (one per input triangle)", program, attrib_count, accel->tri_count);
    return VKR_ERR_EXTENT;
  }
  if (attrib_count && !attribs) { set_error("%s: attribs is NULL", program); return VKR_ERR_NULL; }
  vkr_raster_scene sc {};
  sc.textures = textures; sc.texture_count = texture_count;
  std::vector<Pyramid> pyramids;
  VKR_TRY(make_pyramids(&sc, program, &pyramids));
  const std::string what = std::string(program) + ": texture";
  for (const Pyramid& p : pyramids)  // REPEAT addresses the whole level
    for (int m = 0; m < p.count; m++) VKR_TRY(require_whole_frame(p.mip[m], what.c_str(), "a texture is sampled with REPEAT: windows are not supported"));
  const CutoutLayout lay(texture_count);
  if (scratch_bytes < lay.total) {
    set_error("%s: scratch too small (%llu bytes, %llu needed)", program, (unsigned long long)scratch_bytes, (unsigned long long)lay.total);
    return VKR_ERR_EXTENT;
  }
  f->attribs = attribs;
  f->textures = (const Pyramid*)((uint8_t*)scratch + lay.textures);
  f->texture_count = texture_count;
  f->alpha_lod = cutout->alpha_lod;
  f->opaque_mask = cutout->opaque_texture_mask;
  store_table<4>(pyramids, f->textures, stream);
  return VKR_OK;
}

}  // namespace vkr

#endif
