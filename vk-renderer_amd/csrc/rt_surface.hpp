// rt_surface.hpp — what the pixel passes that cast one ray per pixel from the visible surface share (shadow_mask_rt.hip,
// reflections_rt.hip): the pixel of a lane, the surface point of that pixel, and the host preamble for "depth + normal +
// structure + one RGBA8 output, whole frames, one extent".  k_gtao_rt (accel.hip) is no such pass: it runs one wave per pixel,
// samples by uv and supports windows.
#ifndef VKR_RT_SURFACE_HPP
#define VKR_RT_SURFACE_HPP

#include "accel_traverse.hpp"

namespace vkr {

// The head of such a pass's kernel argument.  All of it wave-uniform, read through scalar loads.
struct RtSurfaceArgs {
  Tex depth, normal, out;  // one extent
  Mat4 inverse_camera;
  Proj pr;
  AccelView accel;
};

// One lane per pixel of out; a wave is an 8 x 8 pixel tile, wave w of the block the tile (w & 1, w >> 1) of its 16 x 16.
struct RtPixel {
  int wave, lx, ly;
  bool inside;
  int cx, cy;     // a lane outside the image reads texel (0, 0) and writes nothing
  float d;        // the depth at (cx, cy)
  bool geometry;  // inside, and not the sky
};
VKR_DEV RtPixel rt_pixel(const RtSurfaceArgs& a) {
  RtPixel p;
  const i2 blk = xcd_block<8, 8>();  // chunks of 128 x 128 pixels
  const int lane = threadIdx.x & 63;
  p.wave = threadIdx.x >> 6;
  p.lx = blk.x * 16 + (p.wave & 1) * 8 + (lane & 7);
  p.ly = blk.y * 16 + (p.wave >> 1) * 8 + (lane >> 3);
  p.inside = p.lx < a.out.w && p.ly < a.out.h;
  p.cx = p.inside ? p.lx : 0; p.cy = p.inside ? p.ly : 0;
  p.d = d24_to_float(*(const uint32_t*)(a.depth.p + toff(a.depth, p.cx, p.cy, 4)));
  p.geometry = p.inside && p.d < 1.0f;
  return p;
}

// The surface seen through the centre of that pixel: its world position, its normal, and the ray origin pushed off the surface
// along the normal.  Called by the whole wave once any lane has a ray to cast.
struct RtSurface { f3 world, n, origin; };
VKR_DEV RtSurface rt_surface(const RtSurfaceArgs& a, const RtPixel& p, float normal_offset) {
  RtSurface s;
  const f2 uv = mk2(pixel_centre_uv(p.cx, (float)a.out.w), pixel_centre_uv(p.cy, (float)a.out.h));
  const f3 view = reconstruct_view_vec(uv, p.d, a.pr);
  s.world = xyz(mul(a.inverse_camera, mk4(view.x, view.y, view.z, 1.0f)));
  s.n = decode_normal(FmtRG16U::load(a.normal, p.cx, p.cy));
  s.origin = madd(s.world, normal_offset, s.n);
  return s;
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// The preamble in the two parts between which an entry checks its own parameters; `program` prefixes every text, `out_name` is
// the output's parameter name.  First the NULL refusals.
inline int rt_surface_require(const char* program, const char* out_name, const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel,
                              const void* params, const vkr_img* out) {
  if (!depth) { set_error("%s: depth is NULL", program); return VKR_ERR_NULL; }
  if (!normal) { set_error("%s: normal is NULL", program); return VKR_ERR_NULL; }
  if (!accel) { set_error("%s: NULL acceleration structure", program); return VKR_ERR_NULL; }
  if (!params) { set_error("%s: params is NULL", program); return VKR_ERR_NULL; }
  if (!out) { set_error("%s: %s is NULL", program, out_name); return VKR_ERR_NULL; }
  return VKR_OK;
}

constexpr const char* RT_WHOLE_FRAME = "windows are not supported (the rays reach anywhere: a single-GPU pass)";

// Then the three images (every format before any window), the camera of a vkr_*_rt_params and the view of the structure.
template <class Params>
inline int rt_surface_bind(const char* program, const char* out_name, const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel,
                           const Params* params, const vkr_img* out, RtSurfaceArgs* a) {
  const struct { const vkr_img* img; uint32_t format; const char* name; Tex* tex; int max_side; } bind[3] = {
      {depth, VKR_FMT_D24_UNORM_S8, "depth", &a->depth, INT32_MAX},
      {normal, VKR_FMT_RG16_UNORM, "normal", &a->normal, INT32_MAX},
      {out, VKR_FMT_RGBA8_UNORM, out_name, &a->out, 65535}};
  char what[96];
  for (const auto& b : bind) {
    std::snprintf(what, sizeof what, "%s.%s", program, b.name);
    VKR_TRY(make_tex(b.img, 0, b.format, what, b.tex));
  }
  for (const auto& b : bind) {
    std::snprintf(what, sizeof what, "%s: %s", program, b.name);
    VKR_TRY(require_whole_frame(*b.tex, what, RT_WHOLE_FRAME, b.max_side));
  }
  load_mat(a->inverse_camera, params->inverse_camera);
  load_proj(a->pr, params->fovy, params->aspect, params->znear, params->zfar);
  a->accel = view_of(accel);
  return VKR_OK;
}

// The one-extent refusal; a pass with a further image says whether that one differs and what to add to the text.
inline int rt_surface_one_extent(const char* program, const char* out_name, const RtSurfaceArgs& a, bool other_differs = false, const char* suffix = "") {
  if (a.depth.w != a.out.w || a.depth.h != a.out.h || a.normal.w != a.out.w || a.normal.h != a.out.h || other_differs) {
    set_error("%s: depth is %dx%d, normal %dx%d, %s %dx%d%s: one extent expected", program, a.depth.w, a.depth.h, a.normal.w, a.normal.h, out_name,
              a.out.w, a.out.h, suffix);
    return VKR_ERR_EXTENT;
  }
  return VKR_OK;
}

}  // namespace vkr

#endif
