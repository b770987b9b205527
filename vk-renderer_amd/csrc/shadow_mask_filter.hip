// shadow_mask_filter.hip — entry vkr_shadow_mask_filter: the edge-aware reconstruction filter of the shadow mask.
//
// No reference program.  The traced mask of shadow_mask_rt_soft.hip casts S rays per pixel and light from one of P x P sample
// patterns; this pass combines the P x P neighbouring patterns: per pixel the mean of the mask over the taps |dx|, |dy| < R with
// the tent weights (R - |dx|)(R - |dy|), over those taps that lie on the pixel's surface (normal and plane test against the
// G-buffer), in unsigned integers, rounded half up.  The rule is frozen in DESIGN_NUMERICS.md (Shadow mask, filter) and restated in
// tests/shadow_mask_filter_reference.py.  Only the accept decisions are floating point: the sums do not depend on their order.
//
// The schedule: one lane per pixel, a wave an 8 x 8 tile, a block 16 x 16 in the tile order of rt_pixel().  The
// block stages its (16 + 2(R-1))^2 window of mask texels in LDS.  A wave whose own (8 + 2(R-1))^2 window holds one single value
// (taps outside the image not counted) copies its texel: with every tap equal to v the rule gives (2 A v + A) / (2 A) = v.  A block
// with a wave that is not flat stages the guide records of its window once per texel — world position, normal, |view z| or the sky
// mark, 28 bytes — and its waves that are not flat walk the taps out of LDS, the four channels as two words of packed 16-bit lanes
// (the largest sum is R^4 * 255 = 65280 at R = 4).
#include "vkr_host.hpp"

#include <cmath>

// tools/shadow_mask_filter_timing.py builds the library again with -DVKR_SHADOW_FILTER_EARLY_OUT=0 (tools/build_variants.sh), to
// measure one against the other, and compares their bytes.  The library is built with the default.
#ifndef VKR_SHADOW_FILTER_EARLY_OUT
#define VKR_SHADOW_FILTER_EARLY_OUT 1
#endif

namespace vkr {

#define SMF_MAX_REACH 4

// All of it wave-uniform: a kernel argument, read through scalar loads
struct ShadowFilterArgs {
  Tex depth, normal, mask, out;  // one extent
  Mat4 inverse_camera;
  Proj pr;
  float normal_min_dot, plane_tolerance;
};

// The guide of one texel, computed as rt_surface() (rt_surface.hpp) computes the surface point of a pixel.  az: |view z| of a
// geometry texel (NaN stays NaN), -1 for the sky.
struct FilterGuide { f3 world, n; float az; };
VKR_DEV FilterGuide filter_guide(const ShadowFilterArgs& a, int x, int y) {
  FilterGuide g;
  const float d = FmtD24::load(a.depth, x, y);
  const f2 uv = mk2(pixel_centre_uv(x, (float)a.out.w), pixel_centre_uv(y, (float)a.out.h));
  const f3 view = reconstruct_view_vec(uv, d, a.pr);
  g.world = xyz(mul(a.inverse_camera, mk4(view.x, view.y, view.z, 1.0f)));
  g.n = decode_normal(FmtRG16U::load(a.normal, x, y));
  g.az = d < 1.0f ? fabsf(view.z) : -1.0f;
  return g;
}

template <int R>
__global__ __launch_bounds__(256) void k_shadow_mask_filter(ShadowFilterArgs a) {
  const i2 blk = xcd_block<8, 8>();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = (wave & 1) * 8, ty = (wave >> 1) * 8;    // this wave's tile in the block
  const int px = tx + (lane & 7), py = ty + (lane >> 3);  // this lane's pixel in the block
  const int gx = blk.x * 16 + px, gy = blk.y * 16 + py;
  const int w = a.out.w, h = a.out.h;
  const bool inside = gx < w && gy < h;
  if constexpr (R == 1) {  // the centre tap alone: a copy
    if (inside) *texel_ptr<uint32_t>(a.out, gx, gy) = *texel_ptr<const uint32_t>(a.mask, gx, gy);
  } else {
    constexpr int B = R - 1;        // the border of a window
    constexpr int WS = 16 + 2 * B;  // side of the block's window
    constexpr int WW = 8 + 2 * B;   // side of a wave's window
    constexpr int N = WS * WS;
    __shared__ uint32_t s_mask[N];
    __shared__ float s_guide[7][N];  // world xyz, normal xyz, az; struct of arrays
    const int x0 = blk.x * 16 - B, y0 = blk.y * 16 - B;  // the window's origin in the image

    // the window of mask texels; an entry outside the image holds 0 and is never counted
    for (int e = tid; e < N; e += 256) {
      const int wy = e / WS, wx = e - wy * WS, x = x0 + wx, y = y0 + wy;
      const bool in = x >= 0 && x < w && y >= 0 && y < h;
      s_mask[e] = in ? *texel_ptr<const uint32_t>(a.mask, x, y) : 0u;
    }
    __syncthreads();
    const int centre = (py + B) * WS + px + B;
    const uint32_t own = s_mask[centre];

    // flat: every texel of the wave's window inside the image equals the tile's first texel.  A tile whose first texel lies
    // outside the image has nothing to write: flat.
    bool flat = blk.x * 16 + tx >= w || blk.y * 16 + ty >= h;  // wave-uniform
    if (!flat && VKR_SHADOW_FILTER_EARLY_OUT) {
      const uint32_t first = s_mask[(ty + B) * WS + tx + B];
      bool differs = false;
      for (int e = lane; e < WW * WW; e += 64) {
        const int wy = e / WW, wx = e - wy * WW;
        const int x = x0 + tx + wx, y = y0 + ty + wy;
        const bool in = x >= 0 && x < w && y >= 0 && y < h;
        differs |= in && s_mask[(ty + wy) * WS + tx + wx] != first;
      }
      flat = __ballot(differs) == 0ull;
    }
    if (__syncthreads_or(!flat) == 0) {  // the whole block is flat
      if (inside) *texel_ptr<uint32_t>(a.out, gx, gy) = own;
      return;
    }

    // the guide records of the block's window, once per texel; outside the image: the sky mark, rejected like the sky
    for (int e = tid; e < N; e += 256) {
      const int wy = e / WS, wx = e - wy * WS, x = x0 + wx, y = y0 + wy;
      const bool in = x >= 0 && x < w && y >= 0 && y < h;
      FilterGuide g;
      g.world = mk3(0.0f, 0.0f, 0.0f); g.n = g.world; g.az = -1.0f;
      if (in) g = filter_guide(a, x, y);
      s_guide[0][e] = g.world.x; s_guide[1][e] = g.world.y; s_guide[2][e] = g.world.z;
      s_guide[3][e] = g.n.x; s_guide[4][e] = g.n.y; s_guide[5][e] = g.n.z;
      s_guide[6][e] = g.az;
    }
    __syncthreads();

    uint32_t result = own;  // a flat wave, the sky
    const float az = s_guide[6][centre];
    if (!flat && !(az < 0.0f)) {  // flat is wave-uniform
      const f3 Wg = mk3(s_guide[0][centre], s_guide[1][centre], s_guide[2][centre]);
      const f3 ng = mk3(s_guide[3][centre], s_guide[4][centre], s_guide[5][centre]);
      const float plane_max = a.plane_tolerance * az;
      uint32_t A = 0, lo = 0, hi = 0;  // lo: channels 0 and 2, hi: channels 1 and 3, 16 bits each
#pragma unroll 1
      for (int dy = -B; dy <= B; dy++) {  // a row of taps at a time: unrolled whole, R = 4 holds 110 registers (4 waves per SIMD)
#pragma unroll
        for (int dx = -B; dx <= B; dx++) {
          const uint32_t wgt = (uint32_t)((R - (dy < 0 ? -dy : dy)) * (R - (dx < 0 ? -dx : dx)));
          const int e = centre + dy * WS + dx;
          bool accept = true;
          if (dx != 0 || dy != 0) {
            const f3 Wt = mk3(s_guide[0][e], s_guide[1][e], s_guide[2][e]);
            const f3 nt = mk3(s_guide[3][e], s_guide[4][e], s_guide[5][e]);
            accept = !(s_guide[6][e] < 0.0f) && dot(ng, nt) >= a.normal_min_dot && fabsf(dot(ng, Wt - Wg)) <= plane_max;
          }
          const uint32_t t = s_mask[e], m = accept ? wgt : 0u;
          A += m;
          lo += m * (t & 0x00FF00FFu);
          hi += m * ((t >> 8) & 0x00FF00FFu);
        }
      }
      const uint32_t A2 = 2u * A;
      const uint32_t c0 = (2u * (lo & 0xFFFFu) + A) / A2, c2 = (2u * (lo >> 16) + A) / A2;
      const uint32_t c1 = (2u * (hi & 0xFFFFu) + A) / A2, c3 = (2u * (hi >> 16) + A) / A2;
      result = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
    }
    if (inside) *texel_ptr<uint32_t>(a.out, gx, gy) = result;
  }
}

// whether two images' rows share a byte
inline bool memory_overlaps(const Tex& a, const Tex& b) {
  const uintptr_t a0 = (uintptr_t)a.p, a1 = a0 + (uintptr_t)a.pitch * (uintptr_t)a.h;
  const uintptr_t b0 = (uintptr_t)b.p, b1 = b0 + (uintptr_t)b.pitch * (uintptr_t)b.h;
  return a0 < b1 && b0 < a1;
}

constexpr const char* FILTER_WHOLE_FRAME = "windows are not supported (the taps cross strip borders: a single-GPU pass)";

// every gate of the entry and its kernel argument
inline int shadow_filter_args(const char* program, const vkr_img* depth, const vkr_img* normal, const vkr_img* mask,
                              const vkr_shadow_filter_params* params, const vkr_img* out_mask, ShadowFilterArgs* a) {
  static_assert(sizeof(vkr_shadow_filter_params) == 96, "vkr_shadow_filter_params: a matrix, four floats and four words");
  if (!depth) { set_error("%s: depth is NULL", program); return VKR_ERR_NULL; }
  if (!normal) { set_error("%s: normal is NULL", program); return VKR_ERR_NULL; }
  if (!mask) { set_error("%s: mask is NULL", program); return VKR_ERR_NULL; }
  if (!params) { set_error("%s: params is NULL", program); return VKR_ERR_NULL; }
  if (!out_mask) { set_error("%s: out_mask is NULL", program); return VKR_ERR_NULL; }
  if (params->reach < 1 || params->reach > SMF_MAX_REACH) {
    set_error("%s: reach %u, expected 1..%d", program, params->reach, SMF_MAX_REACH);
    return VKR_ERR_EXTENT;
  }
  if (std::isnan(params->normal_min_dot)) { set_error("%s: normal_min_dot is NaN", program); return VKR_ERR_EXTENT; }
  if (std::isnan(params->plane_tolerance)) { set_error("%s: plane_tolerance is NaN", program); return VKR_ERR_EXTENT; }
  if (params->reserved != 0) { set_error("%s: reserved is %u, must be 0", program, params->reserved); return VKR_ERR_EXTENT; }
  // every format before any window, as rt_surface_bind
  const struct { const vkr_img* img; uint32_t format; const char* name; Tex* tex; } bind[4] = {
      {depth, VKR_FMT_D24_UNORM_S8, "depth", &a->depth},
      {normal, VKR_FMT_RG16_UNORM, "normal", &a->normal},
      {mask, VKR_FMT_RGBA8_UNORM, "mask", &a->mask},
      {out_mask, VKR_FMT_RGBA8_UNORM, "out_mask", &a->out}};
  char what[96];
  for (const auto& b : bind) {
    std::snprintf(what, sizeof what, "%s.%s", program, b.name);
    VKR_TRY(make_tex(b.img, 0, b.format, what, b.tex));
  }
  for (const auto& b : bind) {
    std::snprintf(what, sizeof what, "%s: %s", program, b.name);
    VKR_TRY(require_whole_frame(*b.tex, what, FILTER_WHOLE_FRAME, b.tex == &a->out ? 65535 : INT32_MAX));
  }
  for (const auto& b : bind)
    if (b.tex->w != a->out.w || b.tex->h != a->out.h) {
      set_error("%s: depth is %dx%d, normal %dx%d, mask %dx%d, out_mask %dx%d: one extent expected", program, a->depth.w, a->depth.h, a->normal.w,
                a->normal.h, a->mask.w, a->mask.h, a->out.w, a->out.h);
      return VKR_ERR_EXTENT;
    }
  if (memory_overlaps(a->mask, a->out)) {
    set_error("%s: mask and out_mask overlap in memory (the taps read neighbours: not in place)", program);
    return VKR_ERR_LAYOUT;
  }
  load_mat(a->inverse_camera, params->inverse_camera);
  load_proj(a->pr, params->fovy, params->aspect, params->znear, params->zfar);
  a->normal_min_dot = params->normal_min_dot;
  a->plane_tolerance = params->plane_tolerance;
  return VKR_OK;
}

}  // namespace vkr

using namespace vkr;

extern "C" int vkr_shadow_mask_filter(const vkr_img* depth, const vkr_img* normal, const vkr_img* mask, const vkr_shadow_filter_params* params,
                                      const vkr_img* out_mask, void* stream) {
  ShadowFilterArgs a;
  VKR_TRY(shadow_filter_args("shadow_mask_filter", depth, normal, mask, params, out_mask, &a));
  const dim3 grid = grid2d(a.out.w, a.out.h, dim3(16, 16));
  switch (params->reach) {  // wave-uniform: a template parameter, so that the tap loops unroll with constant weights
    case 1: hipLaunchKernelGGL(k_shadow_mask_filter<1>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL(k_shadow_mask_filter<2>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 3: hipLaunchKernelGGL(k_shadow_mask_filter<3>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(k_shadow_mask_filter<4>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
  }
  return launch_status("shadow_mask_filter");
}
