// shadow_mask_accumulate.hip — entry vkr_shadow_mask_accumulate: the temporal accumulation of the shadow mask, and the host-only
// table vkr_shadow_disk_samples_frame that gives every frame of a cycle its own rotation of the sample patterns.
//
// No reference program.  Per pixel the running mean of the mask over the frames in which the pixel saw the same world point: the
// pixel is reprojected by its velocity to the nearest texel of the previous frame, that texel's surface point (previous depth
// through the previous inverse camera) must lie on the pixel's tangent plane (the plane test of shadow_mask_filter.hip), and then
// the history of that texel, in 65535ths, takes the new mask with the weight 1 / n'.  The rule is frozen in DESIGN_NUMERICS.md
// (Shadow mask, temporal accumulation) and restated in tests/shadow_mask_accumulate_reference.py.  Only the validity decision is
// floating point: the update is unsigned integers.
//
// The schedule: one launch, no LDS (the gather is one texel per image).  A lane owns four horizontally adjacent
// pixels, so that the R8 count plane is written a dword per lane; a wave is 16 lanes x 4 rows = 64 x 4 pixels, a block of four
// waves 64 x 16: every row of a wave is 256 contiguous bytes of the 4-byte images.
#include "vkr_host.hpp"

#include <cmath>

// tools/shadow_mask_accumulate_timing.py builds the library again with -DVKR_SHADOW_ACCUM_PLAIN_DIVIDE=1 (tools/build_variants.sh)
// to measure the generic 32-bit divide against accum_divide() below.  The library is built with the default.
#ifndef VKR_SHADOW_ACCUM_PLAIN_DIVIDE
#define VKR_SHADOW_ACCUM_PLAIN_DIVIDE 0
#endif

namespace vkr {

#define SMA_PIXELS 4  // horizontally adjacent pixels of a lane

// All of it wave-uniform: a kernel argument, read through scalar loads
struct ShadowAccumArgs {
  Tex depth, normal, velocity, prev_depth, mask, history, count;  // one extent
  Tex out_history, out_count, out;
  Mat4 inverse_camera, prev_inverse_camera;
  Proj pr;
  float plane_tolerance;
  uint32_t cap;  // max_count - 1: the most frames the history weighs
  uint32_t reset;
};

// num / n for num < 2^24 and 1 <= n <= 255, given rinv = 1.0f / (float)n (the IEEE quotient).  (float)num is exact, the product
// is within 2^-23 of the quotient relatively: for n >= 2 the truncated estimate is off by at most one either way (n = 1 is
// exact), which the remainder tells.  vkr_selftest_accum_division compares with `/` on every such pair.
VKR_DEV uint32_t accum_divide(uint32_t num, uint32_t n, float rinv) {
#if VKR_SHADOW_ACCUM_PLAIN_DIVIDE
  (void)rinv;
  return num / n;
#else
  uint32_t q = (uint32_t)((float)num * rinv);
  const int r = (int)(num - __umul24(q, n));
  if (r < 0) q--;
  else if (r >= (int)n) q++;
  return q;
#endif
}

__global__ __launch_bounds__(256) void k_shadow_mask_accumulate(ShadowAccumArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w = a.out.w, h = a.out.h;
  const int x0 = ((int)blockIdx.x * 16 + (lane & 15)) * SMA_PIXELS;
  const int y = (int)blockIdx.y * 16 + wave * 4 + (lane >> 4);
  if (x0 >= w || y >= h) return;
  const float wf = (float)w, hf = (float)h;
  const float uvy = pixel_centre_uv(y, hf);
  uint32_t counts = 0u;  // the four count bytes of this lane
#pragma unroll
  for (int i = 0; i < SMA_PIXELS; i++) {
    const int x = x0 + i;
    if (x >= w) break;
    const uint32_t m = *texel_ptr<const uint32_t>(a.mask, x, y);
    uint32_t n1 = 1u;                                              // n'
    uint32_t H[4] = {0u, 0u, 0u, 0u};                              // the history the mean continues; unused at n' = 1
    const float d = FmtD24::load(a.depth, x, y);
    if (a.reset == 0u && d < 1.0f) {
      const f2 uv = mk2(pixel_centre_uv(x, wf), uvy);
      const f2 vel = FmtRG16F::load(a.velocity, x, y);
      const float fx = (uv.x + vel.x) * wf, fy = (uv.y + vel.y) * hf;
      if (fx >= 0.0f && fx < wf && fy >= 0.0f && fy < hf) {        // a compare with a NaN is false
        const int qx = (int)fx, qy = (int)fy;                      // floor of a non-negative float below the extent: inside
        const uint32_t n = *texel_ptr<const uint8_t>(a.count, qx, qy);
        const float dq = FmtD24::load(a.prev_depth, qx, qy);
        if (n >= 1u && dq < 1.0f) {
          const f3 view = reconstruct_view_vec(uv, d, a.pr);
          const f3 Wg = xyz(mul(a.inverse_camera, mk4(view.x, view.y, view.z, 1.0f)));
          const f3 ng = decode_normal(FmtRG16U::load(a.normal, x, y));
          const f2 uvq = mk2(pixel_centre_uv(qx, wf), pixel_centre_uv(qy, hf));
          const f3 viewq = reconstruct_view_vec(uvq, dq, a.pr);
          const f3 Wq = xyz(mul(a.prev_inverse_camera, mk4(viewq.x, viewq.y, viewq.z, 1.0f)));
          if (fabsf(dot(ng, Wq - Wg)) <= a.plane_tolerance * fabsf(view.z)) {
            const uint2 hq = *texel_ptr<const uint2>(a.history, qx, qy);
            H[0] = hq.x & 0xFFFFu; H[1] = hq.x >> 16; H[2] = hq.y & 0xFFFFu; H[3] = hq.y >> 16;
            n1 = (n < a.cap ? n : a.cap) + 1u;                       // cap = 0 (max_count 1): n' = 1, the mask alone
          }
        }
      }
    }
    const float rinv = 1.0f / (float)n1;
    const uint32_t half = n1 >> 1, old = n1 - 1u;
    uint32_t Hn[4], o[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint32_t mc = (m >> (8 * c)) & 0xFFu;
      Hn[c] = accum_divide(__umul24(H[c], old) + 257u * mc + half, n1, rinv);  // below 2^24
      o[c] = (255u * Hn[c] + 32767u) / 65535u;
    }
    *texel_ptr<uint2>(a.out_history, x, y) = make_uint2(Hn[0] | (Hn[1] << 16), Hn[2] | (Hn[3] << 16));
    *texel_ptr<uint32_t>(a.out, x, y) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
    counts |= n1 << (8 * i);
  }
  // the count plane: a dword where the lane's four texels exist and the address allows it, bytes otherwise
  uint8_t* cp = texel_ptr<uint8_t>(a.out_count, x0, y);
  if (x0 + SMA_PIXELS <= w && ((uintptr_t)cp & 3u) == 0u) {
    *(uint32_t*)cp = counts;
  } else {
    for (int i = 0; i < SMA_PIXELS && x0 + i < w; i++) cp[i] = (uint8_t)(counts >> (8 * i));
  }
}

// every numerator below 2^24 over every n' in 1..255; *counter += the number of quotients that differ from `/`
__global__ __launch_bounds__(256) void k_selftest_accum_division(uint32_t* counter) {
  uint32_t bad = 0u;
  for (uint32_t n = 1u; n <= 255u; n++) {
    const float rinv = 1.0f / (float)n;
    for (uint32_t num = blockIdx.x * 256u + threadIdx.x; num < (1u << 24); num += gridDim.x * 256u)
      if (accum_divide(num, n, rinv) != num / n) ++bad;
  }
  if (bad) atomicAdd(counter, bad);
}

// whether two images' rows share a byte
inline bool accum_overlap(const Tex& a, const Tex& b) {
  const uintptr_t a0 = (uintptr_t)a.p, a1 = a0 + (uintptr_t)a.pitch * (uintptr_t)a.h;
  const uintptr_t b0 = (uintptr_t)b.p, b1 = b0 + (uintptr_t)b.pitch * (uintptr_t)b.h;
  return a0 < b1 && b0 < a1;
}

constexpr const char* ACCUM_WHOLE_FRAME = "windows are not supported (the reprojection reaches across strips: a single-GPU pass)";

// every gate of the entry and its kernel argument
inline int shadow_accum_args(const char* program, const vkr_img* depth, const vkr_img* normal, const vkr_img* velocity, const vkr_img* prev_depth,
                             const vkr_img* mask, const vkr_img* history, const vkr_img* history_count, const vkr_shadow_accum_params* params,
                             const vkr_img* out_history, const vkr_img* out_count, const vkr_img* out_mask, ShadowAccumArgs* a) {
  static_assert(sizeof(vkr_shadow_accum_params) == 160, "vkr_shadow_accum_params: two matrices, four floats and four words");
  const struct { const vkr_img* img; uint32_t format; const char* name; Tex* tex; bool output; } bind[10] = {
      {depth, VKR_FMT_D24_UNORM_S8, "depth", &a->depth, false},
      {normal, VKR_FMT_RG16_UNORM, "normal", &a->normal, false},
      {velocity, VKR_FMT_RG16_SFLOAT, "velocity", &a->velocity, false},
      {prev_depth, VKR_FMT_D24_UNORM_S8, "prev_depth", &a->prev_depth, false},
      {mask, VKR_FMT_RGBA8_UNORM, "mask", &a->mask, false},
      {history, VKR_FMT_RGBA16_UNORM, "history", &a->history, false},
      {history_count, VKR_FMT_R8_UNORM, "history_count", &a->count, false},
      {out_history, VKR_FMT_RGBA16_UNORM, "out_history", &a->out_history, true},
      {out_count, VKR_FMT_R8_UNORM, "out_count", &a->out_count, true},
      {out_mask, VKR_FMT_RGBA8_UNORM, "out_mask", &a->out, true}};
  for (const auto& b : bind)
    if (!b.img) { set_error("%s: %s is NULL", program, b.name); return VKR_ERR_NULL; }
  if (!params) { set_error("%s: params is NULL", program); return VKR_ERR_NULL; }
  if (params->max_count < 1 || params->max_count > 255) {
    set_error("%s: max_count %u, expected 1..255", program, params->max_count);
    return VKR_ERR_EXTENT;
  }
  if (std::isnan(params->plane_tolerance)) { set_error("%s: plane_tolerance is NaN", program); return VKR_ERR_EXTENT; }
  if (params->reset > 1) { set_error("%s: reset is %u, must be 0 or 1", program, params->reset); return VKR_ERR_EXTENT; }
  if (params->reserved != 0) { set_error("%s: reserved is %u, must be 0", program, params->reserved); return VKR_ERR_EXTENT; }
  // every format before any window, as rt_surface_bind
  char what[96];
  for (const auto& b : bind) {
    std::snprintf(what, sizeof what, "%s.%s", program, b.name);
    VKR_TRY(make_tex(b.img, 0, b.format, what, b.tex));
  }
  for (const auto& b : bind) {
    std::snprintf(what, sizeof what, "%s: %s", program, b.name);
    VKR_TRY(require_whole_frame(*b.tex, what, ACCUM_WHOLE_FRAME, 65535));
  }
  for (const auto& b : bind)
    if (b.tex->w != a->out.w || b.tex->h != a->out.h) {
      set_error("%s: %s is %dx%d, out_mask %dx%d: one extent expected", program, b.name, b.tex->w, b.tex->h, a->out.w, a->out.h);
      return VKR_ERR_EXTENT;
    }
  // A pixel reads the history and the count of another texel: never in place.  mask and out_mask are read and written by the same
  // lane at the same texel: the same image is allowed, any other overlap is not.
  for (const auto& o : bind) {
    if (!o.output) continue;
    for (const auto& b : bind) {
      if (b.tex == o.tex || !accum_overlap(*b.tex, *o.tex)) continue;
      if (o.tex == &a->out && b.tex == &a->mask && a->mask.p == a->out.p && a->mask.pitch == a->out.pitch) continue;
      set_error("%s: %s and %s overlap in memory (the gather reads other texels: only mask and out_mask may be one image)", program, b.name, o.name);
      return VKR_ERR_LAYOUT;
    }
  }
  load_mat(a->inverse_camera, params->inverse_camera);
  load_mat(a->prev_inverse_camera, params->prev_inverse_camera);
  load_proj(a->pr, params->fovy, params->aspect, params->znear, params->zfar);
  a->plane_tolerance = params->plane_tolerance;
  a->cap = params->max_count - 1u;
  a->reset = params->reset;
  return VKR_OK;
}

}  // namespace vkr

using namespace vkr;

extern "C" int vkr_shadow_mask_accumulate(const vkr_img* depth, const vkr_img* normal, const vkr_img* velocity, const vkr_img* prev_depth,
                                          const vkr_img* mask, const vkr_img* history, const vkr_img* history_count,
                                          const vkr_shadow_accum_params* params, const vkr_img* out_history, const vkr_img* out_count,
                                          const vkr_img* out_mask, void* stream) {
  ShadowAccumArgs a;
  VKR_TRY(shadow_accum_args("shadow_mask_accumulate", depth, normal, velocity, prev_depth, mask, history, history_count, params, out_history,
                            out_count, out_mask, &a));
  const dim3 grid((a.out.w + 16 * SMA_PIXELS - 1) / (16 * SMA_PIXELS), (a.out.h + 15) / 16, 1);
  hipLaunchKernelGGL(k_shadow_mask_accumulate, grid, dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("shadow_mask_accumulate");
}

extern "C" int vkr_selftest_accum_division(uint32_t* device_counter, void* stream) {
  if (!device_counter) { set_error("selftest_accum_division: NULL counter"); return VKR_ERR_NULL; }
  hipLaunchKernelGGL(k_selftest_accum_division, dim3(1024), dim3(256), 0, (hipStream_t)stream, device_counter);
  return launch_status("selftest_accum_division");
}

// Host only: vkr_shadow_disk_samples with the rotation of frame `frame` of a cycle of `frame_count`.  The expression of the angle
// is vkr_shadow_disk_samples' at frame_count 1, operation for operation: the same floats.
extern "C" void vkr_shadow_disk_samples_frame(uint32_t sample_count, uint32_t pattern_side, uint32_t frame, uint32_t frame_count, float* out) {
  if (!out || sample_count < 1 || sample_count > 64 || (pattern_side != 1 && pattern_side != 2 && pattern_side != 4)) return;
  if (frame_count < 1 || frame_count > 64) return;
  const uint32_t patterns = pattern_side * pattern_side;
  const double two_pi = 6.283185307179586;
  for (uint32_t p = 0; p < patterns; p++)
    for (uint32_t k = 0; k < sample_count; k++) {
      const double rho = std::sqrt(((double)k + 0.5) / (double)sample_count);
      const double phi = (double)k * 2.399963229728653 +
                         two_pi * (double)(((7u * p) % patterns) * frame_count + frame % frame_count) / (double)(patterns * frame_count);
      out[((size_t)p * sample_count + k) * 2] = (float)(rho * std::cos(phi));
      out[((size_t)p * sample_count + k) * 2 + 1] = (float)(rho * std::sin(phi));
    }
}
