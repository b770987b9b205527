// shadow_mask.hip — program "shadow_mask".
//
// No reference program: the reference rasterises its shadow maps (scene_renderer.cpp:222-274) and binds layer 0 to the shading
// pass, whose shader never samples it.  This is the lookup that makes the maps useful: per full-resolution pixel the visibility
// of up to four lights as a box of 1, 9 or 25 integer depth compares, one RGBA8_UNORM texel out (channel l = light l).
// The rule is frozen in DESIGN_NUMERICS.md (Shadow mask) and restated in tests/shadow_mask_reference.py.
//
// Roofline: 8 compulsory bytes per pixel (depth 4 read, mask 4 written); the taps of neighbouring pixels fall into the same or
// neighbouring map texels, so a wave's (2 r + 1)^2 dword loads per light hit a handful of cache lines.  16 multiply-adds, three
// IEEE divisions and one more for passes / taps per light: what paces it is an estimate.
#include "vkr_host.hpp"

namespace vkr {

#define SM_BX 16  // a wave is 16 x 4 pixels of a 16 x 16 block: neighbouring pixels' taps share cache lines
#define SM_BY 16
#define SM_MAX_LAYERS 4

struct ShadowLayer {
  const uint8_t* p;
  int pitch;
};

// All of it wave-uniform: a kernel argument, read through scalar loads; the light loop indexes it with a uniform index, so the
// matrix of the light at hand sits in SGPRs.
struct ShadowMaskArgs {
  Tex depth, out;
  Proj pr;
  int size;              // edge of every layer
  uint32_t layer_count;  // 1..4
  uint32_t bias;         // saturated at 2^24 by the launcher: code + nothing wraps in 32 bits
  ShadowLayer layer[SM_MAX_LAYERS];
  Mat4 m[SM_MAX_LAYERS];  // mvps[l] * inverse_camera
};

// passes of the (2 R + 1)^2 box around (tx, ty): a tap outside the map passes, one inside passes when code <= d24 + bias.
// Every address is clamped into the map, so that the loads of a row go out together, unconditionally, before any compare.
template <int R> VKR_DEV uint32_t box_passes(const ShadowLayer& L, int size, int tx, int ty, uint32_t code, uint32_t bias) {
  constexpr int N = 2 * R + 1;
  uint32_t xoff[N];
  bool xin[N];
#pragma unroll
  for (int i = 0; i < N; i++) {
    const int x = tx + i - R;
    xin[i] = (uint32_t)x < (uint32_t)size;
    xoff[i] = (uint32_t)iclamp(x, 0, size - 1) * 4u;
  }
  uint32_t passes = 0;
#pragma unroll
  for (int j = 0; j < N; j++) {
    const int y = ty + j - R;
    const bool yin = (uint32_t)y < (uint32_t)size;
    const uint8_t* row = L.p + __umul24((uint32_t)iclamp(y, 0, size - 1), (uint32_t)L.pitch);
    uint32_t word[N];
#pragma unroll
    for (int i = 0; i < N; i++) word[i] = *(const uint32_t*)(row + xoff[i]);
#pragma unroll
    for (int i = 0; i < N; i++) passes += (!(yin && xin[i]) || code <= (word[i] & 0xFFFFFFu) + bias) ? 1u : 0u;
  }
  return passes;
}

// one lane per pixel of out (== depth's extent)
template <int R>
__global__ __launch_bounds__(SM_BX * SM_BY) void k_shadow_mask(ShadowMaskArgs a) {
  const i2 blk = xcd_block<8, 8>();  // chunks of 128 x 128 pixels
  const int lx = blk.x * SM_BX + threadIdx.x;
  const int ly = blk.y * SM_BY + threadIdx.y;
  if (lx >= a.out.w || ly >= a.out.h) return;
  const float d = d24_to_float(*(const uint32_t*)(a.depth.p + toff(a.depth, lx, ly, 4)));
  uint32_t result = 0xFFFFFFFFu;
  if (d < 1.0f) {
    const f2 uv = mk2(pixel_centre_uv(lx, (float)a.out.w), pixel_centre_uv(ly, (float)a.out.h));
    const f3 view = reconstruct_view_vec(uv, d, a.pr);
    const float fsize = (float)a.size;
    constexpr float taps = (float)((2 * R + 1) * (2 * R + 1));
    for (uint32_t l = 0; l < a.layer_count; l++) {
      const f4 clip = mul(a.m[l], mk4(view.x, view.y, view.z, 1.0f));
      const f3 ndc = mk3(clip.x / clip.w, clip.y / clip.w, clip.z / clip.w);  // IEEE division
      // lit without taps; the negated compares take every NaN with them
      const bool lit = clip.w <= 0.0f || !(ndc.x >= -1.0f && ndc.x <= 1.0f) || !(ndc.y >= -1.0f && ndc.y <= 1.0f) || !(ndc.z <= 1.0f);
      if (lit) continue;
      const uint32_t code = (uint32_t)rintf(vclamp(ndc.z, 0.0f, 1.0f) * 16777215.0f);
      const int tx = iclamp(f2i(floorf(cfma(0.5f, ndc.x, 0.5f) * fsize)), 0, a.size - 1);
      const int ty = iclamp(f2i(floorf(cfma(0.5f, ndc.y, 0.5f) * fsize)), 0, a.size - 1);
      const uint32_t passes = box_passes<R>(a.layer[l], a.size, tx, ty, code, a.bias);
      const uint32_t v = float_to_unorm8((float)passes / taps);
      const uint32_t sh = 8u * l;
      result = (result & ~(0xFFu << sh)) | (v << sh);
    }
  }
  *texel_ptr<uint32_t>(a.out, lx, ly) = result;
}

}  // namespace vkr

using namespace vkr;

extern "C" int vkr_shadow_mask(const vkr_img* depth, const vkr_img* layers, const vkr_shadow_mask_params* params, const vkr_img* out_mask,
                               void* stream) {
  if (!depth) { set_error("shadow_mask: depth is NULL"); return VKR_ERR_NULL; }
  if (!layers) { set_error("shadow_mask: layers is NULL"); return VKR_ERR_NULL; }
  if (!params) { set_error("shadow_mask: params is NULL"); return VKR_ERR_NULL; }
  if (!out_mask) { set_error("shadow_mask: out_mask is NULL"); return VKR_ERR_NULL; }
  if (params->layer_count < 1 || params->layer_count > SM_MAX_LAYERS) {
    set_error("shadow_mask: layer_count %u, expected 1..%d", params->layer_count, SM_MAX_LAYERS);
    return VKR_ERR_EXTENT;
  }
  if (params->radius > 2) { set_error("shadow_mask: radius %u, expected 0..2 (1, 9 or 25 taps)", params->radius); return VKR_ERR_EXTENT; }
  if (params->reserved != 0) { set_error("shadow_mask: reserved is %u, must be 0", params->reserved); return VKR_ERR_EXTENT; }
  ShadowMaskArgs a;
  VKR_TRY(make_tex(depth, 0, VKR_FMT_D24_UNORM_S8, "shadow_mask.depth", &a.depth));
  VKR_TRY(make_tex(out_mask, 0, VKR_FMT_RGBA8_UNORM, "shadow_mask.out_mask", &a.out));
  VKR_TRY(require_whole_frame(a.depth, "shadow_mask: depth", "windows are not supported (the taps reach anywhere: a single-GPU pass)"));
  VKR_TRY(require_whole_frame(a.out, "shadow_mask: out_mask", "windows are not supported (the taps reach anywhere: a single-GPU pass)", 65535));
  if (a.depth.w != a.out.w || a.depth.h != a.out.h) {
    set_error("shadow_mask: depth is %dx%d, out_mask %dx%d: one extent expected", a.depth.w, a.depth.h, a.out.w, a.out.h);
    return VKR_ERR_EXTENT;
  }
  a.layer_count = params->layer_count;
  a.size = 0;
  for (uint32_t l = 0; l < SM_MAX_LAYERS; l++) {
    if (l >= a.layer_count) { a.layer[l] = a.layer[0]; continue; }
    Tex t;
    VKR_TRY(make_tex(&layers[l], 0, VKR_FMT_D24_UNORM_S8, "shadow_mask.layers", &t));
    VKR_TRY(require_whole_frame(t, "shadow_mask: layers", "windows are not supported (single-GPU pass)"));
    if (l == 0) a.size = t.w;
    if (t.w != t.h || t.w != a.size) {
      set_error("shadow_mask: layers: layer %u is %dx%d, every layer must be square and of one extent (layer 0: %dx%d)", l, t.w, t.h, a.size, a.size);
      return VKR_ERR_EXTENT;
    }
    a.layer[l].p = t.p;
    a.layer[l].pitch = t.pitch;
  }
  // M_l = mvps[l] * inverse_camera, accumulated in double, rounded once (column-major, m[4 * column + row])
  for (uint32_t l = 0; l < SM_MAX_LAYERS; l++)
    for (int col = 0; col < 4; col++)
      for (int row = 0; row < 4; row++) {
        double acc = 0.0;
        for (int k = 0; k < 4; k++) acc += (double)params->mvps[l].m[4 * k + row] * (double)params->inverse_camera.m[4 * col + k];
        a.m[l].m[4 * col + row] = l < a.layer_count ? (float)acc : 0.0f;
      }
  load_proj(a.pr, params->fovy, params->aspect, params->znear, params->zfar);
  a.bias = params->bias < (1u << 24) ? params->bias : (1u << 24);  // code < 2^24: any larger bias passes every tap as well
  const dim3 block(SM_BX, SM_BY);
  void (*kernel)(ShadowMaskArgs) = params->radius == 0 ? k_shadow_mask<0> : params->radius == 1 ? k_shadow_mask<1> : k_shadow_mask<2>;
  hipLaunchKernelGGL(kernel, grid2d(a.out.w, a.out.h, block), block, 0, (hipStream_t)stream, a);
  return launch_status("shadow_mask");
}
