// ssao.hip — program "ssao".
//
// Reference: src/ssao.cpp:54-97 and shaders/ssao/shader.{vert,frag}: the reference's first ambient-occlusion pass.  One
// surface in (depth, the base mip of the view), one out (R8_UNORM of any extent: the shader works in uv).  Per pixel: one
// bilinear depth tap to reconstruct the view position, then 16 projected sphere samples with one bilinear depth tap each.
// No tap depends on another, and nothing but the pixel's own position decides where they fall.
//
// Roofline: 5 compulsory bytes per pixel (4 read, 1 written) against 17 bilinear footprints (34 8-byte loads) and 48 IEEE
// divisions.  Measured at 2.5 % of the stream read's rate: not HBM; which of the texture-address path and the VALU paces it is
// an estimate.
#include "vkr_host.hpp"

namespace vkr {

#define SSAO_SAMPLES 16
#define SSAO_BATCH 4     // footprints whose loads are issued together
#define SSAO_BX 16       // a wave is 16 x 4 pixels of a 16 x 16 block: neighbouring pixels' taps share cache lines
#define SSAO_BY 16

// All of it wave-uniform: a kernel argument, read through scalar loads, so matrix and samples sit in SGPRs.
struct SsaoArgs {
  Tex depth, out;
  Mat4 projection;
  Proj pr;
  float samples[SSAO_SAMPLES][3];
};

// texture(depth, uv).  PAIR: each footprint row as one 8-byte load (pair_taps; needs a depth image at least 2 texels wide).
template <bool PAIR> VKR_DEV BilinearTaps tap_issue(const Tex& depth, f2 uv) {
  if (PAIR) return pair_taps(depth, pair_footprint(depth, uv));
  return bilinear_taps_u32(depth, uv);
}

// shader.frag:21-41, one thread per output pixel
template <bool PAIR>
__global__ __launch_bounds__(SSAO_BX * SSAO_BY) void k_ssao(SsaoArgs a) {
  const i2 blk = xcd_block<8, 8>();  // chunks of 128 x 128 output pixels
  const int lx = blk.x * SSAO_BX + threadIdx.x;
  const int ly = blk.y * SSAO_BY + threadIdx.y;
  if (lx >= a.out.w || ly >= a.out.h) return;
  const f2 screen_uv = mk2(pixel_centre_uv(lx, (float)a.out.w), pixel_centre_uv(ly, (float)a.out.h));
  const float frag_depth = taps_resolve<FmtD24>(tap_issue<PAIR>(a.depth, screen_uv));
  const f3 camera_pos = reconstruct_view_vec(screen_uv, frag_depth, a.pr);

  float sum = 0.0f;
#pragma unroll
  for (int base = 0; base < SSAO_SAMPLES; base += SSAO_BATCH) {
    BilinearTaps taps[SSAO_BATCH];
    float pos_depth[SSAO_BATCH];
#pragma unroll
    for (int k = 0; k < SSAO_BATCH; k++) {
      const float* s = a.samples[base + k];
      const f3 pos = madd(camera_pos, 0.05f, mk3(s[0], s[1], s[2]));
      // IEEE division: a sample on the eye plane has w = 0, and the infinities / NaNs that follow are part of the result
      const f4 clip = mul(a.projection, mk4(pos.x, pos.y, pos.z, 1.0f));
      const f3 ndc = mk3(clip.x / clip.w, clip.y / clip.w, clip.z / clip.w);
      const f2 sample_uv = mk2(cfma(0.5f, ndc.x, 0.5f), cfma(0.5f, ndc.y, 0.5f));
      taps[k] = tap_issue<PAIR>(a.depth, sample_uv);
      pos_depth[k] = ndc.z;
    }
#pragma unroll
    for (int k = 0; k < SSAO_BATCH; k++) {
      const float sample_depth = taps_resolve<FmtD24>(taps[k]);
      sum += (pos_depth[k] < sample_depth + 0.0000001f) ? 1.0f : 0.0f;
    }
  }
  sum /= (float)SSAO_SAMPLES;  // k / 16: exact
  *texel_ptr<uint8_t>(a.out, lx, ly) = (uint8_t)float_to_unorm8(sum);
}

}  // namespace vkr

using namespace vkr;

extern "C" int vkr_ssao(const vkr_img* depth, const vkr_ssao_params* params, const vkr_img* out_occlusion, void* stream) {
  if (!depth) { set_error("ssao: depth is NULL"); return VKR_ERR_NULL; }
  if (!params) { set_error("ssao: params is NULL"); return VKR_ERR_NULL; }
  if (!out_occlusion) { set_error("ssao: out_occlusion is NULL"); return VKR_ERR_NULL; }
  SsaoArgs a;
  VKR_TRY(make_tex(depth, 0, VKR_FMT_D24_UNORM_S8, "ssao.depth", &a.depth));
  VKR_TRY(make_tex(out_occlusion, 0, VKR_FMT_R8_UNORM, "ssao.out_occlusion", &a.out));
  VKR_TRY(require_whole_frame(a.depth, "ssao: depth", "windows are not supported (the taps reach anywhere: a single-GPU pass)"));
  VKR_TRY(require_whole_frame(a.out, "ssao: out_occlusion", "windows are not supported (the taps reach anywhere: a single-GPU pass)", 65535));
  load_mat(a.projection, params->projection);
  load_proj(a.pr, params->fovy, params->aspect, params->znear, params->zfar);
  for (int i = 0; i < SSAO_SAMPLES; i++)
    for (int c = 0; c < 3; c++) a.samples[i][c] = params->samples[i][c];
  const dim3 block(SSAO_BX, SSAO_BY);
  void (*kernel)(SsaoArgs) = a.depth.w >= 2 ? k_ssao<true> : k_ssao<false>;
  hipLaunchKernelGGL(kernel, grid2d(a.out.w, a.out.h, block), block, 0, (hipStream_t)stream, a);
  return launch_status("ssao");
}
