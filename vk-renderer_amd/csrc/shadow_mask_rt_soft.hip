// shadow_mask_rt_soft.hip — programs "shadow_mask_rt_soft" and "shadow_mask_rt_soft_cutout".
//
// No reference program.  The traced shadow mask of shadow_mask_rt.hip for lights with a size: per full-resolution pixel and light
// S any-hit rays towards S points of a disk around the light that faces the surface point, and the share of them that arrive, in
// 255ths, in the light's channel.  The points come from a table of P x P patterns that tiles the image; a light with radius 0 is
// traced as the hard pass traces it.  The rule is frozen in DESIGN_NUMERICS.md (Shadow mask, ray traced, area lights) and restated
// in tests/shadow_mask_rt_soft_reference.py.
//
// The tile shape and the stacks are the hard pass's: a wave is an 8 x 8 pixel tile, a block four waves with one 64-word stack each
// in LDS.  The light loop and the sample loop are wave-uniform; the table is read per lane (the pattern differs per pixel; at most
// 8 KiB, it stays in cache).  The light-volume cull (shadow_mask_rt_soft.hpp) settles the lanes that see the whole disk with one
// box descent per light instead of S walks; it measured slower in every case and is not built into the library.
#include "ray_cutout.hpp"
#include "shadow_mask_rt_soft.hpp"

#include <cmath>

// tools/shadow_mask_rt_soft_timing.py builds this file again with the other settings of the cull (1: the cull; 2: its report, see
// shadow_mask_rt_soft.hpp) under other entry names, to measure one against the other, and tests/test_shadow_mask_rt_soft_gpu.py
// compares their bytes; the library is built with the defaults
#ifndef VKR_SHADOW_RT_SOFT_CULL
#define VKR_SHADOW_RT_SOFT_CULL 0
#endif
#ifndef VKR_SHADOW_RT_SOFT_ENTRY
#define VKR_SHADOW_RT_SOFT_ENTRY vkr_shadow_mask_rt_soft
#define VKR_SHADOW_RT_SOFT_CUTOUT_ENTRY vkr_shadow_mask_rt_soft_cutout
#define VKR_SHADOW_RT_SOFT_LIBRARY 1
#endif

namespace vkr {

__global__ __launch_bounds__(256) void k_shadow_mask_rt_soft(ShadowMaskRtSoftArgs a) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  shadow_mask_rt_soft_pixels<VKR_SHADOW_RT_SOFT_CULL>(
      a, stacks, [&](f3 o, f3 d, bool cast, uint32_t* stack) { return wave_any_hit_ray(a.accel, o, d, a.tmin, 1.0f, cast, stack); });
}

// the same with the cutout filter in the walk
__global__ __launch_bounds__(256) void k_shadow_mask_rt_soft_cutout(ShadowMaskRtSoftArgs a, CutoutFilter f) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  shadow_mask_rt_soft_pixels<VKR_SHADOW_RT_SOFT_CULL>(
      a, stacks, [&](f3 o, f3 d, bool cast, uint32_t* stack) { return wave_any_hit_walk<true>(a.accel, o, d, a.tmin, 1.0f, cast, stack, f); });
}

}  // namespace vkr

using namespace vkr;

extern "C" int VKR_SHADOW_RT_SOFT_ENTRY(const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel, const vkr_shadow_rt_params* params,
                                        const vkr_shadow_rt_soft* soft, const vkr_img* out_mask, void* stream) {
  ShadowMaskRtSoftArgs a;
  VKR_TRY(shadow_mask_rt_args("shadow_mask_rt_soft", depth, normal, accel, params, out_mask, &a));
  VKR_TRY(shadow_mask_rt_soft_args("shadow_mask_rt_soft", soft, &a));
  const dim3 tiles(16, 16);
  hipLaunchKernelGGL(k_shadow_mask_rt_soft, grid2d(a.out.w, a.out.h, tiles), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("shadow_mask_rt_soft");
}

extern "C" int VKR_SHADOW_RT_SOFT_CUTOUT_ENTRY(const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel, const vkr_hit_attrib* attribs,
                                               uint32_t attrib_count, const vkr_img* textures, uint32_t texture_count,
                                               const vkr_shadow_rt_params* params, const vkr_ray_cutout* cutout, const vkr_shadow_rt_soft* soft,
                                               const vkr_img* out_mask, void* scratch, uint64_t scratch_bytes, void* stream) {
  ShadowMaskRtSoftArgs a;
  VKR_TRY(shadow_mask_rt_args("shadow_mask_rt_soft_cutout", depth, normal, accel, params, out_mask, &a));
  VKR_TRY(shadow_mask_rt_soft_args("shadow_mask_rt_soft_cutout", soft, &a));
  CutoutFilter f;
  VKR_TRY(bind_cutout("shadow_mask_rt_soft_cutout", accel, attribs, attrib_count, textures, texture_count, cutout, scratch, scratch_bytes, (hipStream_t)stream, &f));
  const dim3 tiles(16, 16);
  hipLaunchKernelGGL(k_shadow_mask_rt_soft_cutout, grid2d(a.out.w, a.out.h, tiles), dim3(256), 0, (hipStream_t)stream, a, f);
  return launch_status("shadow_mask_rt_soft_cutout");
}

#ifdef VKR_SHADOW_RT_SOFT_LIBRARY
// Host only: the table generator of the frame and of Python.  A Vogel spiral of S points in the unit disk, turned per pattern.
extern "C" void vkr_shadow_disk_samples(uint32_t sample_count, uint32_t pattern_side, float* out) {
  if (!out || sample_count < 1 || sample_count > SMRT_SOFT_MAX_SAMPLES || (pattern_side != 1 && pattern_side != 2 && pattern_side != 4)) return;
  const uint32_t patterns = pattern_side * pattern_side;
  const double two_pi = 6.283185307179586;
  for (uint32_t p = 0; p < patterns; p++)
    for (uint32_t k = 0; k < sample_count; k++) {
      const double rho = std::sqrt(((double)k + 0.5) / (double)sample_count);
      const double phi = (double)k * 2.399963229728653 + two_pi * (double)((7u * p) % patterns) / (double)patterns;
      out[((size_t)p * sample_count + k) * 2] = (float)(rho * std::cos(phi));
      out[((size_t)p * sample_count + k) * 2 + 1] = (float)(rho * std::sin(phi));
    }
}
#endif
