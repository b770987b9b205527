// shadow_mask_rt_soft.hpp — program "shadow_mask_rt_soft" but for the walk: the kernel argument, the pass over the pixels of a
// block with the any-hit of a lane's ray handed in, the light-volume cull, and the gates the entries add to shadow_mask_rt.hpp's.
// The rule is frozen in DESIGN_NUMERICS.md (Shadow mask, ray traced, area lights) and restated in
// tests/shadow_mask_rt_soft_reference.py.
#ifndef VKR_SHADOW_MASK_RT_SOFT_HPP
#define VKR_SHADOW_MASK_RT_SOFT_HPP

#include "shadow_mask_rt.hpp"

namespace vkr {

#define SMRT_SOFT_MAX_SAMPLES 64

// All of it wave-uniform: a kernel argument, read through scalar loads
struct ShadowMaskRtSoftArgs : ShadowMaskRtArgs {
  float radius[SMRT_MAX_LIGHTS];
  uint32_t sample_count;   // S, 1..64
  uint32_t pattern_side;   // P: 1, 2 or 4
  const float* samples;    // [P * P][S][2]
};

// dvec of sample (u, v) of the disk of `radius` around the tip of dvec, in the frame (T, B) across it
VKR_DEV f3 soft_sample_dvec(f3 dvec, f3 T, f3 B, float radius, float u, float v) {
  const f3 e = mk3(cfma(v, B.x, u * T.x), cfma(v, B.y, u * T.y), cfma(v, B.z, u * T.z));
  return mk3(cfma(radius, e.x, dvec.x), cfma(radius, e.y, dvec.y), cfma(radius, e.z, dvec.z));
}

// The light-volume cull's descent: does the box [lo, hi] of this lane overlap the widened box of any triangle?  Called by the
// whole wave; `live` false: the lane has no box and only follows.  The walk of wave_any_hit_walk with a box in place of the ray
// and of the triangle test: a lane retires on its first overlap.  A comparison with a NaN is false: such a box overlaps nothing.
VKR_DEV bool wave_box_overlaps_any(const AccelView& a, f3 lo, f3 hi, bool live, uint32_t* stack) {
  bool pending = live, found = false;
  if (a.node_count == 0) return false;
  uint32_t node = 0;
  int sp = 0;
  for (;;) {
    const vkr_accel_node nd = a.nodes[node];
    const bool overlap = pending && lo.x <= nd.hi[0] && hi.x >= nd.lo[0] && lo.y <= nd.hi[1] && hi.y >= nd.lo[1] && lo.z <= nd.hi[2] && hi.z >= nd.lo[2];
    if (__ballot(overlap) != 0ull) {
      if (nd.count == 0u) {  // interior: the second child waits, the first is next
        stack[sp] = nd.first + 1u;
        sp++;
        node = nd.first;
        continue;
      }
      bool test = overlap;
      for (uint32_t k = 0; k < nd.count; k++) {
        const vkr_accel_tri& tr = a.tris[nd.first + k];
        if (test && lo.x <= tr.hi[0] && hi.x >= tr.lo[0] && lo.y <= tr.hi[1] && hi.y >= tr.lo[1] && lo.z <= tr.hi[2] && hi.z >= tr.lo[2]) {
          found = true; pending = false; test = false;
        }
        if (__ballot(test) == 0ull) break;
      }
      if (__ballot(pending) == 0ull) break;
    }
    if (sp == 0) break;
    sp--;
    node = __builtin_amdgcn_readfirstlane(stack[sp]);
  }
  return found;
}

// the pass; `walk(origin, dvec, cast, stack)` is the any-hit of a lane's ray, called by the whole wave.  MODE 1, the cull: per light
// with a radius, the lanes whose S segment boxes together overlap no triangle box count their cast samples and walk nothing.
// MODE 0: every cast sample is walked.  MODE 2 is the cull's own measurement (tools/shadow_mask_rt_soft_timing.py), never an
// entry of the library: no ray is walked, and the channel of a light with a radius reads 255 where the cull settles the lane.
template <int MODE, class Walk>
VKR_DEV void shadow_mask_rt_soft_pixels(const ShadowMaskRtSoftArgs& a, uint32_t (*stacks)[ACCEL_STACK], const Walk& walk) {
  constexpr bool CULL = MODE != 0;
  const RtPixel p = rt_pixel(a);
  uint32_t result = 0xFFFFFFFFu;
  if (__ballot(p.geometry) != 0ull) {  // the whole wave
    const RtSurface s = rt_surface(a, p, a.normal_offset);
    const uint32_t S = a.sample_count, pm = a.pattern_side - 1u;
    // the pattern of this pixel; a lane outside the image reads a pattern of the table like any other
    const float* table = a.samples + (size_t)((((uint32_t)p.ly & pm) * a.pattern_side + ((uint32_t)p.lx & pm)) * S) * 2u;
    for (uint32_t l = 0; l < a.light_count; l++) {  // wave-uniform
      const f3 light = mk3(a.lights[l][0], a.lights[l][1], a.lights[l][2]);
      const f3 dvec = a.lights[l][3] != 0.0f ? light - s.origin : light;
      const float radius = a.radius[l];
      uint32_t code;
      if (radius == 0.0f) {  // wave-uniform: the hard pass's step, dvec untouched
        const bool cast = p.geometry && dot(s.n, dvec) > 0.0f;
        bool lit = false;
        if (__ballot(cast) != 0ull) lit = cast && !walk(s.origin, dvec, cast, stacks[p.wave]);
        code = lit ? 255u : 0u;
      } else {
        f3 T, B;
        tangent_frame(normalize(dvec), &T, &B);
        uint32_t visible = 0;
        bool walks = p.geometry;
        if constexpr (CULL) {
          // the union of the segment boxes of the cast samples, each as LaneRay makes it (mul, then add; fminf / fmaxf drop a NaN)
          f3 lo = mk3(INFINITY, INFINITY, INFINITY), hi = mk3(-INFINITY, -INFINITY, -INFINITY);
          uint32_t casts = 0;
          for (uint32_t k = 0; k < S; k++) {
            const f3 d = soft_sample_dvec(dvec, T, B, radius, table[2u * k], table[2u * k + 1u]);
            if (p.geometry && dot(s.n, d) > 0.0f) {
              casts++;
              const float ax = s.origin.x + a.tmin * d.x, ay = s.origin.y + a.tmin * d.y, az = s.origin.z + a.tmin * d.z;
              const float bx = s.origin.x + 1.0f * d.x, by = s.origin.y + 1.0f * d.y, bz = s.origin.z + 1.0f * d.z;
              lo = mk3(fminf(lo.x, fminf(ax, bx)), fminf(lo.y, fminf(ay, by)), fminf(lo.z, fminf(az, bz)));
              hi = mk3(fmaxf(hi.x, fmaxf(ax, bx)), fmaxf(hi.y, fmaxf(ay, by)), fmaxf(hi.z, fmaxf(az, bz)));
            }
          }
          const bool any = casts != 0u;
          walks = false;
          if (__ballot(any) != 0ull) walks = wave_box_overlaps_any(a.accel, lo, hi, any, stacks[p.wave]);
          if (!walks) visible = casts;  // every ray of this lane misses
        }
        if (MODE != 2 && (!CULL || __ballot(walks) != 0ull)) {  // the whole wave
          for (uint32_t k = 0; k < S; k++) {  // wave-uniform
            const f3 d = soft_sample_dvec(dvec, T, B, radius, table[2u * k], table[2u * k + 1u]);
            const bool cast = walks && dot(s.n, d) > 0.0f;  // false for the part of the disk below the horizon and for any NaN
            if (__ballot(cast) != 0ull && cast && !walk(s.origin, d, cast, stacks[p.wave])) visible++;
          }
        }
        code = MODE == 2 ? (walks ? 0u : 255u) : (510u * visible + S) / (2u * S);
      }
      if (p.geometry) result = (result & ~(0xFFu << (8u * l))) | (code << (8u * l));
    }
  }
  if (p.inside) *texel_ptr<uint32_t>(a.out, p.lx, p.ly) = result;
}

// the gates the soft entries add, under `program`'s prefix, and the rest of the kernel argument; after shadow_mask_rt_args
inline int shadow_mask_rt_soft_args(const char* program, const vkr_shadow_rt_soft* soft, ShadowMaskRtSoftArgs* a) {
  static_assert(sizeof(vkr_shadow_rt_soft) == 40, "vkr_shadow_rt_soft: four radii, two words, a pointer and two words");
  if (!soft) { set_error("%s: soft is NULL", program); return VKR_ERR_NULL; }
  if (!soft->samples) { set_error("%s: samples is NULL", program); return VKR_ERR_NULL; }
  if (soft->sample_count < 1 || soft->sample_count > SMRT_SOFT_MAX_SAMPLES) {
    set_error("%s: sample_count %u, expected 1..%d", program, soft->sample_count, SMRT_SOFT_MAX_SAMPLES);
    return VKR_ERR_EXTENT;
  }
  if (soft->pattern_side != 1 && soft->pattern_side != 2 && soft->pattern_side != 4) {
    set_error("%s: pattern_side %u, expected 1, 2 or 4", program, soft->pattern_side);
    return VKR_ERR_EXTENT;
  }
  for (uint32_t l = 0; l < a->light_count; l++)
    if (!(soft->radius[l] >= 0.0f) || std::isinf(soft->radius[l])) {
      set_error("%s: light %u has radius %g, expected a finite radius >= 0", program, l, (double)soft->radius[l]);
      return VKR_ERR_EXTENT;
    }
  if (soft->reserved[0] != 0 || soft->reserved[1] != 0) {
    set_error("%s: soft reserved is %u, %u, must be 0", program, soft->reserved[0], soft->reserved[1]);
    return VKR_ERR_EXTENT;
  }
  for (uint32_t l = 0; l < SMRT_MAX_LIGHTS; l++) a->radius[l] = l < a->light_count ? soft->radius[l] : 0.0f;
  a->sample_count = soft->sample_count;
  a->pattern_side = soft->pattern_side;
  a->samples = soft->samples;
  return VKR_OK;
}

}  // namespace vkr

#endif
