// gtao_slice.hpp — what the programs that integrate an occlusion arc over a screen-space slice share: the 4x4 slice-direction
// slot, the exact slice frame, the horizon walk, the horizon clamp and the arc (gtao/main.comp:84-108,198-248,276-278,
// gtao/main.frag:66-90,164-186, sssr/trace.comp:123-139).  Callers: k_gtao_main (gtao.hip), k_gtao_v2 and k_screen_trace
// (variants.hip), k_gtao_rt (accel.hip, the slot only) and the trace epilogue (ssr.hip).
#pragma once
#include "vkr_device.hpp"

namespace vkr {

// 16 * gtao_direction(pos): the pixel's entry in the table of 16 slice angles, a pattern that repeats every 4x4 pixels
VKR_DEV int gtao_dir_slot(int gx, int gy) { return (((gx + gy) & 3) << 2) + (gx & 3); }

// The exact slice frame (DESIGN_NUMERICS.md: the argument of the acos that follows reaches +-1 when the surface is seen
// edge-on in the slice, and whether it rounds past — NaN, which zeroes the arc — is decided by its last bit).
// slice_normal: normal of the plane through the view direction w0 and `toward`; normal_projected: the surface normal
// projected into that plane; X: the in-plane axis perpendicular to w0 (main.frag takes another axis and ignores it).
// FUSED: the projection is one fused multiply-add per component (main.comp under the numeric contract) or a product and a
// difference rounded one after the other (main.frag, trace.comp); the two differ in the last bit and each program keeps its own.
struct SliceFrame { f3 slice_normal, normal_projected, X; };
template <bool FUSED> VKR_DEV SliceFrame slice_frame(f3 w0, f3 toward, f3 normal) {
  SliceFrame s;
  s.slice_normal = normalize(cross(w0, toward));
  const float d = dot(normal, s.slice_normal);
  s.normal_projected = FUSED ? madd(normal, -d, s.slice_normal) : normal - d * s.slice_normal;
  s.X = normalize(cross(s.slice_normal, w0));
  return s;
}
// n: the angle between the projected normal and the view direction, from the projected normal's cosine against `axis`
VKR_DEV float slice_normal_angle(f3 normal_projected, f3 axis) { return VKR_PI / 2.0f - acosf(dot(normalize(normal_projected), axis)); }

// the horizon angle h limited to a quarter turn past the projected normal's angle n
VKR_DEV float clamp_horizon(float h, float n) { return vmin(n + vmin(h - n, VKR_PI / 2.0f), h); }
// the arc integral of the slice between the view direction and the clamped horizon, without its weight
VKR_DEV float horizon_arc(float h, float n) { return vmax((-cosf(2.0f * h - n) + cosf(n)) + (2.0f * h) * sinf(n), 0.0f); }
// the cosine-weighted arc as main.comp:246-248 (MIS) and trace.comp:127-134 weigh it
VKR_DEV float arc_occlusion(float h, float n, float len_np) { return (((1.0f / VKR_PI) * len_np) * 0.25f) * horizon_arc(h, n); }

// main.comp:84-108 == main.frag:66-90: the largest cosine, against the view direction v, of the directions from camera_start
// to the surface under STEPS samples of a screen-space segment; the walk ends where the surface recedes by more than 0.1
// (MAX_THIKNESS).  sample_uv(i): texture coordinate of sample i = 1 .. STEPS; depth_at(uv): texture(depth, uv);
// max_of(a, b): the running maximum.  The break test is exact.  The cosine is max()-reduced and then goes through acos,
// whose slope is unbounded at +-1: where the depth has no coherence the offset to a sample is all but parallel to the view
// direction, the cosine sits one or two ulps from 1 and the last bit moves the horizon by 3e-4 rad — an arc of the order of
// 1e-4, which is the whole value where the arc is small.  EXACT_COS: dot(v, normalize(offset)) in the shader's operation order
// (bit for bit the contract's cosine: main.frag, main_deinterleaved.comp and main.comp without MIS store the bare arc);
// otherwise the dot product scaled by the hardware rsq (1 ulp, another order: main.comp under MIS, on the frame's chain,
// where the blend with the trace's term swamps that arc).
template <int STEPS, bool EXACT_COS = false, class SampleUv, class DepthAt, class MaxOf>
VKR_DEV float horizon_walk(const Proj& pr, f3 camera_start, f3 v, SampleUv sample_uv, DepthAt depth_at, MaxOf max_of) {
  float h_cos = -1.0f;
  float previous_z = camera_start.z;
#pragma unroll 1
  for (int i = 1; i <= STEPS; i++) {
    const f2 tc = sample_uv(i);
    const float sample_depth = depth_at(tc);
    const f3 sample_pos = reconstruct_view_vec(tc, sample_depth, pr);
    if (sample_pos.z > previous_z + 0.1f) break;
    previous_z = sample_pos.z;
    const f3 sample_offset = sample_pos - camera_start;
    h_cos = max_of(h_cos, EXACT_COS ? dot(v, normalize(sample_offset)) : dot(v, sample_offset) * fast_rsq(dot(sample_offset, sample_offset)));
  }
  return h_cos;
}

}  // namespace vkr
