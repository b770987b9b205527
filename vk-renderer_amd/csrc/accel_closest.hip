// accel_closest.hip — vkr_accel_closest: the closest hit of arbitrary rays, the ray-level entry of wave_closest_hit
// (accel_traverse.hpp; DESIGN_NUMERICS.md, "Ray query, closest hit").  Where vkr_accel_query / vkr_accel_occluded say whether
// anything is hit, this says where (t), on which input triangle (index) and at which barycentrics (u, v), so that something can
// be shaded there: program "reflections_rt" (reflections_rt.hip) is the first consumer.  The kernel is k_accel_occluded's with
// another walk; a ray's answer is one 16-byte store.
#include "vkr_host.hpp"
#include "accel_traverse.hpp"

// tools/reflections_rt_timing.py builds this file a second time with the child-ordering walk under another entry name, to
// measure the ordering against the plain descent; the library is built with the defaults
#ifndef VKR_CLOSEST_WALK
#define VKR_CLOSEST_WALK wave_closest_hit
#endif
#ifndef VKR_CLOSEST_ENTRY
#define VKR_CLOSEST_ENTRY vkr_accel_closest
#define VKR_CLOSEST_KERNEL k_accel_closest
#endif
#ifndef VKR_CLOSEST_KERNEL  // a second build lives beside the library in one process: its kernel needs a name of its own
#define VKR_CLOSEST_KERNEL k_accel_closest_variant
#endif

namespace vkr {

__global__ __launch_bounds__(256) void VKR_CLOSEST_KERNEL(AccelView a, const float* org, const float* dir, float tmin, float tmax,
                                                       uint32_t n, vkr_accel_hit* out) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  const RayLane r = load_ray_lane(org, dir, n, stacks);
  vkr_accel_hit h;
  VKR_CLOSEST_WALK(a, r.o, r.d, tmin, tmax, r.live, r.stack, &h);
  if (r.live) store_u32x4((uint8_t*)(out + r.i), __float_as_uint(h.t), __float_as_uint(h.u), __float_as_uint(h.v), h.index);
}

}  // namespace vkr

using namespace vkr;

extern "C" int VKR_CLOSEST_ENTRY(const vkr_accel* accel, const float* origins, const float* dirs, float tmin, float tmax, uint32_t n,
                                 vkr_accel_hit* out_hits, void* stream) {
  static_assert(sizeof(vkr_accel_hit) == 16, "vkr_accel_hit: three floats and an index, one 16-byte store");
  VKR_TRY(check_ray_batch("accel_closest", accel, origins, dirs, out_hits, n));
  if (n == 0) return VKR_OK;
  if (((uintptr_t)out_hits & 15u) != 0) { set_error("accel_closest: out_hits must be 16-byte aligned"); return VKR_ERR_LAYOUT; }
  hipLaunchKernelGGL(VKR_CLOSEST_KERNEL, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, view_of(accel), origins, dirs, tmin, tmax, n, out_hits);
  return launch_status("accel_closest");
}
