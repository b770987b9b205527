// scene_normals.hip — vkr_scene_triangle_normals: the world-space vertex normals of a raster scene's triangles on the device, one
// vkr_hit_normal per triangle in the order of vkr_scene_triangles: what program "reflections_rt_lit" interpolates at a hit, and
// what the host mirror recomputes beside the triangles when draws move (scene::SceneAccelerationStructure::refit).  The draw
// table, the corners of a lane's triangle and every gate are scene_triangles.hpp's; the table holds transforms[].normal.
#include "scene_triangles.hpp"

namespace vkr {

static_assert(sizeof(vkr_hit_normal) == 48, "the 16-byte stores below assume this size");

__global__ __launch_bounds__(256) void k_scene_triangle_normals(SceneTriArgs a) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= a.total) return;
  TriDraw d;
  uint64_t vi[3];
  const bool inside = scene_triangle_corners(a, g, &d, vi);
  float4* dst = (float4*)((vkr_hit_normal*)a.out + g);
  if (!inside) {  // as vkr_scene_triangles: nothing is read outside the vertex buffer
    const float nan = __uint_as_float(0x7FC00000u);
#pragma unroll
    for (int k = 0; k < 3; k++) dst[k] = make_float4(nan, nan, nan, 0.0f);
    return;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const vkr_raster_vertex* v = a.vertices + vi[k];
    const float x = v->norm[0], y = v->norm[1], z = v->norm[2];
    float n[3];
#pragma unroll
    for (int r = 0; r < 3; r++) n[r] = (d.m[0][r] * x + d.m[1][r] * y) + d.m[2][r] * z;  // no translation; every product and sum rounded on its own
    dst[k] = make_float4(n[0], n[1], n[2], 0.0f);
  }
}

}  // namespace vkr

using namespace vkr;

extern "C" int vkr_scene_triangle_normals(const vkr_raster_scene* scene, vkr_hit_normal* out, uint64_t out_capacity, void* scratch,
                                          uint64_t scratch_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SceneTriArgs a;
  bool launch = false;
  VKR_TRY(scene_triangles_args("scene_triangle_normals", scene, out, out_capacity, scratch, scratch_bytes, true, stream, &a, &launch));
  if (!launch) return VKR_OK;
  hipLaunchKernelGGL(k_scene_triangle_normals, dim3((a.total + 255) / 256), dim3(256), 0, stream, a);
  return launch_status("scene_triangle_normals");
}
