// scene_triangles.hpp — what vkr_scene_triangles (accel_refit.hip) and vkr_scene_triangle_normals (scene_normals.hip) share: the
// draw table in scratch, the kernel argument, the vertices of a lane's triangle, and every gate of the two entries.
#ifndef VKR_SCENE_TRIANGLES_HPP
#define VKR_SCENE_TRIANGLES_HPP

#include "raster_common.hpp"

#include <vector>

namespace vkr {

struct TriDraw {      // 64 bytes
  float m[4][3];      // m[c][r] of the draw's matrix: the three rows that make a position (model) or a normal (normal; m[3] unused)
  uint32_t index_offset, vertex_offset, tri_base, tri_count;
};
struct SceneTriArgs {
  const vkr_raster_vertex* vertices;
  const uint32_t* indices;
  const TriDraw* draws;
  void* out;
  uint32_t vertex_count, draw_count, total;
};

// the draw of global triangle g and the vertex buffer indices of its three corners; false: one lies outside the vertex buffer (a
// triangle the rasterisers do not draw; nothing may be read for it)
VKR_DEV bool scene_triangle_corners(const SceneTriArgs& a, uint32_t g, TriDraw* d, uint64_t vi[3]) {
  *d = a.draws[draw_of(a.draws, a.draw_count, g)];
  const uint32_t j = g - d->tri_base;
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    vi[k] = (uint64_t)a.indices[d->index_offset + 3u * j + (uint32_t)k] + d->vertex_offset;  // check_scene: the index range is inside
    inside = inside && vi[k] < a.vertex_count;
  }
  return inside;
}

inline uint64_t scene_triangles_scratch(uint32_t draw_count) { return align_up(sizeof(TriDraw) * (uint64_t)(draw_count ? draw_count : 1u), 256); }

// Every gate of an entry under `program`'s prefix, its kernel argument and the upload of the draw table (recorded on the stream:
// the last step before the launch).  normals: the table holds transforms[].normal and out must be 16-byte aligned.  *launch is
// false where there is nothing to do.
inline int scene_triangles_args(const char* program, const vkr_raster_scene* scene, void* out, uint64_t out_capacity, void* scratch,
                                uint64_t scratch_bytes, bool normals, hipStream_t stream, SceneTriArgs* args, bool* launch) {
  *launch = false;
  if (!scene) { set_error("%s: NULL scene", program); return VKR_ERR_NULL; }
  uint64_t total = 0;
  VKR_TRY(check_scene(program, scene, false, &total));
  if (total == 0) return VKR_OK;
  if (total > (1u << 30)) { set_error("%s: %llu triangles, at most 2^30", program, (unsigned long long)total); return VKR_ERR_EXTENT; }
  if (!out || !scratch) { set_error("%s: NULL output or scratch", program); return VKR_ERR_NULL; }
  if (normals && ((uintptr_t)out & 15u) != 0) { set_error("%s: out must be 16-byte aligned", program); return VKR_ERR_LAYOUT; }
  if (total > out_capacity) {
    set_error("%s: %llu triangles do not fit into %llu", program, (unsigned long long)total, (unsigned long long)out_capacity);
    return VKR_ERR_EXTENT;
  }
  const uint64_t need = scene_triangles_scratch(scene->draw_count);
  if (scratch_bytes < need) { set_error("%s: scratch too small (%llu bytes, %llu needed)", program, (unsigned long long)scratch_bytes, (unsigned long long)need); return VKR_ERR_EXTENT; }
  std::vector<TriDraw> draws(scene->draw_count);
  uint32_t tri_base = 0;
  for (uint32_t i = 0; i < scene->draw_count; i++) {
    const vkr_raster_draw& s = scene->draws[i];
    const vkr_mat4& m = normals ? scene->transforms[s.transform_index].normal : scene->transforms[s.transform_index].model;
    TriDraw& d = draws[i];
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 3; r++) d.m[c][r] = m.m[c * 4 + r];
    d.index_offset = s.index_offset; d.vertex_offset = s.vertex_offset;
    d.tri_base = tri_base; d.tri_count = s.index_count / 3u;
    tri_base += d.tri_count;
  }
  SceneTriArgs& a = *args;
  a.vertices = scene->vertices; a.indices = scene->indices;
  a.draws = (const TriDraw*)scratch;
  a.out = out;
  a.vertex_count = scene->vertex_count; a.draw_count = scene->draw_count; a.total = tri_base;
  store_table<32>(draws, a.draws, stream);
  *launch = true;
  return VKR_OK;
}

}  // namespace vkr

#endif
