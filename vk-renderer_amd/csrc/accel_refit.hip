// accel_refit.hip — moving geometry under a fixed topology: vkr_accel_refit (device), vkr_accel_refit_layout (host, no GPU),
// vkr_accel_download, and vkr_scene_triangles, which makes the world-space triangles of a raster scene on the device.
//
// The topology stays the host builder's: every record slot keeps its input index, every node its `first` and `count`.  From the new
// vertices the records are recomputed by make_record (accel_record.hpp, the builder's own), then the node boxes bottom-up as exact
// unions — from scratch, never grown.  Every answer of the ray query is that of the frozen test looped over all triangles whatever
// the hierarchy, so a refitted structure answers bit for bit like one built from the moved triangles (DESIGN_NUMERICS.md, "Ray
// query: refit"); only the time of a walk depends on how well the old topology still fits.
//
// Schedule.  No byte is handed from one workgroup to another inside a launch: no counter, no flag.  A node's
// box depends on boxes of smaller height only (refit_schedule), and what one level writes the next reads after a kernel
// boundary, or after __syncthreads() inside the single workgroup of the tail:
//   k_accel_refit_records  one lane per record slot: nine floats in, four 16-byte stores out
//   k_accel_refit_level    one lane per node of one height, launched once per height while the level has more nodes than
//                          ACCEL_REFIT_TAIL_NODES
//   k_accel_refit_tail     one workgroup: every remaining height up to the root
// Level sizes never grow with the height, so the levels of the tail are the last ones.
#include "raster_common.hpp"
#include "accel_record.hpp"
#include "scene_triangles.hpp"

#include <vector>

namespace vkr {

// a level of at most this many nodes belongs to the tail (one node per lane of its single workgroup); a larger one gets a launch
constexpr uint32_t ACCEL_REFIT_TAIL_NODES = 256;

static_assert(sizeof(vkr_accel_tri) == 64 && sizeof(vkr_accel_node) == 32, "the 16-byte stores below assume these sizes");

__global__ __launch_bounds__(256) void k_accel_refit_records(vkr_accel_tri* tris, const float* verts, uint32_t n) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint32_t index = tris[j].index;  // < n: written by vkr_accel_create, rewritten unchanged
  const float* src = verts + 9ull * index;
  float v[9];
#pragma unroll
  for (int k = 0; k < 9; k++) v[k] = src[k];
  vkr_accel_tri r;
  make_record(v, index, r);
  float4* dst = (float4*)(tris + j);
  dst[0] = make_float4(r.v0[0], r.v0[1], r.v0[2], __uint_as_float(r.index));
  dst[1] = make_float4(r.e1[0], r.e1[1], r.e1[2], r.e2[0]);
  dst[2] = make_float4(r.e2[1], r.e2[2], r.lo[0], r.lo[1]);
  dst[3] = make_float4(r.lo[2], r.hi[0], r.hi[1], r.hi[2]);
}

// the box of node `id` from what lies below it: a leaf's records (all of this refit, written by an earlier launch), an interior
// node's two children (of smaller height: an earlier launch, or an earlier level of the tail); first and count stay
VKR_DEV void refit_node(vkr_accel_node* nodes, const vkr_accel_tri* tris, uint32_t id) {
  const uint32_t first = nodes[id].first, count = nodes[id].count;
  UnionBox b;
  if (count == 0u) {
    const vkr_accel_node c0 = nodes[first], c1 = nodes[first + 1u];
    b.take(c0.lo, c0.hi);
    b.take(c1.lo, c1.hi);
  } else {
    for (uint32_t k = 0; k < count; k++) {
      const float4 p = ((const float4*)(tris + first + k))[2], q = ((const float4*)(tris + first + k))[3];
      const float lo[3] = {p.z, p.w, q.x}, hi[3] = {q.y, q.z, q.w};
      b.take(lo, hi);
    }
  }
  float4* dst = (float4*)(nodes + id);
  dst[0] = make_float4(b.lo[0], b.lo[1], b.lo[2], __uint_as_float(first));
  dst[1] = make_float4(b.hi[0], b.hi[1], b.hi[2], __uint_as_float(count));
}

// order: the ids of ONE level
__global__ __launch_bounds__(256) void k_accel_refit_level(vkr_accel_node* nodes, const vkr_accel_tri* tris, const uint32_t* order, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) refit_node(nodes, tris, order[i]);
}

// the level offsets of the tail travel as kernel arguments: begin[l] .. begin[l + 1] in `order`, l in [0, levels)
struct RefitTail { uint32_t levels; uint32_t begin[ACCEL_MAX_DEPTH + 2]; };

__global__ __launch_bounds__(ACCEL_REFIT_TAIL_NODES) void k_accel_refit_tail(vkr_accel_node* nodes, const vkr_accel_tri* tris, const uint32_t* order, RefitTail t) {
  for (uint32_t l = 0; l < t.levels; l++) {
    const uint32_t begin = t.begin[l], end = t.begin[l + 1u];
    for (uint32_t i = begin + threadIdx.x; i < end; i += ACCEL_REFIT_TAIL_NODES) refit_node(nodes, tris, order[i]);
    __syncthreads();  // this workgroup's stores of the level before any of its lanes reads them as children
  }
}

// ---- vkr_scene_triangles (the draw table, the corners and the gates: scene_triangles.hpp) --------------------------------------------
__global__ __launch_bounds__(256) void k_scene_triangles(SceneTriArgs a) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= a.total) return;
  TriDraw d;
  uint64_t vi[3];
  const bool inside = scene_triangle_corners(a, g, &d, vi);
  float* dst = (float*)a.out + 9ull * g;
  if (!inside) {  // a triangle the rasterisers do not draw and no ray hits; nothing is read outside the vertex buffer
#pragma unroll
    for (int k = 0; k < 9; k++) dst[k] = __uint_as_float(0x7FC00000u);
    return;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const vkr_raster_vertex* v = a.vertices + vi[k];
    const float x = v->pos[0], y = v->pos[1], z = v->pos[2];
#pragma unroll
    for (int r = 0; r < 3; r++) dst[3 * k + r] = ((d.m[0][r] * x + d.m[1][r] * y) + d.m[2][r] * z) + d.m[3][r];  // every product and sum rounded on its own
  }
}

}  // namespace vkr

using namespace vkr;

extern "C" int vkr_accel_refit(vkr_accel* accel, const float* tri_vertices, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!accel) { set_error("vkr_accel_refit: NULL acceleration structure"); return VKR_ERR_NULL; }
  if (accel->tri_count == 0 || accel->node_count == 0) return VKR_OK;
  if (!tri_vertices) { set_error("vkr_accel_refit: NULL triangles"); return VKR_ERR_NULL; }
  const uint32_t n = accel->tri_count;
  hipLaunchKernelGGL(k_accel_refit_records, dim3((n + 255) / 256), dim3(256), 0, stream, accel->tris, tri_vertices, n);
  const std::vector<uint32_t>& lb = accel->level_begin;
  const uint32_t levels = (uint32_t)lb.size() - 1u;
  uint32_t l = 0;
  for (; l < levels && lb[l + 1] - lb[l] > ACCEL_REFIT_TAIL_NODES; l++) {
    const uint32_t count = lb[l + 1] - lb[l];
    hipLaunchKernelGGL(k_accel_refit_level, dim3((count + 255) / 256), dim3(256), 0, stream, accel->nodes, accel->tris, accel->order + lb[l], count);
  }
  RefitTail t;
  t.levels = levels - l;  // >= 1: the root's level has one node
  for (uint32_t k = 0; k < ACCEL_MAX_DEPTH + 2; k++) t.begin[k] = lb[l + k < levels ? l + k : levels];
  hipLaunchKernelGGL(k_accel_refit_tail, dim3(1), dim3(ACCEL_REFIT_TAIL_NODES), 0, stream, accel->nodes, accel->tris, accel->order, t);
  return launch_status("vkr_accel_refit");
}

extern "C" int vkr_accel_refit_schedule(const vkr_accel* accel, uint32_t* level_sizes, uint32_t level_capacity, uint32_t* level_count,
                                        uint32_t* tail_nodes) {
  if (!accel || !level_count) { set_error("vkr_accel_refit_schedule: NULL argument"); return VKR_ERR_NULL; }
  const uint32_t levels = accel->node_count ? (uint32_t)accel->level_begin.size() - 1u : 0u;
  if (levels > level_capacity || (levels && !level_sizes)) { set_error("vkr_accel_refit_schedule: %u levels do not fit into %u", levels, level_capacity); return VKR_ERR_EXTENT; }
  for (uint32_t l = 0; l < levels; l++) level_sizes[l] = accel->level_begin[l + 1] - accel->level_begin[l];
  *level_count = levels;
  if (tail_nodes) *tail_nodes = ACCEL_REFIT_TAIL_NODES;
  return VKR_OK;
}

extern "C" int vkr_accel_refit_layout(vkr_accel_node* nodes, uint32_t node_count, vkr_accel_tri* tris, uint32_t tri_count, const float* tri_vertices) {
  if ((!nodes && node_count) || (!tris && tri_count)) { set_error("vkr_accel_refit_layout: NULL arrays"); return VKR_ERR_NULL; }
  if (!tri_vertices && tri_count) { set_error("vkr_accel_refit_layout: NULL triangles"); return VKR_ERR_NULL; }
  // the topology is checked whole before anything is written
  for (uint32_t i = 0; i < node_count; i++) {
    const uint64_t first = nodes[i].first, count = nodes[i].count;
    if (count == 0) {
      if (first <= i || first + 1 >= node_count) {
        set_error("vkr_accel_refit_layout: node %u: children %llu and %llu are not stored behind it inside the %u nodes", i, (unsigned long long)first,
                  (unsigned long long)first + 1, node_count);
        return VKR_ERR_EXTENT;
      }
    } else if (first + count > tri_count) {
      set_error("vkr_accel_refit_layout: node %u: records [%llu, +%llu) outside the %u records", i, (unsigned long long)first, (unsigned long long)count, tri_count);
      return VKR_ERR_EXTENT;
    }
  }
  for (uint32_t j = 0; j < tri_count; j++)
    if (tris[j].index >= tri_count) {
      set_error("vkr_accel_refit_layout: record %u: input index %u outside the %u triangles", j, tris[j].index, tri_count);
      return VKR_ERR_EXTENT;
    }
  for (uint32_t j = 0; j < tri_count; j++) make_record(tri_vertices + 9 * (size_t)tris[j].index, tris[j].index, tris[j]);
  for (uint32_t i = node_count; i-- > 0;) {  // children lie behind their parent: from the last node to the first
    UnionBox b;
    if (nodes[i].count == 0) {
      for (uint32_t c = nodes[i].first; c < nodes[i].first + 2u; c++) b.take(nodes[c].lo, nodes[c].hi);
    } else {
      for (uint32_t k = 0; k < nodes[i].count; k++) b.take(tris[nodes[i].first + k].lo, tris[nodes[i].first + k].hi);
    }
    for (int k = 0; k < 3; k++) { nodes[i].lo[k] = b.lo[k]; nodes[i].hi[k] = b.hi[k]; }
  }
  return VKR_OK;
}

extern "C" int vkr_accel_download(const vkr_accel* accel, vkr_accel_node* nodes, uint32_t node_capacity, vkr_accel_tri* tris, uint32_t tri_capacity,
                                  void* stream) {
  if (!accel) { set_error("vkr_accel_download: NULL acceleration structure"); return VKR_ERR_NULL; }
  if ((!nodes && accel->node_count) || (!tris && accel->tri_count)) { set_error("vkr_accel_download: NULL output"); return VKR_ERR_NULL; }
  if (accel->node_count > node_capacity || accel->tri_count > tri_capacity) {
    set_error("vkr_accel_download: %u nodes and %u records do not fit into %u and %u", accel->node_count, accel->tri_count, node_capacity, tri_capacity);
    return VKR_ERR_EXTENT;
  }
  hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  if (e == hipSuccess && accel->node_count) e = hipMemcpy(nodes, accel->nodes, accel->node_count * sizeof(vkr_accel_node), hipMemcpyDeviceToHost);
  if (e == hipSuccess && accel->tri_count) e = hipMemcpy(tris, accel->tris, accel->tri_count * sizeof(vkr_accel_tri), hipMemcpyDeviceToHost);
  if (e != hipSuccess) { set_error("vkr_accel_download: %s", hipGetErrorString(e)); return (int)e; }
  return VKR_OK;
}

extern "C" uint64_t vkr_scene_triangles_scratch_bytes(uint32_t draw_count) { return scene_triangles_scratch(draw_count); }

extern "C" int vkr_scene_triangles(const vkr_raster_scene* scene, float* out_tri_vertices, uint64_t out_tri_capacity, void* scratch, uint64_t scratch_bytes,
                                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SceneTriArgs a;
  bool launch = false;
  VKR_TRY(scene_triangles_args("scene_triangles", scene, out_tri_vertices, out_tri_capacity, scratch, scratch_bytes, false, stream, &a, &launch));
  if (!launch) return VKR_OK;
  hipLaunchKernelGGL(k_scene_triangles, dim3((a.total + 255) / 256), dim3(256), 0, stream, a);
  return launch_status("scene_triangles");
}
