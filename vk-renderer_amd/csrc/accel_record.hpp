// accel_record.hpp — the rule that turns vertices into the bytes of the ray-query structure, written once for the host builder
// (accel.hip: layout), the host refit (accel_refit.hip: vkr_accel_refit_layout) and the device refit (accel_refit.hip: the
// kernels): a triangle's record, the union of boxes, and the order in which node boxes can be recomputed bottom-up.
//
// Nothing here multiplies and then adds, so no fused multiply-add can be formed under either numeric contract (and the build
// never contracts on its own): the margin is an add followed by a multiply by a power of two, the edges are differences, the box
// bounds a minimum / maximum and one subtraction / addition.  Host and device therefore compute the same bits
// (DESIGN_NUMERICS.md, "Ray query: refit").
#ifndef VKR_ACCEL_RECORD_HPP
#define VKR_ACCEL_RECORD_HPP

#include <vector>

#include "accel_traverse.hpp"

namespace vkr {

#define VKR_HD __host__ __device__ __forceinline__

// std::min / std::max as the builder always used them: `b < a ? b : a` and `a < b ? b : a`.  A NaN second argument is never
// taken and a NaN first one stays, so an accumulator that starts finite or infinite never becomes NaN.
VKR_HD float keep_min(float a, float b) { return b < a ? b : a; }
VKR_HD float keep_max(float a, float b) { return a < b ? b : a; }

// v: 9 floats of one triangle -> its record (everything the device test reads)
VKR_HD void make_record(const float* v, uint32_t index, vkr_accel_tri& r) {
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < 9; k++) s = keep_max(s, fabsf(v[k]));
  const float margin = (s + 1.0f) * 0x1p-12f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    r.v0[k] = v[k];
    r.e1[k] = v[3 + k] - v[k];
    r.e2[k] = v[6 + k] - v[k];
    r.lo[k] = keep_min(keep_min(v[k], v[3 + k]), v[6 + k]) - margin;
    r.hi[k] = keep_max(keep_max(v[k], v[3 + k]), v[6 + k]) + margin;
  }
  r.index = index;
}

// A box under construction: starts empty (+inf, -inf), takes boxes with keep_min / keep_max (a NaN bound never enters)
struct UnionBox {
  float lo[3], hi[3];
  VKR_HD UnionBox() : lo {INFINITY, INFINITY, INFINITY}, hi {-INFINITY, -INFINITY, -INFINITY} {}
  VKR_HD void take(const float* blo, const float* bhi) {
#pragma unroll
    for (int k = 0; k < 3; k++) { lo[k] = keep_min(lo[k], blo[k]); hi[k] = keep_max(hi[k], bhi[k]); }
  }
};

// ---- the refit schedule (host, computed once at vkr_accel_create) ---------------------------------------------------------------
// height of a node: 0 for a leaf, 1 + the larger height of its two children otherwise.  A node's box depends only on boxes of
// smaller height, so all nodes of one height can be recomputed at once.  order: the node ids sorted by (height, id);
// level_begin[h] .. level_begin[h + 1]: the nodes of height h in `order`.  Level sizes never grow with the height (every node of
// height h + 1 owns a child of height h, and no two nodes share a child).  Children are stored behind their parent, so one
// pass from the last node to the first sees every child before its parent.
inline void refit_schedule(const std::vector<vkr_accel_node>& nodes, std::vector<uint32_t>* order, std::vector<uint32_t>* level_begin) {
  const size_t n = nodes.size();
  std::vector<uint32_t> height(n, 0u);
  uint32_t top = 0;
  for (size_t i = n; i-- > 0;) {
    if (nodes[i].count == 0u) {
      const uint32_t a = height[nodes[i].first], b = height[nodes[i].first + 1u];
      height[i] = 1u + (a > b ? a : b);
    }
    if (height[i] > top) top = height[i];
  }
  level_begin->assign(n ? top + 2u : 1u, 0u);
  for (size_t i = 0; i < n; i++) (*level_begin)[height[i] + 1u]++;
  for (size_t h = 1; h < level_begin->size(); h++) (*level_begin)[h] += (*level_begin)[h - 1];
  order->resize(n);
  std::vector<uint32_t> at(level_begin->begin(), level_begin->end());
  for (size_t i = 0; i < n; i++) (*order)[at[height[i]]++] = (uint32_t)i;
}

}  // namespace vkr

#endif
