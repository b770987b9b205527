// accel_traverse.hpp — the ray query against the scene's structure: the view of the structure, the frozen triangle test, the
// set-up and node test of a lane's ray, the candidate filter, the any-hit descent, the closest-hit walk, and what the ray-level
// entries share (the kernel's preamble and the host's refusals).  Every walk gives the answer of the frozen test looped over all
// triangles (DESIGN_NUMERICS.md, "Ray query", "Ray query, the per-ray cull", "Ray query, closest hit" and "Ray query, cutouts").
#ifndef VKR_ACCEL_TRAVERSE_HPP
#define VKR_ACCEL_TRAVERSE_HPP

#include <vector>

#include "vkr_host.hpp"

struct vkr_accel {
  vkr_accel_node* nodes;  // device
  vkr_accel_tri* tris;    // device
  uint32_t node_count, tri_count;
  // the refit schedule (accel_record.hpp: refit_schedule), made by vkr_accel_create and read by vkr_accel_refit alone
  uint32_t* order = nullptr;          // device, node_count ids sorted by (height, id)
  std::vector<uint32_t> level_begin;  // host: the nodes of height h are order[level_begin[h] .. level_begin[h + 1])
};

namespace vkr {

// the traversal stack holds one entry per level below the root; the build makes a leaf at this depth whatever it holds
constexpr int ACCEL_MAX_DEPTH = 48;
constexpr int ACCEL_STACK = 64;

struct AccelView { const vkr_accel_node* nodes; const vkr_accel_tri* tris; uint32_t node_count; };
inline AccelView view_of(const vkr_accel* accel) { return AccelView{accel->nodes, accel->tris, accel->node_count}; }

// ---- the frozen fp32 triangle test (DESIGN_NUMERICS.md) ----------------------------------------------------------------
// Moller-Trumbore in this operation order, every product and sum rounded on its own (no fused multiply-add under either
// numeric contract); det == 0 is a miss, the edges are inclusive, tmin <= t <= tmax, and the point o + t * d (mul, then add)
// must lie in the triangle's widened box.  NaN anywhere makes a comparison false: a miss.  On a hit t, u, v are the values
// the sequence rounds to.
VKR_DEV bool ray_triangle_closest(f3 o, f3 d, float tmin, float tmax, const vkr_accel_tri& tr, float* t_out, float* u_out, float* v_out) {
  const float e1x = tr.e1[0], e1y = tr.e1[1], e1z = tr.e1[2];
  const float e2x = tr.e2[0], e2y = tr.e2[1], e2z = tr.e2[2];
  const float px = d.y * e2z - d.z * e2y, py = d.z * e2x - d.x * e2z, pz = d.x * e2y - d.y * e2x;
  const float det = (e1x * px + e1y * py) + e1z * pz;
  if (det == 0.0f) return false;
  const float inv = 1.0f / det;
  const float tx = o.x - tr.v0[0], ty = o.y - tr.v0[1], tz = o.z - tr.v0[2];
  const float u = ((tx * px + ty * py) + tz * pz) * inv;
  const float qx = ty * e1z - tz * e1y, qy = tz * e1x - tx * e1z, qz = tx * e1y - ty * e1x;
  const float v = ((d.x * qx + d.y * qy) + d.z * qz) * inv;
  const float t = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
  if (!(u >= 0.0f && v >= 0.0f && u + v <= 1.0f && t >= tmin && t <= tmax)) return false;
  const float hx = o.x + t * d.x, hy = o.y + t * d.y, hz = o.z + t * d.z;
  if (!(hx >= tr.lo[0] && hx <= tr.hi[0] && hy >= tr.lo[1] && hy <= tr.hi[1] && hz >= tr.lo[2] && hz <= tr.hi[2])) return false;
  *t_out = t; *u_out = u; *v_out = v;
  return true;
}
// the any-hit form: whether, not where
VKR_DEV bool ray_hits_triangle(f3 o, f3 d, float tmin, float tmax, const vkr_accel_tri& tr) {
  float t, u, v;
  return ray_triangle_closest(o, d, tmin, tmax, tr, &t, &u, &v);
}

// ---- a lane's ray against a node box -----------------------------------------------------------------------------------------
// One axis of the slab term: the reciprocal of the direction component, or NaN where the component is zero, denormal-small,
// huge, infinite or NaN.  A NaN reciprocal makes both slab parameters of the axis NaN, and slab_keep_*() never take a NaN:
// the axis then constrains nothing and the segment-box term alone decides.  Inside [2^-100, 2^100] the reciprocal is a normal
// number with one rounding: no 0 * inf, no overflowed or denormal quotient.
VKR_DEV float slab_reciprocal(float d) {
  const float m = fabsf(d);
  return (m >= 0x1p-100f && m <= 0x1p100f) ? 1.0f / d : __uint_as_float(0x7FC00000u);
}
// running maximum / minimum that never take a NaN candidate (the comparison with a NaN is false) and keep a NaN they hold
VKR_DEV float slab_keep_max(float acc, float x) { return x > acc ? x : acc; }
VKR_DEV float slab_keep_min(float acc, float x) { return x < acc ? x : acc; }

// What a lane keeps of its segment o + t * d, t in [tmin, tmax], to decide whether it enters a node.
//
// The segment-box term: the box spanned by o + tmin * d and o + tmax * d, computed as the triangle test computes its hit point
// (mul, then add: rounding is monotonic, so every such point of t in [tmin, tmax] lies between them).  Node boxes are exact
// unions of the triangles' widened boxes, so a node box that contains a hit point always overlaps the segment box: the term
// cannot discard a triangle the test would hit.  It is exact and cheap for short rays (the 0.2-long rays of gtao_rt_main).
//
// SLAB adds the per-ray term for long rays (a shadow ray runs from the surface to the light; the box of a diagonal segment
// covers much of the scene): the slab interval of the ray against the node box, widened by `margin` and rounded outward, must
// meet [tmin, t_far].  It only ever REJECTS on a comparison that is true, so every NaN accepts the node.  Without SLAB the
// struct is the six floats of the segment box.
template <bool SLAB>
struct LaneRay {
  float lox, loy, loz, hix, hiy, hiz;
  f3 o;
  float tmin, ix, iy, iz, mx, my, mz;
  bool px, py, pz;

  VKR_DEV LaneRay(f3 o_, f3 d, float tmin_, float tmax) {
    const float ax = o_.x + tmin_ * d.x, ay = o_.y + tmin_ * d.y, az = o_.z + tmin_ * d.z;
    const float bx = o_.x + tmax * d.x, by = o_.y + tmax * d.y, bz = o_.z + tmax * d.z;
    lox = fminf(ax, bx); loy = fminf(ay, by); loz = fminf(az, bz);
    hix = fmaxf(ax, bx); hiy = fmaxf(ay, by); hiz = fmaxf(az, bz);
    if constexpr (SLAB) {
      o = o_;
      tmin = tmin_;
      // once per ray: the sum of the nine magnitudes bounds every coordinate met along the segment (a sum, not a maximum: an
      // infinity or a NaN in any of them reaches the margin and switches the slab term off); margin = sum * 2^-21 + 2^-126
      const float reach = (((fabsf(o.x) + fabsf(o.y)) + (fabsf(o.z) + fabsf(ax))) + ((fabsf(ay) + fabsf(az)) + (fabsf(bx) + fabsf(by)))) + fabsf(bz);
      const float margin = reach * 0x1p-21f + 0x1p-126f;
      ix = slab_reciprocal(d.x); iy = slab_reciprocal(d.y); iz = slab_reciprocal(d.z);
      // the box side the ray enters through, per axis, is lo for a positive component; the margin pushes it outward
      px = ix > 0.0f; py = iy > 0.0f; pz = iz > 0.0f;
      mx = px ? margin : -margin; my = py ? margin : -margin; mz = pz ? margin : -margin;
    }
  }

  // `live` false: the lane enters nothing.  t_far: the far end of the slab term's range (tmax, or a closer hit already found);
  // the segment box and the margin stay those of [tmin, tmax].  The early return changes no answer: it keeps the code of the
  // short-ray walk what its pinned registers were measured with (a branch round the node's loads), while with the slab term the
  // test stays straight-line (a branch there cost vkr_accel_occluded 1.6 %: DESIGN.md 7.9, the fold).
  VKR_DEV bool enters(const vkr_accel_node nd, bool live, float t_far) const {
    if constexpr (!SLAB) { if (!live) return false; }
    bool overlap = live && lox <= nd.hi[0] && hix >= nd.lo[0] && loy <= nd.hi[1] && hiy >= nd.lo[1] && loz <= nd.hi[2] && hiz >= nd.lo[2];
    if constexpr (SLAB) {
      const float nx = (((px ? nd.lo[0] : nd.hi[0]) - o.x) - mx) * ix, fx = (((px ? nd.hi[0] : nd.lo[0]) - o.x) + mx) * ix;
      const float ny = (((py ? nd.lo[1] : nd.hi[1]) - o.y) - my) * iy, fy = (((py ? nd.hi[1] : nd.lo[1]) - o.y) + my) * iy;
      const float nz = (((pz ? nd.lo[2] : nd.hi[2]) - o.z) - mz) * iz, fz = (((pz ? nd.hi[2] : nd.lo[2]) - o.z) + mz) * iz;
      float tn = slab_keep_max(slab_keep_max(slab_keep_max(tmin, nx), ny), nz);
      float tf = slab_keep_min(slab_keep_min(slab_keep_min(t_far, fx), fy), fz);
      tn = tn - (fabsf(tn) * 0x1p-20f + 0x1p-126f);  // outward: the near side down, the far side up (inf - inf = NaN accepts)
      tf = tf + (fabsf(tf) * 0x1p-20f + 0x1p-126f);
      if (tn > tf) overlap = false;
    }
    return overlap;
  }
};

// ---- the candidate filter ----------------------------------------------------------------------------------------------------
// A walk asks its filter whether a candidate — a triangle the frozen test accepts for the lane's ray at (u, v) — is really
// there.  keep(index, u, v, cand) is called by the whole wave with the wave-uniform input index of the leaf slot; cand: this lane
// has the candidate; it returns cand, or false where the filter removes it.  The default accepts everything and is never called:
// the walks without a filter are the code they were before there was one.  ray_cutout.hpp has the filter of alpha cutouts.
struct AcceptAll {
  static constexpr bool ALL = true;
  VKR_DEV bool keep(uint32_t, float, float, bool cand) const { return cand; }
};

// ---- any hit ---------------------------------------------------------------------------------------------------------------
// Any-hit of this lane's segment.  Every lane of the wave calls it: node and triangle addresses are wave-uniform, the wave
// descends when any pending lane enters the node (a ballot), a lane retires on its first hit and the wave leaves when every
// lane has hit or the stack is empty.  `live` false: the lane has no ray and only follows.  `stack`: ACCEL_STACK words of LDS
// owned by this wave.  With a filter a lane retires only on a candidate the filter keeps, and goes on through the rest of the
// leaf and of the tree otherwise.
template <bool SLAB, class Filter = AcceptAll>
VKR_DEV bool wave_any_hit_walk(const AccelView& a, f3 o, f3 d, float tmin, float tmax, bool live, uint32_t* stack, const Filter& filter = Filter()) {
  const LaneRay<SLAB> ray(o, d, tmin, tmax);
  bool pending = live, hit = false;
  if (a.node_count == 0) return false;
  uint32_t node = 0;
  int sp = 0;
  for (;;) {
    const vkr_accel_node nd = a.nodes[node];
    const bool overlap = ray.enters(nd, pending, tmax);
    if (__ballot(overlap) != 0ull) {
      if (nd.count == 0u) {  // interior: the second child waits, the first is next
        stack[sp] = nd.first + 1u;
        sp++;
        node = nd.first;
        continue;
      }
      bool test = overlap;
      for (uint32_t k = 0; k < nd.count; k++) {
        const vkr_accel_tri tr = a.tris[nd.first + k];
        if constexpr (Filter::ALL) {
          if (test && ray_hits_triangle(o, d, tmin, tmax, tr)) { hit = true; pending = false; test = false; }
        } else {
          float t = 0.0f, u = 0.0f, v = 0.0f;
          const bool cand = test && ray_triangle_closest(o, d, tmin, tmax, tr, &t, &u, &v);
          if (filter.keep(tr.index, u, v, cand)) { hit = true; pending = false; test = false; }
        }
        if (__ballot(test) == 0ull) break;
      }
      if (__ballot(pending) == 0ull) break;
    }
    if (sp == 0) break;
    sp--;
    node = __builtin_amdgcn_readfirstlane(stack[sp]);
  }
  return hit;
}
// the walk for short rays (the segment box alone) and the walk for long rays (the segment box AND the slab term)
VKR_DEV bool wave_any_hit(const AccelView& a, f3 o, f3 d, float tmin, float tmax, bool live, uint32_t* stack) {
  return wave_any_hit_walk<false>(a, o, d, tmin, tmax, live, stack);
}
VKR_DEV bool wave_any_hit_ray(const AccelView& a, f3 o, f3 d, float tmin, float tmax, bool live, uint32_t* stack) {
  return wave_any_hit_walk<true>(a, o, d, tmin, tmax, live, stack);
}

// ---- closest hit -----------------------------------------------------------------------------------------------------------
// Closest hit of this lane's segment: of all triangles the frozen test accepts in [tmin, tmax] the one with the smallest t, of
// equal t (==) the one with the smallest input index; *hit is (0, 0, 0, 0xFFFFFFFF) where there is none.  The wave descends as
// in the any-hit walk, but a lane never retires: it keeps its best candidate, tests a triangle against [tmin, t_best]
// (inclusive, so that a triangle of equal t and lower index stays reachable) and enters a node with t_best as t_far.  The walk
// ends when the stack is empty.  Since the winner is defined by (t, index) alone, the answer does not depend on the order in
// which nodes are visited.  NEAR_FIRST: at an interior node the child that more lanes enter is visited first (t_best shrinks
// earlier).  With a filter only a candidate the filter keeps becomes the best one (a removed candidate never shrinks the far
// bound); the filter is asked after the (t, index) compare, so a candidate that cannot win costs no fetch.
template <bool NEAR_FIRST, class Filter = AcceptAll>
VKR_DEV void wave_closest_hit_walk(const AccelView& a, f3 o, f3 d, float tmin, float tmax, bool live, uint32_t* stack, vkr_accel_hit* hit,
                                   const Filter& filter = Filter()) {
  const LaneRay<true> ray(o, d, tmin, tmax);
  float t_best = tmax, u_best = 0.0f, v_best = 0.0f;
  uint32_t index_best = 0xFFFFFFFFu;
  if (a.node_count != 0) {
    uint32_t node = 0;
    int sp = 0;
    for (;;) {
      const vkr_accel_node nd = a.nodes[node];
      const bool overlap = ray.enters(nd, live, t_best);
      if (__ballot(overlap) != 0ull) {
        if (nd.count == 0u) {  // interior: one child waits, the other is next
          uint32_t swap = 0u;
          if (NEAR_FIRST) {
            const vkr_accel_node c0 = a.nodes[nd.first], c1 = a.nodes[nd.first + 1u];
            swap = __popcll(__ballot(ray.enters(c1, live, t_best))) > __popcll(__ballot(ray.enters(c0, live, t_best))) ? 1u : 0u;
          }
          stack[sp] = nd.first + (1u - swap);
          sp++;
          node = nd.first + swap;
          continue;
        }
        for (uint32_t k = 0; k < nd.count; k++) {
          const vkr_accel_tri tr = a.tris[nd.first + k];
          if constexpr (Filter::ALL) {
            float t, u, v;
            if (overlap && ray_triangle_closest(o, d, tmin, t_best, tr, &t, &u, &v) && (t < t_best || (t == t_best && tr.index < index_best))) {
              t_best = t; u_best = u; v_best = v; index_best = tr.index;
            }
          } else {
            float t = 0.0f, u = 0.0f, v = 0.0f;
            const bool cand = overlap && ray_triangle_closest(o, d, tmin, t_best, tr, &t, &u, &v) && (t < t_best || (t == t_best && tr.index < index_best));
            if (filter.keep(tr.index, u, v, cand)) { t_best = t; u_best = u; v_best = v; index_best = tr.index; }
          }
        }
      }
      if (sp == 0) break;
      sp--;
      node = __builtin_amdgcn_readfirstlane(stack[sp]);
    }
  }
  const bool found = index_best != 0xFFFFFFFFu;
  hit->t = found ? t_best : 0.0f;
  hit->u = u_best;
  hit->v = v_best;
  hit->index = index_best;
}
VKR_DEV void wave_closest_hit(const AccelView& a, f3 o, f3 d, float tmin, float tmax, bool live, uint32_t* stack, vkr_accel_hit* hit) {
  wave_closest_hit_walk<false>(a, o, d, tmin, tmax, live, stack, hit);
}
// the walk with the children ordered by the lanes that enter them (measured against the plain one: DESIGN.md 7.9)
VKR_DEV void wave_closest_hit_ordered(const AccelView& a, f3 o, f3 d, float tmin, float tmax, bool live, uint32_t* stack, vkr_accel_hit* hit) {
  wave_closest_hit_walk<true>(a, o, d, tmin, tmax, live, stack, hit);
}

// ---- the ray-level entries (vkr_accel_query, vkr_accel_occluded, vkr_accel_closest) -------------------------------------------
// A wave holds 64 consecutive rays and a block of 256 four waves, with one stack each in the kernel's LDS.  Lane i of the grid
// has ray i; past n it has none and follows its wave with a zero ray.
struct RayLane { uint32_t i; bool live; f3 o, d; uint32_t* stack; };
VKR_DEV RayLane load_ray_lane(const float* org, const float* dir, uint32_t n, uint32_t (*stacks)[ACCEL_STACK]) {
  RayLane r;
  r.i = blockIdx.x * 256u + threadIdx.x;
  r.live = r.i < n;
  r.o = mk3(0.0f, 0.0f, 0.0f);
  r.d = mk3(0.0f, 0.0f, 0.0f);
  if (r.live) {
    r.o = mk3(org[3 * r.i], org[3 * r.i + 1], org[3 * r.i + 2]);
    r.d = mk3(dir[3 * r.i], dir[3 * r.i + 1], dir[3 * r.i + 2]);
  }
  r.stack = stacks[threadIdx.x >> 6];
  return r;
}

// What the three entries refuse alike, under the entry's own prefix.  No rays is not an error whatever the pointers are: the
// caller returns VKR_OK for n == 0 right after this.
inline int check_ray_batch(const char* entry, const vkr_accel* accel, const float* origins, const float* dirs, const void* out, uint32_t n) {
  if (!accel) { set_error("%s: NULL acceleration structure", entry); return VKR_ERR_NULL; }
  if (n == 0) return VKR_OK;
  if (!origins || !dirs || !out) { set_error("%s: NULL rays or output", entry); return VKR_ERR_NULL; }
  if (n > (1u << 30)) { set_error("%s: %u rays, at most 2^30 per call", entry, n); return VKR_ERR_EXTENT; }
  return VKR_OK;
}

}  // namespace vkr

#endif
