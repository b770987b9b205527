// accel_traverse.hpp — the device side of the ray query, shared by accel.hip (vkr_accel_query, vkr_accel_occluded,
// gtao_rt_main) and shadow_mask_rt.hip: the view of the structure, the frozen triangle test and the two wave-wide walks.
//
// wave_any_hit culls a node when the box of the whole segment misses the node box: exact and cheap for the 0.2-long rays of
// gtao_rt_main.  wave_any_hit_ray is the walk for long rays (a shadow ray runs from the surface to the light; the box of a
// diagonal segment covers much of the scene): the same descent, stack, ballot and lane retirement, with a per-ray slab test
// ANDed to the segment-box term.  Both give the answer of the frozen test looped over all triangles (DESIGN_NUMERICS.md,
// "Ray query" and "Ray query, the per-ray cull").  wave_closest_hit (accel_closest.hip, reflections_rt.hip) is the third walk:
// where, on which triangle and at which barycentrics the ray hits first ("Ray query, closest hit").
#ifndef VKR_ACCEL_TRAVERSE_HPP
#define VKR_ACCEL_TRAVERSE_HPP

#include "vkr_device.hpp"

struct vkr_accel {
  vkr_accel_node* nodes;  // device
  vkr_accel_tri* tris;    // device
  uint32_t node_count, tri_count;
};

namespace vkr {

// the traversal stack holds one entry per level below the root; the build makes a leaf at this depth whatever it holds
constexpr int ACCEL_MAX_DEPTH = 48;
constexpr int ACCEL_STACK = 64;

struct AccelView {
  const vkr_accel_node* nodes;
  const vkr_accel_tri* tris;
  uint32_t node_count;
};

// ---- the frozen fp32 triangle test (DESIGN_NUMERICS.md) ----------------------------------------------------------------
// Moller-Trumbore in this operation order, every product and sum rounded on its own (no fused multiply-add under either
// numeric contract); det == 0 is a miss, the edges are inclusive, tmin <= t <= tmax, and the point o + t * d (mul, then add)
// must lie in the triangle's widened box.  NaN anywhere makes a comparison false: a miss.
VKR_DEV bool ray_hits_triangle(f3 o, f3 d, float tmin, float tmax, const vkr_accel_tri& tr) {
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
  return hx >= tr.lo[0] && hx <= tr.hi[0] && hy >= tr.lo[1] && hy <= tr.hi[1] && hz >= tr.lo[2] && hz <= tr.hi[2];
}

// Any-hit of this lane's segment o + t * d, t in [tmin, tmax].  Every lane of the wave calls it (the walk is wave-uniform);
// `live` false: the lane has no ray and only follows.  `stack`: ACCEL_STACK words of LDS owned by this wave.
VKR_DEV bool wave_any_hit(const AccelView& a, f3 o, f3 d, float tmin, float tmax, bool live, uint32_t* stack) {
  const float ax = o.x + tmin * d.x, ay = o.y + tmin * d.y, az = o.z + tmin * d.z;
  const float bx = o.x + tmax * d.x, by = o.y + tmax * d.y, bz = o.z + tmax * d.z;
  const float lox = fminf(ax, bx), loy = fminf(ay, by), loz = fminf(az, bz);
  const float hix = fmaxf(ax, bx), hiy = fmaxf(ay, by), hiz = fmaxf(az, bz);
  bool pending = live, hit = false;
  if (a.node_count == 0) return false;
  uint32_t node = 0;
  int sp = 0;
  for (;;) {
    const vkr_accel_node nd = a.nodes[node];
    const bool overlap = pending && lox <= nd.hi[0] && hix >= nd.lo[0] && loy <= nd.hi[1] && hiy >= nd.lo[1] &&
                         loz <= nd.hi[2] && hiz >= nd.lo[2];
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
        if (test && ray_hits_triangle(o, d, tmin, tmax, tr)) { hit = true; pending = false; test = false; }
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

// ---- the per-ray cull of wave_any_hit_ray (DESIGN_NUMERICS.md, "Ray query, the per-ray cull") ------------------------------
// One axis of the slab test: the reciprocal of the direction component, or NaN where the component is zero, denormal-small,
// huge, infinite or NaN.  A NaN reciprocal makes both slab parameters of the axis NaN, and slab_keep() never takes a NaN:
// the axis then constrains nothing and the segment-box term alone decides.  Inside [2^-100, 2^100] the reciprocal is a normal
// number with one rounding: no 0 * inf, no overflowed or denormal quotient.
VKR_DEV float slab_reciprocal(float d) {
  const float m = fabsf(d);
  return (m >= 0x1p-100f && m <= 0x1p100f) ? 1.0f / d : __uint_as_float(0x7FC00000u);
}
// running maximum / minimum that never take a NaN candidate (the comparison with a NaN is false) and keep a NaN they hold
VKR_DEV float slab_keep_max(float acc, float x) { return x > acc ? x : acc; }
VKR_DEV float slab_keep_min(float acc, float x) { return x < acc ? x : acc; }

// wave_any_hit for long rays: the same walk, the same answer.  A node is visited by a lane when its segment box overlaps the
// node box (the proven term of wave_any_hit) AND the slab interval of the ray against the node box, widened by `margin` and
// rounded outward, meets [tmin, tmax].  Written so that the cull only ever REJECTS on a comparison that is true: every NaN
// accepts the node.
VKR_DEV bool wave_any_hit_ray(const AccelView& a, f3 o, f3 d, float tmin, float tmax, bool live, uint32_t* stack) {
  const float ax = o.x + tmin * d.x, ay = o.y + tmin * d.y, az = o.z + tmin * d.z;
  const float bx = o.x + tmax * d.x, by = o.y + tmax * d.y, bz = o.z + tmax * d.z;
  const float lox = fminf(ax, bx), loy = fminf(ay, by), loz = fminf(az, bz);
  const float hix = fmaxf(ax, bx), hiy = fmaxf(ay, by), hiz = fmaxf(az, bz);
  // once per ray: the sum of the nine magnitudes bounds every coordinate met along the segment (a sum, not a maximum: an
  // infinity or a NaN in any of them reaches the margin and switches the slab term off); margin = sum * 2^-21 + 2^-126
  const float reach = (((fabsf(o.x) + fabsf(o.y)) + (fabsf(o.z) + fabsf(ax))) + ((fabsf(ay) + fabsf(az)) + (fabsf(bx) + fabsf(by)))) + fabsf(bz);
  const float margin = reach * 0x1p-21f + 0x1p-126f;
  const float ix = slab_reciprocal(d.x), iy = slab_reciprocal(d.y), iz = slab_reciprocal(d.z);
  // the box side the ray enters through, per axis, is lo for a positive component; the margin pushes it outward
  const bool px = ix > 0.0f, py = iy > 0.0f, pz = iz > 0.0f;
  const float mx = px ? margin : -margin, my = py ? margin : -margin, mz = pz ? margin : -margin;
  bool pending = live, hit = false;
  if (a.node_count == 0) return false;
  uint32_t node = 0;
  int sp = 0;
  for (;;) {
    const vkr_accel_node nd = a.nodes[node];
    bool overlap = pending && lox <= nd.hi[0] && hix >= nd.lo[0] && loy <= nd.hi[1] && hiy >= nd.lo[1] &&
                   loz <= nd.hi[2] && hiz >= nd.lo[2];
    {
      const float nx = (((px ? nd.lo[0] : nd.hi[0]) - o.x) - mx) * ix, fx = (((px ? nd.hi[0] : nd.lo[0]) - o.x) + mx) * ix;
      const float ny = (((py ? nd.lo[1] : nd.hi[1]) - o.y) - my) * iy, fy = (((py ? nd.hi[1] : nd.lo[1]) - o.y) + my) * iy;
      const float nz = (((pz ? nd.lo[2] : nd.hi[2]) - o.z) - mz) * iz, fz = (((pz ? nd.hi[2] : nd.lo[2]) - o.z) + mz) * iz;
      float tn = slab_keep_max(slab_keep_max(slab_keep_max(tmin, nx), ny), nz);
      float tf = slab_keep_min(slab_keep_min(slab_keep_min(tmax, fx), fy), fz);
      tn = tn - (fabsf(tn) * 0x1p-20f + 0x1p-126f);  // outward: the near side down, the far side up (inf - inf = NaN accepts)
      tf = tf + (fabsf(tf) * 0x1p-20f + 0x1p-126f);
      if (tn > tf) overlap = false;
    }
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
        if (test && ray_hits_triangle(o, d, tmin, tmax, tr)) { hit = true; pending = false; test = false; }
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

// ---- closest hit (DESIGN_NUMERICS.md, "Ray query, closest hit") -------------------------------------------------------------
// ray_hits_triangle that also hands back what it computed: the same arithmetic in the same order, so a triangle is accepted
// here exactly when it is accepted there, and t, u, v are the values the frozen sequence rounds to.
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

// Closest hit of this lane's segment: of all triangles the frozen test accepts in [tmin, tmax] the one with the smallest t, of
// equal t (==) the one with the smallest input index; *hit is (0, 0, 0, 0xFFFFFFFF) where there is none.  The descent, stack,
// ballots and lane following are wave_any_hit_ray's.  A lane never retires: it keeps its best candidate and tests a triangle
// against [tmin, t_best] (inclusive, so that a triangle of equal t and lower index stays reachable); the slab term of the cull
// starts its far bound at t_best, the segment box and the margin stay those of [tmin, tmax].  The walk ends when the stack is
// empty.  Since the winner is defined by (t, index) alone, the answer does not depend on the order in which nodes are visited.
// NEAR_FIRST: at an interior node the child that more lanes enter is visited first (t_best shrinks earlier).
template <bool NEAR_FIRST>
VKR_DEV void wave_closest_hit_walk(const AccelView& a, f3 o, f3 d, float tmin, float tmax, bool live, uint32_t* stack, vkr_accel_hit* hit) {
  const float ax = o.x + tmin * d.x, ay = o.y + tmin * d.y, az = o.z + tmin * d.z;
  const float bx = o.x + tmax * d.x, by = o.y + tmax * d.y, bz = o.z + tmax * d.z;
  const float lox = fminf(ax, bx), loy = fminf(ay, by), loz = fminf(az, bz);
  const float hix = fmaxf(ax, bx), hiy = fmaxf(ay, by), hiz = fmaxf(az, bz);
  const float reach = (((fabsf(o.x) + fabsf(o.y)) + (fabsf(o.z) + fabsf(ax))) + ((fabsf(ay) + fabsf(az)) + (fabsf(bx) + fabsf(by)))) + fabsf(bz);
  const float margin = reach * 0x1p-21f + 0x1p-126f;
  const float ix = slab_reciprocal(d.x), iy = slab_reciprocal(d.y), iz = slab_reciprocal(d.z);
  const bool px = ix > 0.0f, py = iy > 0.0f, pz = iz > 0.0f;
  const float mx = px ? margin : -margin, my = py ? margin : -margin, mz = pz ? margin : -margin;
  float t_best = tmax, u_best = 0.0f, v_best = 0.0f;
  uint32_t index_best = 0xFFFFFFFFu;
  // the node test of wave_any_hit_ray with t_best as the far end of the parameter range
  auto enters = [&](const vkr_accel_node& nd) {
    bool overlap = live && lox <= nd.hi[0] && hix >= nd.lo[0] && loy <= nd.hi[1] && hiy >= nd.lo[1] && loz <= nd.hi[2] && hiz >= nd.lo[2];
    const float nx = (((px ? nd.lo[0] : nd.hi[0]) - o.x) - mx) * ix, fx = (((px ? nd.hi[0] : nd.lo[0]) - o.x) + mx) * ix;
    const float ny = (((py ? nd.lo[1] : nd.hi[1]) - o.y) - my) * iy, fy = (((py ? nd.hi[1] : nd.lo[1]) - o.y) + my) * iy;
    const float nz = (((pz ? nd.lo[2] : nd.hi[2]) - o.z) - mz) * iz, fz = (((pz ? nd.hi[2] : nd.lo[2]) - o.z) + mz) * iz;
    float tn = slab_keep_max(slab_keep_max(slab_keep_max(tmin, nx), ny), nz);
    float tf = slab_keep_min(slab_keep_min(slab_keep_min(t_best, fx), fy), fz);
    tn = tn - (fabsf(tn) * 0x1p-20f + 0x1p-126f);
    tf = tf + (fabsf(tf) * 0x1p-20f + 0x1p-126f);
    if (tn > tf) overlap = false;
    return overlap;
  };
  if (a.node_count != 0) {
    uint32_t node = 0;
    int sp = 0;
    for (;;) {
      const vkr_accel_node nd = a.nodes[node];
      const bool overlap = enters(nd);
      if (__ballot(overlap) != 0ull) {
        if (nd.count == 0u) {  // interior: one child waits, the other is next
          uint32_t swap = 0u;
          if (NEAR_FIRST) {
            const vkr_accel_node c0 = a.nodes[nd.first], c1 = a.nodes[nd.first + 1u];
            swap = __popcll(__ballot(enters(c1))) > __popcll(__ballot(enters(c0))) ? 1u : 0u;
          }
          stack[sp] = nd.first + (1u - swap);
          sp++;
          node = nd.first + swap;
          continue;
        }
        for (uint32_t k = 0; k < nd.count; k++) {
          const vkr_accel_tri tr = a.tris[nd.first + k];
          float t, u, v;
          if (overlap && ray_triangle_closest(o, d, tmin, t_best, tr, &t, &u, &v) && (t < t_best || (t == t_best && tr.index < index_best))) {
            t_best = t; u_best = u; v_best = v; index_best = tr.index;
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

}  // namespace vkr

#endif
