// raster_common.hpp — what the compute rasterisers share (raster.hip: program "gbuf_opaque_taa", cubemap.hip: program
// "cubemap_probe"): the frozen raster rules — exact 64-bit edge functions of 24.8 coordinates, the top-left fill rule, the
// 8-bit sub-pixel snap, the near-plane clip, D24 depth — the small / large split of the work, and the scene sampler
// (REPEAT, trilinear, sRGB).  One definition, so the two programs cannot drift apart.
#pragma once
#include "vkr_host.hpp"

namespace vkr {

#define RASTER_MAX_TEXTURES 32
#define RASTER_GUARD_PX 1048576.0f  // |screen coordinate| beyond this: the triangle is dropped (documented limit)

// differences of 24.8 coordinates fit 32 bits, their products need 64 (v_mad_i64_i32)
VKR_DEV long long edge_fn(int ax, int ay, int bx, int by, int px, int py) {
  return (long long)(bx - ax) * (long long)(py - ay) - (long long)(by - ay) * (long long)(px - ax);
}
// top-left rule for an edge a->b of a triangle with positive area2 under edge_fn (y down)
VKR_DEV bool is_top_left(int ax, int ay, int bx, int by) {
  const int dx = bx - ax, dy = by - ay;
  return dy < 0 || (dy == 0 && dx > 0);
}

// Sutherland-Hodgman of one triangle against the near plane z_clip >= 0 on vertices of N floats each (every output of the vertex
// shader, clip z at index ZI): in[3] -> poly[4], returns the vertex count (0, 3 or 4; the fan (0, 1, 2), (0, 2, 3) gives the
// sub-triangles).  A crossing is p + t (q - p) of every output, always from the inside vertex p, so both orientations of a shared
// edge agree.  Written as a table over the three inside bits (the walk "emit p_k if inside, emit the crossing of edge k if it
// crosses", unrolled per case) with per-float selects, so the polygon stays in registers: no indexed store.
template <int N, int ZI> VKR_DEV int clip_near(const float (&in)[3][N], float (&poly)[4][N]) {
  const float z0 = in[0][ZI], z1 = in[1][ZI], z2 = in[2][ZI];
  const bool i0 = z0 >= 0.0f, i1 = z1 >= 0.0f, i2 = z2 >= 0.0f;
  const int mask = (i0 ? 1 : 0) | (i1 ? 2 : 0) | (i2 ? 4 : 0);
  // crossing of edge a -> b from its inside end (the value is only used where the edge crosses)
  const float t01 = i0 ? z0 / (z0 - z1) : z1 / (z1 - z0), t12 = i1 ? z1 / (z1 - z2) : z2 / (z2 - z1), t20 = i2 ? z2 / (z2 - z0) : z0 / (z0 - z2);
#pragma unroll
  for (int c = 0; c < N; c++) {
    const float p0 = in[0][c], p1 = in[1][c], p2 = in[2][c];
    const float c01 = i0 ? p0 + t01 * (p1 - p0) : p1 + t01 * (p0 - p1);
    const float c12 = i1 ? p1 + t12 * (p2 - p1) : p2 + t12 * (p1 - p2);
    const float c20 = i2 ? p2 + t20 * (p0 - p2) : p0 + t20 * (p2 - p0);
    // mask: 1: p0 c01 c20   2: c01 p1 c12   4: c12 p2 c20   3: p0 p1 c12 c20   5: p0 c01 c12 p2   6: c01 p1 p2 c20   7: p0 p1 p2
    poly[0][c] = i0 ? p0 : (i1 ? c01 : c12);
    poly[1][c] = (mask == 1 || mask == 5) ? c01 : (mask == 4 ? p2 : p1);
    poly[2][c] = (mask == 1 || mask == 4) ? c20 : (mask >= 6 ? p2 : c12);
    poly[3][c] = mask == 5 ? p2 : c20;
  }
  return mask == 0 ? 0 : ((mask == 3 || mask == 5 || mask == 6) ? 4 : 3);
}

// clip position -> 24.8 window coordinates of a width x height viewport, clip w and z / w; false: behind the eye or beyond the guard band
VKR_DEV bool snap_vertex(f4 p, int width, int height, int* x, int* y, float* w, float* z) {
  if (!(p.w > 0.0f)) return false;
  const float xs = ((p.x / p.w) * 0.5f + 0.5f) * (float)width;
  const float ys = ((p.y / p.w) * 0.5f + 0.5f) * (float)height;
  if (!(fabsf(xs) <= RASTER_GUARD_PX && fabsf(ys) <= RASTER_GUARD_PX)) return false;
  *x = (int)rintf(xs * 256.0f);
  *y = (int)rintf(ys * 256.0f);
  *w = p.w;
  *z = p.z / p.w;
  return true;
}

// coverage + depth of pixel (px, py); lambda: screen-space barycentrics
template <class T> VKR_DEV bool cover(const T& t, int px, int py, float lambda[3], uint32_t* d24) {
  const int X = (px << 8) + 128, Y = (py << 8) + 128;
  const long long e0 = edge_fn(t.x[1], t.y[1], t.x[2], t.y[2], X, Y);
  const long long e1 = edge_fn(t.x[2], t.y[2], t.x[0], t.y[0], X, Y);
  const long long e2 = edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], X, Y);
  if (e0 < 0 || e1 < 0 || e2 < 0) return false;
  if (e0 == 0 && !is_top_left(t.x[1], t.y[1], t.x[2], t.y[2])) return false;
  if (e1 == 0 && !is_top_left(t.x[2], t.y[2], t.x[0], t.y[0])) return false;
  if (e2 == 0 && !is_top_left(t.x[0], t.y[0], t.x[1], t.y[1])) return false;
  const double inv = t.inv_area2;
  lambda[0] = (float)((double)e0 * inv);
  lambda[1] = (float)((double)e1 * inv);
  lambda[2] = (float)((double)e2 * inv);
  const float depth = (lambda[0] * t.z[0] + lambda[1] * t.z[1]) + lambda[2] * t.z[2];
  if (!(depth >= 0.0f && depth <= 1.0f)) return false;  // depth clipping (far plane; near was clipped)
  *d24 = (uint32_t)rintf(depth * 16777215.0f);
  return true;
}
// barycentrics at an arbitrary (possibly uncovered) pixel, for the forward differences of uv
template <class T> VKR_DEV void lambda_at(const T& t, int px, int py, float lambda[3]) {
  const int X = (px << 8) + 128, Y = (py << 8) + 128;
  const double inv = t.inv_area2;
  lambda[0] = (float)((double)edge_fn(t.x[1], t.y[1], t.x[2], t.y[2], X, Y) * inv);
  lambda[1] = (float)((double)edge_fn(t.x[2], t.y[2], t.x[0], t.y[0], X, Y) * inv);
  lambda[2] = (float)((double)edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], X, Y) * inv);
}
template <class T> VKR_DEV void perspective(const T& t, const float lambda[3], float b[3]) {
  const float q0 = lambda[0] / t.w[0], q1 = lambda[1] / t.w[1], q2 = lambda[2] / t.w[2];
  const float s = (q0 + q1) + q2;
  b[0] = q0 / s; b[1] = q1 / s; b[2] = q2 / s;
}

VKR_DEV int wrap_repeat(int i, int n) {
  if ((n & (n - 1)) == 0) return i & (n - 1);  // power-of-two extent (every mip of the usual texture): no integer division
  const int m = i % n;
  return m < 0 ? m + n : m;
}
// texture(sampler2D, uv) of an RGBA8_SRGB mip chain: REPEAT, bilinear, linear between the two mips of `lod`
// `lut`: the sRGB decode table (srgb_lut_stage), in LDS where the caller has staged it
VKR_DEV f4 sample_level_repeat(const Tex& t, f2 uv, const float* lut) {
  const float x = cfma(uv.x, (float)t.fw, -0.5f), y = cfma(uv.y, (float)t.fh, -0.5f);
  const float x0f = floorf(x), y0f = floorf(y);
  const float fx = x - x0f, fy = y - y0f;
  const int x0 = wrap_repeat(f2i(x0f), t.fw), y0 = wrap_repeat(f2i(y0f), t.fh);
  const int x1 = wrap_repeat(x0 + 1, t.fw), y1 = wrap_repeat(y0 + 1, t.fh);
  auto dec = [&](int tx, int ty) {
    const uint32_t v = *texel_ptr<const uint32_t>(t, tx, ty);
    return mk4(lut[v & 0xFFu], lut[(v >> 8) & 0xFFu], lut[(v >> 16) & 0xFFu], unorm8_to_float(v >> 24));
  };
  return mix4(mix4(dec(x0, y0), dec(x1, y0), fx), mix4(dec(x0, y1), dec(x1, y1), fx), fy);
}
VKR_DEV f4 sample_trilinear(const Pyramid& p, f2 uv, f2 duvdx, f2 duvdy, const float* lut) {
  const float w = (float)p.mip[0].fw, h = (float)p.mip[0].fh;
  // rho^2 = max squared footprint; lod = log2(rho).  The level pair comes from the exponent of rho^2
  // (exact), only the blend factor from log2f (smooth) — a libm ulp must not flip the pair.
  const float rx2 = (duvdx.x * w) * (duvdx.x * w) + (duvdx.y * h) * (duvdx.y * h);
  const float ry2 = (duvdy.x * w) * (duvdy.x * w) + (duvdy.y * h) * (duvdy.y * h);
  const float r2 = vmax(rx2, ry2);
  int l0 = 0;
  float f = 0.0f;
  if (r2 > 1.0f && r2 < 3.0e38f) {
    l0 = ilogbf(r2) >> 1;  // floor(log2(rho))
    f = vclamp(0.5f * log2f(r2) - (float)l0, 0.0f, 1.0f);
  }
  if (l0 >= p.count - 1) { l0 = p.count - 1; f = 0.0f; }  // sampler LOD range [0, 10] and the chain length
  const int l1 = min(l0 + 1, p.count - 1);
  const f4 a = sample_level_repeat(p.mip[l0], uv, lut);
  if (f == 0.0f || l1 == l0) return a;
  return mix4(a, sample_level_repeat(p.mip[l1], uv, lut), f);
}

// pixel bounding box (centres that can be covered), clipped to the viewport; false when empty
template <class T> VKR_DEV bool tri_bbox(const T& t, int width, int height, int* x0, int* y0, int* x1, int* y1) {
  const int minx = min(t.x[0], min(t.x[1], t.x[2])), maxx = max(t.x[0], max(t.x[1], t.x[2]));
  const int miny = min(t.y[0], min(t.y[1], t.y[2])), maxy = max(t.y[0], max(t.y[1], t.y[2]));
  *x0 = max((minx - 128) >> 8, 0); *x1 = min((maxx - 128) >> 8, width - 1);
  *y0 = max((miny - 128) >> 8, 0); *y1 = min((maxy - 128) >> 8, height - 1);
  return *x0 <= *x1 && *y0 <= *y1;
}
#define RASTER_SMALL_BLOCKS 64  // sub-triangles whose bounding box has more 8x8 blocks go to the shared-work kernel
#define RASTER_LARGE_CHUNK 16   // blocks per work item of the shared-work kernel
#define RASTER_LARGE_GRID 2048  // its blocks of four waves: chunk c goes to wave c mod (4 x grid)
struct LargeEntry { uint32_t rec, first_chunk; };  // a listed sub-triangle and the index of its first chunk

// Largest value edge a->b takes over the pixel centres X in [X0, X1], Y in [Y0, Y1] (24.8): when it is negative no pixel of
// the block is inside the triangle (an edge function is linear, its maximum over a box sits at a corner)
VKR_DEV long long edge_max(int ax, int ay, int bx, int by, int X0, int Y0, int X1, int Y1) {
  const int dx = bx - ax, dy = by - ay;
  return (long long)dx * (long long)((dx > 0 ? Y1 : Y0) - ay) - (long long)dy * (long long)((dy > 0 ? X0 : X1) - ax);
}
// the 8x8 pixel block at (bx0, by0) lies wholly outside one edge of t (half the blocks of a large triangle's bounding box):
// nothing to test per pixel
template <class T> VKR_DEV bool block_outside(const T& t, int bx0, int by0) {
  const int X0 = (bx0 << 8) + 128, Y0 = (by0 << 8) + 128, X1 = X0 + 7 * 256, Y1 = Y0 + 7 * 256;
  return edge_max(t.x[1], t.y[1], t.x[2], t.y[2], X0, Y0, X1, Y1) < 0 || edge_max(t.x[2], t.y[2], t.x[0], t.y[0], X0, Y0, X1, Y1) < 0 ||
         edge_max(t.x[0], t.y[0], t.x[1], t.y[1], X0, Y0, X1, Y1) < 0;
}
// 8x8 blocks a bounding box touches
VKR_DEV int bbox_blocks(int x0, int y0, int x1, int y1) { return ((x1 >> 3) - (x0 >> 3) + 1) * ((y1 >> 3) - (y0 >> 3) + 1); }
// the entry of the large-triangle list that owns chunk c: the last one with first_chunk <= c (the list is sorted by first_chunk)
VKR_DEV LargeEntry large_entry_of(const LargeEntry* list, uint32_t n, uint32_t c) {
  uint32_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (list[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
  }
  return list[lo];
}

// c = a * b with GLSL's mat4 * mat4 (column-major, each element a dot product accumulated left to right)
inline void mat_mul(Mat4& c, const vkr_mat4& a, const vkr_mat4& b) {
  for (int col = 0; col < 4; col++)
    for (int row = 0; row < 4; row++) {
      float s = a.m[0 * 4 + row] * b.m[col * 4 + 0];
      for (int k = 1; k < 4; k++) s = s + a.m[k * 4 + row] * b.m[col * 4 + k];
      c.m[col * 4 + row] = s;
    }
}

inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

}  // namespace vkr
