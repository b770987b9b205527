// raster_common.hpp — what the three compute rasterisers share (raster.hip: program "gbuf_opaque_taa", cubemap.hip: program
// "cubemap_probe", shadow.hip: program "default_shadow").  Device side: the frozen raster rules — exact 64-bit edge functions
// of 24.8 coordinates, the top-left fill rule, the 8-bit sub-pixel snap, the near-plane clip, D24 depth — the scene sampler
// (REPEAT, trilinear, sRGB), the uv of a fragment, the tail of triangle setup (snap, orientation, small / large lists) and
// the coverage stage: CoverTri and walk_blocks(), which hand every covered texel to the calling program's fragment functor.
// Host side: scene validation, the texture table, the upload of a table through kernel arguments and the carving of scratch.
// One definition of each, so the programs cannot drift apart; a program keeps its records, its vertex shader and its fragment.
#pragma once
#include <climits>
#include <string>
#include <vector>

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
  float depth = (lambda[0] * t.z[0] + lambda[1] * t.z[1]) + lambda[2] * t.z[2];
  // A weighted mean of corner depths that are all <= 1 is <= 1; only the fp32 rounding of the rounded weights can lift it an ulp
  // above (pinholes in a triangle that lies on the far plane).  Such a fragment is on the far plane, not beyond it.
  if (depth > 1.0f && fmaxf(t.z[0], fmaxf(t.z[1], t.z[2])) <= 1.0f) depth = 1.0f;
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

// uv and its forward differences at pixel (px, py) of record t with the uv corners uv0..uv2 (lambda: its screen-space
// barycentrics there): what the fragment shader's texture() calls see (implicit derivatives as differences to the right /
// lower pixel).  b: the perspective-correct barycentrics, for the caller's other attributes
struct FragUv { f2 uv, ddx, ddy; float b[3]; };
template <class T>
VKR_DEV FragUv fragment_uv(const T& t, const f2& uv0, const f2& uv1, const f2& uv2, int px, int py, const float lambda[3]) {
  FragUv f;
  perspective(t, lambda, f.b);
  float lx1[3], ly1[3], bx1[3], by1[3];
  lambda_at(t, px + 1, py, lx1);
  lambda_at(t, px, py + 1, ly1);
  perspective(t, lx1, bx1);
  perspective(t, ly1, by1);
  auto at = [&](const float b[3]) { return mk2((b[0] * uv0.x + b[1] * uv1.x) + b[2] * uv2.x, (b[0] * uv0.y + b[1] * uv1.y) + b[2] * uv2.y); };
  f.uv = at(f.b);
  f.ddx = at(bx1) - f.uv; f.ddy = at(by1) - f.uv;
  return f;
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
  // the first centre at or after the smallest coordinate (rounded up), the last at or before the largest (rounded down)
  *x0 = max((minx + 127) >> 8, 0); *x1 = min((maxx - 128) >> 8, width - 1);
  *y0 = max((miny + 127) >> 8, 0); *y1 = min((maxy - 128) >> 8, height - 1);
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

// the draw that owns global triangle `gtri` (draws are consecutive ranges [tri_base, tri_base + tri_count))
template <class D> VKR_DEV uint32_t draw_of(const D* draws, uint32_t count, uint32_t gtri) {
  uint32_t lo = 0, hi = count - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (draws[mid].tri_base <= gtri) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- the tail of triangle setup (cubemap.hip, shadow.hip) ----
// planes of the clip volume that p lies outside of: x < -w, x > w, y < -w, y > w, z < 0.  A triangle whose three masks share a
// bit cannot cover a texel centre
VKR_DEV uint32_t frustum_out_mask(f4 p) {
  return (p.x < -p.w ? 1u : 0u) | (p.x > p.w ? 2u : 0u) | (p.y < -p.w ? 4u : 0u) | (p.y > p.w ? 8u : 0u) | (p.z < 0.0f ? 16u : 0u);
}
// Snaps the clip positions of three clipped corners and normalises the orientation (cull none: both windings are drawn):
// fills x, y, z, w and inv_area2 of a record.  false: a corner is behind the eye or beyond the guard band, or the area is 0.
// *flip: corners 1 and 2 were exchanged; the caller exchanges its other attributes likewise.
VKR_DEV bool snap_orient(f4 c0, f4 c1, f4 c2, int width, int height, int (&x)[3], int (&y)[3], float (&z)[3], float (&w)[3],
                         double* inv_area2, bool* flip) {
  bool ok = snap_vertex(c0, width, height, &x[0], &y[0], &w[0], &z[0]);
  ok = snap_vertex(c1, width, height, &x[1], &y[1], &w[1], &z[1]) && ok;
  ok = snap_vertex(c2, width, height, &x[2], &y[2], &w[2], &z[2]) && ok;
  if (!ok) return false;
  long long area2 = edge_fn(x[0], y[0], x[1], y[1], x[2], y[2]);
  if (area2 == 0) return false;
  *flip = area2 < 0;
  if (*flip) {
    int ti = x[1]; x[1] = x[2]; x[2] = ti;
    ti = y[1]; y[1] = y[2]; y[2] = ti;
    float tf = w[1]; w[1] = w[2]; w[2] = tf;
    tf = z[1]; z[1] = z[2]; z[2] = tf;
    area2 = -area2;
  }
  *inv_area2 = 1.0 / (double)area2;
  return true;
}
// Lists record `rec`, whose bounding box touches nb blocks.  A large record takes a list slot AND its range of chunks with
// one 64-bit atomicAdd on *large_state (entries << 32 | chunks), so the large list is sorted by first_chunk
VKR_DEV void list_append(uint32_t rec, int nb, unsigned long long* large_state, LargeEntry* large_list, unsigned long long* small_count,
                         uint32_t* small_list) {
  if (nb > RASTER_SMALL_BLOCKS) {
    const uint32_t chunks = (uint32_t)(nb + RASTER_LARGE_CHUNK - 1) / RASTER_LARGE_CHUNK;
    const unsigned long long v = atomicAdd(large_state, (1ull << 32) | (unsigned long long)chunks);
    large_list[(uint32_t)(v >> 32)] = LargeEntry {rec, (uint32_t)v};
  } else {
    small_list[(uint32_t)atomicAdd(small_count, 1ull)] = rec;
  }
}

// ---- the coverage stage ----
// What coverage and depth need of a record, copied into registers once per triangle: the rasterising waves issue atomics
// between their reads of the record, and the compiler must otherwise assume those change it and reload.
struct CoverTri {
  int x[3], y[3];
  float z[3];
  double inv_area2;
  template <class T> VKR_DEV explicit CoverTri(const T& t) : x {t.x[0], t.x[1], t.x[2]}, y {t.y[0], t.y[1], t.y[2]}, z {t.z[0], t.z[1], t.z[2]}, inv_area2 {t.inv_area2} {}
};
// One wave walks the 8x8 texel blocks [first, first + count) of t's bounding box in the width x height viewport (row-major
// inside the box, cut off at its last block), one texel per lane, and calls frag(px, py, lambda, d24) for every covered
// texel; what a fragment does (alpha test, which atomic, where) is the program's.  A box of more than max_blocks is not walked.
template <class F>
VKR_DEV void walk_blocks(const CoverTri& t, int width, int height, int first, int count, int max_blocks, int lane, const F& frag) {
  int x0, y0, x1, y1;
  if (!tri_bbox(t, width, height, &x0, &y0, &x1, &y1)) return;
  const int nb = bbox_blocks(x0, y0, x1, y1);
  if (nb > max_blocks) return;
  const int bw = (x1 >> 3) - (x0 >> 3) + 1;
  const int end = count < nb - first ? first + count : nb;
  for (int b = first; b < end; b++) {
    const int bx0 = ((x0 >> 3) + b % bw) << 3, by0 = ((y0 >> 3) + b / bw) << 3;
    if (block_outside(t, bx0, by0)) continue;
    const int px = bx0 + (lane & 7), py = by0 + (lane >> 3);
    if (px < x0 || px > x1 || py < y0 || py > y1) continue;  // the bounding box is clipped to the viewport: the texel exists
    float lambda[3];
    uint32_t d24;
    if (cover(t, px, py, lambda, &d24)) frag(px, py, lambda, d24);
  }
}
// The coverage kernels are launched with COVER_BLOCK threads (the kernels' launch bounds and the entry points' launches both
// use the constant).  This wave's index among the waves of such a launch, and their number: the stride of a loop over a list
#define COVER_BLOCK_WAVES 4u
#define COVER_BLOCK (64u * COVER_BLOCK_WAVES)
VKR_DEV uint32_t wave_index() { return blockIdx.x * COVER_BLOCK_WAVES + (threadIdx.x >> 6); }
VKR_DEV uint32_t wave_count() { return gridDim.x * COVER_BLOCK_WAVES; }

// ---- host side ----
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

// A program's scratch is its parts one after the other, each padded to 256 bytes.  The program writes the sequence of take()
// calls once, in its layout struct; the size function reads `at` of it, the entry point the offsets: they cannot disagree.
struct ScratchCarver {
  uint64_t at = 0;
  uint64_t take(uint64_t bytes) { const uint64_t offset = at; at += align_up(bytes, 256); return offset; }
};

// A table (draw constants, texture pyramids) travels as kernel arguments, N elements per launch, into scratch: no host staging
// memory has to outlive the call and nothing synchronises
template <class T, int N> struct TableChunk { T e[N]; };
template <class T, int N> __global__ void k_store_table(TableChunk<T, N> c, T* dst, uint32_t n) {
  if (threadIdx.x < n) dst[threadIdx.x] = c.e[threadIdx.x];
}
template <int N, class T> inline void store_table(const std::vector<T>& src, const T* dst, hipStream_t stream) {
  const uint32_t count = (uint32_t)src.size();
  for (uint32_t i = 0; i < count; i += N) {
    TableChunk<T, N> c;
    const uint32_t n = count - i < (uint32_t)N ? count - i : (uint32_t)N;
    for (uint32_t k = 0; k < (uint32_t)N; k++) c.e[k] = src[i + (k < n ? k : 0)];  // the tail repeats an element: defined bytes
    hipLaunchKernelGGL((k_store_table<T, N>), dim3(1), dim3(64), 0, stream, c, const_cast<T*>(dst) + i, n);
  }
}

// the mip chains of scene->textures as the sampler reads them
inline int make_pyramids(const vkr_raster_scene* scene, const char* program, std::vector<Pyramid>* out) {
  if (scene->texture_count && !scene->textures) {
    set_error("%s: scene: %u textures but a NULL texture array", program, scene->texture_count);
    return VKR_ERR_NULL;
  }
  const std::string what = std::string(program) + ".texture";
  out->resize(scene->texture_count);
  for (uint32_t i = 0; i < scene->texture_count; i++) {
    const vkr_img& t = scene->textures[i];
    Pyramid& p = (*out)[i];
    if (t.mip_count < 1 || t.mip_count > VKR_MAX_MIPS) { set_error("%s: texture %u: bad mip count", program, i); return VKR_ERR_MIPS; }
    p.count = (int)t.mip_count;
    for (int m = 0; m < (int)t.mip_count; m++) VKR_TRY(make_tex(&t, m, VKR_FMT_RGBA8_SRGB, what.c_str(), &p.mip[m]));
    for (int m = (int)t.mip_count; m < 16; m++) p.mip[m] = p.mip[0];
  }
  return VKR_OK;
}

// What every entry point checks of a scene before it launches anything: the arrays exist when there are draws, and every draw
// stays inside them (the index range in 64 bits: offset + count of two uint32_t can wrap).  wants_textures: the program reads
// the textures, so both texture indices of a draw are checked too (0xFFFFFFFF: none) — also the material index for the cube
// bake, which samples only albedo: a scene is valid or not, whichever program sees it.  *total_tris: every triangle of the scene.
inline int check_scene(const char* program, const vkr_raster_scene* scene, bool wants_textures, uint64_t* total_tris) {
  if (scene->draw_count && (!scene->draws || !scene->transforms || !scene->vertices || !scene->indices)) {
    set_error("%s: scene: %u draws but a NULL vertex, index, transform or draw array", program, scene->draw_count);
    return VKR_ERR_NULL;
  }
  *total_tris = 0;
  for (uint32_t i = 0; i < scene->draw_count; i++) {
    const vkr_raster_draw& s = scene->draws[i];
    if (s.transform_index >= scene->transform_count) {
      set_error("%s: scene: draw %u: transform_index %u outside the %u transforms", program, i, s.transform_index, scene->transform_count);
      return VKR_ERR_EXTENT;
    }
    if ((uint64_t)s.index_offset + s.index_count > scene->index_count) {
      set_error("%s: scene: draw %u: indices [%u, +%u) outside the %u indices", program, i, s.index_offset, s.index_count, scene->index_count);
      return VKR_ERR_EXTENT;
    }
    const bool bad_albedo = s.albedo_index != 0xFFFFFFFFu && s.albedo_index >= scene->texture_count;
    const bool bad_material = s.mr_index != 0xFFFFFFFFu && s.mr_index >= scene->texture_count;
    if (wants_textures && (bad_albedo || bad_material)) {
      set_error("%s: scene: draw %u: texture index (albedo %u, material %u) outside the %u textures", program, i, s.albedo_index, s.mr_index,
                scene->texture_count);
      return VKR_ERR_EXTENT;
    }
    *total_tris += s.index_count / 3u;
  }
  return VKR_OK;
}

}  // namespace vkr
