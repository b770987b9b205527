// probe.hip — the octahedral probe programs of probe_renderer.{hpp,cpp}: cube2oct (cube -> octahedral colour + depth),
// probe_downsample (min-depth mip chain of one probe) and trace_probe (screen-space reflections traced through a grid of
// probes).  Literal ports in the numeric contract of vkr_device.hpp; the frozen choices (cube face ties, corner taps,
// float -> int truncation) are listed in DESIGN_NUMERICS.md.  tests/probe_reference.py restates every kernel in numpy.
#include "vkr_host.hpp"

namespace vkr {

// ---- array images: layer l of mip m lies at layer 0's mip m plus l * stride[m] ----------------------------------------------
struct LayerArray {
  Tex mip[VKR_MAX_MIPS];         // layer 0
  long long stride[VKR_MAX_MIPS];  // bytes from one layer to the next, per mip
  int mips, layers;
};

static int make_layer_array(const vkr_img* layers, uint32_t count, uint32_t format, int mips, const char* what, LayerArray* out) {
  if (!layers || count == 0) { set_error("%s: no array layers", what); return VKR_ERR_NULL; }
  if (mips < 1 || mips > VKR_MAX_MIPS) { set_error("%s: %d mips, needs 1..%d", what, mips, VKR_MAX_MIPS); return VKR_ERR_MIPS; }
  out->mips = mips;
  out->layers = (int)count;
  for (int m = 0; m < mips; m++) {
    VKR_TRY(make_tex(&layers[0], m, format, what, &out->mip[m]));
    const Tex& t0 = out->mip[m];
    VKR_TRY(require_whole_frame(t0, what, "array layers cannot be windows"));
    out->stride[m] = 0;
    for (uint32_t l = 1; l < count; l++) {
      Tex t;
      VKR_TRY(make_tex(&layers[l], m, format, what, &t));
      if (!same_layout(t, t0) || layers[l].mip_count != layers[0].mip_count) {
        set_error("%s: layer %u does not share layer 0's extent, pitch and mips", what, l);
        return VKR_ERR_EXTENT;
      }
      const long long d = (long long)(t.p - t0.p);
      if (l == 1) out->stride[m] = d;
      if (d != (long long)l * out->stride[m]) { set_error("%s: layer %u of mip %d is not at a regular distance", what, l, m); return VKR_ERR_LAYOUT; }
    }
  }
  return VKR_OK;
}

VKR_DEV const uint8_t* layer_texel(const LayerArray& a, int mip, int layer, int x, int y, int bpp) {
  return a.mip[mip].p + (long long)layer * a.stride[mip] + toff(a.mip[mip], x, y, bpp);
}

// ---- octahedral.glsl ----------------------------------------------------------------------------------------------------
VKR_DEV float o_sign_nz(float k) { return (k >= 0.0f) ? 1.0f : -1.0f; }
VKR_DEV float sign0(float k) { return k > 0.0f ? 1.0f : (k < 0.0f ? -1.0f : 0.0f); }
// the folded vector of oct_decode / oct_center: uv = 2 (uv - 0.5), (u, v, 1 - |u| - |v|), lower hemisphere folded
VKR_DEV f3 oct_fold(f2 uv) {
  const float u = 2.0f * (uv.x - 0.5f), v = 2.0f * (uv.y - 0.5f);
  f3 r = mk3(u, v, (1.0f - fabsf(u)) - fabsf(v));
  if (r.z < 0.0f) {
    const float nx = (1.0f - fabsf(r.y)) * o_sign_nz(r.x), ny = (1.0f - fabsf(r.x)) * o_sign_nz(r.y);
    r.x = nx; r.y = ny;
  }
  return r;
}
VKR_DEV f3 oct_decode(f2 uv) { return normalize(oct_fold(uv)); }
VKR_DEV f3 oct_center(f2 uv) { const f3 v = oct_fold(uv); return normalize(mk3(sign0(v.x), sign0(v.y), sign0(v.z))); }
VKR_DEV f2 oct_encode(f3 v) {
  const float l1norm = (fabsf(v.x) + fabsf(v.y)) + fabsf(v.z);
  const float inv = 1.0f / l1norm;
  f2 r = mk2(v.x * inv, v.y * inv);
  if (v.z < 0.0f) r = mk2((1.0f - fabsf(r.y)) * o_sign_nz(r.x), (1.0f - fabsf(r.x)) * o_sign_nz(r.y));
  return mk2(cfma(0.5f, r.x, 0.5f), cfma(0.5f, r.y, 0.5f));
}
VKR_DEV float encode_oct_depth(float z, float n, float f) { return f / (f - n) + (f * n) / ((-z) * (f - n)); }
VKR_DEV float decode_oct_depth(float d, float n, float f) { return -(n * f) / cfma(d, f - n, -f); }

// ---- cube2oct ----------------------------------------------------------------------------------------------------------
struct Cube2OctArgs {
  Tex color[6], distance[6];
  Tex oct_color, oct_depth;
  int tex_w, tex_h;
};

struct CubeTexel { float r, g, b, a, d; };

// direction of texel (i, j) of face f in units of half a texel (major axis = n), for i, j in [-1, n]
VKR_DEV void face_dir(int f, int sc, int tc, int n, int* r) {
  switch (f) {
    case 0: r[0] = n; r[1] = -tc; r[2] = -sc; break;
    case 1: r[0] = -n; r[1] = -tc; r[2] = sc; break;
    case 2: r[0] = sc; r[1] = n; r[2] = tc; break;
    case 3: r[0] = sc; r[1] = -n; r[2] = -tc; break;
    case 4: r[0] = sc; r[1] = -tc; r[2] = n; break;
    default: r[0] = -sc; r[1] = -tc; r[2] = -n; break;
  }
}
// (sc, tc) of a direction on face f (the Vulkan face table)
VKR_DEV void face_coords(int f, const int* r, int* sc, int* tc) {
  switch (f) {
    case 0: *sc = -r[2]; *tc = -r[1]; break;
    case 1: *sc = r[2]; *tc = -r[1]; break;
    case 2: *sc = r[0]; *tc = r[2]; break;
    case 3: *sc = r[0]; *tc = -r[2]; break;
    case 4: *sc = r[0]; *tc = -r[1]; break;
    default: *sc = -r[0]; *tc = -r[1]; break;
  }
}
VKR_DEV int edge_index(int v, int n) { return v >= n ? n - 1 : (v <= -n ? 0 : (v + n - 1) >> 1); }
// texel (i, j) of face f with exactly one coordinate one past an edge: the texel of the neighbouring face that touches it
VKR_DEV void across_edge(int f, int i, int j, int n, int* f2, int* i2, int* j2) {
  int r[3];
  face_dir(f, 2 * i + 1 - n, 2 * j + 1 - n, n, r);
  const int ax = abs(r[0]), ay = abs(r[1]);
  int nf;
  if (ax > n) nf = r[0] > 0 ? 0 : 1;
  else if (ay > n) nf = r[1] > 0 ? 2 : 3;
  else nf = r[2] > 0 ? 4 : 5;
  int sc, tc;
  face_coords(nf, r, &sc, &tc);
  *f2 = nf; *i2 = edge_index(sc, n); *j2 = edge_index(tc, n);
}
VKR_DEV CubeTexel load_cube_texel(const Cube2OctArgs& a, int f, int i, int j) {
  const uint32_t c = *(const uint32_t*)(a.color[f].p + toff(a.color[f], i, j, 4));
  CubeTexel t;
  t.r = srgb8_to_float(c & 0xFFu); t.g = srgb8_to_float((c >> 8) & 0xFFu); t.b = srgb8_to_float((c >> 16) & 0xFFu);
  t.a = unorm8_to_float(c >> 24);
  t.d = half_bits_to_float(*(const uint16_t*)(a.distance[f].p + toff(a.distance[f], i, j, 2)));
  return t;
}
// the frozen seamless tap: inside the face, across one edge, or a corner (mean of the three texels that meet there)
VKR_DEV CubeTexel cube_tap(const Cube2OctArgs& a, int f, int i, int j, int n) {
  const bool out_i = i < 0 || i >= n, out_j = j < 0 || j >= n;
  if (!out_i && !out_j) return load_cube_texel(a, f, i, j);
  const int ci = iclamp(i, 0, n - 1), cj = iclamp(j, 0, n - 1);
  int g, gi, gj;
  if (!out_i || !out_j) { across_edge(f, i, j, n, &g, &gi, &gj); return load_cube_texel(a, g, gi, gj); }
  const CubeTexel t0 = load_cube_texel(a, f, ci, cj);
  across_edge(f, i, cj, n, &g, &gi, &gj);
  const CubeTexel t1 = load_cube_texel(a, g, gi, gj);
  across_edge(f, ci, j, n, &g, &gi, &gj);
  const CubeTexel t2 = load_cube_texel(a, g, gi, gj);
  CubeTexel t;
  t.r = ((t0.r + t1.r) + t2.r) / 3.0f; t.g = ((t0.g + t1.g) + t2.g) / 3.0f; t.b = ((t0.b + t1.b) + t2.b) / 3.0f;
  t.a = ((t0.a + t1.a) + t2.a) / 3.0f; t.d = ((t0.d + t1.d) + t2.d) / 3.0f;
  return t;
}
VKR_DEV CubeTexel lerp_texel(CubeTexel p, CubeTexel q, float t) {
  CubeTexel r;
  r.r = mixf(p.r, q.r, t); r.g = mixf(p.g, q.g, t); r.b = mixf(p.b, q.b, t); r.a = mixf(p.a, q.a, t); r.d = mixf(p.d, q.d, t);
  return r;
}
// texture(samplerCube, dir) on both cubes: face by the largest |component| (ties: x, then y, then z), s = 0.5 sc / |ma| + 0.5
VKR_DEV CubeTexel sample_cube(const Cube2OctArgs& a, f3 dir) {
  const float ax = fabsf(dir.x), ay = fabsf(dir.y), az = fabsf(dir.z);
  int f;
  float sc, tc, ma;
  if (ax >= ay && ax >= az) { f = dir.x < 0.0f ? 1 : 0; ma = ax; sc = f == 0 ? -dir.z : dir.z; tc = -dir.y; }
  else if (ay >= az) { f = dir.y < 0.0f ? 3 : 2; ma = ay; sc = dir.x; tc = f == 2 ? dir.z : -dir.z; }
  else { f = dir.z < 0.0f ? 5 : 4; ma = az; sc = f == 4 ? dir.x : -dir.x; tc = -dir.y; }
  const float s = cfma(0.5f, sc / ma, 0.5f), t = cfma(0.5f, tc / ma, 0.5f);
  const int n = a.color[0].w;
  const float x = cfma(s, (float)n, -0.5f), y = cfma(t, (float)n, -0.5f);
  const float x0f = floorf(x), y0f = floorf(y);
  const float fx = x - x0f, fy = y - y0f;
  const int x0 = f2i(x0f), y0 = f2i(y0f);
  const CubeTexel t00 = cube_tap(a, f, x0, y0, n), t10 = cube_tap(a, f, x0 + 1, y0, n);
  const CubeTexel t01 = cube_tap(a, f, x0, y0 + 1, n), t11 = cube_tap(a, f, x0 + 1, y0 + 1, n);
  return lerp_texel(lerp_texel(t00, t10, fx), lerp_texel(t01, t11, fx), fy);
}

// cube2oct/shader.comp:14-32
__global__ __launch_bounds__(64) void k_cube2oct(Cube2OctArgs a) {
  const int x = blockIdx.x * 8 + (threadIdx.x & 7), y = blockIdx.y * 8 + (threadIdx.x >> 3);
  if (x >= a.tex_w || y >= a.tex_h) return;
  const f2 uv = mk2((float)x / (float)a.tex_w, (float)y / (float)a.tex_h);
  const f3 dir = oct_decode(uv);
  const CubeTexel c = sample_cube(a, dir);
  const f3 view_dir = dir * c.d;
  const f3 front = oct_center(uv);
  const float depth = encode_oct_depth(vclamp(dot(view_dir, front), VKR_PROBE_ZNEAR, VKR_PROBE_ZFAR), VKR_PROBE_ZNEAR, VKR_PROBE_ZFAR);
  *texel_ptr<uint32_t>(a.oct_color, x, y) =
      float_to_unorm8(c.r) | (float_to_unorm8(c.g) << 8) | (float_to_unorm8(c.b) << 16) | (float_to_unorm8(c.a) << 24);
  *texel_ptr<uint16_t>(a.oct_depth, x, y) = (uint16_t)float_to_unorm16(depth);
}

// ---- probe_downsample ---------------------------------------------------------------------------------------------------
// probe_downsample/shader.frag: a fetch at min(2 pixel + o, size) past the last texel reads 0
VKR_DEV float fetch_r16u(const Tex& t, int x, int y) {
  if (x >= t.w || y >= t.h) return 0.0f;
  return unorm16_to_float(*(const uint16_t*)(t.p + toff(t, x, y, 2)));
}
__global__ __launch_bounds__(64) void k_probe_downsample(Tex src, Tex dst) {
  const int x = blockIdx.x * 8 + (threadIdx.x & 7), y = blockIdx.y * 8 + (threadIdx.x >> 3);
  if (x >= dst.w || y >= dst.h) return;
  const int px = 2 * x, py = 2 * y;
  float m = 1000.0f;
  m = vmin(fetch_r16u(src, min(px, src.w), min(py, src.h)), m);
  m = vmin(fetch_r16u(src, min(px, src.w), min(py + 1, src.h)), m);
  m = vmin(fetch_r16u(src, min(px + 1, src.w), min(py, src.h)), m);
  m = vmin(fetch_r16u(src, min(px + 1, src.w), min(py + 1, src.h)), m);
  *texel_ptr<uint16_t>(dst, x, y) = (uint16_t)float_to_unorm16(m);
}

// ---- trace_probe ----------------------------------------------------------------------------------------------------------
#define PROBE_MISS 0
#define PROBE_HIT 1
#define PROBE_UNKNOWN 2
#define PROBE_TRACE_STEPS 25
#define PROBE_MAX_T 3.402823466e+38f

struct TraceProbeArgs {
  Tex depth, normal, out;
  LayerArray color, pdepth;
  Mat4 inverse_view;
  f3 probe_min, probe_step;
  int grid;
  Proj pr;
  int tex_w, tex_h;
};

// One mip of the probe depth array as the march reads it.  The march picks the mip per lane, and a per-lane index into the
// kernel arguments becomes vector loads of the descriptor before every texel; the block copies the table into LDS once.
struct MipEntry {
  const uint8_t* p;
  long long stride;
  int pitch, w, h;
};

// texelFetch(PROBE_DEPTH_TEX, ivec3(pos, layer), mip): the coordinate truncates toward zero; outside the mip or past the
// last mip reads 0
VKR_DEV float probe_depth_fetch(const TraceProbeArgs& a, const MipEntry* mips, f2 pos, int layer, int mip) {
  if (mip >= a.pdepth.mips) return 0.0f;
  const int x = f2i_index(pos.x), y = f2i_index(pos.y);
  const MipEntry& t = mips[mip];
  if ((unsigned)x >= (unsigned)t.w || (unsigned)y >= (unsigned)t.h) return 0.0f;
  return unorm16_to_float(*(const uint16_t*)(t.p + (long long)layer * t.stride + __umul24((uint32_t)y, (uint32_t)t.pitch) + (uint32_t)x * 2u));
}
// textureLod(PROBE_DEPTH_TEX, vec3(uv, layer), 0): bilinear, clamp-to-edge on mip 0
VKR_DEV float probe_depth_bilinear(const TraceProbeArgs& a, f2 uv, int layer) {
  const Tex& t = a.pdepth.mip[0];
  const float x = cfma(uv.x, (float)t.w, -0.5f), y = cfma(uv.y, (float)t.h, -0.5f);
  const float x0f = floorf(x), y0f = floorf(y);
  const float fx = x - x0f, fy = y - y0f;
  const int x0 = f2i(x0f), y0 = f2i(y0f);
  const int xa = iclamp(x0, 0, t.w - 1), xb = iclamp(x0 + 1, 0, t.w - 1), ya = iclamp(y0, 0, t.h - 1), yb = iclamp(y0 + 1, 0, t.h - 1);
  const float t00 = unorm16_to_float(*(const uint16_t*)layer_texel(a.pdepth, 0, layer, xa, ya, 2));
  const float t10 = unorm16_to_float(*(const uint16_t*)layer_texel(a.pdepth, 0, layer, xb, ya, 2));
  const float t01 = unorm16_to_float(*(const uint16_t*)layer_texel(a.pdepth, 0, layer, xa, yb, 2));
  const float t11 = unorm16_to_float(*(const uint16_t*)layer_texel(a.pdepth, 0, layer, xb, yb, 2));
  return mixf(mixf(t00, t10, fx), mixf(t01, t11, fx), fy);
}
// texture(PROBE_COLOR_TEX, vec3(uv, layer)): RGBA8_UNORM, bilinear, clamp-to-edge, stored back as RGBA8_UNORM
VKR_DEV uint32_t probe_color_sample(const TraceProbeArgs& a, f2 uv, int layer) {
  const Tex& t = a.color.mip[0];
  const float x = cfma(uv.x, (float)t.w, -0.5f), y = cfma(uv.y, (float)t.h, -0.5f);
  const float x0f = floorf(x), y0f = floorf(y);
  const float fx = x - x0f, fy = y - y0f;
  const int x0 = f2i(x0f), y0 = f2i(y0f);
  const int xa = iclamp(x0, 0, t.w - 1), xb = iclamp(x0 + 1, 0, t.w - 1), ya = iclamp(y0, 0, t.h - 1), yb = iclamp(y0 + 1, 0, t.h - 1);
  const uint32_t c00 = *(const uint32_t*)layer_texel(a.color, 0, layer, xa, ya, 4);
  const uint32_t c10 = *(const uint32_t*)layer_texel(a.color, 0, layer, xb, ya, 4);
  const uint32_t c01 = *(const uint32_t*)layer_texel(a.color, 0, layer, xa, yb, 4);
  const uint32_t c11 = *(const uint32_t*)layer_texel(a.color, 0, layer, xb, yb, 4);
  uint32_t out = 0;
#pragma unroll
  for (int ch = 0; ch < 4; ch++) {
    const int sh = 8 * ch;
    const float v = mixf(mixf(unorm8_to_float((c00 >> sh) & 0xFFu), unorm8_to_float((c10 >> sh) & 0xFFu), fx),
                         mixf(unorm8_to_float((c01 >> sh) & 0xFFu), unorm8_to_float((c11 >> sh) & 0xFFu), fx), fy);
    out |= float_to_unorm8(v) << sh;
  }
  return out;
}

// trace_probe/shader.comp:218-267 (most_detailed_mip 0, 25 steps; valid_hit is always true)
VKR_DEV f3 hierarchical_raymarch(const TraceProbeArgs& a, const MipEntry* mips, int layer, f3 origin, f3 direction) {
  const f3 inv_direction = mk3(direction.x != 0.0f ? 1.0f / direction.x : PROBE_MAX_T, direction.y != 0.0f ? 1.0f / direction.y : PROBE_MAX_T,
                               direction.z != 0.0f ? 1.0f / direction.z : PROBE_MAX_T);
  int current_mip = 0;
  const f2 screen_size = mk2((float)a.pdepth.mip[0].w, (float)a.pdepth.mip[0].h);
  f2 res = screen_size;
  f2 res_inv = mk2(1.0f / res.x, 1.0f / res.y);
  f2 uv_offset = mk2(0.005f / screen_size.x, 0.005f / screen_size.y);  // 0.005 * exp2(0) / screen_size
  uv_offset.x = direction.x < 0.0f ? -uv_offset.x : uv_offset.x;
  uv_offset.y = direction.y < 0.0f ? -uv_offset.y : uv_offset.y;
  const f2 floor_offset = mk2(direction.x < 0.0f ? 0.0f : 1.0f, direction.y < 0.0f ? 0.0f : 1.0f);
  // initial_advance_ray (:175-182)
  float current_t;
  {
    const f2 cur = res * xy(origin);
    const float px = cfma(floorf(cur.x) + floor_offset.x, res_inv.x, uv_offset.x);
    const float py = cfma(floorf(cur.y) + floor_offset.y, res_inv.y, uv_offset.y);
    current_t = vmin((px - origin.x) * inv_direction.x, (py - origin.y) * inv_direction.y);
  }
  f3 position = madd(origin, current_t, direction);
#pragma unroll 1
  for (int i = 0; i < PROBE_TRACE_STEPS && current_mip >= 0; i++) {
    const f2 mip_pos = res * xy(position);
    const float surface_z = probe_depth_fetch(a, mips, mip_pos, layer, current_mip);
    // advance_ray (:184-212)
    const float px = cfma(floorf(mip_pos.x) + floor_offset.x, res_inv.x, uv_offset.x);
    const float py = cfma(floorf(mip_pos.y) + floor_offset.y, res_inv.y, uv_offset.y);
    const float tx = (px - origin.x) * inv_direction.x, ty = (py - origin.y) * inv_direction.y;
    float tz = (surface_z - origin.z) * inv_direction.z;
    tz = direction.z > 0.0f ? tz : PROBE_MAX_T;
    const float t_min = vmin(vmin(vmin(tx, ty), tz), 1.0f);
    const bool above_surface = surface_z > position.z;
    const bool skipped_tile = t_min != tz && above_surface;
    current_t = above_surface ? t_min : current_t;
    position = madd(origin, current_t, direction);
    current_mip += skipped_tile ? 1 : -1;
    res = res * (skipped_tile ? 0.5f : 2.0f);
    res_inv = res_inv * (skipped_tile ? 2.0f : 0.5f);
  }
  return position;
}

// trace_probe/shader.comp:269-324
VKR_DEV int trace_segment_hi(const TraceProbeArgs& a, const MipEntry* mips, f3 ray_origin, f3 ray_dir, float t0, float t1, float& tmin, int layer, f2& stop_tc) {
  f3 probe_start = madd(ray_origin, t0 + 0.001f, ray_dir);
  const f3 probe_end = madd(ray_origin, t1 - 0.001f, ray_dir);
  const f3 d = probe_start - probe_end;
  if (dot(d, d) < 0.001f) probe_start = ray_dir;
  const f2 start_oct = oct_encode(normalize(probe_start));
  const f2 end_oct = oct_encode(normalize(probe_end));
  const f3 front = oct_center((start_oct + end_oct) * 0.5f);
  const float start_depth = encode_oct_depth(dot(probe_start, front), VKR_PROBE_ZNEAR, VKR_PROBE_ZFAR) - 0.0005f;
  const float end_depth = encode_oct_depth(dot(probe_end, front), VKR_PROBE_ZNEAR, VKR_PROBE_ZFAR);
  const f3 p_start = mk3(start_oct.x, start_oct.y, start_depth);
  const f3 p_end = mk3(end_oct.x, end_oct.y, end_depth);
  const f3 p_stop = hierarchical_raymarch(a, mips, layer, p_start, p_end - p_start);
  stop_tc = xy(p_stop);
  const f3 stop_dir = oct_decode(stop_tc);
  const float coef = decode_oct_depth(p_stop.z, VKR_PROBE_ZNEAR, VKR_PROBE_ZFAR) / dot(stop_dir, front);
  const f3 ray_stop = stop_dir * coef;
  const f3 diff = ray_stop - ray_origin;
  tmin = sqrtf(dot(diff, diff));
  const float sampled_depth = probe_depth_bilinear(a, stop_tc, layer);
  if (p_stop.z > 1.0f) return PROBE_MISS;
  if (p_stop.z > sampled_depth + 0.0005f) return PROBE_UNKNOWN;
  if (p_stop.z > sampled_depth - 0.0005f) return PROBE_HIT;
  return PROBE_MISS;
}

// trace_probe/shader.comp:380-408 (the overload that takes the probe)
VKR_DEV int trace_one_probe(const TraceProbeArgs& a, const MipEntry* mips, f3 ray_origin, f3 ray_dir, int probe, float& tmin, float tmax, f2& hit) {
  const float px = (float)(probe % a.grid), py = (float)(probe / a.grid);
  const f3 probe_origin = mk3(cfma(px, a.probe_step.x, a.probe_min.x), cfma(0.0f, a.probe_step.y, a.probe_min.y),
                              cfma(py, a.probe_step.z, a.probe_min.z));
  const f3 o = ray_origin - probe_origin;
  const f3 dir = normalize(ray_dir);
  // compute_trace_segments (:101-115): t = origin * -(1 / dir), sorted by three swap_min
  float tx = o.x * -(1.0f / dir.x), ty = o.y * -(1.0f / dir.y), tz = o.z * -(1.0f / dir.z);
  float m;
  m = vmin(tx, ty); ty = vmax(tx, ty); tx = m;
  m = vmin(ty, tz); tz = vmax(ty, tz); ty = m;
  m = vmin(tx, ty); ty = vmax(tx, ty); tx = m;
  const float s0 = tmin, s1 = vclamp(tx, tmin, tmax), s2 = vclamp(ty, tmin, tmax), s3 = vclamp(tz, tmin, tmax), s4 = tmax;
#pragma unroll 1
  for (int i = 0; i < 4; i++) {
    const float lo = i == 0 ? s0 : (i == 1 ? s1 : (i == 2 ? s2 : s3));
    const float hi = i == 0 ? s1 : (i == 1 ? s2 : (i == 2 ? s3 : s4));
    if (fabsf(hi - lo) >= 0.002f) {
      const int r = trace_segment_hi(a, mips, o, dir, lo, hi, tmin, probe, hit);
      if (r != PROBE_MISS) return r;
    }
  }
  return PROBE_MISS;
}

// trace_probe/shader.comp:48-82 + 326-347 + 410-441; one lane per pixel
__global__ __launch_bounds__(64) void k_trace_probe(TraceProbeArgs a) {
  __shared__ MipEntry mips[VKR_MAX_MIPS];
  if ((int)threadIdx.x < a.pdepth.mips) {
    const Tex& t = a.pdepth.mip[threadIdx.x];
    mips[threadIdx.x] = MipEntry{t.p, a.pdepth.stride[threadIdx.x], t.pitch, t.w, t.h};
  }
  __syncthreads();
  const int x = blockIdx.x * 8 + (threadIdx.x & 7), y = blockIdx.y * 8 + (threadIdx.x >> 3);
  if (x >= a.tex_w || y >= a.tex_h) return;
  uint32_t* dst = texel_ptr<uint32_t>(a.out, x, y);
  const f2 uv = mk2((float)x / (float)a.tex_w, (float)y / (float)a.tex_h);
  const float pixel_depth = sample<FmtD24>(a.depth, uv);
  if (pixel_depth >= 1.0f) { *dst = 0u; return; }
  const f3 view_vec = reconstruct_view_vec(uv, pixel_depth, a.pr);
  const f3 N = decode_normal(sample<FmtRG16U>(a.normal, uv));
  f3 world_pos = xyz(mul(a.inverse_view, mk4(view_vec.x, view_vec.y, view_vec.z, 1.0f)));
  world_pos = madd(world_pos, 1e-6f, N);
  const f3 camera_pos = xyz(mul(a.inverse_view, mk4(0.0f, 0.0f, 0.0f, 1.0f)));
  const f3 V = normalize(world_pos - camera_pos);
  world_pos = madd(world_pos, -1e-6f, V);
  const f3 R = reflect(V, N);

  // get_start_probe_index (:326-332)
  const float cx = vclamp((world_pos.x - a.probe_min.x) / a.probe_step.x, 0.0f, (float)(a.grid - 2));
  const float cz = vclamp((world_pos.z - a.probe_min.z) / a.probe_step.z, 0.0f, (float)(a.grid - 2));
  const int bx = (int)floorf(cx), by = (int)floorf(cz);
  // trace (:410-441)
  const float tmax = 30.0f;
  float tmin = 0.0f;
  int i = 0, result = PROBE_UNKNOWN, probe = 0;
  f2 hit = mk2(0.0f, 0.0f);
#pragma unroll 1
  for (int left = 4; left > 0; left--) {
    probe = (by + ((i >> 1) & 1)) * a.grid + bx + (i & 1);
    result = trace_one_probe(a, mips, world_pos, R, probe, tmin, tmax, hit);
    if (result != PROBE_UNKNOWN) break;
    i = (i + 3) & 3;
  }
  *dst = result == PROBE_HIT ? probe_color_sample(a, hit, probe) : 0u;
}

}  // namespace vkr

using namespace vkr;

static int check_single(const Tex& t, const char* what) { return require_whole_frame(t, what, "windows are not supported (single-GPU pass)"); }

extern "C" int vkr_cube2oct(const vkr_img* cube_color, const vkr_img* cube_distance, const vkr_img* oct_color, const vkr_img* oct_depth,
                            void* stream) {
  if (!cube_color || !cube_distance) { set_error("cube2oct: NULL cube"); return VKR_ERR_NULL; }
  Cube2OctArgs a;
  for (int f = 0; f < 6; f++) {
    VKR_TRY(make_tex(&cube_color[f], 0, VKR_FMT_RGBA8_SRGB, "cube2oct.cube_color", &a.color[f]));
    VKR_TRY(make_tex(&cube_distance[f], 0, VKR_FMT_R16_SFLOAT, "cube2oct.cube_distance", &a.distance[f]));
    VKR_TRY(check_single(a.color[f], "cube2oct.cube_color"));
    VKR_TRY(check_single(a.distance[f], "cube2oct.cube_distance"));
    if (a.color[f].w != a.color[f].h || a.color[f].w != a.color[0].w || !same_window(a.distance[f], a.color[f])) {
      set_error("cube2oct: the 6 faces of both cubes must share one square extent");
      return VKR_ERR_EXTENT;
    }
  }
  VKR_TRY(make_tex(oct_color, 0, VKR_FMT_RGBA8_UNORM, "cube2oct.oct_color", &a.oct_color));
  VKR_TRY(make_tex(oct_depth, 0, VKR_FMT_R16_UNORM, "cube2oct.oct_depth", &a.oct_depth));
  VKR_TRY(check_single(a.oct_color, "cube2oct.oct_color"));
  if (!same_window(a.oct_color, a.oct_depth)) { set_error("cube2oct: oct_color and oct_depth differ in extent"); return VKR_ERR_EXTENT; }
  a.tex_w = floor_dispatch_w(a.oct_color);  // (check_single: the window is the whole image)
  a.tex_h = floor_dispatch_h(a.oct_color);
  if (a.tex_w == 0 || a.tex_h == 0) return VKR_OK;
  hipLaunchKernelGGL(k_cube2oct, dim3((a.tex_w + 7) / 8, (a.tex_h + 7) / 8), dim3(64), 0, (hipStream_t)stream, a);
  return launch_status("cube2oct");
}

extern "C" int vkr_probe_downsample(const vkr_img* depth, void* stream) {
  if (!depth || !depth->base) { set_error("probe_downsample: NULL image"); return VKR_ERR_NULL; }
  Tex src;
  VKR_TRY(make_tex(depth, 0, VKR_FMT_R16_UNORM, "probe_downsample.depth", &src));
  VKR_TRY(check_single(src, "probe_downsample.depth"));
  for (uint32_t m = 1; m < depth->mip_count; m++) {
    Tex dst;
    VKR_TRY(make_tex(depth, (int)m, VKR_FMT_R16_UNORM, "probe_downsample.depth", &dst));
    // the reference's render target is desc.width >> m (probe_renderer.cpp:226); the mip extents of the view are that
    if (dst.w != (int)(depth->width >> m) || dst.h != (int)(depth->height >> m)) {
      set_error("probe_downsample: mip %u is %dx%d, expected %ux%u", m, dst.w, dst.h, depth->width >> m, depth->height >> m);
      return VKR_ERR_MIPS;
    }
    hipLaunchKernelGGL(k_probe_downsample, dim3((dst.w + 7) / 8, (dst.h + 7) / 8), dim3(64), 0, (hipStream_t)stream, src, dst);
    VKR_TRY(launch_status("probe_downsample"));
    src = dst;
  }
  return VKR_OK;
}

extern "C" int vkr_trace_probe(const vkr_img* depth, const vkr_img* normal, const vkr_img* color_layers, const vkr_img* depth_layers,
                               uint32_t layer_count, const vkr_probe_trace_consts* consts, const vkr_img* out, void* stream) {
  if (!consts) { set_error("trace_probe: NULL constants"); return VKR_ERR_NULL; }
  if (consts->grid_size < 2 || consts->grid_size > 4096) { set_error("trace_probe: grid_size %u, needs 2..4096", consts->grid_size); return VKR_ERR_EXTENT; }
  if (layer_count < consts->grid_size * consts->grid_size) {
    set_error("trace_probe: %u array layers for a %u x %u grid", layer_count, consts->grid_size, consts->grid_size);
    return VKR_ERR_EXTENT;
  }
  TraceProbeArgs a;
  std::memset(&a, 0, sizeof(a));
  VKR_TRY(make_tex(depth, 0, VKR_FMT_D24_UNORM_S8, "trace_probe.depth", &a.depth));
  VKR_TRY(make_tex(normal, 0, VKR_FMT_RG16_UNORM, "trace_probe.normal", &a.normal));
  VKR_TRY(make_tex(out, 0, VKR_FMT_RGBA8_UNORM, "trace_probe.out", &a.out));
  VKR_TRY(check_single(a.depth, "trace_probe.depth"));
  VKR_TRY(check_single(a.normal, "trace_probe.normal"));
  VKR_TRY(check_single(a.out, "trace_probe.out"));
  if (!same_window(a.depth, a.out) || !same_window(a.normal, a.out)) { set_error("trace_probe: depth, normal and out differ in extent"); return VKR_ERR_EXTENT; }
  if (!color_layers || !depth_layers) { set_error("trace_probe: NULL probe arrays"); return VKR_ERR_NULL; }
  VKR_TRY(make_layer_array(color_layers, layer_count, VKR_FMT_RGBA8_UNORM, 1, "trace_probe.probe_color", &a.color));
  VKR_TRY(make_layer_array(depth_layers, layer_count, VKR_FMT_R16_UNORM, (int)depth_layers[0].mip_count, "trace_probe.probe_depth", &a.pdepth));
  if (!same_window(a.color.mip[0], a.pdepth.mip[0])) { set_error("trace_probe: probe colour and depth arrays differ in extent"); return VKR_ERR_EXTENT; }
  load_mat(a.inverse_view, consts->inverse_view);
  a.grid = (int)consts->grid_size;
  const float gm1 = (float)(consts->grid_size - 1);
  a.probe_min.x = consts->probe_min[0]; a.probe_min.y = consts->probe_min[1]; a.probe_min.z = consts->probe_min[2];
  // probe_step = (probe_max - probe_min) / float(grid_size - 1), evaluated once for the frame
  a.probe_step.x = (consts->probe_max[0] - consts->probe_min[0]) / gm1;
  a.probe_step.y = (consts->probe_max[1] - consts->probe_min[1]) / gm1;
  a.probe_step.z = (consts->probe_max[2] - consts->probe_min[2]) / gm1;
  load_proj(a.pr, consts->fovy, consts->aspect, consts->znear, consts->zfar);
  a.tex_w = floor_dispatch_w(a.out);
  a.tex_h = floor_dispatch_h(a.out);
  if (a.tex_w == 0 || a.tex_h == 0) return VKR_OK;
  hipLaunchKernelGGL(k_trace_probe, dim3((a.tex_w + 7) / 8, (a.tex_h + 7) / 8), dim3(64), 0, (hipStream_t)stream, a);
  return launch_status("trace_probe");
}
