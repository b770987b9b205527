// cubemap.hip — program "cubemap_probe": the cube-face bake of the probe renderer (ProbeRenderer::render_cubemap / render_side,
// probe_renderer.cpp:72-160 + shaders/cubemap_probe/shader.{vert,frag}) as a compute rasteriser over the frozen raster rules of
// raster_common.hpp.  All six faces of one probe go through ONE set of launches: the face is the third dimension of the
// visibility buffer and of the resolve grid, and setup runs per (triangle, face).
//
//   k_cubemap_clear    visibility buffer [6][size][size] := empty
//   k_cubemap_setup    one thread per (triangle, face): vertex shader on the three corners (view_pos = (camera model) pos,
//                      clip = projection view_pos), frustum rejection, near-plane clip (up to two sub-triangles), snap,
//                      orientation -> CubeTri records (128 B: snapped positions, z / w, w, uv, view-space position).  A triangle
//                      whose three corners lie outside one side plane or the near plane of the face writes nothing and is
//                      listed nowhere: the raster kernels never see it.  A surviving record goes to the small list (bounding
//                      box of at most 64 blocks of 8x8 texels) or to the large list (chunks of 16 blocks).
//   k_cubemap_small    the waves of the launch walk the small list, one record per wave at a time, one texel per lane
//   k_cubemap_large    the chunks of the large list, dealt round-robin to all waves (a wall that fills a face is 16 chunks)
//                      both: walk_blocks() of raster_common.hpp; the fragment is the alpha test and the atomicMin of
//                      (D24 << 32 | ~submission index) into the face's slice
//   k_cubemap_resolve  one thread per (texel, face): the winning record, perspective-correct uv and view-space position,
//                      implicit LOD from forward differences, the trilinear sRGB albedo -> RGBA8_SRGB, length(view_pos) -> fp16
//
// shader.frag discards a fragment whose albedo alpha is 0; as in raster.hip the discard is evaluated at coverage time (the very
// expression the resolve evaluates again) and skipped for draws that carry VKR_RASTER_DRAW_OPAQUE_ALBEDO.  A draw without an
// albedo texture is not drawn at all (probe_renderer.cpp:136-138).
#define VKR_FORCE_GLM_COMPAT  // lookAt / perspective of the host mirror, the same code on every machine
#include "../host/glm_compat.hpp"
#include "raster_common.hpp"

namespace vkr {

struct CubeDraw {  // one drawn draw call; view_model[f] = camera(f) * model, multiplied on the host as shader.vert associates it
  Mat4 view_model[6];
  uint32_t albedo_index, index_offset, vertex_offset, tri_base, tri_count, alpha_test, pad0, pad1;
};

// A sub-triangle of one face, ready for rasterisation
struct CubeTri {
  int x[3], y[3];  // 24.8 fixed point
  float z[3], w[3];  // z / w and clip w
  double inv_area2;
  f2 uv[3];
  f3 vp[3];  // view-space position (out_pos of shader.vert)
  uint32_t albedo, alpha_tex;  // texture of the colour; texture whose filtered alpha decides the discard, 0xFFFFFFFF: no test
};
static_assert(sizeof(CubeTri) == 128, "CubeTri is two 64-byte lines");

struct CubeArgs {
  const vkr_raster_vertex* vertices;
  const uint32_t* indices;
  const CubeDraw* draws;
  const Pyramid* tex;  // [RASTER_MAX_TEXTURES]
  unsigned long long* vis;  // [6][size][size]
  CubeTri* setup;  // [6][2 * total triangles], only the valid records are ever written or read
  uint32_t* small_list;  // record indices (face * 2 * total + 2 * triangle + sub)
  LargeEntry* large_list;
  unsigned long long* state;  // [0] large: entries << 32 | chunks, [1] small: entries
  Mat4 projection;
  uint32_t draw_count, total_tris;
  int size;
};

// the vertex shader's outputs as the floats clip_near() interpolates: clip position, view-space position, uv
enum { CV_X, CV_Y, CV_Z, CV_W, CV_VX, CV_VY, CV_VZ, CV_U, CV_V, CV_N };

__global__ void k_cubemap_clear(unsigned long long* vis, size_t n, unsigned long long* state) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) vis[i] = ~0ull;
  if (i < 2) state[i] = 0ull;
}

// one thread per (triangle, face = blockIdx.y)
__global__ __launch_bounds__(256) void k_cubemap_setup(CubeArgs a) {
  const uint32_t gtri = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t face = blockIdx.y;
  if (gtri >= a.total_tris) return;
  const CubeDraw& d = a.draws[draw_of(a.draws, a.draw_count, gtri)];
  const uint32_t tri = gtri - d.tri_base;
  float in[3][CV_N], poly[4][CV_N];
  uint32_t out_mask = 0x1Fu;  // planes every corner so far lies outside of: x < -w, x > w, y < -w, y > w, z < 0
#pragma unroll
  for (int k = 0; k < 3; k++) {  // shader.vert:33-38
    const vkr_raster_vertex v = a.vertices[d.vertex_offset + a.indices[d.index_offset + 3u * tri + (uint32_t)k]];
    const f4 view_pos = mul(d.view_model[face], mk4(v.pos[0], v.pos[1], v.pos[2], 1.0f));
    const f4 p = mul(a.projection, view_pos);
    in[k][CV_X] = p.x; in[k][CV_Y] = p.y; in[k][CV_Z] = p.z; in[k][CV_W] = p.w;
    in[k][CV_VX] = view_pos.x; in[k][CV_VY] = view_pos.y; in[k][CV_VZ] = view_pos.z;
    in[k][CV_U] = v.uv[0]; in[k][CV_V] = v.uv[1];
    out_mask &= frustum_out_mask(p);
  }
  if (out_mask) return;  // wholly outside the face's frustum: no texel centre of the face can be covered
  const int n = clip_near<CV_N, CV_Z>(in, poly);
  const uint32_t alpha_tex = d.alpha_test ? d.albedo_index : 0xFFFFFFFFu;
  // the fan of the clipped polygon: (0, 1, 2) and, for a quad, (0, 2, 3); constant indices keep the polygon in registers
  auto emit = [&](const float (&c0)[CV_N], const float (&c1)[CV_N], const float (&c2)[CV_N], uint32_t sub) {
    CubeTri t;
    bool flip;
    const f4 p0 = mk4(c0[CV_X], c0[CV_Y], c0[CV_Z], c0[CV_W]), p1 = mk4(c1[CV_X], c1[CV_Y], c1[CV_Z], c1[CV_W]);
    const f4 p2 = mk4(c2[CV_X], c2[CV_Y], c2[CV_Z], c2[CV_W]);
    if (!snap_orient(p0, p1, p2, a.size, a.size, t.x, t.y, t.z, t.w, &t.inv_area2, &flip)) return;
    // (values first, then selects: a select between the two arrays' addresses would put the polygon in memory)
    const float u1 = c1[CV_U], v1 = c1[CV_V], u2 = c2[CV_U], v2 = c2[CV_V];
    const float x1 = c1[CV_VX], y1 = c1[CV_VY], z1 = c1[CV_VZ], x2 = c2[CV_VX], y2 = c2[CV_VY], z2 = c2[CV_VZ];
    t.uv[0] = mk2(c0[CV_U], c0[CV_V]);
    t.uv[1] = mk2(flip ? u2 : u1, flip ? v2 : v1);
    t.uv[2] = mk2(flip ? u1 : u2, flip ? v1 : v2);
    t.vp[0] = mk3(c0[CV_VX], c0[CV_VY], c0[CV_VZ]);
    t.vp[1] = mk3(flip ? x2 : x1, flip ? y2 : y1, flip ? z2 : z1);
    t.vp[2] = mk3(flip ? x1 : x2, flip ? y1 : y2, flip ? z1 : z2);
    t.albedo = d.albedo_index; t.alpha_tex = alpha_tex;
    int bx0, by0, bx1, by1;
    if (!tri_bbox(t, a.size, a.size, &bx0, &by0, &bx1, &by1)) return;  // no texel centre inside the bounding box
    const uint32_t rec = face * 2u * a.total_tris + gtri * 2u + sub;
    a.setup[rec] = t;
    list_append(rec, bbox_blocks(bx0, by0, bx1, by1), &a.state[0], a.large_list, &a.state[1], a.small_list);
  };
  if (n >= 3) emit(poly[0], poly[1], poly[2], 0u);
  if (n >= 4) emit(poly[0], poly[2], poly[3], 1u);
}

// the fragment of record `rec` at a covered texel
VKR_DEV auto cube_fragment(const CubeArgs& a, uint32_t rec) {
  const uint32_t alpha_tex = a.setup[rec].alpha_tex;
  return [&a, rec, alpha_tex](int px, int py, const float lambda[3], uint32_t d24) {
    if (alpha_tex != 0xFFFFFFFFu) {  // shader.frag:26-28: out_albedo.a == 0 -> discard (no depth, no colour, no distance)
      const CubeTri& t = a.setup[rec];
      const FragUv f = fragment_uv(t, t.uv[0], t.uv[1], t.uv[2], px, py, lambda);
      if (sample_trilinear(a.tex[alpha_tex], f.uv, f.ddx, f.ddy, (const float*)k_srgb_decode_bits).w == 0.0f) return;
    }
    const uint32_t per_face = 2u * a.total_tris;
    const uint32_t face = rec / per_face, order = rec - face * per_face;  // order: the submission index, later wins a depth tie
    atomicMin(&a.vis[((size_t)face * a.size + py) * a.size + px], ((unsigned long long)d24 << 32) | (0xFFFFFFFFull - (unsigned long long)order));
  };
}

__global__ __launch_bounds__(COVER_BLOCK) void k_cubemap_small(CubeArgs a) {
  const uint32_t n = (uint32_t)a.state[1];
  const int lane = threadIdx.x & 63;
  for (uint32_t i = wave_index(); i < n; i += wave_count()) {
    const uint32_t rec = a.small_list[i];
    const CoverTri t(a.setup[rec]);
    walk_blocks(t, a.size, a.size, 0, INT_MAX, INT_MAX, lane, cube_fragment(a, rec));
  }
}

__global__ __launch_bounds__(COVER_BLOCK) void k_cubemap_large(CubeArgs a) {
  const unsigned long long st = a.state[0];
  const uint32_t n = (uint32_t)(st >> 32), chunks = (uint32_t)st;
  const int lane = threadIdx.x & 63;
  for (uint32_t c = wave_index(); c < chunks; c += wave_count()) {
    const LargeEntry e = large_entry_of(a.large_list, n, c);
    const CoverTri t(a.setup[e.rec]);
    walk_blocks(t, a.size, a.size, (int)(c - e.first_chunk) * RASTER_LARGE_CHUNK, RASTER_LARGE_CHUNK, INT_MAX, lane, cube_fragment(a, e.rec));
  }
}

struct CubeResolveArgs {
  CubeArgs r;
  Tex color, distance;  // face 0; the six layers are a regular array (checked by the entry point)
  uint32_t color_stride, distance_stride;  // bytes between consecutive faces
};

#define CUBE_CLEAR_COLOR 0x000000FFu  // (100, 0, 0, 0) clamped to [0, 1]: codes (255, 0, 0, 0)
#define CUBE_CLEAR_DISTANCE 0x5640u   // 100.0 in fp16

// grid (x, y, face)
__global__ __launch_bounds__(256) void k_cubemap_resolve(CubeResolveArgs a) {
  __shared__ float s_lut[VKR_SRGB_LUT_SIZE], s_thresh[VKR_SRGB_LUT_SIZE];
  srgb_lut_stage(s_lut, threadIdx.y * blockDim.x + threadIdx.x, 256);
  srgb_thresh_stage(s_thresh, threadIdx.y * blockDim.x + threadIdx.x, 256);
  __syncthreads();
  const int px = blockIdx.x * blockDim.x + threadIdx.x;
  const int py = blockIdx.y * blockDim.y + threadIdx.y;
  const uint32_t face = blockIdx.z;
  if (px >= a.r.size || py >= a.r.size) return;
  const unsigned long long key = a.r.vis[((size_t)face * a.r.size + py) * a.r.size + px];
  uint32_t o_color = CUBE_CLEAR_COLOR, o_distance = CUBE_CLEAR_DISTANCE;
  if (key != ~0ull) {
    const uint32_t order = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull);
    const CubeTri& t = a.r.setup[face * 2u * a.r.total_tris + order];
    float lambda[3];
    uint32_t d24 = 0;
    cover(t, px, py, lambda, &d24);
    const FragUv fu = fragment_uv(t, t.uv[0], t.uv[1], t.uv[2], px, py, lambda);
    const float* b = fu.b;
    const f3 pos = mk3((b[0] * t.vp[0].x + b[1] * t.vp[1].x) + b[2] * t.vp[2].x, (b[0] * t.vp[0].y + b[1] * t.vp[1].y) + b[2] * t.vp[2].y,
                       (b[0] * t.vp[0].z + b[1] * t.vp[1].z) + b[2] * t.vp[2].z);
    // shader.frag:22-30
    const f4 out_albedo = sample_trilinear(a.r.tex[t.albedo], fu.uv, fu.ddx, fu.ddy, s_lut);
    o_color = pack_srgb8(out_albedo, s_thresh);
    o_distance = float_to_half_bits(length(pos));
  }
  Tex color = a.color, distance = a.distance;  // face is uniform over the block: scalar address arithmetic
  color.p += (size_t)face * a.color_stride;
  distance.p += (size_t)face * a.distance_stride;
  *texel_ptr<uint32_t>(color, px, py) = o_color;
  *texel_ptr<uint16_t>(distance, px, py) = (uint16_t)o_distance;
}

// calc_matrix, probe_renderer.cpp:56-70
static glm::mat4 cube_face_view(uint32_t side, glm::vec3 pos) {
  glm::vec3 fwd, up {0.f, -1.f, 0.f};
  switch (side) {
    case 0: fwd = glm::vec3 {1.f, 0.f, 0.f}; break;
    case 1: fwd = glm::vec3 {-1.f, 0.f, 0.f}; break;
    case 2: fwd = glm::vec3 {0.f, 1.f, 0.f}; up = glm::vec3 {0.f, 0.f, 1.f}; break;
    case 3: fwd = glm::vec3 {0.f, -1.f, 0.f}; up = glm::vec3 {0.f, 0.f, -1.f}; break;
    case 4: fwd = glm::vec3 {0.f, 0.f, 1.f}; break;
    default: fwd = glm::vec3 {0.f, 0.f, -1.f}; break;
  }
  return glm::lookAt(pos, pos + fwd, up);
}

}  // namespace vkr

using namespace vkr;

#define CUBE_MAX_DRAWS 1024u
#define CUBE_RASTER_GRID 1024  // blocks of four waves of the small and the large kernel

struct CubeLayout {  // offsets of the parts of the scratch, and its size
  uint64_t vis, draws, tex, setup, state, small_list, large_list, total;
  CubeLayout(uint32_t cube_size, uint32_t triangle_count) {
    const uint64_t recs = 12ull * triangle_count;  // 6 faces x 2 sub-triangles
    ScratchCarver c;
    vis = c.take(6ull * cube_size * cube_size * 8u);
    draws = c.take(sizeof(CubeDraw) * CUBE_MAX_DRAWS);
    tex = c.take(sizeof(Pyramid) * RASTER_MAX_TEXTURES);
    setup = c.take(sizeof(CubeTri) * recs);
    state = c.take(256);
    small_list = c.take(sizeof(uint32_t) * recs);
    large_list = c.take(sizeof(LargeEntry) * recs);
    total = c.at;
  }
};

extern "C" uint64_t vkr_cubemap_probe_scratch_bytes(uint32_t cube_size, uint32_t triangle_count) {
  return CubeLayout(cube_size, triangle_count).total;
}

extern "C" int vkr_cubemap_probe(const vkr_raster_scene* scene, const float pos[3], const vkr_img* cube_color, const vkr_img* cube_distance,
                                 void* scratch, uint64_t scratch_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scene || !pos || !scratch || !cube_color || !cube_distance) { set_error("cubemap_probe: NULL argument"); return VKR_ERR_NULL; }
  if (scene->draw_count > CUBE_MAX_DRAWS || scene->texture_count > RASTER_MAX_TEXTURES) {
    set_error("cubemap_probe: at most %u draws and %d textures", CUBE_MAX_DRAWS, RASTER_MAX_TEXTURES);
    return VKR_ERR_EXTENT;
  }
  CubeResolveArgs ra;
  Tex color[6], distance[6];
  for (int f = 0; f < 6; f++) {
    VKR_TRY(make_tex(&cube_color[f], 0, VKR_FMT_RGBA8_SRGB, "cubemap_probe.cube_color", &color[f]));
    VKR_TRY(make_tex(&cube_distance[f], 0, VKR_FMT_R16_SFLOAT, "cubemap_probe.cube_distance", &distance[f]));
    const Tex& c = color[f];
    VKR_TRY(require_whole_frame(c, "cubemap_probe", "windows are not supported (single-GPU pass)"));
    if (c.w != c.h || c.w != color[0].w || !same_window(distance[f], c)) {
      set_error("cubemap_probe: the 6 faces of both cubes must share one square extent");
      return VKR_ERR_EXTENT;
    }
  }
  // the six layers of a cube image are a regular array: one pitch, one stride between consecutive layers
  const ptrdiff_t cs = color[1].p - color[0].p, ds = distance[1].p - distance[0].p;
  for (int f = 1; f < 6; f++) {
    if (color[f].pitch != color[0].pitch || distance[f].pitch != distance[0].pitch || color[f].p - color[f - 1].p != cs ||
        distance[f].p - distance[f - 1].p != ds || cs < (ptrdiff_t)color[0].pitch * color[0].h || ds < (ptrdiff_t)distance[0].pitch * distance[0].h ||
        cs >= (ptrdiff_t)1 << 31 || ds >= (ptrdiff_t)1 << 31) {
      set_error("cubemap_probe: the layers of a cube are not a regular array (one pitch, one layer stride, no overlap)");
      return VKR_ERR_LAYOUT;
    }
  }
  ra.color = color[0]; ra.distance = distance[0];
  ra.color_stride = (uint32_t)cs; ra.distance_stride = (uint32_t)ds;
  const int S = color[0].w;
  std::vector<Pyramid> tex;
  VKR_TRY(make_pyramids(scene, "cubemap_probe", &tex));
  // scratch is sized by every triangle of the scene (what the caller knows); only draws with an albedo texture are drawn
  uint64_t scene_tris = 0;
  VKR_TRY(check_scene("cubemap_probe", scene, true, &scene_tris));
  if (scene_tris >= (1ull << 28)) { set_error("cubemap_probe: too many triangles"); return VKR_ERR_EXTENT; }
  const CubeLayout lay((uint32_t)S, (uint32_t)scene_tris);
  if (scratch_bytes < lay.total) { set_error("cubemap_probe: scratch too small"); return VKR_ERR_EXTENT; }
  const glm::mat4 proj = glm::perspective(glm::radians(90.f), 1.f, 0.05f, 80.f);
  vkr_mat4 views[6];
  for (uint32_t f = 0; f < 6; f++) {
    const glm::mat4 v = cube_face_view(f, glm::vec3 {pos[0], pos[1], pos[2]});
    std::memcpy(views[f].m, &v, sizeof(views[f].m));
  }
  std::vector<CubeDraw> draws;
  draws.reserve(scene->draw_count);
  uint32_t tri_base = 0;
  for (uint32_t i = 0; i < scene->draw_count; i++) {
    const vkr_raster_draw& s = scene->draws[i];
    if (s.albedo_index == 0xFFFFFFFFu || s.index_count < 3) continue;  // probe_renderer.cpp:136-138
    CubeDraw d;
    for (int f = 0; f < 6; f++) mat_mul(d.view_model[f], views[f], scene->transforms[s.transform_index].model);
    d.albedo_index = s.albedo_index; d.index_offset = s.index_offset; d.vertex_offset = s.vertex_offset;
    d.tri_base = tri_base; d.tri_count = s.index_count / 3u;
    d.alpha_test = (s.reserved & VKR_RASTER_DRAW_OPAQUE_ALBEDO) ? 0u : 1u;
    d.pad0 = d.pad1 = 0;
    tri_base += d.tri_count;
    draws.push_back(d);
  }
  CubeArgs r;
  r.vertices = scene->vertices; r.indices = scene->indices;
  uint8_t* const at = (uint8_t*)scratch;
  r.vis = (unsigned long long*)(at + lay.vis);
  r.draws = (const CubeDraw*)(at + lay.draws);
  r.tex = (const Pyramid*)(at + lay.tex);
  r.setup = (CubeTri*)(at + lay.setup);
  r.state = (unsigned long long*)(at + lay.state);
  r.small_list = (uint32_t*)(at + lay.small_list);
  r.large_list = (LargeEntry*)(at + lay.large_list);
  std::memcpy(r.projection.m, &proj, sizeof(r.projection.m));
  r.draw_count = (uint32_t)draws.size(); r.total_tris = tri_base; r.size = S;
  store_table<8>(draws, r.draws, stream);
  store_table<4>(tex, r.tex, stream);
  const size_t npx = 6u * (size_t)S * S;
  hipLaunchKernelGGL(k_cubemap_clear, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, stream, r.vis, npx, r.state);
  if (tri_base) {
    hipLaunchKernelGGL(k_cubemap_setup, dim3((tri_base + 255) / 256, 6), dim3(256), 0, stream, r);
    const uint64_t waves = 12ull * tri_base;  // one per record: 6 faces x 2 sub-triangles
    const uint64_t blocks = waves / COVER_BLOCK_WAVES + 1;
    const unsigned grid = (unsigned)(blocks < CUBE_RASTER_GRID ? blocks : CUBE_RASTER_GRID);
    hipLaunchKernelGGL(k_cubemap_small, dim3(grid), dim3(COVER_BLOCK), 0, stream, r);
    hipLaunchKernelGGL(k_cubemap_large, dim3(grid), dim3(COVER_BLOCK), 0, stream, r);
  }
  ra.r = r;
  dim3 block(64, 4);
  hipLaunchKernelGGL(k_cubemap_resolve, dim3((S + 63) / 64, (S + 3) / 4, 6), block, 0, stream, ra);
  return launch_status("cubemap_probe");
}
