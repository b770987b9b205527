// raster.hip — program "gbuf_opaque_taa": the G-buffer raster stage of the reference
// (SceneRenderer::draw_taa, scene_renderer.cpp:140-220 + shaders/gbuf/opaque_taa.{vert,frag}) as a
// compute rasterizer.
//
//   k_raster_clear    visibility buffer := empty
//   k_raster_setup    one thread per triangle: vertex shader on its three corners, near-plane clip (up to
//                     two sub-triangles), 8-bit sub-pixel snap, orientation -> ScreenTri records in scratch
//                     in scratch; records whose bounding box exceeds 64 blocks of 8x8 pixels go to a work list
//   k_raster_small    one wave per triangle walks the (<= 64) blocks of its bounding box, one pixel per lane
//   k_raster_large    the listed triangles, their bounding boxes cut into chunks of 16 blocks that are dealt to all
//                     waves of the launch (a screen-filling quad does not serialise on a few waves)
//                     both: walk_blocks() of raster_common.hpp — fill rule on exact 64-bit edge functions of 24.8
//                     coordinates, D24 depth; the fragment is the alpha test and the atomicMin
//                     of (depth << 32 | ~record) — LESS_OR_EQUAL with later triangles winning ties
//                     (gpu/pipelines.hpp:128)
//   k_raster_resolve  one thread per pixel: the winning triangle's record, perspective-correct attributes,
//                     implicit LOD from forward differences, trilinear sRGB fetches, stores
//
// opaque_taa.frag:32-34 discards a fragment whose albedo alpha is 0: it then writes neither depth nor any
// attachment.  A visibility buffer commits coverage before shading, so the discard is evaluated at coverage
// time: for draws with an albedo texture the covering lane computes the fragment's uv, its forward-difference
// LOD and the filtered alpha (the very expression the resolve evaluates again) and skips the atomicMin when
// it is 0.  A caller that knows a texture has no alpha-0 texel in any mip level sets
// VKR_RASTER_DRAW_OPAQUE_ALBEDO on the draw and the test is skipped (the result cannot differ).
//
// Coverage and depth are integer-exact functions of the snapped vertices, so they are bit-equal to
// the oracle's immediate-mode rasterizer; colour / normal / velocity follow the frozen fp32 contract.
#include "raster_common.hpp"

namespace vkr {

struct DrawDev {  // one draw call, matrices premultiplied on the host exactly as the vertex shader does
  Mat4 mvp, prev_mvp, normal_mat;
  uint32_t albedo_index, mr_index, index_offset, vertex_offset;
  uint32_t tri_base, tri_count, alpha_test, pad1;  // alpha_test: the discard of opaque_taa.frag:32 can fire for this draw
};

struct RasterArgs {
  const vkr_raster_vertex* vertices;
  const uint32_t* indices;
  const DrawDev* draws;
  const Pyramid* tex;  // [RASTER_MAX_TEXTURES] in scratch
  uint32_t draw_count;
  unsigned long long* vis;
  struct ScreenTri* setup;  // [2 * total triangles]: sub-triangle records written by k_raster_setup
  int width, height;  // framebuffer = whole frame
  float jitter_x, jitter_y;
};

struct VsOut { f4 position, pos_after, pos_before; f3 normal; f2 uv; };

// opaque_taa.vert:35-45
VKR_DEV VsOut vertex_shader(const RasterArgs& a, const DrawDev& d, uint32_t index) {
  const vkr_raster_vertex v = a.vertices[d.vertex_offset + a.indices[d.index_offset + index]];
  VsOut o;
  o.normal = normalize(xyz(mul(d.normal_mat, mk4(v.norm[0], v.norm[1], v.norm[2], 0.0f))));
  o.uv = mk2(v.uv[0], v.uv[1]);
  const f4 out_vector = mul(d.mvp, mk4(v.pos[0], v.pos[1], v.pos[2], 1.0f));
  o.position = mk4(out_vector.x + out_vector.w * a.jitter_x, out_vector.y + out_vector.w * a.jitter_y, out_vector.z, out_vector.w);
  o.pos_after = out_vector;
  o.pos_before = mul(d.prev_mvp, mk4(v.pos[0], v.pos[1], v.pos[2], 1.0f));
  return o;
}

VKR_DEV VsOut vs_lerp(const VsOut& p, const VsOut& q, float t) {  // p + t (q - p), every output
  VsOut o;
#define L1(F) o.F = p.F + t * (q.F - p.F)
  L1(position.x); L1(position.y); L1(position.z); L1(position.w);
  L1(pos_after.x); L1(pos_after.y); L1(pos_after.z); L1(pos_after.w);
  L1(pos_before.x); L1(pos_before.y); L1(pos_before.z); L1(pos_before.w);
  L1(normal.x); L1(normal.y); L1(normal.z);
  L1(uv.x); L1(uv.y);
#undef L1
  return o;
}

// A triangle ready for rasterisation: snapped screen positions (8 sub-pixel bits), 1/w-space data
struct ScreenTri {
  int x[3], y[3];  // 24.8 fixed point, |v| <= 2^28 (guard band)
  float w[3], z[3];  // clip w and z / w
  long long area2;
  double inv_area2;  // 1.0 / (double)area2, once per triangle: every pixel's barycentrics multiply by it
  VsOut v[3];
  uint32_t alpha_tex;  // albedo texture whose filtered alpha decides the discard, 0xFFFFFFFF: no test
  bool valid;
};


// Vertex shader on the three corners + near-plane clip (z_clip >= 0) -> sub-triangle `sub` (0 or 1).
// Returns the number of sub-triangles the clipped polygon has (0, 1 or 2) in *count.
VKR_DEV ScreenTri setup_triangle(const RasterArgs& a, const DrawDev& d, uint32_t tri, int sub, int* count) {
  ScreenTri t;
  t.valid = false;
  t.alpha_tex = d.alpha_test ? d.albedo_index : 0xFFFFFFFFu;
  VsOut in[3], poly[4];
  for (int k = 0; k < 3; k++) in[k] = vertex_shader(a, d, 3u * tri + (uint32_t)k);
  int n = 0;
  for (int k = 0; k < 3; k++) {  // Sutherland-Hodgman against z >= 0
    const VsOut& p = in[k];
    const VsOut& q = in[(k + 1) % 3];
    const bool pin = p.position.z >= 0.0f, qin = q.position.z >= 0.0f;
    if (pin) poly[n++] = p;
    if (pin != qin) {
      // always interpolate from the inside vertex so both orientations of a shared edge agree
      const VsOut& s = pin ? p : q;
      const VsOut& e = pin ? q : p;
      poly[n++] = vs_lerp(s, e, s.position.z / (s.position.z - e.position.z));
    }
  }
  *count = n < 3 ? 0 : n - 2;
  if (sub >= *count) return t;
  t.v[0] = poly[0]; t.v[1] = poly[1 + sub]; t.v[2] = poly[2 + sub];
  for (int k = 0; k < 3; k++)
    if (!snap_vertex(t.v[k].position, a.width, a.height, &t.x[k], &t.y[k], &t.w[k], &t.z[k])) return t;
  t.area2 = edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
  if (t.area2 == 0) return t;
  if (t.area2 < 0) {  // cull none: both windings are drawn; normalise the orientation
    const VsOut tv = t.v[1]; t.v[1] = t.v[2]; t.v[2] = tv;
    int tl = t.x[1]; t.x[1] = t.x[2]; t.x[2] = tl;
    tl = t.y[1]; t.y[1] = t.y[2]; t.y[2] = tl;
    float tf = t.w[1]; t.w[1] = t.w[2]; t.w[2] = tf;
    tf = t.z[1]; t.z[1] = t.z[2]; t.z[2] = tf;
    t.area2 = -t.area2;
  }
  t.inv_area2 = 1.0 / (double)t.area2;
  t.valid = true;
  return t;
}

#define BARY(F) ((b[0] * t.v[0].F + b[1] * t.v[1].F) + b[2] * t.v[2].F)

__global__ void k_raster_clear(unsigned long long* vis, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) vis[i] = ~0ull;
}


// one thread per triangle; a large sub-triangle takes a list slot AND its range of chunks with one 64-bit atomicAdd on
// *large_state (entries << 32 | chunks), so the list is sorted by first_chunk
// (every draw of the frame in one launch: a draw of a few thousand triangles does not fill the chip on its own)
__global__ __launch_bounds__(256) void k_raster_setup(RasterArgs a, uint32_t total_tris, unsigned long long* large_state, LargeEntry* large_list) {
  const uint32_t gtri = blockIdx.x * blockDim.x + threadIdx.x;
  if (gtri >= total_tris) return;
  const DrawDev d = a.draws[draw_of(a.draws, a.draw_count, gtri)];
  const uint32_t tri = gtri - d.tri_base;
  for (int sub = 0; sub < 2; sub++) {
    int count;
    ScreenTri t = setup_triangle(a, d, tri, sub, &count);
    if (sub >= count) t.valid = false;
    const uint32_t rec = (d.tri_base + tri) * 2u + (uint32_t)sub;
    a.setup[rec] = t;
    int x0, y0, x1, y1;
    if (t.valid && tri_bbox(t, a.width, a.height, &x0, &y0, &x1, &y1)) {
      const int nb = bbox_blocks(x0, y0, x1, y1);
      if (nb > RASTER_SMALL_BLOCKS) {
        const uint32_t chunks = (uint32_t)(nb + RASTER_LARGE_CHUNK - 1) / RASTER_LARGE_CHUNK;
        const unsigned long long v = atomicAdd(large_state, (1ull << 32) | (unsigned long long)chunks);
        large_list[(uint32_t)(v >> 32)] = LargeEntry {rec, (uint32_t)v};
      }
    }
  }
}

// the fragment of record `rec` at a covered pixel
VKR_DEV auto raster_fragment(const RasterArgs& a, uint32_t rec) {
  const uint32_t alpha_tex = a.setup[rec].alpha_tex;
  return [&a, rec, alpha_tex](int px, int py, const float lambda[3], uint32_t d24) {
    if (alpha_tex != 0xFFFFFFFFu) {  // opaque_taa.frag:32-34: out_albedo.a == 0 -> discard (no depth, no colour)
      const ScreenTri& t = a.setup[rec];
      const FragUv f = fragment_uv(t, t.v[0].uv, t.v[1].uv, t.v[2].uv, px, py, lambda);
      // only alpha is used: the colour decodes fold away
      if (sample_trilinear(a.tex[alpha_tex], f.uv, f.ddx, f.ddy, (const float*)k_srgb_decode_bits).w == 0.0f) return;
    }
    atomicMin(&a.vis[(size_t)py * a.width + px], ((unsigned long long)d24 << 32) | (0xFFFFFFFFull - (unsigned long long)rec));
  };
}

// small triangles: one wave per triangle walks its (at most 64) blocks; a larger sub-triangle is left to k_raster_large
__global__ __launch_bounds__(COVER_BLOCK) void k_raster_small(RasterArgs a, uint32_t total_tris) {
  const uint32_t gtri = wave_index();
  const int lane = threadIdx.x & 63;
  if (gtri >= total_tris) return;
  for (uint32_t sub = 0; sub < 2; sub++) {
    const uint32_t rec = gtri * 2u + sub;
    if (!a.setup[rec].valid) continue;
    const CoverTri t(a.setup[rec]);
    walk_blocks(t, a.width, a.height, 0, INT_MAX, RASTER_SMALL_BLOCKS, lane, raster_fragment(a, rec));
  }
}

// large triangles: their bounding boxes are cut into chunks of RASTER_LARGE_CHUNK blocks, all chunks of all listed
// triangles are dealt round-robin to the waves of the launch (a screen-filling quad is 4096 chunks at 4K: every wave
// of the launch works on it, none serialises)
__global__ __launch_bounds__(COVER_BLOCK) void k_raster_large(RasterArgs a, const unsigned long long* large_state, const LargeEntry* large_list) {
  const unsigned long long st = *large_state;
  const uint32_t n = (uint32_t)(st >> 32), chunks = (uint32_t)st;
  const int lane = threadIdx.x & 63;
  for (uint32_t c = wave_index(); c < chunks; c += wave_count()) {
    const LargeEntry e = large_entry_of(large_list, n, c);
    const CoverTri t(a.setup[e.rec]);
    walk_blocks(t, a.width, a.height, (int)(c - e.first_chunk) * RASTER_LARGE_CHUNK, RASTER_LARGE_CHUNK, INT_MAX, lane, raster_fragment(a, e.rec));
  }
}

struct ResolveArgs {
  RasterArgs r;
  Tex albedo, normal, material, velocity, depth;
};

__global__ __launch_bounds__(256) void k_raster_resolve(ResolveArgs a) {
  __shared__ float s_lut[VKR_SRGB_LUT_SIZE], s_thresh[VKR_SRGB_LUT_SIZE];
  srgb_lut_stage(s_lut, threadIdx.y * blockDim.x + threadIdx.x, 256);
  srgb_thresh_stage(s_thresh, threadIdx.y * blockDim.x + threadIdx.x, 256);
  __syncthreads();
  const int lx = blockIdx.x * blockDim.x + threadIdx.x;
  const int ly = blockIdx.y * blockDim.y + threadIdx.y;
  if (lx >= a.albedo.w || ly >= a.albedo.h) return;
  const int px = a.albedo.ox + lx, py = a.albedo.oy + ly;
  const unsigned long long key = a.r.vis[(size_t)py * a.r.width + px];
  uint32_t o_albedo = 0u, o_normal = 0u, o_material = 0u, o_velocity = 0u, o_depth = 0x00FFFFFFu;  // cleared attachments
  if (key != ~0ull) {
    const uint32_t gid2 = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull);
    const uint32_t gid = gid2 >> 1;
    const DrawDev& d = a.r.draws[draw_of(a.r.draws, a.r.draw_count, gid)];
    const ScreenTri& t = a.r.setup[gid2];
    float lambda[3];
    uint32_t d24 = 0;
    cover(t, px, py, lambda, &d24);
    const FragUv fu = fragment_uv(t, t.v[0].uv, t.v[1].uv, t.v[2].uv, px, py, lambda);
    const float* b = fu.b;
    const f3 in_normal = mk3(BARY(normal.x), BARY(normal.y), BARY(normal.z));
    const f2 in_uv = fu.uv;
    const f4 pa = mk4(BARY(pos_after.x), BARY(pos_after.y), BARY(pos_after.z), BARY(pos_after.w));
    const f4 pb = mk4(BARY(pos_before.x), BARY(pos_before.y), BARY(pos_before.z), BARY(pos_before.w));
    const f2 ddx = fu.ddx, ddy = fu.ddy;
    // opaque_taa.frag:26-46
    f4 out_albedo = mk4(0.5f, 0.5f, 0.5f, 1.0f);
    if (d.albedo_index != 0xFFFFFFFFu) out_albedo = sample_trilinear(a.r.tex[d.albedo_index], in_uv, ddx, ddy, s_lut);
    f4 out_material = mk4(0.5f, 0.9f, 0.5f, 0.5f);
    if (d.mr_index != 0xFFFFFFFFu) out_material = sample_trilinear(a.r.tex[d.mr_index], in_uv, ddx, ddy, s_lut);
    const f2 en = encode_normal(in_normal);
    const f2 vel = mk2(0.5f * (pb.x / pb.w - pa.x / pa.w), 0.5f * (pb.y / pb.w - pa.y / pa.w));
    o_albedo = pack_srgb8(out_albedo, s_thresh);
    o_material = pack_srgb8(out_material, s_thresh);
    o_normal = float_to_unorm16(en.x) | (float_to_unorm16(en.y) << 16);
    o_velocity = pack_half2(vel.x, vel.y);
    o_depth = (uint32_t)(key >> 32);
  }
  *texel_ptr<uint32_t>(a.albedo, lx, ly) = o_albedo;
  *texel_ptr<uint32_t>(a.normal, lx, ly) = o_normal;
  *texel_ptr<uint32_t>(a.material, lx, ly) = o_material;
  *texel_ptr<uint32_t>(a.velocity, lx, ly) = o_velocity;
  *texel_ptr<uint32_t>(a.depth, lx, ly) = o_depth;
}


}  // namespace vkr

using namespace vkr;


#define RASTER_MAX_DRAWS 1024u

struct RasterLayout {  // offsets of the parts of the scratch, and its size
  uint64_t vis, draws, tex, setup, large_state, large_list, total;
  RasterLayout(uint32_t width, uint32_t height, uint32_t triangle_count) {
    ScratchCarver c;
    vis = c.take((uint64_t)width * height * 8u);
    draws = c.take(sizeof(DrawDev) * RASTER_MAX_DRAWS);
    tex = c.take(sizeof(Pyramid) * RASTER_MAX_TEXTURES);
    setup = c.take(sizeof(ScreenTri) * 2u * (uint64_t)triangle_count);
    large_state = c.take(256);
    large_list = c.take(sizeof(LargeEntry) * 2u * (uint64_t)triangle_count);
    total = c.at;
  }
};

extern "C" uint64_t vkr_raster_scratch_bytes(uint32_t width, uint32_t height, uint32_t triangle_count) {
  return RasterLayout(width, height, triangle_count).total;
}

extern "C" int vkr_raster_gbuffer(const vkr_raster_scene* scene, const vkr_gbuf_const* consts, const vkr_img* albedo,
                                  const vkr_img* normal, const vkr_img* material, const vkr_img* velocity, const vkr_img* depth,
                                  void* scratch, uint64_t scratch_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scene || !consts || !scratch) { set_error("gbuf_opaque_taa: NULL argument"); return VKR_ERR_NULL; }
  if (scene->draw_count > RASTER_MAX_DRAWS || scene->texture_count > RASTER_MAX_TEXTURES) {
    set_error("gbuf_opaque_taa: at most %u draws and %d textures", RASTER_MAX_DRAWS, RASTER_MAX_TEXTURES);
    return VKR_ERR_EXTENT;
  }
  ResolveArgs ra;
  VKR_TRY(make_tex(albedo, 0, VKR_FMT_RGBA8_SRGB, "gbuf_opaque_taa.albedo", &ra.albedo));
  VKR_TRY(make_tex(normal, 0, VKR_FMT_RG16_UNORM, "gbuf_opaque_taa.normal", &ra.normal));
  VKR_TRY(make_tex(material, 0, VKR_FMT_RGBA8_SRGB, "gbuf_opaque_taa.material", &ra.material));
  VKR_TRY(make_tex(velocity, 0, VKR_FMT_RG16_SFLOAT, "gbuf_opaque_taa.velocity", &ra.velocity));
  VKR_TRY(make_tex(depth, 0, VKR_FMT_D24_UNORM_S8, "gbuf_opaque_taa.depth", &ra.depth));
  if (!same_window(ra.albedo, ra.normal) || !same_window(ra.albedo, ra.material) || !same_window(ra.albedo, ra.velocity) ||
      !same_window(ra.albedo, ra.depth)) {
    set_error("gbuf_opaque_taa: attachments differ in extent");
    return VKR_ERR_EXTENT;
  }
  const int W = ra.albedo.fw, H = ra.albedo.fh;
  uint64_t total_tris = 0;
  VKR_TRY(check_scene("gbuf_opaque_taa", scene, true, &total_tris));
  if (total_tris >= 0x7FFFFFFFull) { set_error("gbuf_opaque_taa: too many triangles"); return VKR_ERR_EXTENT; }
  const RasterLayout lay((uint32_t)W, (uint32_t)H, (uint32_t)total_tris);
  if (scratch_bytes < lay.total) { set_error("gbuf_opaque_taa: scratch too small"); return VKR_ERR_EXTENT; }
  std::vector<Pyramid> tex;
  VKR_TRY(make_pyramids(scene, "gbuf_opaque_taa", &tex));
  // per-draw constants: view_projection * model exactly as opaque_taa.vert:39,44 multiplies them
  std::vector<DrawDev> draws(scene->draw_count);
  uint32_t tri_base = 0;
  for (uint32_t i = 0; i < scene->draw_count; i++) {
    const vkr_raster_draw& s = scene->draws[i];
    DrawDev& d = draws[i];
    mat_mul(d.mvp, consts->view_projection, scene->transforms[s.transform_index].model);
    mat_mul(d.prev_mvp, consts->prev_view_projection, scene->transforms[s.transform_index].model);
    load_mat(d.normal_mat, scene->transforms[s.transform_index].normal);
    d.albedo_index = s.albedo_index; d.mr_index = s.mr_index;
    d.index_offset = s.index_offset; d.vertex_offset = s.vertex_offset;
    d.tri_base = tri_base; d.tri_count = s.index_count / 3u;
    d.alpha_test = (s.albedo_index != 0xFFFFFFFFu && !(s.reserved & VKR_RASTER_DRAW_OPAQUE_ALBEDO)) ? 1u : 0u;
    d.pad1 = 0;
    tri_base += d.tri_count;
  }
  RasterArgs r;
  r.vertices = scene->vertices; r.indices = scene->indices;
  uint8_t* const at = (uint8_t*)scratch;
  r.vis = (unsigned long long*)(at + lay.vis);
  r.draws = (const DrawDev*)(at + lay.draws);
  r.tex = (const Pyramid*)(at + lay.tex);
  r.setup = (ScreenTri*)(at + lay.setup);
  unsigned long long* large_state = (unsigned long long*)(at + lay.large_state);
  LargeEntry* large_list = (LargeEntry*)(at + lay.large_list);
  r.draw_count = scene->draw_count;
  r.width = W; r.height = H;
  r.jitter_x = consts->jitter[0]; r.jitter_y = consts->jitter[1];
  store_table<8>(draws, r.draws, stream);
  store_table<4>(tex, r.tex, stream);
  const size_t npx = (size_t)W * H;
  hipLaunchKernelGGL(k_raster_clear, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, stream, r.vis, npx);
  {
    hipError_t e = hipMemsetAsync(large_state, 0, 256, stream);
    if (e != hipSuccess) { set_error("gbuf_opaque_taa: %s", hipGetErrorString(e)); return (int)e; }
  }
  if (tri_base) {
    hipLaunchKernelGGL(k_raster_setup, dim3((tri_base + 255) / 256), dim3(256), 0, stream, r, tri_base, large_state, large_list);
    hipLaunchKernelGGL(k_raster_small, dim3((tri_base + COVER_BLOCK_WAVES - 1) / COVER_BLOCK_WAVES), dim3(COVER_BLOCK), 0, stream, r, tri_base);
  }
  // every draw's large triangles in one launch: submission order is carried by the record index in the key
  hipLaunchKernelGGL(k_raster_large, dim3(RASTER_LARGE_GRID), dim3(COVER_BLOCK), 0, stream, r, large_state, large_list);
  ra.r = r;
  dim3 block(64, 4);
  hipLaunchKernelGGL(k_raster_resolve, grid2d(ra.albedo.w, ra.albedo.h, block), block, 0, stream, ra);
  return launch_status("gbuf_opaque_taa");
}
