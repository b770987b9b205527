// shadow.hip — program "default_shadow": the shadow-map pass of the scene renderer (SceneRenderer::render_shadow,
// scene_renderer.cpp:222-274 + shaders/shadows/default.{vert,frag}) as a depth-only compute rasteriser over the frozen raster
// rules of raster_common.hpp.  default.vert is gl_Position = mvp * model * vec4(pos, 1) (opaque_taa.vert:39 without jitter),
// default.frag is empty: every covered fragment writes its depth, a cutout casts a solid shadow.
//
// Depth has no attributes and a depth tie stores the same word whichever triangle wins, so there is no visibility buffer and
// no resolve: coverage issues a 32-bit no-return atomicMin straight into the D24S8 layer (stencil byte 0, so the word IS the
// 24-bit depth and unsigned min is LESS_OR_EQUAL).  All layers of one call go through ONE set of launches, the layer is a
// dimension of every grid, and each layer has its own lists.
//
//   k_store_table          per-(layer, draw) constants (mvp = light matrix * model, multiplied on the host) -> scratch
//   k_shadow_clear        grid (texels, layer): every texel of the layer := 0x00FFFFFF (depth 1, stencil 0); list counters := 0
//   k_shadow_setup        one thread per (triangle, layer): vertex shader on the three corners, frustum rejection, near-plane
//                         clip (up to two sub-triangles), snap, orientation -> ShadowTri records (48 B: snapped positions, z / w,
//                         1 / area).  A triangle whose three corners lie outside one side plane or the near plane of the layer's
//                         frustum writes nothing and is listed nowhere.  A surviving record goes to the layer's small list
//                         (bounding box of at most 64 blocks of 8x8 texels) or to its large list (chunks of 16 blocks).
//   k_shadow_small        grid (waves, layer): the waves walk the layer's small list, one record per wave at a time
//   k_shadow_large        grid (waves, layer): the chunks of the layer's large list, dealt round-robin to the waves
//                         both: walk_blocks() of raster_common.hpp, the fragment is the atomicMin of the D24 word
#include "raster_common.hpp"

namespace vkr {

#define SHADOW_MAX_LAYERS 8u
#define SHADOW_MAX_DRAWS 1024u
#define SHADOW_RASTER_GRID 2048u  // blocks of four waves per layer of the small and the large kernel: 8 waves on every SIMD of 256 CUs

struct ShadowDraw {  // one draw call seen from one light; mvp = light * model, multiplied on the host as default.vert associates it
  Mat4 mvp;
  uint32_t index_offset, vertex_offset, tri_base, tri_count;
};
static_assert(sizeof(ShadowDraw) == 80, "ShadowDraw: 32 of them are one launch's arguments");

// A sub-triangle of one layer, ready for rasterisation: all that cover(), tri_bbox() and block_outside() read
struct ShadowTri {
  int x[3], y[3];  // 24.8 fixed point
  float z[3];      // z / w
  uint32_t pad;
  double inv_area2;
};
static_assert(sizeof(ShadowTri) == 48, "ShadowTri is three 16-byte loads");

struct ShadowLayer { uint8_t* p; int pitch, pad; };

struct ShadowArgs {
  const vkr_raster_vertex* vertices;
  const uint32_t* indices;
  const ShadowDraw* draws;         // [layer][draw_count]
  ShadowTri* setup;                // [layer][2 * total triangles], only the valid records are ever written or read
  uint32_t* small_list;            // [layer][2 * total triangles] record indices inside the layer (2 * triangle + sub)
  LargeEntry* large_list;          // [layer][2 * total triangles]
  unsigned long long* state;       // [layer][2]: large (entries << 32 | chunks), small (entries)
  ShadowLayer layer[SHADOW_MAX_LAYERS];
  uint32_t draw_count, total_tris, vertex_count;
  int size;
};

// grid (ceil(size * size / 256), layer)
__global__ __launch_bounds__(256) void k_shadow_clear(ShadowArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t layer = blockIdx.y;
  if (i < 2u) a.state[layer * 2u + i] = 0ull;
  const uint32_t px = i % (uint32_t)a.size, py = i / (uint32_t)a.size;
  if (py >= (uint32_t)a.size) return;
  const ShadowLayer L = a.layer[layer];
  ((uint32_t*)(L.p + (size_t)py * (size_t)L.pitch))[px] = 0x00FFFFFFu;
}

// clip position of default.vert as the floats clip_near() interpolates
enum { SV_X, SV_Y, SV_Z, SV_W, SV_N };

// grid (ceil(triangles / 256), layer)
__global__ __launch_bounds__(256) void k_shadow_setup(ShadowArgs a) {
  const uint32_t gtri = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t layer = blockIdx.y;
  if (gtri >= a.total_tris) return;
  const ShadowDraw* draws = a.draws + (size_t)layer * a.draw_count;
  const ShadowDraw& d = draws[draw_of(draws, a.draw_count, gtri)];
  const uint32_t tri = gtri - d.tri_base;
  float in[3][SV_N], poly[4][SV_N];
  uint32_t out_mask = 0x1Fu;  // planes every corner so far lies outside of: x < -w, x > w, y < -w, y > w, z < 0
#pragma unroll
  for (int k = 0; k < 3; k++) {  // default.vert
    const uint32_t vi = d.vertex_offset + a.indices[d.index_offset + 3u * tri + (uint32_t)k];
    if (vi >= a.vertex_count) return;  // an index outside the vertex buffer: the triangle is not drawn
    const vkr_raster_vertex v = a.vertices[vi];
    const f4 p = mul(d.mvp, mk4(v.pos[0], v.pos[1], v.pos[2], 1.0f));
    in[k][SV_X] = p.x; in[k][SV_Y] = p.y; in[k][SV_Z] = p.z; in[k][SV_W] = p.w;
    out_mask &= frustum_out_mask(p);
  }
  if (out_mask) return;  // wholly outside the layer's frustum: no texel centre can be covered
  const int n = clip_near<SV_N, SV_Z>(in, poly);
  const size_t per_layer = 2u * (size_t)a.total_tris;
  // the fan of the clipped polygon: (0, 1, 2) and, for a quad, (0, 2, 3); constant indices keep the polygon in registers
  auto emit = [&](const float (&c0)[SV_N], const float (&c1)[SV_N], const float (&c2)[SV_N], uint32_t sub) {
    ShadowTri t;
    float w[3];  // clip w: depth has no perspective-correct attribute to divide by it
    bool flip;   // and none to exchange with the corners
    const f4 p0 = mk4(c0[SV_X], c0[SV_Y], c0[SV_Z], c0[SV_W]), p1 = mk4(c1[SV_X], c1[SV_Y], c1[SV_Z], c1[SV_W]);
    const f4 p2 = mk4(c2[SV_X], c2[SV_Y], c2[SV_Z], c2[SV_W]);
    if (!snap_orient(p0, p1, p2, a.size, a.size, t.x, t.y, t.z, w, &t.inv_area2, &flip)) return;
    t.pad = 0u;
    int bx0, by0, bx1, by1;
    if (!tri_bbox(t, a.size, a.size, &bx0, &by0, &bx1, &by1)) return;  // no texel centre inside the bounding box
    const uint32_t rec = gtri * 2u + sub;
    a.setup[layer * per_layer + rec] = t;
    unsigned long long* state = a.state + layer * 2u;  // [0] large, [1] small
    list_append(rec, bbox_blocks(bx0, by0, bx1, by1), &state[0], a.large_list + layer * per_layer, &state[1], a.small_list + layer * per_layer);
  };
  if (n >= 3) emit(poly[0], poly[1], poly[2], 0u);
  if (n >= 4) emit(poly[0], poly[2], poly[3], 1u);
}

// the fragment of a covered texel of layer L: its depth
VKR_DEV auto shadow_fragment(const ShadowLayer& L) {
  return [&L](int px, int py, const float*, uint32_t d24) {
    uint32_t* texel = (uint32_t*)(L.p + (size_t)py * (size_t)L.pitch) + px;
    // No read of the texel first.  A plain (cacheable, possibly stale) load could skip the atomic when d24 >= loaded — a texel only
    // decreases during a call, so a stale value is >= the current one and the skip would be right — but the load's latency then
    // sits in every iteration of the wave's loop over its blocks, which a no-return atomic does not: measured 10 - 16 % slower on
    // the procedural scene.
    atomicMin(texel, d24);  // result unused: a no-return atomic.  A tie stores the same word, so LESS and LESS_OR_EQUAL agree
  };
}

__global__ __launch_bounds__(COVER_BLOCK) void k_shadow_small(ShadowArgs a) {
  const uint32_t layer = blockIdx.y;
  const size_t base = (size_t)layer * 2u * a.total_tris;
  const ShadowLayer L = a.layer[layer];
  const uint32_t n = (uint32_t)a.state[layer * 2u + 1u];
  const int lane = threadIdx.x & 63;
  for (uint32_t i = wave_index(); i < n; i += wave_count()) {
    const CoverTri t(a.setup[base + a.small_list[base + i]]);
    walk_blocks(t, a.size, a.size, 0, INT_MAX, INT_MAX, lane, shadow_fragment(L));
  }
}

__global__ __launch_bounds__(COVER_BLOCK) void k_shadow_large(ShadowArgs a) {
  const uint32_t layer = blockIdx.y;
  const size_t base = (size_t)layer * 2u * a.total_tris;
  const ShadowLayer L = a.layer[layer];
  const unsigned long long st = a.state[layer * 2u];
  const uint32_t n = (uint32_t)(st >> 32), chunks = (uint32_t)st;
  const int lane = threadIdx.x & 63;
  for (uint32_t c = wave_index(); c < chunks; c += wave_count()) {
    const LargeEntry e = large_entry_of(a.large_list + base, n, c);
    const CoverTri t(a.setup[base + e.rec]);
    walk_blocks(t, a.size, a.size, (int)(c - e.first_chunk) * RASTER_LARGE_CHUNK, RASTER_LARGE_CHUNK, INT_MAX, lane, shadow_fragment(L));
  }
}

}  // namespace vkr

using namespace vkr;

struct ShadowLayout {  // offsets of the parts of the scratch, and its size
  uint64_t draws, state, setup, small_list, large_list, total;
  ShadowLayout(uint32_t layer_count, uint32_t triangle_count) {
    const uint64_t recs = 2ull * layer_count * triangle_count;
    ScratchCarver c;
    draws = c.take(sizeof(ShadowDraw) * SHADOW_MAX_DRAWS * (uint64_t)layer_count);
    state = c.take(256);
    setup = c.take(sizeof(ShadowTri) * recs);
    small_list = c.take(sizeof(uint32_t) * recs);
    large_list = c.take(sizeof(LargeEntry) * recs);
    total = c.at;
  }
};

// (`size` takes no part today: the pass has no per-texel scratch.  It stays in the signature so that a caller sizes this pass
// as it sizes the other rasterisers.)
extern "C" uint64_t vkr_default_shadow_scratch_bytes(uint32_t size, uint32_t layer_count, uint32_t triangle_count) {
  (void)size;
  return ShadowLayout(layer_count, triangle_count).total;
}

extern "C" int vkr_default_shadow(const vkr_raster_scene* scene, const vkr_mat4* mvps, const vkr_img* layers, uint32_t layer_count,
                                  void* scratch, uint64_t scratch_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scene) { set_error("default_shadow: scene is NULL"); return VKR_ERR_NULL; }
  if (!mvps) { set_error("default_shadow: mvps is NULL"); return VKR_ERR_NULL; }
  if (!layers) { set_error("default_shadow: layers is NULL"); return VKR_ERR_NULL; }
  if (!scratch) { set_error("default_shadow: scratch is NULL"); return VKR_ERR_NULL; }
  if (layer_count < 1 || layer_count > SHADOW_MAX_LAYERS) { set_error("default_shadow: layer_count %u, expected 1..%u", layer_count, SHADOW_MAX_LAYERS); return VKR_ERR_EXTENT; }
  if (scene->draw_count > SHADOW_MAX_DRAWS) { set_error("default_shadow: scene has %u draws, at most %u", scene->draw_count, SHADOW_MAX_DRAWS); return VKR_ERR_EXTENT; }
  ShadowArgs r;
  std::memset(&r, 0, sizeof(r));
  Tex first;
  for (uint32_t l = 0; l < layer_count; l++) {
    Tex t;
    VKR_TRY(make_tex(&layers[l], 0, VKR_FMT_D24_UNORM_S8, "default_shadow.layers", &t));
    VKR_TRY(require_whole_frame(t, "default_shadow: layers", "windows are not supported (single-GPU pass)"));
    if (l == 0) first = t;
    if (t.w != t.h || t.w != first.w) {
      set_error("default_shadow: layers: layer %u is %dx%d, every layer must be square and of one extent (layer 0: %dx%d)", l, t.w, t.h, first.w, first.h);
      return VKR_ERR_EXTENT;
    }
    r.layer[l].p = const_cast<uint8_t*>(t.p);
    r.layer[l].pitch = t.pitch;
  }
  const int S = first.w;
  uint64_t total_tris = 0;
  VKR_TRY(check_scene("default_shadow", scene, false, &total_tris));  // default.frag reads no texture
  if (total_tris * 2u * SHADOW_MAX_LAYERS >= (1ull << 31)) { set_error("default_shadow: scene: too many triangles"); return VKR_ERR_EXTENT; }
  const ShadowLayout lay(layer_count, (uint32_t)total_tris);
  const uint64_t need = lay.total;
  if (scratch_bytes < need) { set_error("default_shadow: scratch too small (%llu bytes, %llu needed)", (unsigned long long)scratch_bytes, (unsigned long long)need); return VKR_ERR_EXTENT; }
  // per-(layer, draw) constants: mvp * model exactly as default.vert multiplies them; draws without a triangle are left out
  std::vector<ShadowDraw> draws;
  uint32_t draw_count = 0;
  for (uint32_t l = 0; l < layer_count; l++) {
    uint32_t tri_base = 0;
    for (uint32_t i = 0; i < scene->draw_count; i++) {
      const vkr_raster_draw& s = scene->draws[i];
      if (s.index_count < 3) continue;
      ShadowDraw d;
      mat_mul(d.mvp, mvps[l], scene->transforms[s.transform_index].model);
      d.index_offset = s.index_offset; d.vertex_offset = s.vertex_offset;
      d.tri_base = tri_base; d.tri_count = s.index_count / 3u;
      tri_base += d.tri_count;
      draws.push_back(d);
    }
    if (l == 0) draw_count = (uint32_t)draws.size();
  }
  r.vertices = scene->vertices; r.indices = scene->indices;
  uint8_t* const at = (uint8_t*)scratch;
  r.draws = (const ShadowDraw*)(at + lay.draws);
  r.state = (unsigned long long*)(at + lay.state);
  r.setup = (ShadowTri*)(at + lay.setup);
  r.small_list = (uint32_t*)(at + lay.small_list);
  r.large_list = (LargeEntry*)(at + lay.large_list);
  r.draw_count = draw_count; r.total_tris = (uint32_t)total_tris; r.vertex_count = scene->vertex_count;
  r.size = S;
  store_table<32>(draws, r.draws, stream);
  const uint32_t npx = (uint32_t)S * (uint32_t)S;
  hipLaunchKernelGGL(k_shadow_clear, dim3((npx + 255u) / 256u, layer_count), dim3(256), 0, stream, r);
  if (total_tris && draw_count) {
    hipLaunchKernelGGL(k_shadow_setup, dim3(((uint32_t)total_tris + 255u) / 256u, layer_count), dim3(256), 0, stream, r);
    const uint64_t waves = 2ull * total_tris;
    const uint64_t blocks = waves / COVER_BLOCK_WAVES + 1;
    const unsigned grid = (unsigned)(blocks < SHADOW_RASTER_GRID ? blocks : SHADOW_RASTER_GRID);
    hipLaunchKernelGGL(k_shadow_small, dim3(grid, layer_count), dim3(COVER_BLOCK), 0, stream, r);
    hipLaunchKernelGGL(k_shadow_large, dim3(grid, layer_count), dim3(COVER_BLOCK), 0, stream, r);
  }
  return launch_status("default_shadow");
}
