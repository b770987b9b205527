// accel.hip — the scene's acceleration structure and the ray query: vkr_accel_layout / _create / _destroy / _info (host),
// vkr_accel_query and vkr_accel_occluded (any-hit of arbitrary rays, on the walk for short and for long rays) and program
// "gtao_rt_main" (gtao.cpp:150-196 + gtao/rt_main.frag).  The query itself — AccelView, the frozen triangle test, the walks and
// what the ray-level entries share — is accel_traverse.hpp.
//
// MI355X has no ray-tracing hardware, so the traversal is software.  The hierarchy is one level over world-space triangles
// (an any-hit query of a static scene gains nothing from instancing); it is built once per scene on the host (binned SAH,
// deterministic) and read-only for every query on the device.  accel_refit.hip moves it to new vertex positions under the same
// topology; the record rule it shares with the build here is accel_record.hpp.
//
// Traversal: a wave of 64 rays walks the hierarchy TOGETHER, with scalar loads of nodes and triangles and the node order on a
// per-wave stack in LDS (no private array: nothing goes to scratch).  gtao_rt_main runs one wave per pixel, one lane per
// direction: the 64 rays of a pixel share their origin and are 0.2 long, so the wave visits few nodes.  No cull of a walk can
// discard a triangle the frozen test would hit (the argument stands beside LaneRay in accel_traverse.hpp), so the result is
// that of a brute-force loop over all triangles (tests/test_accel_gpu.py).
#include "vkr_host.hpp"
#include "accel_traverse.hpp"
#include "accel_record.hpp"
#include "gtao_slice.hpp"

#include <algorithm>
#include <vector>

namespace vkr {

constexpr int ACCEL_BINS = 16;
constexpr uint32_t ACCEL_MAX_LEAF = 8;

// the two any-hit ray-level entries: ray i of the batch on the walk for short rays and on the walk for long rays
__global__ __launch_bounds__(256) void k_accel_query(AccelView a, const float* org, const float* dir, float tmin, float tmax,
                                                     uint32_t n, uint32_t* out) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  const RayLane r = load_ray_lane(org, dir, n, stacks);
  const bool hit = wave_any_hit(a, r.o, r.d, tmin, tmax, r.live, r.stack);
  if (r.live) out[r.i] = hit ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_accel_occluded(AccelView a, const float* org, const float* dir, float tmin, float tmax,
                                                        uint32_t n, uint32_t* out) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  const RayLane r = load_ray_lane(org, dir, n, stacks);
  const bool hit = wave_any_hit_ray(a, r.o, r.d, tmin, tmax, r.live, r.stack);
  if (r.live) out[r.i] = hit ? 1u : 0u;
}

// ---- gtao_rt_main ---------------------------------------------------------------------------------------------------------
struct GtaoRtArgs {
  Tex depth, normal, out;
  Mat4 camera_to_world;
  Proj pr;
  float rot_cs[16][2];  // (cos, sin) of 2 PI (rotation + k / 16), host libm
  AccelView accel;
  const float4* directions;
};

// rt_main.frag:67-108; one wave per pixel of the window, lane i = direction i
__global__ __launch_bounds__(256) void k_gtao_rt(GtaoRtArgs a) {
  __shared__ uint32_t stacks[4][ACCEL_STACK];
  const int lane = threadIdx.x & 63;
  const int pix = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
  if (pix >= a.out.w * a.out.h) return;  // the whole wave
  const int lx = pix % a.out.w, ly = pix / a.out.w;
  const int gx = lx + a.out.ox, gy = ly + a.out.oy;
  const f2 uv = mk2(pixel_centre_uv(gx, (float)a.out.fw), pixel_centre_uv(gy, (float)a.out.fh));
  uint2* dst = texel_ptr<uint2>(a.out, lx, ly);
  const float frag_depth = sample<FmtD24>(a.depth, uv);
  if (frag_depth >= 1.0f) {  // the whole wave
    if (lane == 0) *dst = make_uint2(0x3C000000u, 0u);  // (0, 1, 0, 0)
    return;
  }
  const f3 view_vec = reconstruct_view_vec(uv, frag_depth, a.pr);
  f3 world = xyz(mul(a.camera_to_world, mk4(view_vec.x, view_vec.y, view_vec.z, 1.0f)));
  const f3 normal = decode_normal(sample<FmtRG16U>(a.normal, uv));
  world = madd(world, 1e-6f, normal);
  f3 tangent, bitangent;
  tangent_frame(normal, &tangent, &bitangent);  // rt_main.frag:50-61,84-86
  const int slot = gtao_dir_slot(gx, gy);
  tangent = normalize(madd(tangent * a.rot_cs[slot][0], a.rot_cs[slot][1], bitangent));
  orthonormalise(normal, &tangent, &bitangent);

  const float4 r = a.directions[lane];
  f3 dir = normalize(mk3(r.x, r.y, r.z));
  dir = normalize(madd(madd(normal * dir.z, dir.x, tangent), dir.y, bitangent));
  const f3 scaled = dir * 0.2f;
  const bool hit = wave_any_hit(a.accel, world, scaled, 1e-12f, 1.0f, true, stacks[threadIdx.x >> 6]);
  float v = hit ? 0.0f : vmax(dot(dir, normal), 0.0f);
  // the sum over the 64 directions as a butterfly: every lane ends with the same value
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v = v + __shfl_xor(v, k, 64);
  const float occlusion = 2.0f * (v / 64.0f);
  if (lane == 0) *dst = make_uint2(float_to_half_bits(occlusion) | (0x3C00u << 16), 0u);
}

// ---- host: the build ------------------------------------------------------------------------------------------------------
struct BuildTri { float lo[3], hi[3], c[3]; uint32_t rec; };

struct Builder {
  std::vector<BuildTri> prims;
  std::vector<vkr_accel_node> nodes;
  uint32_t capacity;

  static void box_of(const BuildTri* p, uint32_t n, float lo[3], float hi[3]) {
    for (int k = 0; k < 3; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (uint32_t i = 0; i < n; i++)
      for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], p[i].lo[k]); hi[k] = std::max(hi[k], p[i].hi[k]); }
  }
  static float area(const float lo[3], const float hi[3]) {
    const float dx = std::max(hi[0] - lo[0], 0.0f), dy = std::max(hi[1] - lo[1], 0.0f), dz = std::max(hi[2] - lo[2], 0.0f);
    return dx * dy + dy * dz + dz * dx;
  }

  // node `at` over prims [begin, begin + n)
  void build(uint32_t at, uint32_t begin, uint32_t n, int depth) {
    vkr_accel_node& nd = nodes[at];
    box_of(&prims[begin], n, nd.lo, nd.hi);
    uint32_t split = 0;  // number of prims on the left; 0: leaf
    // above ACCEL_MAX_LEAF triangles the best plane is taken even where SAH prefers a leaf; where the centroids do not spread
    // (no plane at all) the range is halved in its present order
    const bool must_split = n > ACCEL_MAX_LEAF && depth < ACCEL_MAX_DEPTH;
    if (n > 2 && depth < ACCEL_MAX_DEPTH) split = choose_split(begin, n, must_split);
    if (must_split && split == 0) split = n / 2;
    if (split == 0) { nodes[at].first = begin; nodes[at].count = n; return; }
    const uint32_t left = (uint32_t)nodes.size();
    nodes.push_back(vkr_accel_node{});
    nodes.push_back(vkr_accel_node{});
    nodes[at].first = left;
    nodes[at].count = 0;
    build(left, begin, split, depth + 1);
    build(left + 1, begin + split, n - split, depth + 1);
  }

  // binned SAH over the centroid box; of equal costs the lower axis, then the lower bin wins.  Partitions the range (stable:
  // the same input always gives the same order) and returns the left count, or 0 when a leaf is cheaper / no plane exists.
  uint32_t choose_split(uint32_t begin, uint32_t n, bool must_split) {
    BuildTri* p = &prims[begin];
    float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = 0; i < n; i++)
      for (int k = 0; k < 3; k++) { clo[k] = std::min(clo[k], p[i].c[k]); chi[k] = std::max(chi[k], p[i].c[k]); }
    float blo[3], bhi[3];
    box_of(p, n, blo, bhi);
    const float parent_area = area(blo, bhi);
    double best = must_split ? INFINITY : (double)n;  // leaf cost: one test per triangle
    int best_axis = -1, best_bin = 0;
    for (int axis = 0; axis < 3; axis++) {
      const float ext = chi[axis] - clo[axis];
      if (!(ext > 0.0f)) continue;
      uint32_t cnt[ACCEL_BINS] = {};
      float lo[ACCEL_BINS][3], hi[ACCEL_BINS][3];
      for (int b = 0; b < ACCEL_BINS; b++) for (int k = 0; k < 3; k++) { lo[b][k] = INFINITY; hi[b][k] = -INFINITY; }
      for (uint32_t i = 0; i < n; i++) {
        const int b = bin_of(p[i].c[axis], clo[axis], ext);
        cnt[b]++;
        for (int k = 0; k < 3; k++) { lo[b][k] = std::min(lo[b][k], p[i].lo[k]); hi[b][k] = std::max(hi[b][k], p[i].hi[k]); }
      }
      // sweep: left = bins [0, b], right = bins (b, BINS)
      float rlo[ACCEL_BINS][3], rhi[ACCEL_BINS][3];
      uint32_t rcnt[ACCEL_BINS];
      float accl[3] = {INFINITY, INFINITY, INFINITY}, acch[3] = {-INFINITY, -INFINITY, -INFINITY};
      uint32_t acc = 0;
      for (int b = ACCEL_BINS - 1; b > 0; b--) {
        for (int k = 0; k < 3; k++) { accl[k] = std::min(accl[k], lo[b][k]); acch[k] = std::max(acch[k], hi[b][k]); }
        acc += cnt[b];
        for (int k = 0; k < 3; k++) { rlo[b][k] = accl[k]; rhi[b][k] = acch[k]; }
        rcnt[b] = acc;
      }
      float llo[3] = {INFINITY, INFINITY, INFINITY}, lhi[3] = {-INFINITY, -INFINITY, -INFINITY};
      uint32_t lcnt = 0;
      for (int b = 0; b < ACCEL_BINS - 1; b++) {
        for (int k = 0; k < 3; k++) { llo[k] = std::min(llo[k], lo[b][k]); lhi[k] = std::max(lhi[k], hi[b][k]); }
        lcnt += cnt[b];
        if (lcnt == 0 || rcnt[b + 1] == 0) continue;
        const double cost = 1.0 + (parent_area > 0.0f
            ? ((double)area(llo, lhi) * lcnt + (double)area(rlo[b + 1], rhi[b + 1]) * rcnt[b + 1]) / parent_area
            : 0.5 * n);
        if (cost < best) { best = cost; best_axis = axis; best_bin = b; }
      }
    }
    if (best_axis < 0) return 0;
    const float c0 = clo[best_axis], ext = chi[best_axis] - clo[best_axis];
    const int axis = best_axis, bin = best_bin;
    BuildTri* mid = std::stable_partition(p, p + n, [&](const BuildTri& t) { return bin_of(t.c[axis], c0, ext) <= bin; });
    return (uint32_t)(mid - p);
  }
  // the bin is chosen by comparisons before anything is converted: a NaN or infinite centroid, or an infinite centroid extent,
  // gives a quotient that no int holds (NaN goes to bin 0); for every finite quotient this is the truncation it always was
  static int bin_of(float c, float lo, float ext) {
    const double x = (double)(c - lo) / (double)ext * ACCEL_BINS;
    if (!(x >= 0.0)) return 0;
    if (x >= (double)ACCEL_BINS) return ACCEL_BINS - 1;
    return (int)x;
  }
};

static int layout(const float* verts, uint32_t tri_count, std::vector<vkr_accel_node>& nodes, std::vector<vkr_accel_tri>& tris) {
  if (!verts && tri_count) { set_error("vkr_accel_layout: NULL triangles"); return VKR_ERR_NULL; }
  if (tri_count > (1u << 30)) { set_error("vkr_accel_layout: %u triangles, at most 2^30", tri_count); return VKR_ERR_EXTENT; }
  std::vector<vkr_accel_tri> recs(tri_count);
  Builder b;
  b.prims.resize(tri_count);
  for (uint32_t i = 0; i < tri_count; i++) {
    make_record(verts + 9 * (size_t)i, i, recs[i]);
    BuildTri& t = b.prims[i];
    for (int k = 0; k < 3; k++) { t.lo[k] = recs[i].lo[k]; t.hi[k] = recs[i].hi[k]; t.c[k] = 0.5f * t.lo[k] + 0.5f * t.hi[k]; }
    t.rec = i;
  }
  nodes.clear();
  tris.clear();
  if (tri_count == 0) return VKR_OK;
  b.nodes.reserve(2 * (size_t)tri_count);
  b.nodes.push_back(vkr_accel_node{});
  b.build(0, 0, tri_count, 0);
  nodes.swap(b.nodes);
  tris.resize(tri_count);
  for (uint32_t i = 0; i < tri_count; i++) tris[i] = recs[b.prims[i].rec];
  return VKR_OK;
}

}  // namespace vkr

using namespace vkr;

extern "C" int vkr_accel_layout(const float* tri_vertices, uint32_t tri_count, vkr_accel_node* nodes, uint32_t node_capacity,
                                vkr_accel_tri* tris, uint32_t* node_count) {
  if ((!nodes && node_capacity) || (!tris && tri_count) || !node_count) { set_error("vkr_accel_layout: NULL output"); return VKR_ERR_NULL; }
  std::vector<vkr_accel_node> n;
  std::vector<vkr_accel_tri> t;
  VKR_TRY(layout(tri_vertices, tri_count, n, t));
  if (n.size() > node_capacity) {
    set_error("vkr_accel_layout: %zu nodes do not fit into %u (room for max(1, 2 * tri_count - 1) is always enough)", n.size(), node_capacity);
    return VKR_ERR_EXTENT;
  }
  if (!n.empty()) std::memcpy(nodes, n.data(), n.size() * sizeof(vkr_accel_node));
  if (!t.empty()) std::memcpy(tris, t.data(), t.size() * sizeof(vkr_accel_tri));
  *node_count = (uint32_t)n.size();
  return VKR_OK;
}

extern "C" int vkr_accel_create(const float* tri_vertices, uint32_t tri_count, vkr_accel** out) {
  if (!out) { set_error("vkr_accel_create: NULL output"); return VKR_ERR_NULL; }
  *out = nullptr;
  std::vector<vkr_accel_node> n;
  std::vector<vkr_accel_tri> t;
  VKR_TRY(layout(tri_vertices, tri_count, n, t));
  vkr_accel* a = new vkr_accel{nullptr, nullptr, (uint32_t)n.size(), (uint32_t)t.size()};
  hipError_t e = hipSuccess;
  if (!n.empty()) {
    e = hipMalloc((void**)&a->nodes, n.size() * sizeof(vkr_accel_node));
    if (e == hipSuccess) e = hipMalloc((void**)&a->tris, t.size() * sizeof(vkr_accel_tri));
    if (e == hipSuccess) e = hipMemcpy(a->nodes, n.data(), n.size() * sizeof(vkr_accel_node), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a->tris, t.data(), t.size() * sizeof(vkr_accel_tri), hipMemcpyHostToDevice);
    // the order in which vkr_accel_refit recomputes the node boxes: no query reads it
    std::vector<uint32_t> order;
    refit_schedule(n, &order, &a->level_begin);
    if (e == hipSuccess) e = hipMalloc((void**)&a->order, order.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(a->order, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    set_error("vkr_accel_create: upload failed: %s", hipGetErrorString(e));
    vkr_accel_destroy(a);
    return (int)e;
  }
  *out = a;
  return VKR_OK;
}

extern "C" int vkr_accel_destroy(vkr_accel* accel) {
  if (!accel) return VKR_OK;
  if (accel->nodes) (void)hipFree(accel->nodes);
  if (accel->tris) (void)hipFree(accel->tris);
  if (accel->order) (void)hipFree(accel->order);
  delete accel;
  return VKR_OK;
}

extern "C" int vkr_accel_info(const vkr_accel* accel, uint32_t* node_count, uint32_t* tri_count) {
  if (!accel) { set_error("vkr_accel_info: NULL acceleration structure"); return VKR_ERR_NULL; }
  if (node_count) *node_count = accel->node_count;
  if (tri_count) *tri_count = accel->tri_count;
  return VKR_OK;
}

extern "C" int vkr_accel_query(const vkr_accel* accel, const float* origins, const float* dirs, float tmin, float tmax, uint32_t n,
                               uint32_t* out_hit, void* stream) {
  VKR_TRY(check_ray_batch("accel_query", accel, origins, dirs, out_hit, n));
  if (n == 0) return VKR_OK;
  hipLaunchKernelGGL(k_accel_query, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, view_of(accel), origins, dirs, tmin, tmax, n, out_hit);
  return launch_status("accel_query");
}

extern "C" int vkr_accel_occluded(const vkr_accel* accel, const float* origins, const float* dirs, float tmin, float tmax, uint32_t n,
                                  uint32_t* out_hit, void* stream) {
  VKR_TRY(check_ray_batch("accel_occluded", accel, origins, dirs, out_hit, n));
  if (n == 0) return VKR_OK;
  hipLaunchKernelGGL(k_accel_occluded, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, view_of(accel), origins, dirs, tmin, tmax, n, out_hit);
  return launch_status("accel_occluded");
}

extern "C" int vkr_gtao_rt_main(const vkr_gtao_rt_params* params, const vkr_img* depth, const vkr_img* normal, const vkr_accel* accel,
                                const float* directions, const vkr_img* out_raw, const vkr_gtao_rt_push* push, void* stream) {
  if (!params || !push) { set_error("gtao_rt_main: NULL params"); return VKR_ERR_NULL; }
  if (!accel) { set_error("gtao_rt_main: NULL acceleration structure (binding 3)"); return VKR_ERR_NULL; }
  if (!directions) { set_error("gtao_rt_main: NULL random directions (binding 4)"); return VKR_ERR_NULL; }
  GtaoRtArgs a;
  VKR_TRY(make_tex(depth, 0, VKR_FMT_D24_UNORM_S8, "gtao_rt_main.depth", &a.depth));
  VKR_TRY(make_tex(normal, 0, VKR_FMT_RG16_UNORM, "gtao_rt_main.normal", &a.normal));
  VKR_TRY(make_tex(out_raw, 0, VKR_FMT_RGBA16_SFLOAT, "gtao_rt_main.out", &a.out));
  if (((uintptr_t)directions & 15u) != 0) { set_error("gtao_rt_main: directions must be 16-byte aligned"); return VKR_ERR_LAYOUT; }
  load_mat(a.camera_to_world, params->camera_to_world);
  load_proj(a.pr, params->fovy, params->aspect, params->znear, params->zfar);
  fill_slice_table(a.rot_cs, push->rotation, 0.0f);  // rt_main.frag:89: angle = 2 PI (rotation + gtao_direction(pixel))
  a.accel = view_of(accel);
  a.directions = (const float4*)directions;
  const uint32_t pixels = (uint32_t)a.out.w * (uint32_t)a.out.h;
  hipLaunchKernelGGL(k_gtao_rt, dim3((pixels + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("gtao_rt_main");
}
