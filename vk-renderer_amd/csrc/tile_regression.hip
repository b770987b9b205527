// tile_regression.hip — program "tile_regression".
//
// Reference: src/advanced_ssr.cpp:497-538 and shaders/advanced_ssr/regression.comp: the third member of the tile-classified SSR
// experiment.  One 8 x 8 tile of the half-resolution depth in (mip 0 of the bound view), one RGBA32F texel per tile out:
// (plane.xyz, mean squared residual), plane the least-squares solution of plane . r = 1 over the tile's 64 view vectors r
// rotated to world axes.  The arithmetic is one frozen fp32 sequence (DESIGN_NUMERICS.md, Tile regression): the fit is badly
// conditioned in fp32, so the result is only meaningful as that sequence.
//
// Shape: a tile is exactly one wave64, lane i = ly * 8 + lx the reference's gl_LocalInvocationIndex.  The shader's three
// shared-memory trees become xor butterflies over the wave (offsets 32 .. 1): fp32 addition is commutative, so every lane ends
// with the bits the tree leaves in s[0], every lane solves the 3 x 3 system redundantly, and there is no LDS, no barrier and
// no broadcast.  A block is four waves = four tiles side by side: one row of loads is 32 texels, 128 contiguous bytes.
// Lanes outside the depth view and tiles outside the output are predicated (clamped load, r = 0, no store): no lane leaves
// before the last cross-lane operation.
//
// Roofline: 4 bytes read per half-resolution texel, 16 written per tile (4.25 bytes per texel in all) against ~110 VALU
// operations, 5 IEEE divisions and 60 cross-lane steps (permlane swaps and DPP moves, none through LDS) per lane.
#include "vkr_host.hpp"

namespace vkr {

#define TILE_REGRESSION_TILE 8
#define TILE_REGRESSION_WAVES 4  // tiles per block, side by side

// All of it wave-uniform: a kernel argument, read through scalar loads.
struct TileRegressionArgs {
  Tex depth, out;
  Mat4 camera_to_world;
  Proj pr;
};

// v of another lane through a DPP control word (all lanes are active here: every source lane is valid)
template <int CTRL> VKR_DEV float dpp_move(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// The sum over the wave's 64 lanes in the order of the reference's tree: every lane adds the value of lane i ^ off, off = 32 .. 1,
// without the LDS crossbar.  v_permlane32_swap / v_permlane16_swap of v with itself leave (x, y) = (v of the lower, v of the
// upper) half / row of the pair in both of them, and x + y = y + x: lane i ^ 32, lane i ^ 16.  Within a row of 16 lanes DPP:
// row_ror:8 is lane i ^ 8; row_half_mirror (i ^ 7) followed by quad_perm [3,2,1,0] (i ^ 3) is lane i ^ 4; quad_perm [2,3,0,1] and
// [1,0,3,2] are lanes i ^ 2 and i ^ 1.
VKR_DEV float butterfly_sum(float v) {
  const auto h32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(h32[0]) + __uint_as_float(h32[1]);
  const auto h16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(h16[0]) + __uint_as_float(h16[1]);
  v = v + dpp_move<0x128>(v);
  v = v + dpp_move<0x01B>(dpp_move<0x141>(v));
  v = v + dpp_move<0x04E>(v);
  v = v + dpp_move<0x0B1>(v);
  return v;
}
VKR_DEV f3 butterfly_sum(f3 v) { return mk3(butterfly_sum(v.x), butterfly_sum(v.y), butterfly_sum(v.z)); }

// regression.comp:22-101, one wave per tile
__global__ __launch_bounds__(64 * TILE_REGRESSION_WAVES) void k_tile_regression(TileRegressionArgs a) {
  const int lane = threadIdx.x;
  const int tx = blockIdx.x * TILE_REGRESSION_WAVES + threadIdx.y, ty = blockIdx.y;
  const int px = tx * TILE_REGRESSION_TILE + (lane & 7), py = ty * TILE_REGRESSION_TILE + (lane >> 3);
  const bool inside = px < a.depth.w && py < a.depth.h;
  const int cx = min(px, a.depth.w - 1), cy = min(py, a.depth.h - 1);  // the load of an outside lane stays in the image

  // :25-37; no half-texel offset, plain IEEE divisions (pixel 0 gives 0)
  const float d = FmtD24::load(a.depth, cx, cy);
  const f2 screen_uv = mk2((float)cx / (float)a.depth.w, (float)cy / (float)a.depth.h);
  const f3 view = reconstruct_view_vec(screen_uv, d, a.pr);
  const f4 world = mul(a.camera_to_world, mk4(view.x, view.y, view.z, 1.0f));
  const f4 origin = mul(a.camera_to_world, mk4(0.0f, 0.0f, 0.0f, 1.0f));
  f3 r = xyz(world) - xyz(origin);
  if (!inside) r = mk3(0.0f, 0.0f, 0.0f);  // counted in the division by 64 all the same

  // :40-59
  const f3 s1 = butterfly_sum(r);
  const f3 s2 = butterfly_sum(r * r);
  const f3 sx = butterfly_sum(mk3(r.x * r.y, r.x * r.z, r.y * r.z));

  // :61-71, in every lane
  Mat3 equ;
  equ.m[0] = s2.x; equ.m[1] = sx.x; equ.m[2] = sx.y;
  equ.m[3] = sx.x; equ.m[4] = s2.y; equ.m[5] = sx.z;
  equ.m[6] = sx.y; equ.m[7] = sx.z; equ.m[8] = s2.z;
  const f3 plane = mul_unfused(inverse_adjugate(equ), s1);

  // :75-96
  float sse = dot(plane, r) - 1.0f;
  sse *= sse;
  if (is_nan(sse)) sse = 1e10f;
  const float mean = butterfly_sum(sse) / (float)(TILE_REGRESSION_TILE * TILE_REGRESSION_TILE);

  // :98-101; imageStore outside the image is dropped
  if (lane == 0 && tx < a.out.w && ty < a.out.h) {
    U32x4 texel;
    texel.x = __float_as_uint(plane.x); texel.y = __float_as_uint(plane.y); texel.z = __float_as_uint(plane.z); texel.w = __float_as_uint(mean);
    *texel_ptr<U32x4>(a.out, tx, ty) = texel;
  }
}

}  // namespace vkr

using namespace vkr;

extern "C" int vkr_tile_regression(const vkr_img* depth, const vkr_img* out_planes, const vkr_tile_regression_push* push, void* stream) {
  if (!depth) { set_error("tile_regression: depth is NULL"); return VKR_ERR_NULL; }
  if (!out_planes) { set_error("tile_regression: out_planes is NULL"); return VKR_ERR_NULL; }
  if (!push) { set_error("tile_regression: push is NULL"); return VKR_ERR_NULL; }
  TileRegressionArgs a;
  VKR_TRY(make_tex(depth, 0, VKR_FMT_D24_UNORM_S8, "tile_regression.depth", &a.depth));
  VKR_TRY(make_tex(out_planes, 0, VKR_FMT_RGBA32_SFLOAT, "tile_regression.out_planes", &a.out));
  VKR_TRY(require_whole_frame(a.depth, "tile_regression: depth", "windows are not supported (tiles would straddle owners: a single-GPU pass)"));
  VKR_TRY(require_whole_frame(a.out, "tile_regression: out_planes", "windows are not supported (tiles would straddle owners: a single-GPU pass)"));
  const int tiles_w = (a.depth.w + TILE_REGRESSION_TILE - 1) / TILE_REGRESSION_TILE, tiles_h = (a.depth.h + TILE_REGRESSION_TILE - 1) / TILE_REGRESSION_TILE;
  if (a.out.w > tiles_w || a.out.h > tiles_h) {
    set_error("tile_regression: out_planes is %dx%d, a %dx%d depth view has %dx%d tiles (a tile further out has no pixel)", a.out.w, a.out.h,
              a.depth.w, a.depth.h, tiles_w, tiles_h);
    return VKR_ERR_EXTENT;
  }
  if (a.out.h > 65535) { set_error("tile_regression: out_planes is %d texels high, at most 65535", a.out.h); return VKR_ERR_EXTENT; }
  load_mat(a.camera_to_world, push->camera_to_world);
  load_proj(a.pr, push->fovy, push->aspect, push->znear, push->zfar);
  const dim3 block(64, TILE_REGRESSION_WAVES);
  const dim3 grid((a.out.w + TILE_REGRESSION_WAVES - 1) / TILE_REGRESSION_WAVES, a.out.h);
  hipLaunchKernelGGL(k_tile_regression, grid, block, 0, (hipStream_t)stream, a);
  return launch_status("tile_regression");
}
