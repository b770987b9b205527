// transfer.hip — image transfers: vkr_clear_image, vkr_blit_image, vkr_gen_mipmaps.
//
// Reference: util_passes.cpp (clear_depth / clear_color / blit_image / gen_mipmaps record vkCmdClear*Image and
// vkCmdBlitImage) and scene/images.cpp:93-160 (the blit chain that builds a texture's mips at load time).  Transfers are
// whole-image operations: every entry refuses a descriptor that is a window of a larger frame.
//
// Numerics (DESIGN_NUMERICS.md, "Image transfers"): a texel is decoded to float RGBA (absent channels 0, 0, 0, 1) with the
// library's exact decodes and stored with the destination format's store rule; the blit's only arithmetic is the
// coordinate u = (i + 0.5) * (src / dst) and, for LINEAR, the bilinear mix of vkr_device.hpp.  The mip chain follows the
// project's one mip rule (scene.build_mips): ((a + b) + (c + d)) * 0.25 of the 2x2 block of the STORED previous level.
// Roofline: HBM.  A blit moves src + dst bytes once, a clear the destination once, a mip chain 4/3 of level 0.
#include "vkr_host.hpp"
#include "image_codec.hpp"
#include <algorithm>

namespace vkr {

VKR_DEV uint8_t* wptr(const Tex& t, int x, int y, int bpp) { return const_cast<uint8_t*>(t.p) + toff(t, x, y, bpp); }

// ---- any colour format <-> float RGBA through image_codec.hpp (the format is wave-uniform: a scalar branch) ----------------
// lut / thresh: the sRGB tables staged in LDS (only read for RGBA8_SRGB).  Anything but a colour format: (0, 0, 0, 1) / zeros.
VKR_DEV f4 load_rgba(const Tex& t, uint32_t fmt, int x, int y, const float* lut) {
  f4 c = mk4(0.0f, 0.0f, 0.0f, 1.0f);
  with_colour_format(fmt, [&](auto codec) { c = codec.decode(load_raw<codec.bpp>(t.p + toff(t, x, y, codec.bpp)), lut); });
  return c;
}
VKR_DEV Raw encode_rgba(uint32_t fmt, f4 c, const float* thresh) {
  Raw o = raw_words(0u);
  with_colour_format(fmt, [&](auto codec) { o = codec.encode(c, thresh); });
  return o;
}
// the texel (x, y) of an image of `bpp` bytes a texel
VKR_DEV void store_texel(const Tex& t, int bpp, int x, int y, const Raw& o) {
  uint8_t* p = wptr(t, x, y, bpp);
  switch (bpp) {
    case 1: store_raw<1>(p, o); break;
    case 2: store_raw<2>(p, o); break;
    case 4: store_raw<4>(p, o); break;
    case 8: store_raw<8>(p, o); break;
    default: store_raw<16>(p, o); break;
  }
}
VKR_DEV bool is_srgb(uint32_t fmt) { return fmt == VKR_FMT_RGBA8_SRGB; }

// ---- clear -------------------------------------------------------------------------------------------------------------------
// Every mip of the view from ONE launch: mip m owns blocks [first[m], first[m + 1]), each block 64 x 4 threads, a thread
// 16 bytes of a row (16 is a multiple of every texel size, so every 16-byte piece of a row holds the same pattern).  Only
// the texels of a row are written, never the padding up to the pitch: a layer view of an array leaves its neighbours alone.
struct ClearArgs {
  Tex mip[VKR_MAX_MIPS];
  uint32_t first[VKR_MAX_MIPS + 1];
  uint32_t blocks_x[VKR_MAX_MIPS];
  uint32_t mips, format, bpp;
  float color[4];
  float depth;
  uint32_t stencil;
};
__global__ __launch_bounds__(256) void k_transfer_clear(ClearArgs a) {
  __shared__ float s_thr[VKR_SRGB_LUT_SIZE];
  __shared__ Raw s_word;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  if (is_srgb(a.format)) { srgb_thresh_stage(s_thr, tid, 256); __syncthreads(); }
  if (tid == 0) {
    Raw w;
    if (a.format == VKR_FMT_D24_UNORM_S8) {
      w.x = (uint32_t)rintf(vclamp(a.depth, 0.0f, 1.0f) * 16777215.0f) | ((a.stencil & 0xFFu) << 24);
      w.y = w.z = w.w = 0u;
    } else {
      w = encode_rgba(a.format, mk4(a.color[0], a.color[1], a.color[2], a.color[3]), s_thr);
    }
    // the 16-byte pattern: the texel's bytes repeated
    if (a.bpp == 1) { w.x &= 0xFFu; w.x |= w.x << 8; w.x |= w.x << 16; }
    if (a.bpp == 2) { w.x &= 0xFFFFu; w.x |= w.x << 16; }
    if (a.bpp <= 4) w.y = w.x;
    if (a.bpp <= 8) { w.z = w.x; w.w = w.y; }
    s_word = w;
  }
  __syncthreads();
  const Raw w = s_word;
  uint32_t m = 0;
  while (m + 1 < a.mips && blockIdx.x >= a.first[m + 1]) m++;
  const Tex& t = a.mip[m];
  const uint32_t b = blockIdx.x - a.first[m];
  const uint32_t bx = b % a.blocks_x[m], by = b / a.blocks_x[m];
  const uint32_t row = by * 4u + threadIdx.y, row_bytes = (uint32_t)t.w * a.bpp;
  const uint32_t off = (bx * 64u + threadIdx.x) * 16u;
  if (row >= (uint32_t)t.h || off >= row_bytes) return;
  uint8_t* p = const_cast<uint8_t*>(t.p) + __umul24(row, (uint32_t)t.pitch) + off;
  const uint32_t n = min(16u, row_bytes - off);
  if (n == 16u && (((uintptr_t)p) & 3u) == 0u) { store_u32x4(p, w.x, w.y, w.z, w.w); return; }
  const uint32_t words[4] = {w.x, w.y, w.z, w.w};  // tail of a row, or a row that is not dword aligned (1- and 2-byte texels)
  for (uint32_t i = 0; i < n; i++) p[i] = (uint8_t)(words[i >> 2] >> ((i & 3u) * 8u));
}

// ---- blit --------------------------------------------------------------------------------------------------------------------
// One thread per destination texel.  u = (i + 0.5) * (src_w / dst_w) — the quotient is evaluated once on the host — and the
// same in v.  NEAREST: texel floor(u).  LINEAR: taps floor(u - 0.5) and + 1 clamped to the edge, weight frac(u - 0.5), mixed
// with the sampler's mix (rows first, then columns).  D24S8 (equal extents, NEAREST) copies the stored word.
struct BlitArgs {
  Tex src, dst;
  uint32_t src_format, dst_format, dst_bpp;
  float scale_x, scale_y;
};
template <bool LINEAR> __global__ __launch_bounds__(256) void k_transfer_blit(BlitArgs a) {
  __shared__ float s_lut[VKR_SRGB_LUT_SIZE], s_thr[VKR_SRGB_LUT_SIZE];
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const bool tables = is_srgb(a.src_format) || is_srgb(a.dst_format);
  if (tables) { srgb_lut_stage(s_lut, tid, 256); srgb_thresh_stage(s_thr, tid, 256); __syncthreads(); }
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= a.dst.w || y >= a.dst.h) return;
  const float u = ((float)x + 0.5f) * a.scale_x, v = ((float)y + 0.5f) * a.scale_y;
  if (a.src_format == VKR_FMT_D24_UNORM_S8) {
    const int sx = iclamp(f2i(floorf(u)), 0, a.src.w - 1), sy = iclamp(f2i(floorf(v)), 0, a.src.h - 1);
    *texel_ptr<uint32_t>(a.dst, x, y) = *(const uint32_t*)(a.src.p + toff(a.src, sx, sy, 4));
    return;
  }
  f4 c;
  if (LINEAR) {
    const Footprint f = footprint_at(u - 0.5f, v - 0.5f);
    const int xa = iclamp(f.x0, 0, a.src.w - 1), xb = iclamp(f.x0 + 1, 0, a.src.w - 1);
    const int ya = iclamp(f.y0, 0, a.src.h - 1), yb = iclamp(f.y0 + 1, 0, a.src.h - 1);
    const f4 t00 = load_rgba(a.src, a.src_format, xa, ya, s_lut), t10 = load_rgba(a.src, a.src_format, xb, ya, s_lut);
    const f4 t01 = load_rgba(a.src, a.src_format, xa, yb, s_lut), t11 = load_rgba(a.src, a.src_format, xb, yb, s_lut);
    c = mix4(mix4(t00, t10, f.fx), mix4(t01, t11, f.fx), f.fy);
  } else {
    const int sx = iclamp(f2i(floorf(u)), 0, a.src.w - 1), sy = iclamp(f2i(floorf(v)), 0, a.src.h - 1);
    c = load_rgba(a.src, a.src_format, sx, sy, s_lut);
  }
  store_texel(a.dst, (int)a.dst_bpp, x, y, encode_rgba(a.dst_format, c, s_thr));
}

// ---- mip chain ---------------------------------------------------------------------------------------------------------------
// The project's one mip rule (scene.build_mips): level extents max(1, s / 2); destination texel (X, Y) averages the source
// texels (2X, 2Y), (x1, 2Y), (2X, y1), (x1, y1) with x1 = min(2X + 1, w - 1) — the clamp only acts where the source extent is 1;
// an odd extent drops its last row / column — as ((a + b) + (c + d)) * 0.25 in fp32 per channel, decoded from and encoded to
// the STORED texel, so every level is computed from the quantised previous one.  mip_reduce is the only place the rule is
// written: both schedules call it on the same stored texels and therefore leave the same bytes.
template <int FMT> struct MipRaw { typedef uint32_t T; };
template <> struct MipRaw<VKR_FMT_RGBA16_SFLOAT> { typedef uint2 T; };
template <int FMT> constexpr int mip_bpp() { return Codec<FMT>::bpp; }
// MipRaw<FMT>::T is the used dwords of a Raw
template <int FMT> VKR_DEV typename MipRaw<FMT>::T mip_raw(const Raw& r) {
  if constexpr (mip_bpp<FMT>() == 8) return make_uint2(r.x, r.y); else return r.x;
}
template <int FMT> VKR_DEV typename MipRaw<FMT>::T mip_load(const Tex& t, int x, int y) {
  return mip_raw<FMT>(load_raw<mip_bpp<FMT>()>(t.p + toff(t, x, y, mip_bpp<FMT>())));
}
// texels (x, y) and (x + 1, y) as one load where the texel size allows it (1- and 2-byte texels: two loads, as measured)
template <int FMT> VKR_DEV void mip_load_pair(const Tex& t, int x, int y, typename MipRaw<FMT>::T& l, typename MipRaw<FMT>::T& r) {
  if constexpr (mip_bpp<FMT>() >= 4) {
    Raw a, b;
    load_raw_pair<mip_bpp<FMT>()>(t.p + toff(t, x, y, mip_bpp<FMT>()), a, b);
    l = mip_raw<FMT>(a); r = mip_raw<FMT>(b);
  } else { l = mip_load<FMT>(t, x, y); r = mip_load<FMT>(t, x + 1, y); }
}
template <int FMT> VKR_DEV void mip_store(const Tex& t, int x, int y, typename MipRaw<FMT>::T v) {
  Raw o;
  if constexpr (mip_bpp<FMT>() == 8) o = raw_words(v.x, v.y); else o = raw_words(v);
  store_raw<mip_bpp<FMT>()>(wptr(t, x, y, mip_bpp<FMT>()), o);
}
VKR_DEV float avg4(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }
template <int FMT> VKR_DEV typename MipRaw<FMT>::T mip_reduce(typename MipRaw<FMT>::T a, typename MipRaw<FMT>::T b, typename MipRaw<FMT>::T c,
                                                              typename MipRaw<FMT>::T d, const float* lut, const float* thresh) {
  if constexpr (FMT == VKR_FMT_RGBA8_SRGB) {
    uint32_t o = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const int sh = ch * 8;
      o |= float_to_srgb8_lds(avg4(lut[(a >> sh) & 0xFFu], lut[(b >> sh) & 0xFFu], lut[(c >> sh) & 0xFFu], lut[(d >> sh) & 0xFFu]), thresh) << sh;
    }
    return o | (float_to_unorm8(avg4(unorm8_to_float(a >> 24), unorm8_to_float(b >> 24), unorm8_to_float(c >> 24), unorm8_to_float(d >> 24))) << 24);
  } else if constexpr (FMT == VKR_FMT_RGBA8_UNORM) {
    uint32_t o = 0u;
#pragma unroll
    for (int ch = 0; ch < 4; ch++) {
      const int sh = ch * 8;
      o |= float_to_unorm8(avg4(unorm8_to_float((a >> sh) & 0xFFu), unorm8_to_float((b >> sh) & 0xFFu), unorm8_to_float((c >> sh) & 0xFFu),
                                unorm8_to_float((d >> sh) & 0xFFu))) << sh;
    }
    return o;
  } else if constexpr (FMT == VKR_FMT_RGBA16_SFLOAT) {
    auto lo = [](uint32_t v) { return half_bits_to_float(v & 0xFFFFu); };
    auto hi = [](uint32_t v) { return half_bits_to_float(v >> 16); };
    uint2 o;
    o.x = pack_half2(avg4(lo(a.x), lo(b.x), lo(c.x), lo(d.x)), avg4(hi(a.x), hi(b.x), hi(c.x), hi(d.x)));
    o.y = pack_half2(avg4(lo(a.y), lo(b.y), lo(c.y), lo(d.y)), avg4(hi(a.y), hi(b.y), hi(c.y), hi(d.y)));
    return o;
  } else if constexpr (FMT == VKR_FMT_RG16_SFLOAT) {
    auto lo = [](uint32_t v) { return half_bits_to_float(v & 0xFFFFu); };
    auto hi = [](uint32_t v) { return half_bits_to_float(v >> 16); };
    return pack_half2(avg4(lo(a), lo(b), lo(c), lo(d)), avg4(hi(a), hi(b), hi(c), hi(d)));
  } else if constexpr (FMT == VKR_FMT_R16_SFLOAT) {
    return float_to_half_bits(avg4(half_bits_to_float(a), half_bits_to_float(b), half_bits_to_float(c), half_bits_to_float(d)));
  } else if constexpr (FMT == VKR_FMT_R32_SFLOAT) {
    return __float_as_uint(avg4(__uint_as_float(a), __uint_as_float(b), __uint_as_float(c), __uint_as_float(d)));
  } else {  // R8_UNORM
    return float_to_unorm8(avg4(unorm8_to_float(a), unorm8_to_float(b), unorm8_to_float(c), unorm8_to_float(d)));
  }
}
// destination texel (X, Y) from the previous level in memory
template <int FMT> VKR_DEV typename MipRaw<FMT>::T mip_texel_from_memory(const Tex& src, int X, int Y, const float* lut, const float* thresh) {
  typename MipRaw<FMT>::T a, b, c, d;
  const int x0 = 2 * X, y0 = 2 * Y, y1 = min(y0 + 1, src.h - 1);
  if (x0 + 1 < src.w) {
    mip_load_pair<FMT>(src, x0, y0, a, b);
    mip_load_pair<FMT>(src, x0, y1, c, d);
  } else {  // a source one texel wide: the second tap is the first
    a = b = mip_load<FMT>(src, x0, y0);
    c = d = mip_load<FMT>(src, x0, y1);
  }
  return mip_reduce<FMT>(a, b, c, d, lut, thresh);
}
template <int FMT> VKR_DEV void mip_tables(float* lut, float* thresh, int tid) {
  if constexpr (FMT == VKR_FMT_RGBA8_SRGB) { srgb_lut_stage(lut, tid, 256); srgb_thresh_stage(thresh, tid, 256); __syncthreads(); }
}
#define VKR_MIP_TABLE_SIZE(FMT) ((FMT) == VKR_FMT_RGBA8_SRGB ? VKR_SRGB_LUT_SIZE : 1)

// Schedule "per level": one launch per level, one thread per destination texel (the reference's shape: one blit per level).
template <int FMT> __global__ __launch_bounds__(256) void k_mips_level(Tex src, Tex dst) {
  __shared__ float s_lut[VKR_MIP_TABLE_SIZE(FMT)], s_thr[VKR_MIP_TABLE_SIZE(FMT)];
  mip_tables<FMT>(s_lut, s_thr, threadIdx.y * 64 + threadIdx.x);
  const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y;
  if (X >= dst.w || Y >= dst.h) return;
  mip_store<FMT>(dst, X, Y, mip_texel_from_memory<FMT>(src, X, Y, s_lut, s_thr));
}

// Schedule "fused": a block of 256 threads takes a 64 x 64 tile of the source level and writes up to MIP_FUSED_LEVELS levels:
// the first from memory (four texels per thread), the others from the previous level's STORED texels kept in LDS.  Extents
// halve with floor, so tile (bx, by) of level k + 1 reads exactly tile (bx, by) of level k: no block needs a neighbour's
// texels at any size.  A texel that does not exist (X >= w) is never read: its parent would not exist either, except below a
// source one texel wide, where the clamp selects texel 0.  The chain of a 4096^2 image is two launches, the second a single block.
#define MIP_FUSED_LEVELS 6
// the schedule vkr_gen_mipmaps takes when no switch forces one (profiles/transfer.json)
#define VKR_MIPS_DEFAULT_FUSED 1
struct MipFusedArgs {
  Tex src;
  Tex dst[MIP_FUSED_LEVELS];
  int levels;
};
// level k >= 2 of the tile: n x n destination texels from the 2n x 2n stored texels `sp`; `prev` / `d`: the two levels' extents
template <int FMT> VKR_DEV void mip_fused_step(const typename MipRaw<FMT>::T* sp, typename MipRaw<FMT>::T* dp, const Tex& prev, const Tex& d, int n,
                                               const float* lut, const float* thresh) {
  const int tid = threadIdx.x;
  if (tid >= n * n) return;
  const int lx = tid % n, ly = tid / n;
  const int X = blockIdx.x * n + lx, Y = blockIdx.y * n + ly;
  typename MipRaw<FMT>::T v {};
  if (X < d.w && Y < d.h) {
    const int sn = 2 * n;
    const int x0 = 2 * lx, y0 = 2 * ly;  // local to the tile; the clamp in global coordinates
    const int x1 = min(2 * X + 1, prev.w - 1) - (int)blockIdx.x * sn, y1 = min(2 * Y + 1, prev.h - 1) - (int)blockIdx.y * sn;
    v = mip_reduce<FMT>(sp[y0 * sn + x0], sp[y0 * sn + x1], sp[y1 * sn + x0], sp[y1 * sn + x1], lut, thresh);
    mip_store<FMT>(d, X, Y, v);
  }
  if (dp) dp[ly * n + lx] = v;
}
template <int FMT> __global__ __launch_bounds__(256) void k_mips_fused(MipFusedArgs a) {
  typedef typename MipRaw<FMT>::T Raw;
  __shared__ float s_lut[VKR_MIP_TABLE_SIZE(FMT)], s_thr[VKR_MIP_TABLE_SIZE(FMT)];
  __shared__ Raw s1[32 * 32], s2[16 * 16], s3[8 * 8], s4[4 * 4], s5[2 * 2];
  const int tid = threadIdx.x;
  mip_tables<FMT>(s_lut, s_thr, tid);
#pragma unroll
  for (int j = 0; j < 4; j++) {  // level 1: 32 x 32 texels, rows of 32 lanes
    const int lx = tid & 31, ly = (tid >> 5) + 8 * j;
    const int X = blockIdx.x * 32 + lx, Y = blockIdx.y * 32 + ly;
    Raw v {};
    if (X < a.dst[0].w && Y < a.dst[0].h) {
      v = mip_texel_from_memory<FMT>(a.src, X, Y, s_lut, s_thr);
      mip_store<FMT>(a.dst[0], X, Y, v);
    }
    s1[ly * 32 + lx] = v;
  }
  if (a.levels < 2) return;
  __syncthreads();
  mip_fused_step<FMT>(s1, s2, a.dst[0], a.dst[1], 16, s_lut, s_thr);
  if (a.levels < 3) return;
  __syncthreads();
  mip_fused_step<FMT>(s2, s3, a.dst[1], a.dst[2], 8, s_lut, s_thr);
  if (a.levels < 4) return;
  __syncthreads();
  mip_fused_step<FMT>(s3, s4, a.dst[2], a.dst[3], 4, s_lut, s_thr);
  if (a.levels < 5) return;
  __syncthreads();
  mip_fused_step<FMT>(s4, s5, a.dst[3], a.dst[4], 2, s_lut, s_thr);
  if (a.levels < 6) return;
  __syncthreads();
  mip_fused_step<FMT>(s5, (Raw*)nullptr, a.dst[4], a.dst[5], 1, s_lut, s_thr);
}

}  // namespace vkr

using namespace vkr;

// a transfer's image: present, of a known format, and whole (not a window of a larger frame)
static int whole_image(const vkr_img* d, const char* what) {
  if (!d || !d->base) { set_error("%s: NULL image", what); return VKR_ERR_NULL; }
  if (vkr_format_bytes(d->format) == 0) { set_error("%s: unknown format %u", what, d->format); return VKR_ERR_FORMAT; }
  if (!whole_frame(d->origin_x, d->origin_y, d->width, d->height, d->full_width, d->full_height)) {
    set_error("%s: a window (%d,%d)+(%ux%u) of a %ux%u frame: transfers are whole-image operations", what, d->origin_x, d->origin_y, d->width,
              d->height, d->full_width, d->full_height);
    return VKR_ERR_EXTENT;
  }
  if (d->mip_count == 0 || d->mip_count > VKR_MAX_MIPS) { set_error("%s: bad mip count %u", what, d->mip_count); return VKR_ERR_MIPS; }
  return VKR_OK;
}

extern "C" int vkr_clear_image(const vkr_img* img, const vkr_clear_value* value, void* stream) {
  VKR_TRY(whole_image(img, "clear_image.img"));
  if (!value) { set_error("clear_image: NULL value"); return VKR_ERR_NULL; }
  ClearArgs a {};
  a.mips = img->mip_count; a.format = img->format; a.bpp = vkr_format_bytes(img->format);
  uint32_t total = 0;
  for (uint32_t m = 0; m < a.mips; m++) {
    VKR_TRY(make_tex(img, (int)m, img->format, "clear_image.img", &a.mip[m]));
    a.blocks_x[m] = ((uint32_t)a.mip[m].w * a.bpp + 1023u) / 1024u;
    a.first[m] = total;
    total += a.blocks_x[m] * (((uint32_t)a.mip[m].h + 3u) / 4u);
  }
  a.first[a.mips] = total;
  std::memcpy(a.color, value->color, sizeof(a.color));
  a.depth = value->depth; a.stencil = value->stencil;
  hipLaunchKernelGGL(k_transfer_clear, dim3(total), dim3(64, 4), 0, (hipStream_t)stream, a);
  return launch_status("clear_image");
}

extern "C" int vkr_blit_image(const vkr_img* src, const vkr_img* dst, uint32_t filter, void* stream) {
  VKR_TRY(whole_image(src, "blit_image.src"));
  VKR_TRY(whole_image(dst, "blit_image.dst"));
  if (filter != VKR_FILTER_NEAREST && filter != VKR_FILTER_LINEAR) { set_error("blit_image: unknown filter %u", filter); return VKR_ERR_FORMAT; }
  const bool sd = src->format == VKR_FMT_D24_UNORM_S8, dd = dst->format == VKR_FMT_D24_UNORM_S8;
  if (sd != dd) { set_error("blit_image: D24_UNORM_S8 blits only to D24_UNORM_S8 (src format %u, dst format %u)", src->format, dst->format); return VKR_ERR_FORMAT; }
  if (sd && filter != VKR_FILTER_NEAREST) { set_error("blit_image: a D24_UNORM_S8 blit needs the NEAREST filter"); return VKR_ERR_FORMAT; }
  if (sd && (src->width != dst->width || src->height != dst->height)) {
    set_error("blit_image: a D24_UNORM_S8 blit needs equal extents (%ux%u -> %ux%u)", src->width, src->height, dst->width, dst->height);
    return VKR_ERR_EXTENT;
  }
  BlitArgs a {};
  VKR_TRY(make_tex(src, 0, src->format, "blit_image.src", &a.src));
  VKR_TRY(make_tex(dst, 0, dst->format, "blit_image.dst", &a.dst));
  if (a.src.p == a.dst.p) { set_error("blit_image: src and dst are the same memory"); return VKR_ERR_LAYOUT; }
  a.src_format = src->format; a.dst_format = dst->format; a.dst_bpp = vkr_format_bytes(dst->format);
  a.scale_x = (float)a.src.w / (float)a.dst.w;
  a.scale_y = (float)a.src.h / (float)a.dst.h;
  const dim3 block(64, 4);
  if (filter == VKR_FILTER_LINEAR) hipLaunchKernelGGL(k_transfer_blit<true>, grid2d(a.dst.w, a.dst.h, block), block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_transfer_blit<false>, grid2d(a.dst.w, a.dst.h, block), block, 0, (hipStream_t)stream, a);
  return launch_status("blit_image");
}

template <int FMT> static int gen_mipmaps_launch(const Tex* lv, uint32_t mips, bool fused, hipStream_t stream) {
  if (!fused) {
    const dim3 block(64, 4);
    for (uint32_t m = 1; m < mips; m++) {
      hipLaunchKernelGGL(k_mips_level<FMT>, grid2d(lv[m].w, lv[m].h, block), block, 0, stream, lv[m - 1], lv[m]);
      VKR_TRY(launch_status("gen_mipmaps"));
    }
    return VKR_OK;
  }
  for (uint32_t s = 0; s + 1 < mips; s += MIP_FUSED_LEVELS) {
    MipFusedArgs a;
    a.src = lv[s];
    a.levels = (int)std::min<uint32_t>(MIP_FUSED_LEVELS, mips - 1 - s);
    for (int k = 0; k < MIP_FUSED_LEVELS; k++) a.dst[k] = lv[s + 1 + (uint32_t)(k < a.levels ? k : a.levels - 1)];
    const dim3 grid((a.dst[0].w + 31) / 32, (a.dst[0].h + 31) / 32);
    hipLaunchKernelGGL(k_mips_fused<FMT>, grid, dim3(256), 0, stream, a);
    VKR_TRY(launch_status("gen_mipmaps"));
  }
  return VKR_OK;
}

extern "C" int vkr_gen_mipmaps(const vkr_img* img, void* stream) {
  VKR_TRY(whole_image(img, "gen_mipmaps.img"));
  if (img->format == VKR_FMT_D24_UNORM_S8) { set_error("gen_mipmaps.img: D24_UNORM_S8 has no averaged mips (vkr_depth_mips builds the depth pyramid)"); return VKR_ERR_FORMAT; }
  bool has_rule = false;
  with_colour_format(img->format, [&](auto codec) { has_rule = codec.mips; });
  if (!has_rule) { set_error("gen_mipmaps.img: format %u has no mip rule", img->format); return VKR_ERR_FORMAT; }
  Tex lv[VKR_MAX_MIPS];
  for (uint32_t m = 0; m < img->mip_count; m++) {
    VKR_TRY(make_tex(img, (int)m, img->format, "gen_mipmaps.img", &lv[m]));
    // the chain's extents are those of the descriptor's own mip rule, max(1, s >> m) = max(1, previous / 2)
  }
  // the two schedules leave the same bytes; VKR_SWITCH_MIPS_PER_LEVEL / VKR_SWITCH_MIPS_FUSED force one (per level wins if both are set)
  const uint32_t sw = switches();
  const bool fused = (sw & VKR_SWITCH_MIPS_PER_LEVEL) ? false : (sw & VKR_SWITCH_MIPS_FUSED) ? true : VKR_MIPS_DEFAULT_FUSED != 0;
  const hipStream_t s = (hipStream_t)stream;
  int rc = VKR_OK;
  with_colour_format(img->format, [&](auto codec) {
    if constexpr (codec.mips) rc = gen_mipmaps_launch<(int)codec.format>(lv, img->mip_count, fused, s);
  });
  return rc;
}
