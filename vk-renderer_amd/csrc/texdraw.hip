// texdraw.hip — program "texdraw", and the self-test of its sRGB encode.
//
// Reference: src/backbuffer_subpass2.cpp:15-52 and shaders/texdraw/shader.{vert,frag}: the last pass of the reference's frame
// (main.cpp:398) and its debug view.  One colour image of any format in, sampled once per destination pixel through the default
// sampler; all four channels or one of them out, stored to an 8-bit surface of any extent.  The sequence is frozen in
// DESIGN_NUMERICS.md (Texdraw).  Every pixel takes the whole bilinear footprint: cfma((g + 0.5) / W, W, -0.5) is not g for
// every g and W, so equal extents are no special case.
//
// Shape: one thread per destination texel, a wave 32 x 2 texels of a 32 x 8 block, blocks in the XCD-aware order.  Source and
// destination formats are wave-uniform switches of ONE kernel (the source's decode: image_codec.hpp).  A footprint row of a format of at most 8 bytes is one load of
// the texel pair (pair_taps_raw of vkr_device.hpp, for any texel size) where the source is at least two texels wide.  The sRGB
// tables go to LDS only when a side is sRGB.  The rgb encode is float_to_srgb8_fast (an estimate and ONE compare instead of
// the blit's eight dependent LDS reads); -DTEXDRAW_ENCODE_LDS builds the kernel with float_to_srgb8_lds, the variant
// tools/texdraw_timing.py measures it against.
//
// Roofline: HBM.  src + dst bytes once (12 B per pixel for RGBA16_SFLOAT -> RGBA8 at equal extents); DESIGN.md 7.6.
#include "vkr_host.hpp"
#include "image_codec.hpp"

namespace vkr {

#define TEXDRAW_BX 32
#define TEXDRAW_BY 8

struct TexdrawArgs {
  Tex src, dst;
  uint32_t src_format, dst_format, src_bpp, flags;
};

// the four stored texels t00, t10, t01, t11 of the footprint, clamp-to-edge.  pair (needs t.w >= 2): each row as one load of
// the texel pair (pair_rows of vkr_device.hpp; the image is whole, so frame coordinates are window coordinates)
template <int BPP> VKR_DEV void texdraw_taps(const Tex& t, const Footprint& f, bool pair, Raw (&r)[4]) {
  if constexpr (BPP <= 8) {
    if (pair) { pair_taps_raw<BPP>(t, pair_rows<BPP>(t, f), r); return; }
  }
  const int ya = iclamp(f.y0, 0, t.h - 1), yb = iclamp(f.y0 + 1, 0, t.h - 1);
  const int xa = iclamp(f.x0, 0, t.w - 1), xb = iclamp(f.x0 + 1, 0, t.w - 1);
  r[0] = load_raw<BPP>(t.p + toff(t, xa, ya, BPP)); r[1] = load_raw<BPP>(t.p + toff(t, xb, ya, BPP));
  r[2] = load_raw<BPP>(t.p + toff(t, xa, yb, BPP)); r[3] = load_raw<BPP>(t.p + toff(t, xb, yb, BPP));
}

VKR_DEV uint32_t texdraw_srgb8(float x, const float* thresh) {
#ifdef TEXDRAW_ENCODE_LDS
  return float_to_srgb8_lds(x, thresh);
#else
  return float_to_srgb8_fast(x, thresh);
#endif
}

// shader.frag:19-34, one thread per backbuffer texel
__global__ __launch_bounds__(TEXDRAW_BX * TEXDRAW_BY) void k_texdraw(TexdrawArgs a) {
  __shared__ float s_lut[VKR_SRGB_LUT_SIZE], s_thr[VKR_SRGB_LUT_SIZE];
  const int tid = threadIdx.y * TEXDRAW_BX + threadIdx.x;
  const bool src_srgb = a.src_format == VKR_FMT_RGBA8_SRGB, dst_srgb = a.dst_format == VKR_FMT_RGBA8_SRGB;
  if (src_srgb) srgb_lut_stage(s_lut, tid, TEXDRAW_BX * TEXDRAW_BY);
  if (dst_srgb) srgb_thresh_stage(s_thr, tid, TEXDRAW_BX * TEXDRAW_BY);
  if (src_srgb || dst_srgb) __syncthreads();
  const i2 blk = xcd_block<4, 8>();  // chunks of 128 x 64 texels
  const int x = blk.x * TEXDRAW_BX + threadIdx.x, y = blk.y * TEXDRAW_BY + threadIdx.y;
  if (x >= a.dst.w || y >= a.dst.h) return;

  const f2 uv = mk2(pixel_centre_uv(x, (float)a.dst.w), pixel_centre_uv(y, (float)a.dst.h));
  const Footprint f = bilinear_footprint(a.src, uv);
  const bool pair = a.src.w >= 2;
  Raw r[4];
  switch (a.src_bpp) {
    case 1: texdraw_taps<1>(a.src, f, pair, r); break;
    case 2: texdraw_taps<2>(a.src, f, pair, r); break;
    case 4: texdraw_taps<4>(a.src, f, pair, r); break;
    case 8: texdraw_taps<8>(a.src, f, pair, r); break;
    default: texdraw_taps<16>(a.src, f, false, r); break;
  }
  f4 c = mk4(0.0f, 0.0f, 0.0f, 1.0f);  // rows first, then columns, all four channels of the decoded RGBA
  with_colour_format(a.src_format, [&](auto codec) {
    auto dec = [&](const Raw& v) { return codec.decode(v, s_lut); };
    c = mix4(mix4(dec(r[0]), dec(r[1]), f.fx), mix4(dec(r[2]), dec(r[3]), f.fx), f.fy);
  });

  // the shader's four ifs in order: the last set bit wins, a shown channel goes to all four outputs
  const uint32_t fl = a.flags;
  const bool one = (fl & (VKR_TEXDRAW_SHOW_R | VKR_TEXDRAW_SHOW_G | VKR_TEXDRAW_SHOW_B | VKR_TEXDRAW_SHOW_A)) != 0u;
  const float s = (fl & VKR_TEXDRAW_SHOW_A) ? c.w : (fl & VKR_TEXDRAW_SHOW_B) ? c.z : (fl & VKR_TEXDRAW_SHOW_G) ? c.y : c.x;
  uint32_t word;
  if (one) {  // rgb hold one value: one encode
    const uint32_t lin = float_to_unorm8(s);
    const uint32_t col = dst_srgb ? texdraw_srgb8(s, s_thr) : lin;
    word = col | (col << 8) | (col << 16) | (lin << 24);
  } else if (dst_srgb) {
    word = pack_srgb8(c, s_thr, texdraw_srgb8);
  } else {
    word = Codec<VKR_FMT_RGBA8_UNORM>::encode(c, nullptr).x;
  }
  *texel_ptr<uint32_t>(a.dst, x, y) = word;
}

// every fp32 bit pattern through both sRGB encodes; *counter += the number of disagreements
__global__ __launch_bounds__(256) void k_selftest_srgb_encode(uint32_t* counter) {
  __shared__ float s_thr[VKR_SRGB_LUT_SIZE];
  srgb_thresh_stage(s_thr, threadIdx.x, 256);
  __syncthreads();
  uint32_t bad = 0u;
  for (uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x; b < (1ull << 32); b += (uint64_t)gridDim.x * 256u) {
    const float x = __uint_as_float((uint32_t)b);
    if (float_to_srgb8_fast(x, s_thr) != float_to_srgb8_lds(x, s_thr)) ++bad;
  }
  if (bad) atomicAdd(counter, bad);
}

}  // namespace vkr

using namespace vkr;

extern "C" int vkr_texdraw(const vkr_img* target_tex, const vkr_img* backbuffer, const vkr_texdraw_push* push, void* stream) {
  if (!target_tex) { set_error("texdraw: target_tex is NULL"); return VKR_ERR_NULL; }
  if (!backbuffer) { set_error("texdraw: backbuffer is NULL"); return VKR_ERR_NULL; }
  if (!push) { set_error("texdraw: push is NULL"); return VKR_ERR_NULL; }
  if (target_tex->format == VKR_FMT_D24_UNORM_S8) { set_error("texdraw.target_tex: D24_UNORM_S8 is not a colour format"); return VKR_ERR_FORMAT; }
  if (colour_format_bytes(target_tex->format) == 0) { set_error("texdraw.target_tex: unknown format %u", target_tex->format); return VKR_ERR_FORMAT; }
  if (backbuffer->format != VKR_FMT_RGBA8_SRGB && backbuffer->format != VKR_FMT_RGBA8_UNORM) {
    set_error("texdraw.backbuffer: format %u, expected RGBA8_SRGB (%u) or RGBA8_UNORM (%u)", backbuffer->format, VKR_FMT_RGBA8_SRGB, VKR_FMT_RGBA8_UNORM);
    return VKR_ERR_FORMAT;
  }
  for (const vkr_img* d : {target_tex, backbuffer})
    if (d->base && (d->width == 0 || d->height == 0)) {
      set_error("texdraw.%s: zero extent (%ux%u)", d == target_tex ? "target_tex" : "backbuffer", d->width, d->height);
      return VKR_ERR_EXTENT;
    }
  TexdrawArgs a;
  VKR_TRY(make_tex(target_tex, 0, target_tex->format, "texdraw.target_tex", &a.src));
  VKR_TRY(make_tex(backbuffer, 0, backbuffer->format, "texdraw.backbuffer", &a.dst));
  VKR_TRY(require_whole_frame(a.src, "texdraw: target_tex", "windows are not supported (uv spans the whole image: a single-GPU pass)"));
  VKR_TRY(require_whole_frame(a.dst, "texdraw: backbuffer", "windows are not supported (uv spans the whole image: a single-GPU pass)", 65535));
  if (a.src.p == a.dst.p) { set_error("texdraw: target_tex and backbuffer are the same memory"); return VKR_ERR_LAYOUT; }
  a.src_format = target_tex->format; a.dst_format = backbuffer->format;
  a.src_bpp = vkr_format_bytes(target_tex->format);
  a.flags = push->flags;
  const dim3 block(TEXDRAW_BX, TEXDRAW_BY);
  hipLaunchKernelGGL(k_texdraw, grid2d(a.dst.w, a.dst.h, block), block, 0, (hipStream_t)stream, a);
  return launch_status("texdraw");
}

extern "C" int vkr_selftest_srgb_encode(uint32_t* device_counter, void* stream) {
  if (!device_counter) { set_error("selftest_srgb_encode: NULL counter"); return VKR_ERR_NULL; }
  hipLaunchKernelGGL(k_selftest_srgb_encode, dim3(8192), dim3(256), 0, (hipStream_t)stream, device_counter);
  return launch_status("selftest_srgb_encode");
}
