// texdraw.hip — program "texdraw", and the self-test of its sRGB encode.
//
// Reference: src/backbuffer_subpass2.cpp:15-52 and shaders/texdraw/shader.{vert,frag}: the last pass of the reference's frame
// (main.cpp:398) and its debug view.  One colour image of any format in, sampled once per destination pixel through the default
// sampler; all four channels or one of them out, stored to an 8-bit surface of any extent.  The sequence is frozen in
// DESIGN_NUMERICS.md (Texdraw).  Every pixel takes the whole bilinear footprint: cfma((g + 0.5) / W, W, -0.5) is not g for
// every g and W, so equal extents are no special case.
//
// Shape: one thread per destination texel, a wave 32 x 2 texels of a 32 x 8 block, blocks in the XCD-aware order.  Source and
// destination formats are wave-uniform switches of ONE kernel.  A footprint row of a format of at most 8 bytes is one load of
// the texel pair (pair_taps of vkr_device.hpp, for any texel size) where the source is at least two texels wide.  The sRGB
// tables go to LDS only when a side is sRGB.  The rgb encode is float_to_srgb8_fast (an estimate and ONE compare instead of
// the blit's eight dependent LDS reads); -DTEXDRAW_ENCODE_LDS builds the kernel with float_to_srgb8_lds, the variant
// tools/texdraw_timing.py measures it against.
//
// Roofline: HBM.  src + dst bytes once (12 B per pixel for RGBA16_SFLOAT -> RGBA8 at equal extents); DESIGN.md 7.6.
#include "vkr_host.hpp"

namespace vkr {

#define TEXDRAW_BX 32
#define TEXDRAW_BY 8

struct TexdrawArgs {
  Tex src, dst;
  uint32_t src_format, dst_format, src_bpp, flags;
};

// the stored bytes of one texel: `bpp` of them are meaningful, the rest is never read
struct Raw { uint32_t x, y, z, w; };
struct __attribute__((packed, aligned(2))) U16x2 { uint16_t x, y; };
struct __attribute__((packed, aligned(1))) U8x2 { uint8_t x, y; };

template <int BPP> VKR_DEV Raw load_texel(const uint8_t* p) {
  Raw r; r.x = r.y = r.z = r.w = 0u;
  if constexpr (BPP == 16) { const U32x4 v = load_u32x4(p); r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; }
  else if constexpr (BPP == 8) { const U32x2 v = load_u32x2(p); r.x = v.x; r.y = v.y; }
  else if constexpr (BPP == 4) r.x = *(const uint32_t*)p;
  else if constexpr (BPP == 2) r.x = *(const uint16_t*)p;
  else r.x = *p;
  return r;
}
// texels (x, y) and (x + 1, y) as ONE load; BPP <= 8
template <int BPP> VKR_DEV void load_texel_pair(const uint8_t* p, Raw& l, Raw& r) {
  l.x = l.y = l.z = l.w = 0u; r = l;
  if constexpr (BPP == 8) { const U32x4 v = load_u32x4(p); l.x = v.x; l.y = v.y; r.x = v.z; r.y = v.w; }
  else if constexpr (BPP == 4) { const U32x2 v = load_u32x2(p); l.x = v.x; r.x = v.y; }
  else if constexpr (BPP == 2) { const U16x2 v = *(const U16x2*)p; l.x = v.x; r.x = v.y; }
  else { const U8x2 v = *(const U8x2*)p; l.x = v.x; r.x = v.y; }
}

// the footprint of texture(t, uv): sample<>() of vkr_device.hpp up to the fetches
struct TexdrawFootprint { int x0, y0; float fx, fy; };
VKR_DEV TexdrawFootprint texdraw_footprint(const Tex& t, f2 uv) {
  TexdrawFootprint f;
  const float x = cfma(uv.x, (float)t.fw, -0.5f), y = cfma(uv.y, (float)t.fh, -0.5f);
  const float x0f = floorf(x), y0f = floorf(y);
  f.fx = x - x0f; f.fy = y - y0f;
  f.x0 = f2i(x0f); f.y0 = f2i(y0f);
  return f;
}
// the four stored texels t00, t10, t01, t11, clamp-to-edge.  pair (needs t.w >= 2): each row as the pair (xs, xs + 1),
// xs = clamp(x0, 0, w - 2); in the first and last column both taps are the same texel of the pair (pair_footprint).
template <int BPP> VKR_DEV void texdraw_taps(const Tex& t, const TexdrawFootprint& f, bool pair, Raw (&r)[4]) {
  const int ya = iclamp(f.y0, 0, t.h - 1), yb = iclamp(f.y0 + 1, 0, t.h - 1);
  if constexpr (BPP <= 8) {
    if (pair) {
      const int xs = iclamp(f.x0, 0, t.w - 2);
      const bool left_is_y = f.x0 > xs, right_is_x = f.x0 < xs;
      Raw a0, a1, b0, b1;
      load_texel_pair<BPP>(t.p + toff(t, xs, ya, BPP), a0, a1);
      load_texel_pair<BPP>(t.p + toff(t, xs, yb, BPP), b0, b1);
      r[0] = left_is_y ? a1 : a0; r[1] = right_is_x ? a0 : a1;
      r[2] = left_is_y ? b1 : b0; r[3] = right_is_x ? b0 : b1;
      return;
    }
  }
  const int xa = iclamp(f.x0, 0, t.w - 1), xb = iclamp(f.x0 + 1, 0, t.w - 1);
  r[0] = load_texel<BPP>(t.p + toff(t, xa, ya, BPP)); r[1] = load_texel<BPP>(t.p + toff(t, xb, ya, BPP));
  r[2] = load_texel<BPP>(t.p + toff(t, xa, yb, BPP)); r[3] = load_texel<BPP>(t.p + toff(t, xb, yb, BPP));
}
// rows first, then columns, all four channels of the decoded RGBA
template <class Decode> VKR_DEV f4 texdraw_mix(const Raw (&r)[4], float fx, float fy, Decode dec) {
  return mix4(mix4(dec(r[0]), dec(r[1]), fx), mix4(dec(r[2]), dec(r[3]), fx), fy);
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
  const TexdrawFootprint f = texdraw_footprint(a.src, uv);
  const bool pair = a.src.w >= 2;
  Raw r[4];
  switch (a.src_bpp) {
    case 1: texdraw_taps<1>(a.src, f, pair, r); break;
    case 2: texdraw_taps<2>(a.src, f, pair, r); break;
    case 4: texdraw_taps<4>(a.src, f, pair, r); break;
    case 8: texdraw_taps<8>(a.src, f, pair, r); break;
    default: texdraw_taps<16>(a.src, f, false, r); break;
  }
  f4 c;
  switch (a.src_format) {
    case VKR_FMT_RG16_UNORM:
      c = texdraw_mix(r, f.fx, f.fy, [](const Raw& v) { return mk4(unorm16_to_float(v.x & 0xFFFFu), unorm16_to_float(v.x >> 16), 0.0f, 1.0f); });
      break;
    case VKR_FMT_RG16_SFLOAT:
      c = texdraw_mix(r, f.fx, f.fy, [](const Raw& v) { return mk4(half_bits_to_float(v.x & 0xFFFFu), half_bits_to_float(v.x >> 16), 0.0f, 1.0f); });
      break;
    case VKR_FMT_RGBA8_SRGB:
      c = texdraw_mix(r, f.fx, f.fy, [&](const Raw& v) {
        return mk4(s_lut[v.x & 0xFFu], s_lut[(v.x >> 8) & 0xFFu], s_lut[(v.x >> 16) & 0xFFu], unorm8_to_float(v.x >> 24)); });
      break;
    case VKR_FMT_RGBA8_UNORM:
      c = texdraw_mix(r, f.fx, f.fy, [](const Raw& v) {
        return mk4(unorm8_to_float(v.x & 0xFFu), unorm8_to_float((v.x >> 8) & 0xFFu), unorm8_to_float((v.x >> 16) & 0xFFu), unorm8_to_float(v.x >> 24)); });
      break;
    case VKR_FMT_RGBA16_UNORM:
      c = texdraw_mix(r, f.fx, f.fy, [](const Raw& v) {
        return mk4(unorm16_to_float(v.x & 0xFFFFu), unorm16_to_float(v.x >> 16), unorm16_to_float(v.y & 0xFFFFu), unorm16_to_float(v.y >> 16)); });
      break;
    case VKR_FMT_RGBA16_SFLOAT:
      c = texdraw_mix(r, f.fx, f.fy, [](const Raw& v) {
        return mk4(half_bits_to_float(v.x & 0xFFFFu), half_bits_to_float(v.x >> 16), half_bits_to_float(v.y & 0xFFFFu), half_bits_to_float(v.y >> 16)); });
      break;
    case VKR_FMT_R16_SFLOAT: c = texdraw_mix(r, f.fx, f.fy, [](const Raw& v) { return mk4(half_bits_to_float(v.x), 0.0f, 0.0f, 1.0f); }); break;
    case VKR_FMT_R16_UNORM: c = texdraw_mix(r, f.fx, f.fy, [](const Raw& v) { return mk4(unorm16_to_float(v.x), 0.0f, 0.0f, 1.0f); }); break;
    case VKR_FMT_R32_SFLOAT: c = texdraw_mix(r, f.fx, f.fy, [](const Raw& v) { return mk4(__uint_as_float(v.x), 0.0f, 0.0f, 1.0f); }); break;
    case VKR_FMT_R8_UNORM: c = texdraw_mix(r, f.fx, f.fy, [](const Raw& v) { return mk4(unorm8_to_float(v.x), 0.0f, 0.0f, 1.0f); }); break;
    default:  // RGBA32_SFLOAT (the entry lets nothing else through)
      c = texdraw_mix(r, f.fx, f.fy, [](const Raw& v) { return mk4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)); });
      break;
  }

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
    word = texdraw_srgb8(c.x, s_thr) | (texdraw_srgb8(c.y, s_thr) << 8) | (texdraw_srgb8(c.z, s_thr) << 16) | (float_to_unorm8(c.w) << 24);
  } else {
    word = float_to_unorm8(c.x) | (float_to_unorm8(c.y) << 8) | (float_to_unorm8(c.z) << 16) | (float_to_unorm8(c.w) << 24);
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
  switch (target_tex->format) {
    case VKR_FMT_RG16_UNORM: case VKR_FMT_RG16_SFLOAT: case VKR_FMT_RGBA8_SRGB: case VKR_FMT_RGBA8_UNORM: case VKR_FMT_RGBA16_UNORM:
    case VKR_FMT_RGBA16_SFLOAT: case VKR_FMT_R16_SFLOAT: case VKR_FMT_R32_SFLOAT: case VKR_FMT_R8_UNORM: case VKR_FMT_RGBA32_SFLOAT:
    case VKR_FMT_R16_UNORM: break;
    case VKR_FMT_D24_UNORM_S8: set_error("texdraw.target_tex: D24_UNORM_S8 is not a colour format"); return VKR_ERR_FORMAT;
    default: set_error("texdraw.target_tex: unknown format %u", target_tex->format); return VKR_ERR_FORMAT;
  }
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
  if (a.dst.w > 65535 || a.dst.h > 65535) { set_error("texdraw: backbuffer is %dx%d, at most 65535 texels a side", a.dst.w, a.dst.h); return VKR_ERR_EXTENT; }
  for (const Tex* t : {&a.src, &a.dst})
    if (t->ox != 0 || t->oy != 0 || t->w != t->fw || t->h != t->fh) {
      set_error("texdraw: %s: windows are not supported (uv spans the whole image: a single-GPU pass)", t == &a.src ? "target_tex" : "backbuffer");
      return VKR_ERR_EXTENT;
    }
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
