// image_codec.hpp — the colour formats of vkr_postfx.h, each written once: its texel size, stored texel -> float RGBA
// (absent channels 0, 0, 0, 1) and float RGBA -> stored texel, with the library's exact decodes and store rules
// (vkr_device.hpp; DESIGN_NUMERICS.md, "Image transfers").  The passes that take an image of ANY colour format (the
// transfers, texdraw) go through with_colour_format(); a hot-path kernel whose formats are fixed keeps the Fmt* loaders of
// vkr_device.hpp.  D24_UNORM_S8 is not a colour format: whoever binds it handles it.
#pragma once
#include "../../include/vkr_postfx.h"
#include "vkr_device.hpp"

namespace vkr {

#define VKR_HOST_DEV __host__ __device__ __forceinline__

VKR_DEV Raw raw_words(uint32_t x, uint32_t y = 0u, uint32_t z = 0u, uint32_t w = 0u) { Raw r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
VKR_DEV uint32_t pack_unorm16x2(float a, float b) { return float_to_unorm16(a) | (float_to_unorm16(b) << 16); }

// Codec<FMT>: bpp; mips (vkr_gen_mipmaps has a rule for the format); decode(texel, lut) and encode(colour, thresh), where
// lut / thresh are the sRGB tables staged in LDS (only RGBA8_SRGB reads them)
template <uint32_t FMT, int BPP, bool MIPS> struct CodecTraits { static constexpr uint32_t format = FMT; static constexpr int bpp = BPP; static constexpr bool mips = MIPS; };
template <uint32_t FMT> struct Codec;
template <> struct Codec<VKR_FMT_RG16_UNORM> : CodecTraits<VKR_FMT_RG16_UNORM, 4, false> {
  static VKR_DEV f4 decode(const Raw& v, const float*) { return mk4(unorm16_to_float(v.x & 0xFFFFu), unorm16_to_float(v.x >> 16), 0.0f, 1.0f); }
  static VKR_DEV Raw encode(f4 c, const float*) { return raw_words(pack_unorm16x2(c.x, c.y)); } };
template <> struct Codec<VKR_FMT_RG16_SFLOAT> : CodecTraits<VKR_FMT_RG16_SFLOAT, 4, true> {
  static VKR_DEV f4 decode(const Raw& v, const float*) { return mk4(half_bits_to_float(v.x & 0xFFFFu), half_bits_to_float(v.x >> 16), 0.0f, 1.0f); }
  static VKR_DEV Raw encode(f4 c, const float*) { return raw_words(pack_half2(c.x, c.y)); } };
template <> struct Codec<VKR_FMT_RGBA8_SRGB> : CodecTraits<VKR_FMT_RGBA8_SRGB, 4, true> {
  static VKR_DEV f4 decode(const Raw& v, const float* lut) { return mk4(lut[v.x & 0xFFu], lut[(v.x >> 8) & 0xFFu], lut[(v.x >> 16) & 0xFFu], unorm8_to_float(v.x >> 24)); }
  static VKR_DEV Raw encode(f4 c, const float* thresh) { return raw_words(pack_srgb8(c, thresh)); } };
template <> struct Codec<VKR_FMT_RGBA8_UNORM> : CodecTraits<VKR_FMT_RGBA8_UNORM, 4, true> {
  static VKR_DEV f4 decode(const Raw& v, const float*) {
    return mk4(unorm8_to_float(v.x & 0xFFu), unorm8_to_float((v.x >> 8) & 0xFFu), unorm8_to_float((v.x >> 16) & 0xFFu), unorm8_to_float(v.x >> 24)); }
  static VKR_DEV Raw encode(f4 c, const float*) { return raw_words(float_to_unorm8(c.x) | (float_to_unorm8(c.y) << 8) | (float_to_unorm8(c.z) << 16) | (float_to_unorm8(c.w) << 24)); } };
template <> struct Codec<VKR_FMT_RGBA16_UNORM> : CodecTraits<VKR_FMT_RGBA16_UNORM, 8, false> {
  static VKR_DEV f4 decode(const Raw& v, const float*) {
    return mk4(unorm16_to_float(v.x & 0xFFFFu), unorm16_to_float(v.x >> 16), unorm16_to_float(v.y & 0xFFFFu), unorm16_to_float(v.y >> 16)); }
  static VKR_DEV Raw encode(f4 c, const float*) { return raw_words(pack_unorm16x2(c.x, c.y), pack_unorm16x2(c.z, c.w)); } };
template <> struct Codec<VKR_FMT_RGBA16_SFLOAT> : CodecTraits<VKR_FMT_RGBA16_SFLOAT, 8, true> {
  static VKR_DEV f4 decode(const Raw& v, const float*) {
    return mk4(half_bits_to_float(v.x & 0xFFFFu), half_bits_to_float(v.x >> 16), half_bits_to_float(v.y & 0xFFFFu), half_bits_to_float(v.y >> 16)); }
  static VKR_DEV Raw encode(f4 c, const float*) { return raw_words(pack_half2(c.x, c.y), pack_half2(c.z, c.w)); } };
template <> struct Codec<VKR_FMT_R16_SFLOAT> : CodecTraits<VKR_FMT_R16_SFLOAT, 2, true> {
  static VKR_DEV f4 decode(const Raw& v, const float*) { return mk4(half_bits_to_float(v.x), 0.0f, 0.0f, 1.0f); }
  static VKR_DEV Raw encode(f4 c, const float*) { return raw_words(float_to_half_bits(c.x)); } };
template <> struct Codec<VKR_FMT_R16_UNORM> : CodecTraits<VKR_FMT_R16_UNORM, 2, false> {
  static VKR_DEV f4 decode(const Raw& v, const float*) { return mk4(unorm16_to_float(v.x), 0.0f, 0.0f, 1.0f); }
  static VKR_DEV Raw encode(f4 c, const float*) { return raw_words(float_to_unorm16(c.x)); } };
template <> struct Codec<VKR_FMT_R32_SFLOAT> : CodecTraits<VKR_FMT_R32_SFLOAT, 4, true> {
  static VKR_DEV f4 decode(const Raw& v, const float*) { return mk4(__uint_as_float(v.x), 0.0f, 0.0f, 1.0f); }
  static VKR_DEV Raw encode(f4 c, const float*) { return raw_words(__float_as_uint(c.x)); } };
template <> struct Codec<VKR_FMT_R8_UNORM> : CodecTraits<VKR_FMT_R8_UNORM, 1, true> {
  static VKR_DEV f4 decode(const Raw& v, const float*) { return mk4(unorm8_to_float(v.x), 0.0f, 0.0f, 1.0f); }
  static VKR_DEV Raw encode(f4 c, const float*) { return raw_words(float_to_unorm8(c.x)); } };
template <> struct Codec<VKR_FMT_RGBA32_SFLOAT> : CodecTraits<VKR_FMT_RGBA32_SFLOAT, 16, false> {
  static VKR_DEV f4 decode(const Raw& v, const float*) { return mk4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)); }
  static VKR_DEV Raw encode(f4 c, const float*) { return raw_words(__float_as_uint(c.x), __float_as_uint(c.y), __float_as_uint(c.z), __float_as_uint(c.w)); } };

// fn(Codec<fmt>()) for a colour format, nothing for anything else; returns whether fmt is one.  The one switch over the colour
// formats, on the device (fmt is wave-uniform: a scalar branch) and on the host (whitelists, texel sizes, template dispatch).
template <class Fn> VKR_HOST_DEV bool with_colour_format(uint32_t fmt, Fn&& fn) {
  switch (fmt) {
    case VKR_FMT_RG16_UNORM: fn(Codec<VKR_FMT_RG16_UNORM>()); return true;
    case VKR_FMT_RG16_SFLOAT: fn(Codec<VKR_FMT_RG16_SFLOAT>()); return true;
    case VKR_FMT_RGBA8_SRGB: fn(Codec<VKR_FMT_RGBA8_SRGB>()); return true;
    case VKR_FMT_RGBA8_UNORM: fn(Codec<VKR_FMT_RGBA8_UNORM>()); return true;
    case VKR_FMT_RGBA16_UNORM: fn(Codec<VKR_FMT_RGBA16_UNORM>()); return true;
    case VKR_FMT_RGBA16_SFLOAT: fn(Codec<VKR_FMT_RGBA16_SFLOAT>()); return true;
    case VKR_FMT_R16_SFLOAT: fn(Codec<VKR_FMT_R16_SFLOAT>()); return true;
    case VKR_FMT_R16_UNORM: fn(Codec<VKR_FMT_R16_UNORM>()); return true;
    case VKR_FMT_R32_SFLOAT: fn(Codec<VKR_FMT_R32_SFLOAT>()); return true;
    case VKR_FMT_R8_UNORM: fn(Codec<VKR_FMT_R8_UNORM>()); return true;
    case VKR_FMT_RGBA32_SFLOAT: fn(Codec<VKR_FMT_RGBA32_SFLOAT>()); return true;
    default: return false;
  }
}
// bytes per texel of a colour format, 0 for anything else
inline uint32_t colour_format_bytes(uint32_t fmt) {
  uint32_t bpp = 0;
  with_colour_format(fmt, [&](auto codec) { bpp = (uint32_t)decltype(codec)::bpp; });
  return bpp;
}

}  // namespace vkr
