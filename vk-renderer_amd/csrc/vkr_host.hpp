// vkr_host.hpp — host side of the C-ABI shim: descriptor validation, vkr_img -> device
// view conversion, launch error capture.  Shared by the per-pass .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include "../../include/vkr_postfx.h"
#include "vkr_device.hpp"

namespace vkr {

void set_error(const char* fmt, ...);
uint32_t switches();  // VKR_SWITCH_* (common.hip): the environment read once, then vkr_set_switches()

enum {
  VKR_OK = 0,
  VKR_ERR_NULL = 1001,      // a required descriptor / pointer is NULL
  VKR_ERR_FORMAT = 1002,    // an image has a format the program cannot bind
  VKR_ERR_EXTENT = 1003,    // extents / windows of the bound images do not agree
  VKR_ERR_MIPS = 1004,      // not enough mips (downsample_pass.cpp:37-39)
  VKR_ERR_LAYOUT = 1005     // pitch / offset / alignment of a descriptor is unusable
};

inline int mip_dim(uint32_t v, int i) { int r = (int)(v >> i); return r > 0 ? r : 1; }

// validated conversion of one mip of a descriptor
inline int make_tex(const vkr_img* d, int mip, uint32_t want_format, const char* what, Tex* out) {
  if (!d || !d->base) { set_error("%s: NULL image", what); return VKR_ERR_NULL; }
  if (d->format != want_format) { set_error("%s: format %u, expected %u", what, d->format, want_format); return VKR_ERR_FORMAT; }
  if (mip < 0 || mip >= (int)d->mip_count || d->mip_count > VKR_MAX_MIPS) { set_error("%s: mip %d not in view (%u mips)", what, mip, d->mip_count); return VKR_ERR_MIPS; }
  uint32_t bpp = vkr_format_bytes(d->format);
  int w = mip_dim(d->width, mip), h = mip_dim(d->height, mip);
  if (d->width == 0 || d->height == 0 || d->pitch_bytes[mip] < (uint32_t)w * bpp || (d->pitch_bytes[mip] % bpp) != 0 ||
      (((uintptr_t)d->base + d->mip_offset[mip]) % (bpp < 4 ? bpp : 4)) != 0) {
    set_error("%s: bad layout (w %d pitch %u)", what, w, d->pitch_bytes[mip]);
    return VKR_ERR_LAYOUT;
  }
  // texel offsets are 32-bit, rows x pitch a 24-bit multiply (toff() in vkr_device.hpp)
  if (d->pitch_bytes[mip] >= (1u << 24) || h >= (1 << 24) || (uint64_t)d->pitch_bytes[mip] * (uint64_t)h >= (1ull << 32)) {
    set_error("%s: window too large for 32-bit texel offsets (pitch %u x %d rows)", what, d->pitch_bytes[mip], h);
    return VKR_ERR_LAYOUT;
  }
  int fw = mip_dim(d->full_width, mip), fh = mip_dim(d->full_height, mip);
  int ox = d->origin_x >> mip, oy = d->origin_y >> mip;
  if (mip > 0 && d->origin_x >= 0 && d->origin_y >= 0) {
    // Mip extents are floor(extent / 2^mip), at least 1: where the frame's extent is not a multiple of 2^mip, a window
    // that starts in the last, partial texel of a coarse mip (or is shorter than one texel of it) would start past the
    // mip's last row.  Such a level holds no whole texel of the window; it is placed on the frame's last row / column so
    // that the chain can still be built (nothing reads it: a window's levels past the gathered ones are never sampled).
    if (ox + w > fw && w <= fw) ox = fw - w;
    if (oy + h > fh && h <= fh) oy = fh - h;
  }
  if (d->origin_x < 0 || d->origin_y < 0 || ox + w > fw || oy + h > fh) {
    set_error("%s: window (%d,%d)+(%d,%d) outside frame %dx%d at mip %d", what, ox, oy, w, h, fw, fh, mip);
    return VKR_ERR_EXTENT;
  }
  out->p = (const uint8_t*)d->base + d->mip_offset[mip];
  out->pitch = (int)d->pitch_bytes[mip];
  out->w = w; out->h = h; out->fw = fw; out->fh = fh; out->ox = ox; out->oy = oy;
  return VKR_OK;
}

inline bool same_window(const Tex& a, const Tex& b) {
  return a.w == b.w && a.h == b.h && a.fw == b.fw && a.fh == b.fh && a.ox == b.ox && a.oy == b.oy;
}

// same window AND row pitch: texel (x, y) has the same byte offset in both (4-byte formats share bilinear footprints)
inline bool same_layout(const Tex& a, const Tex& b) { return same_window(a, b) && a.pitch == b.pitch; }

// The window is the whole frame (the one statement of the test), and no side exceeds max_side texels.
inline bool whole_frame(int ox, int oy, int64_t w, int64_t h, int64_t fw, int64_t fh) { return ox == 0 && oy == 0 && w == fw && h == fh; }
inline bool whole_frame(const Tex& t, int max_side = INT32_MAX) { return whole_frame(t.ox, t.oy, t.w, t.h, t.fw, t.fh) && t.w <= max_side && t.h <= max_side; }
// The gate of a binding that cannot be a tile of the frame: "<what>: <why>" for a window, then the bound on the sides.
inline int require_whole_frame(const Tex& t, const char* what, const char* why, int max_side = INT32_MAX) {
  if (!whole_frame(t)) { set_error("%s: %s", what, why); return VKR_ERR_EXTENT; }
  if (!whole_frame(t, max_side)) { set_error("%s is %dx%d, at most %d texels a side", what, t.w, t.h, max_side); return VKR_ERR_EXTENT; }
  return VKR_OK;
}

// A whole-frame D24 depth pyramid as the Hi-Z marches bind it: 1 .. VKR_MAX_MIPS levels, every one the whole frame (rays have
// unbounded reach) and at most 65535 texels wide and high (the LDS level table keeps w | h << 16); padded to 16 entries.
inline int bind_depth_pyramid(const vkr_img* d, const char* program, const char* binding, Pyramid* out) {
  char what[96];
  std::snprintf(what, sizeof what, "%s.%s", program, binding);
  if (!d) { set_error("%s: NULL image", what); return VKR_ERR_NULL; }
  if (d->mip_count < 1 || d->mip_count > VKR_MAX_MIPS) { set_error("%s: %u mips (1 .. %d)", what, d->mip_count, VKR_MAX_MIPS); return VKR_ERR_MIPS; }
  out->count = (int)d->mip_count;
  for (int i = 0; i < out->count; i++) {
    Tex& m = out->mip[i];
    int rc = make_tex(d, i, VKR_FMT_D24_UNORM_S8, what, &m);
    if (rc != VKR_OK) return rc;
    if (!whole_frame(m, 65535)) {
      set_error("%s: level %d (%dx%d at (%d,%d) of %dx%d) must cover the whole frame, at most 65535 texels a side", what, i, m.w, m.h, m.ox, m.oy, m.fw, m.fh);
      return VKR_ERR_EXTENT;
    }
  }
  for (int i = out->count; i < 16; i++) out->mip[i] = out->mip[0];
  return VKR_OK;
}

inline void load_mat(Mat4& dst, const vkr_mat4& src) { std::memcpy(dst.m, src.m, sizeof(float) * 16); }

inline void load_proj(Proj& pr, float fovy, float aspect, float znear, float zfar) {
  pr.tg = tanf(fovy / 2.0f);
  pr.aspect = aspect; pr.znear = znear; pr.zfar = zfar;
}
inline void load_proj(Proj& pr, const float fovy_aspect_znear_zfar[4]) {
  load_proj(pr, fovy_aspect_znear_zfar[0], fovy_aspect_znear_zfar[1], fovy_aspect_znear_zfar[2], fovy_aspect_znear_zfar[3]);
}

// The extent a pass of 8 x 4 workgroups covers when the reference floors its group counts (gtao.cpp:145, w / 8 x h / 4
// groups): the ragged edge of the frame is not dispatched, and main.comp:54 derives its texture size from this extent.
inline int floor_dispatch_w(const Tex& t) { return (t.fw / 8) * 8; }
inline int floor_dispatch_h(const Tex& t) { return (t.fh / 4) * 4; }

// (cos, sin) of the 16 slice angles 2 PI (k / 16 + offset + turn), k = 16 * gtao_direction(pixel) (gtao_slice.hpp), host libm:
// main.comp:198,233 (turn = dir_index / dirs_count), main.frag:170 and rt_main.frag:89 (turn = 0)
inline void fill_slice_table(float (*cs)[2], float offset, float turn) {
  const float PI = 3.1415926535897932384626433832795f;
  for (int k = 0; k < 16; k++) {
    const float angle = (2.0f * PI) * (((1.0f / 16.0f) * (float)k + offset) + turn);
    cs[k][0] = cosf(angle);
    cs[k][1] = sinf(angle);
  }
}

inline int launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("%s: launch failed: %s", what, hipGetErrorString(e)); return (int)e; }
  return VKR_OK;
}

#define VKR_TRY(expr) do { int _rc = (expr); if (_rc != VKR_OK) return _rc; } while (0)

inline dim3 grid2d(int w, int h, dim3 block) { return dim3((w + block.x - 1) / block.x, (h + block.y - 1) / block.y, 1); }

}  // namespace vkr
