// ssr_sampling.hpp — what the stochastic SSR trace kernels share around the march: the ray set-up
// (trace.comp / trace_indirect.comp :61-84,143-158 and brdf.glsl:135-155), the hit tests (:94-118) and the ray store.
#pragma once
#include "hiz_march.hpp"

namespace vkr {

// brdf.glsl:135-155; cos/sin(phi), phi = 2*PI*U2, come with the Halton entry (vkr_halton23_fill:
// evaluated in double on the host and rounded once — they steer the march)
VKR_DEV f3 sampleGGXVNDF(f3 Ve, float alpha_x, float alpha_y, float U1, float cos_phi, float sin_phi) {
  f3 Vh = normalize(mk3(alpha_x * Ve.x, alpha_y * Ve.y, Ve.z));
  float lensq = Vh.x * Vh.x + Vh.y * Vh.y;
  f3 T1 = lensq > 0.0f ? mk3(-Vh.y, Vh.x, 0.0f) * (1.0f / sqrt_ieee(lensq)) : mk3(1, 0, 0);
  f3 T2 = cross(Vh, T1);
  float r = sqrt_ieee(U1);
  float t1 = r * cos_phi;
  float t2 = r * sin_phi;
  float s = 0.5f * (1.0f + Vh.z);
  t2 = (1.0f - s) * sqrt_ieee(1.0f - t1 * t1) + s * t2;
  f3 Nh = (t1 * T1 + t2 * T2) + sqrt_ieee(vmax(0.0f, (1.0f - t1 * t1) - t2 * t2)) * Vh;
  return normalize(mk3(alpha_x * Nh.x, alpha_y * Nh.y, vmax(0.0f, Nh.z)));
}

// trace.comp:61-84: the pixel's Halton entry, its tangent frame, the VNDF sample and the reflected direction R (returned);
// fills the ray's start and direction in screen space.  rc.normal and rc.view_vec are the pixel's (:49-58).
VKR_DEV f3 setup_ray(RayConst& rc, f2 screen_uv, float roughness, const float4* halton, uint32_t frame_random, const Proj& pr, float f_over_fn) {
  // trace.comp:61-63,156-158: rand() -> Halton index; sin evaluated in double (it picks the entry)
  const float rdot = dot(screen_uv, mk2(12.9898f, 78.233f));
  const float rnd01 = fractf(sin_hash_arg(rdot) * 43758.5453f);
  const uint32_t index = (f2u(rnd01 * (float)VKR_HALTON_SEQ_SIZE) + frame_random) & (VKR_HALTON_SEQ_SIZE - 1);
  const float4 hv = halton[index];

  // trace.comp:65-77
  f3 tangent, bitangent;
  tangent_frame(rc.normal, &tangent, &bitangent);
  f3 view_dir = -normalize(rc.view_vec);
  view_dir = mk3(dot(view_dir, tangent), dot(view_dir, bitangent), dot(view_dir, rc.normal));
  const f3 brdf_norm = sampleGGXVNDF(view_dir, roughness, roughness, hv.x, hv.z, hv.w);
  const f3 N = (brdf_norm.x * tangent + brdf_norm.y * bitangent) + brdf_norm.z * rc.normal;
  const f3 R = reflect(rc.view_vec, N);

  // trace.comp:79-84
  f3 ray_start = project_view_vec(rc.view_vec + 0.001f * rc.normal, pr, f_over_fn);
  ray_start.z -= 0.0001f;
  f3 ray_dir = project_view_vec(rc.view_vec + R, pr, f_over_fn) - ray_start;
  ray_dir = ray_dir * ((1.0f - ray_start.z) / ray_dir.z);
  rc.origin = ray_start;
  rc.direction = ray_dir;
  rc.inv_direction = safe_inverse(ray_dir);
  return R;
}

// The hit tests of trace.comp:94-118, one predicate each; the callers decide their order.
// :94-99: the ray moved at least 2 px on one axis
VKR_DEV bool ray_moved(f3 out_ray, f3 ray_start, f2 tex_size) {
  const f2 ray_step = mk2(fabsf(out_ray.x - ray_start.x) * tex_size.x, fabsf(out_ray.y - ray_start.y) * tex_size.y);
  return !(vmax(ray_step.x, ray_step.y) < 2.0f);
}
// :101-109: the surface at the hit faces away from the ray (texture(normal, hit uv), not normalised)
VKR_DEV bool hit_faces_away(const Tex& normal, const Mat4& normal_mat, f2 hit_uv, f3 R) {
  return dot(sample_view_normal_raw(normal, normal_mat, hit_uv), R) > 0.0f;
}
// :111-118: the ray ends at most 0.3 behind and 0.1 in front of the surface at the hit (linear depth)
VKR_DEV bool hit_depth_in_window(const Tex& depth0, f3 out_ray, const Proj& pr) {
  const float hit_z = linearize_depth2_unorm(sample<FmtD24>(depth0, xy(out_ray)), pr.znear, pr.zfar);
  const float ray_z = linearize_depth2(out_ray.z, pr.znear, pr.zfar);
  return !(ray_z > hit_z + 0.3f || ray_z < hit_z - 0.1f);
}
// the RGBA16_UNORM ray texel (advanced_ssr.cpp:62): hit position, and the pixel's depth where the hit is valid, else 1
VKR_DEV void store_ray(const Tex& out, int lx, int ly, f3 out_ray, bool valid_hit, float pixel_depth) {
  uint2 o;
  o.x = float_to_unorm16(out_ray.x) | (float_to_unorm16(out_ray.y) << 16);
  o.y = float_to_unorm16(out_ray.z) | (float_to_unorm16(valid_hit ? pixel_depth : 1.0f) << 16);
  *texel_ptr<uint2>(out, lx, ly) = o;
}

}  // namespace vkr
