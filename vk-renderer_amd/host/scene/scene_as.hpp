// scene/scene_as.hpp — the scene's acceleration structure, interface of src/scene/scene_as.hpp:8-24.
//
// The reference builds one bottom-level structure per mesh and a top-level one over the flattened node tree
// (scene_as.cpp:144-157) for VK_KHR_ray_query.  MI355X has no ray-tracing hardware; the ray query is a software traversal of
// the project's own structure (include/vkr_postfx.h vkr_accel, csrc/accel.hip).  For an any-hit query of a static scene two
// levels add nothing, so build_blas() only gathers each mesh's triangles in object space and build_tlas() flattens every node
// into ONE world-space structure:
//   * node transforms are composed as flattern_nodes does: pre_transform * node.transform, children after their parent;
//   * triangle j of primitive p reads vertices vertex_offset + indices[index_offset + 3j + k] (firstVertex of the build
//     range); every triangle is opaque and double-sided, alpha clipping is ignored (scene_as.cpp:57,172);
//   * a vertex goes to world space in fp32 on the host as ((m00 x + m01 y) + m02 z) + m03 per row (each product and sum
//     rounded, no fused multiply-add) — vk-renderer_amd/abi.py scene_triangles() restates it in numpy.
// `tlas` names the structure (a vkr_accel*) that gtao_rt_main binds at binding 3.
#ifndef SCENE_AS_HPP_INCLUDED
#define SCENE_AS_HPP_INCLUDED

#include <vector>

#include "../passes.hpp"

namespace scene {

struct SceneAccelerationStructure {
  SceneAccelerationStructure() = default;
  SceneAccelerationStructure(const SceneAccelerationStructure &) = delete;
  SceneAccelerationStructure &operator=(const SceneAccelerationStructure &) = delete;
  ~SceneAccelerationStructure();

  void build(gpu::TransferCmdPool &transfer_pool, const CompiledScene &source);
  void build_blas(gpu::TransferCmdPool &transfer_pool, const BaseMesh &mesh, const CompiledScene &source);
  void build_tlas(gpu::TransferCmdPool &transfer_pool, const CompiledScene &source);

  // object-space triangles of each mesh, in build_blas() order (9 floats per triangle)
  std::vector<std::vector<float>> blas_triangles;
  // Moves the structure to the pose the node transforms of `source` have NOW, without building it again (vkr_accel_refit): the
  // nodes are flattened as build_tlas() does, vkr_scene_triangles makes the world-space triangles on the device from source's
  // vertex and index buffers (one draw per primitive, node by node, within a node the mesh's primitives in order: the order of
  // build_tlas(); the model matrices travel in a table of the structure's own), and `tlas` is refitted to them, all on `stream`
  // and without a synchronisation.  Only transforms may have changed since build(): another number of triangles is an error (the
  // escape is build()).  hit_attributes is untouched: uvs and textures do not move.  hit_normals moves with the draws:
  // vkr_scene_triangle_normals recomputes it in place from the same draw list, with transpose(inverse(transform)) of every node as
  // its normal matrix, on `stream` like the triangles.
  void refit(const CompiledScene &source, void *stream);
  // the triangles the structure holds on the device after the last refit(), 9 floats per triangle in the order of
  // world_triangles (synchronises `stream`); before any refit() it is world_triangles
  std::vector<float> download_world_triangles(void *stream);

  // the world-space triangles build_tlas() put into the structure (9 floats per triangle).  They stay AS BUILT: refit() does not
  // touch them (the moved ones exist on the device only; download_world_triangles() reads them back)
  std::vector<float> world_triangles;
  VkAccelerationStructureKHR tlas {nullptr};

  // What a closest-hit query needs to shade its hit (program "reflections_rt"): one vkr_hit_attrib per triangle, in the order of
  // world_triangles — the uv of its three vertices and the albedo texture index of its primitive's material (0xFFFFFFFF: none).  A
  // mesh drawn by several nodes yields one record per instance.  blas_attributes: per mesh, in build_blas() order; hit_attributes:
  // the table on the device, uploaded once by build_tlas() (one unused record for a scene without triangles) — vk-renderer_amd/abi.py
  // scene_triangle_attributes() restates it in numpy.
  std::vector<std::vector<vkr_hit_attrib>> blas_attributes;
  std::vector<vkr_hit_attrib> world_attributes;
  gpu::BufferPtr hit_attributes;

  // What a lit hit needs besides (program "reflections_rt_lit"): one vkr_hit_normal per triangle, in the order of world_triangles —
  // the world-space normals of its three vertices, transpose(inverse(node transform)) * norm per row as (m0 x + m1 y) + m2 z in
  // fp32, not normalised (vkr_scene_triangle_normals' rule, which refit() applies on the device; vk-renderer_amd/abi.py
  // scene_triangle_normals() restates it in numpy).  blas_normals: per mesh, object space, 9 floats per triangle; hit_normals: the
  // table on the device, made by build_tlas() (one unused record for a scene without triangles).
  std::vector<std::vector<float>> blas_normals;
  std::vector<vkr_hit_normal> world_normals;
  gpu::BufferPtr hit_normals;
  // the table as it is on the device now (synchronises `stream`)
  std::vector<vkr_hit_normal> download_hit_normals(void *stream);

  // refit(): the moved triangles and the draw table of vkr_scene_triangles, on the device, allocated by the first refit()
  gpu::BufferPtr refit_triangles, refit_scratch;
};

}  // namespace scene

#endif
