// util_passes.hpp — the reference's transfer helpers (src/util_passes.hpp:9-12) on the rendergraph mirror:
//   gen_mipmaps  one task "Genmips" per destination level (transfer_read of level m - 1, transfer_write of level m)
//   clear_depth  task "Clear_depth"  (transfer_write of every mip and layer)
//   clear_color  task "Clear_color"  (transfer_write of every mip and layer)
//   blit_image   task "CopyImage"    (transfer_read of src mip 0, transfer_write of dst mip 0; LINEAR, like the reference)
// Each task calls the image-transfer entries of include/vkr_postfx.h (vkr_gen_mipmaps, vkr_clear_image, vkr_blit_image) on the
// command context's stream.
//
// gen_mipmaps follows the PROJECT's one mip rule (vk-renderer_amd/scene.py build_mips, vkr_gen_mipmaps): level extents
// max(1, s / 2), each texel ((a + b) + (c + d)) * 0.25 of its 2 x 2 block of the stored previous level.  It does NOT follow
// vkCmdBlitImage where an extent is odd (a linear blit would weight three source texels there).  One task per level keeps the
// reference's task list; every task is the chain of one level, so the bytes are those of vkr_gen_mipmaps on the whole image.
//
// gen_perlin_noise2D is not mirrored: its hash fract(sin(x) * 43758.5453) multiplies any difference between two sin
// implementations by about 4e4, so no parity statement is possible, and the reference never calls it.
#ifndef VKR_HOST_UTIL_PASSES_HPP_INCLUDED
#define VKR_HOST_UTIL_PASSES_HPP_INCLUDED

#include "rendergraph/rendergraph.hpp"

void gen_mipmaps(rendergraph::RenderGraph &graph, rendergraph::ImageResourceId image);
void clear_depth(rendergraph::RenderGraph &graph, rendergraph::ImageResourceId image, float val = 1.0);
void clear_color(rendergraph::RenderGraph &graph, rendergraph::ImageResourceId image, VkClearColorValue val);
void blit_image(rendergraph::RenderGraph &graph, rendergraph::ImageResourceId src, rendergraph::ImageResourceId dst);

#endif
