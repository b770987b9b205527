// backbuffer_subpass2.hpp — the tail of the reference's frame (main.cpp:398-401), public interface of
// src/backbuffer_subpass2.hpp:8-19 over the C-ABI program "texdraw" (DESIGN.md 7.6).
//
// add_backbuffer_subpass records task "BackbufSubpass": the graph's backbuffer as colour attachment, `draw_img` (mip 0, one
// level, layer 0) or `image` (the base level of a view of all its mips) sampled in the fragment stage at binding 0, the flags
// as 4 bytes of push constants, one full-screen triangle at the backbuffer's extent.  The reference clears the attachment to 0
// first (the triangle covers every pixel: never visible, the program does not execute it) and draws ImGui afterwards
// (imgui_draw of imgui_pass.hpp: the no-op shim).  add_present_subpass records task "presentPrepare", which executes nothing.
// The flags combine as the shader's four ifs do: the last set bit of R, G, B, A wins.
#ifndef BACKBUFF_SUBPASS2_HPP_INCLUDED
#define BACKBUFF_SUBPASS2_HPP_INCLUDED

#include "rendergraph/rendergraph.hpp"
#include "gpu/gpu.hpp"

enum class DrawTex { ShowAll = 0, ShowR = 1, ShowG = 2, ShowB = 4, ShowA = 8 };

void add_backbuffer_subpass(rendergraph::RenderGraph &graph, rendergraph::ImageResourceId draw_img, VkSampler sampler, DrawTex flags = DrawTex::ShowAll);
void add_backbuffer_subpass(rendergraph::RenderGraph &graph, gpu::ImagePtr &image, VkSampler sampler, DrawTex flags = DrawTex::ShowAll);
void add_present_subpass(rendergraph::RenderGraph &graph);

// the 4 bytes of push constants task "BackbufSubpass" records for `flags` (tests / diagnostics)
vkr_texdraw_push texdraw_push(DrawTex flags);

#endif
