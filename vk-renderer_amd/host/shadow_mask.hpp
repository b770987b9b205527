// shadow_mask.hpp — ShadowMaskPass and create_shadow_mask_texture; like ssao.hpp, the declarations live in passes.hpp.
#pragma once
#include "passes.hpp"
