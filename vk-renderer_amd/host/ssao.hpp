// ssao.hpp — kept so that `#include "ssao.hpp"` of the reference's sources resolves; the declarations live in passes.hpp.
#pragma once
#include "passes.hpp"
