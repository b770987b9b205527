"""Deferred shading in the tiled frame (host/frame.hpp vkrh_tiled_set_shading), the parts that need no GPU: the C entries and
their Python wrappers, the NULL-handle answers, and the row reach of the pass across a strip boundary — re-derived here from
the uv arithmetic of defered_shading/shader.frag:103-130 (csrc/shading.hip) and held against the halo bound the C++ frame
refuses below."""
import inspect
import os
import re

import numpy as np
import pytest

from vk_renderer_amd import host, tiling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_enum(name):
    text = open(os.path.join(ROOT, "vk-renderer_amd", "host", "frame.hpp")).read()
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
    assert m, f"{name} is not in frame.hpp"
    return int(m.group(1))


def test_exports_and_wrappers_exist():
    lib = host.lib()
    assert hasattr(lib, "vkrh_tiled_set_shading") and hasattr(lib, "vkrh_tiled_shading")
    assert callable(host.HostFrame.tiled_set_shading) and callable(host.HostFrame.tiled_shading)
    assert inspect.signature(tiling.TiledFrame.__init__).parameters["shading"].default is False
    assert "skip_halos" in inspect.signature(tiling.native_lockstep_frame).parameters
    # six phases beside the five of the unshaded frame; the config struct the Python side mirrors did not grow
    assert _header_enum("VKRH_TILED_PHASES") == 5 and _header_enum("VKRH_TILED_PHASES_SHADED") == 6
    assert [n for n, _ in host.TiledConfig._fields_] == ["full_width", "full_height", "rank", "world", "halo", "gathered_mips", "force_tiled",
                                                        "albedo_by_gather", "stream", "comm", "row_bounds"]


def test_null_handle_is_an_error_with_a_message():
    lib = host.lib()
    assert lib.vkrh_tiled_set_shading(None, 1) != 0
    assert b"vkrh_tiled_set_shading: NULL tiled frame" in lib.vkrh_last_error()
    assert lib.vkrh_tiled_shading(None) < 0
    assert b"vkrh_tiled_shading: NULL tiled frame" in lib.vkrh_last_error()

    class NoHandle(host.HostFrame):  # the wrappers of a frame that is not native (its handle is None), without making a frame
        def __init__(self):
            self.tiled_handle = None

        def __del__(self):
            pass

    f = NoHandle()
    with pytest.raises(RuntimeError, match="NULL tiled frame"):
        f.tiled_set_shading(True)
    with pytest.raises(RuntimeError, match="NULL tiled frame"):
        f.tiled_shading()


def test_python_tiled_driver_refuses_shading():
    """the Python phases() order (what gloo runs) keeps the TAA ahead of the gather: it has no shaded order and says so before it
    makes a backend"""
    from vk_renderer_amd.camera import FrameSetup

    with pytest.raises(ValueError, match="native=True"):
        tiling.TiledFrame(FrameSetup(256, 320), 0, 2, 1, 2, None, shading=True)
    with pytest.raises(ValueError, match="host backend"):
        tiling.TiledFrame(FrameSetup(256, 320), 0, 1, 1, 1, None, backend=object, shading=True)


def _half_res_rows(gy, H):
    """Half-res rows the shading of full-res row gy reads of occlusion_tex / reflections_tex and of depth mip 1, in float32 as the
    kernel evaluates it: uv = (gy + 0.5) / H; hy = uv * (H / 2) - 0.5; the four textureLodOffset(…, 1, (0|1, 0|1)) taps are
    bilinear at hy and hy + 1, i.e. rows floor(hy) .. floor(hy) + 2, clamped to the image."""
    uv = (np.float32(gy) + np.float32(0.5)) / np.float32(H)
    hy = np.float32(uv * np.float32(H // 2)) - np.float32(0.5)
    y0 = int(np.floor(hy))
    rows = set()
    for oy in (0, 1):            # the offset of the tap
        for j in (0, 1):         # the two rows of its bilinear footprint
            rows.add(min(max(y0 + oy + j, 0), H // 2 - 1))
    return rows


@pytest.mark.parametrize("H", [320, 408, 480, 4320, 8640])
def test_row_reach_of_the_shading_across_a_strip_boundary(H):
    """color_out is needed on strip rows [y0 - 1, y1 + 1) (the TAA reads its four neighbours).  For those rows hy = y / 2 - 0.25:
    an even row 2k reads half-res rows k - 1 .. k + 1, an odd row 2k + 1 reads k .. k + 2.  Over a strip (even bounds) that is 1
    half-res row above its first and 2 below its last — both parities of y0 / 2 and of the row itself are walked."""
    # the per-row footprint, both parities, away from the frame's edge
    for k in (5, 6, H // 4, H // 4 + 1):
        assert _half_res_rows(2 * k, H) == {k - 1, k, k + 1}
        assert _half_res_rows(2 * k + 1, H) == {k, k + 1, k + 2}
    rows = [_half_res_rows(gy, H) for gy in range(H)]
    lo, hi = [min(r) for r in rows], [max(r) for r in rows]
    worst_above = worst_below = 0
    for y0 in range(2, H - 8, 2):                 # every even strip start: y0 / 2 takes both parities
        for y1 in (y0 + 2, y0 + 4, min(H - 2, y0 + 50)):  # ... and strips of both half-res parities
            if y1 <= y0:
                continue
            span = range(y0 - 1, y1 + 1)           # the rows of color_out the strip's TAA reads
            first, last = y0 // 2, y1 // 2 - 1     # the strip's own half-res rows
            worst_above = max(worst_above, first - min(lo[gy] for gy in span))
            worst_below = max(worst_below, max(hi[gy] for gy in span) - last)
    assert (worst_above, worst_below) == (1, 2)
    # the halo carries halo / 2 half-res rows either side: the bound the C++ frame refuses below, and its Python twin
    need_halo = 2 * max(worst_above, worst_below)
    assert need_halo == _header_enum("VKRH_TILED_SHADING_MIN_HALO") == tiling.SHADING_MIN_HALO
    assert tiling.HALO >= need_halo
    # full resolution: rows y0 - 1 .. y1 and the second row of their bilinear footprint stay inside the same halo
    assert need_halo >= 2
