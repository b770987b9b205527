"""One frame cut into horizontal strips, driven kernel by kernel through the request / reply round of the multi-GPU frame on
either backend: what tests/test_hit_exchange_gpu.py does for two equal strips of the synthetic scene, shared, and extended to
uneven strips holding the adversarial content of tests/gbuffer_content.py.

strip_chains() cuts a plain chain's G-buffer into per-rank window chains (each runs its own downsample; the whole-frame pyramid
comes from the plain chain as the all-gather would deliver it; the whole-frame albedo / normal images hold the rank's own rows
and poison elsewhere).  run_round() is the round of every rank: windowed trace, counts, requests, replies from each owner's
window, scatter, deferred normal test, filter."""
import functools

import numpy as np

import gbuffer_content as gc
from vk_renderer_amd.chain import PostFxChain

POISON = 0xA5
GBUFFER = ("depth", "prev_depth", "normal", "albedo", "material", "velocity")
# frame size -> (row bounds of three uneven strips, halo rows)
CUTS = {(206, 226): ([0, 64, 150, 226], 16), (70, 38): ([0, 12, 26, 38], 8)}
CLASSES = ("sky_all", "checker_px", "checker_tile", "depth_noise", "normal_noise", "normal_poles", "material_extremes", "all_noise", None)
CASES = [(name, size) for size in CUTS for name in CLASSES]


def case_id(case):
    return f"{case[0] or 'synthetic'}-{case[1][0]}x{case[1][1]}"


def window(bounds, rank, halo, width, height):
    y0, y1 = max(0, bounds[rank] - halo), min(height, bounds[rank + 1] + halo)
    return (0, y0, width, y1 - y0)


def gather(plain, c):
    """what the exchanges before the trace leave in window chain `c`: the whole-frame pyramid (plain's depth mips 1 .. L - 1, its
    tail rebuilt locally) and the rank's own rows of the whole-frame albedo / downsampled normals (poison elsewhere: a texel
    nobody delivers shows)"""
    src, dst = plain.depth, c.frame_hiz
    src_host, host = src.to_host(), dst.to_host().copy()
    for m in range(dst.mips):
        h = max(1, (plain.H // 2) >> m)
        assert src.pitch[m + 1] == dst.pitch[m]
        host[dst.offset[m]: dst.offset[m] + dst.pitch[m] * h] = src_host[src.offset[m + 1]: src.offset[m + 1] + src.pitch[m + 1] * h]
    dst.upload(host)
    c.hiz_tail(4)
    for src, dst in ((c.albedo, c.frame_albedo), (c.dn, c.frame_normals)):
        host = np.full(dst.nbytes, POISON, dtype=np.uint8)
        o = src.origin[1] * dst.pitch[0]
        host[o: o + src.height * src.pitch[0]] = src.to_host()[: src.height * src.pitch[0]]
        dst.upload(host)


def strip_chains(plain, backend, device, bounds, halo, pdf):
    """a window chain per strip holding the window's rows of plain's G-buffer (plain: downsampled already)"""
    W, H = plain.W, plain.H
    ranks = []
    for r in range(len(bounds) - 1):
        c = PostFxChain(W, H, backend=backend, device=device, setup=plain.setup, window=window(bounds, r, halo, W, H), force_tiled=True)
        c.pdf.upload(pdf)
        oy, wh = c.window[1], c.window[3]
        for name in GBUFFER:
            src, dst = getattr(plain, name), getattr(c, name)
            assert src.pitch[0] == dst.pitch[0]
            host = dst.to_host().copy()
            host[: wh * dst.pitch[0]] = src.to_host()[oy * src.pitch[0]: (oy + wh) * src.pitch[0]]  # (mip 0; the rest is downsample()'s)
            dst.upload(host)
        c.downsample()
        gather(plain, c)
        ranks.append(c)
    return ranks


def pending_floats(c):
    """[h, w, 8] float32 of the pending data: R at [0:3], the hit uv at [4:6]"""
    d = c.pend_data
    rows = d.to_host()[: d.pitch[0] * d.height].reshape(d.height, d.pitch[0])[:, : d.width * 16]
    return np.ascontiguousarray(rows).view(np.float32).reshape(d.height, d.width // 2, 8)


def run_round(ranks, bounds):
    """-> per rank: what the windowed trace stored, the counts and requests, the error words of the owners, and what validate and
    the filter leave"""
    out = []
    for c in ranks:
        c.ssr_trace_windowed(frame_random=0)
        c.sync()
        r = {"row0": c.rays.origin[1], "rays": c.rays.raw(0).copy(), "raw": c.raw.decode(0).copy(), "mask": c.pend_mask.raw(0)[..., 0].copy(), "pend": pending_floats(c).copy()}
        r["counts"] = c.hit_count(bounds)
        q, seg = c.hit_write(bounds, r["counts"])
        r["requests"] = [np.sort(c.buffer_to_host(q).view(np.uint32)[seg[o]: seg[o + 1]]) for o in range(len(ranks))]
        r["errors"] = 0
        for o, owner in enumerate(ranks):
            n = seg[o + 1] - seg[o]
            if n == 0:
                continue
            mine = q[seg[o]: seg[o + 1]]
            rep, err = owner.hit_reply(mine, n)
            r["errors"] += err
            c.hit_scatter(mine, rep, n)
        c.ssr_validate()
        c.ssr_filter()
        c.sync()
        r["validated"], r["reflections"] = c.rays.raw(0).copy(), c.reflections.raw(0).copy()
        r["frame_albedo"], r["frame_normals"] = c.frame_albedo.raw(0).copy(), c.frame_normals.raw(0).copy()
        out.append(r)
    return out


@functools.lru_cache(maxsize=1)
def _pdf():
    c = PostFxChain(64, 64, backend="oracle")
    c.preintegrate_pdf()
    return c.pdf.to_host().copy()


@functools.lru_cache(maxsize=None)
def oracle_round(name, size):
    """the plain oracle frame of class `name` (None: the synthetic scene) and the round of its three strips on the oracle twin,
    computed once -> (plain chain after trace and filter, [per-rank results])"""
    bounds, halo = CUTS[size]
    plain = gc.prepare(name, size, pdf=_pdf())
    plain.downsample()
    ranks = strip_chains(plain, "oracle", None, bounds, halo, _pdf())
    plain.ssr_trace(frame_random=0)
    plain.ssr_filter()
    return plain, run_round(ranks, bounds)


def interior(size, rank, chain_origin_row):
    """the half-res rows of strip `rank` as a slice of a window image whose first row is half-res frame row chain_origin_row"""
    bounds, _ = CUTS[size]
    return slice(bounds[rank] // 2 - chain_origin_row, bounds[rank + 1] // 2 - chain_origin_row)
