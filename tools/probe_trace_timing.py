#!/usr/bin/env python3
"""Times the octahedral probe programs (csrc/probe.hip) with HIP events.

    python tools/probe_trace_timing.py --out profiles/probe_trace.json [--reps 20]
    python tools/probe_trace_timing.py --bake-from-scene --out profiles/probe_bake.json [--reps 20]

Bake: cube2oct + probe_downsample of all 16 probes of a 4 x 4 grid at the reference's sizes (128² cubes, 256² probes with
9 mips).  The cubes are the analytic room of tests/test_probe_gpu.py, uploaded beforehand, so the figure is that of the two
programs alone.  Trace: trace_probe at 1920x1080 and 3840x2160
on the rasterised procedural scene with the frame's camera, over those probes.  Reported: ms per bake / per trace launch
(mean over --reps after a warm-up) and the share of traced pixels that hit.

--bake-from-scene: the bake from geometry, on the procedural scene at detail 16 and 64: vkr_cubemap_probe alone (one 128² cube
at the first grid position) and the whole vkrh_bake_probes of a 4 x 4 grid (128² cubes, 256² probes; 96 cube faces, 16 octahedral
maps, 128 downsample steps, recording included).  Reported: the median of --reps timed runs after a warm-up."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _time(fn, reps):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def _median_ms(fn, reps):
    """median over `reps` runs, each timed on its own with HIP events (fn may do host work: the stream is drained first)"""
    import statistics

    import torch

    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times)


def bake_from_scene(args):
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, host
    from vk_renderer_amd import scene as scn
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.images import ArrayImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("probe_trace_timing: needs a GPU")
    stream = torch.cuda.current_stream().cuda_stream
    grid, probe_size, cube_size = 4, 256, 128
    pmin, pmax = (-6.0, 1.0, 0.0), (6.0, 1.0, 12.0)
    rows = []
    for detail in (16, 64):
        sc = scn.procedural_scene(detail=detail, cutout=True)
        tris = sum(d["index_count"] // 3 for d in sc.draws)
        s, keep = sc.upload("cuda")
        color = ArrayImageBuf(abi.FMT_RGBA8_SRGB, cube_size, cube_size, 6, device="cuda")
        dist = ArrayImageBuf(abi.FMT_R16_SFLOAT, cube_size, cube_size, 6, device="cuda")
        cd, dd = color.descs(), dist.descs()
        nbytes = abi.cubemap_probe_scratch_bytes(cube_size, tris)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ms = _median_ms(lambda: abi.cubemap_probe(s, pmin, cd, dd, scratch.data_ptr(), nbytes, stream), args.reps)
        rows.append({"program": "cubemap_probe", "scene": f"procedural detail {detail}", "triangles": tris, "cube": f"{cube_size}x{cube_size}",
                     "scratch_bytes": nbytes, "ms_per_cube_median": round(ms, 4), "reps": args.reps})
        print(json.dumps(rows[-1]), flush=True)
        frame = host.HostFrame(FrameSetup(256, 144), device="cuda")
        frame.load_scene(sc)
        ms = _median_ms(lambda: frame.bake_probes(pmin, pmax, grid, probe_size, cube_size), max(3, args.reps // 4))
        rows.append({"program": "vkrh_bake_probes", "scene": f"procedural detail {detail}", "triangles": tris, "grid": f"{grid}x{grid}",
                     "cube": f"{cube_size}x{cube_size}", "probe": f"{probe_size}x{probe_size}", "ms_per_bake_median": round(ms, 4),
                     "reps": max(3, args.reps // 4)})
        print(json.dumps(rows[-1]), flush=True)
        frame.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/probe_trace_timing.py --bake-from-scene", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bake-from-scene", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "probe_bake.json" if args.bake_from_scene else "probe_trace.json")
    if args.bake_from_scene:
        return bake_from_scene(args)
    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi
    from vk_renderer_amd.images import ArrayImageBuf, ImageBuf
    import test_probe_gpu as tp

    if not torch.cuda.is_available():
        raise SystemExit("probe_trace_timing: needs a GPU")
    lib = abi.product()
    stream = torch.cuda.current_stream().cuda_stream
    probe_size, cube_size, layers = 256, 128, tp.GRID * tp.GRID
    mips = int(np.floor(np.log2(probe_size))) + 1
    color = ArrayImageBuf(abi.FMT_RGBA8_UNORM, probe_size, probe_size, layers, device="cuda")
    depth = ArrayImageBuf(abi.FMT_R16_UNORM, probe_size, probe_size, layers, mips=mips, device="cuda")
    cubes = [tp._cube_bufs(*tp._room_cube(p, cube_size)) for p in tp._probe_positions()]
    color_descs = [color.desc(k) for k in range(layers)]
    depth_descs = [depth.desc(k) for k in range(layers)]
    mip0_descs = []
    for d in depth_descs:
        m0 = abi.VkrImg.from_buffer_copy(d)
        m0.mip_count = 1
        mip0_descs.append(m0)

    def bake():
        for k in range(layers):
            abi.check(lib.vkr_cube2oct(cubes[k][2], cubes[k][3], C.byref(color_descs[k]), C.byref(mip0_descs[k]), stream), lib)
            abi.check(lib.vkr_probe_downsample(C.byref(depth_descs[k]), stream), lib)

    bake_ms = _time(bake, args.reps)
    rows = [{"program": "cube2oct + probe_downsample", "probes": layers, "cube": f"{cube_size}x{cube_size}",
             "probe": f"{probe_size}x{probe_size}", "mips": mips, "ms_per_bake": round(bake_ms, 4), "reps": args.reps}]
    print(json.dumps(rows[-1]), flush=True)
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        frame = tp._raster_frame(W, H)
        params = frame.gtao_rt_params()
        consts = tp._consts(params)
        out = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda")
        cd, dd, od = color.descs(), depth.descs(), out.desc()
        dimg, nimg = frame.image("depth"), frame.image("normal")

        def trace():
            abi.check(lib.vkr_trace_probe(C.byref(dimg), C.byref(nimg), cd, dd, layers, C.byref(consts), C.byref(od), stream), lib)

        ms = _time(trace, args.reps)
        img = out.raw(0)
        sky = (frame.download("depth").raw(0)[..., 0] & 0xFFFFFF) == 0xFFFFFF
        lit = int(((img != 0).any(-1) & ~sky).sum())
        rows.append({"program": "trace_probe", "frame": f"{W}x{H}", "grid": f"{tp.GRID}x{tp.GRID}", "ms_per_launch": round(ms, 4),
                     "pixels": W * H, "non_sky_pixels": int((~sky).sum()), "non_zero_pixels": lit, "reps": args.reps})
        print(json.dumps(rows[-1]), flush=True)
        frame.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/probe_trace_timing.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
