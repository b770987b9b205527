#!/usr/bin/env python3
"""Times the shadow-map pass (csrc/shadow.hip) with HIP events.

    python tools/shadow_timing.py [--out profiles/shadow_map.json] [--reps 20] [--size 1024]

On the procedural scene (with the cutout fence) at detail 16 and 64, map edge --size, light A of main.cpp:295:
  * vkr_default_shadow with 1 layer and with 4 layers (the lights A, B, C, A of tests/shadow_light.py);
  * vkr_raster_gbuffer on the same scene, size and matrix (zero jitter): the only other way to a depth image of a scene,
    with its five attachments, its visibility buffer and its resolve;
  * the whole VKRH_STAGE_SHADOW of the host frame (one light and four lights; recording included).
Reported: the median of --reps runs, each timed on its own after a warm-up.  No threshold: the numbers go into DESIGN.md."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIGHTS = (((-1.85867, 5.81832, -0.247114), (0.0, 2.0, 1.0)), ((0.3, 0.4, 4.0), (0.0, 1.0, 8.0)), ((-3.0, 2.5, 9.0), (1.0, 0.5, 3.0)))


def _median_ms(fn, reps):
    """median over `reps` runs, each timed on its own with HIP events (fn may do host work: the stream is drained first)"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shadow_map.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--details", default="16,64")
    args = ap.parse_args()
    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, camera, host
    from vk_renderer_amd import scene as scn
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.images import ArrayImageBuf, ImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("shadow_timing: needs a GPU")
    lib = abi.product()
    stream = torch.cuda.current_stream().cuda_stream
    n = args.size
    mats = [camera.shadow_mvp(eye=e, center=c) for e, c in LIGHTS]
    four = [mats[0], mats[1], mats[2], mats[0]]
    rows = []

    def row(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for detail in (int(v) for v in args.details.split(",")):
        sc = scn.procedural_scene(detail=detail, cutout=True)
        tris = sum(d["index_count"] // 3 for d in sc.draws)
        label = f"procedural detail {detail}"
        s, keep = sc.upload("cuda")
        layers = ArrayImageBuf(abi.FMT_D24_UNORM_S8, n, n, 4, device="cuda")
        descs = [layers.desc(l) for l in range(4)]
        for count, use in ((1, [mats[0]]), (4, four)):
            nbytes = abi.default_shadow_scratch_bytes(n, count, tris)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            ms = _median_ms(lambda: abi.default_shadow(s, use, descs[:count], scratch.data_ptr(), nbytes, stream), args.reps)
            covered = float((layers.raw()[0, ..., 0] != 0x00FFFFFF).mean())
            row(program="default_shadow", scene=label, triangles=tris, map=f"{n}x{n}", layers=count, scratch_bytes=nbytes,
                ms_per_call_median=round(ms, 4), covered_layer0=round(covered, 4), reps=args.reps)
            del scratch
        # the G-buffer rasteriser on the same scene, size and matrix
        consts = abi.GbufConst()
        consts.view_projection = consts.prev_view_projection = abi.Mat4.from_np(mats[0])
        fazz = FrameSetup(n, n).fazz
        consts.fovy_aspect_znear_zfar = (C.c_float * 4)(*[float(v) for v in fazz])
        att = [ImageBuf(f, n, n, device="cuda") for f in (abi.FMT_RGBA8_SRGB, abi.FMT_RG16_UNORM, abi.FMT_RGBA8_SRGB, abi.FMT_RG16_SFLOAT, abi.FMT_D24_UNORM_S8)]
        ad = [a.desc() for a in att]
        nbytes = int(lib.vkr_raster_scratch_bytes(n, n, tris))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def gbuffer():
            abi.check(lib.vkr_raster_gbuffer(C.byref(s), C.byref(consts), C.byref(ad[0]), C.byref(ad[1]), C.byref(ad[2]), C.byref(ad[3]), C.byref(ad[4]),
                                             scratch.data_ptr(), nbytes, stream), lib)

        ms = _median_ms(gbuffer, args.reps)
        row(program="gbuf_opaque_taa", scene=label, triangles=tris, map=f"{n}x{n}", scratch_bytes=nbytes, ms_per_call_median=round(ms, 4),
            reps=args.reps, note="same scene, size and matrix; textured draws with their alpha test, five attachments")
        del scratch, att
        # the frame stage
        frame = host.HostFrame(FrameSetup(256, 144), device="cuda")
        frame.load_scene(sc)
        for count, use in ((1, [mats[0]]), (4, four)):
            frame.set_shadow_lights(use, n)
            ms = _median_ms(lambda: frame.run(host.STAGE_SHADOW), args.reps)
            row(program="VKRH_STAGE_SHADOW", scene=label, triangles=tris, map=f"{n}x{n}", lights=count, ms_per_stage_median=round(ms, 4), reps=args.reps)
        frame.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/shadow_timing.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
