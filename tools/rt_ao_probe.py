#!/usr/bin/env python3
"""Times the ray-traced AO pass (task GTAO_rt_main, program gtao_rt_main) on the rasterised procedural scene with HIP
events, beside the screen-space GTAO main pass (task GTAO_main, gtao_compute_main) on the same G-buffer.

    python tools/rt_ao_probe.py --out profiles/rt_ao_probe.json [--reps 20]

Frames of 1920x1080 and 3840x2160 (raw at half resolution), procedural scene at two `detail` levels (sphere tessellation).
Reported per case: ms per launch (mean over --reps after a warm-up), rays traced (64 per non-sky raw pixel), Mrays/s,
and the size of the structure.  Nodes and triangles visited per wave are not counted (the kernel has no counters)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_ao_probe.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--details", default="16,64")
    args = ap.parse_args()
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, host
    from vk_renderer_amd import scene as scn
    from vk_renderer_amd.camera import FrameSetup

    if not torch.cuda.is_available():
        raise SystemExit("rt_ao_probe: needs a GPU")
    rows = []
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for detail in (int(v) for v in args.details.split(",")):
            sc = scn.procedural_scene(detail=detail)
            frame = host.HostFrame(FrameSetup(W, H), device="cuda")
            frame.load_scene(sc)
            frame.run(host.STAGE_LUT)
            frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE)
            torch.cuda.synchronize()
            depth = frame.download("depth").raw(1)[..., 0] & 0xFFFFFF
            live = int((depth < 0xFFFFFF).sum())  # upper bound of non-sky raw pixels (the pass samples between texels)
            times = {}
            for task, stage in (("GTAO_rt_main", host.STAGE_GTAO_RT), ("GTAO_main", host.STAGE_GTAO_MAIN_ONLY)):
                for _ in range(3):
                    frame.run(stage)
                torch.cuda.synchronize()
                frame.enable_task_timing(True, only=task)
                frame.collect_task_times()
                for _ in range(args.reps):
                    frame.run(stage)
                ms, n = frame.collect_task_times()[task]
                frame.enable_task_timing(False)
                times[task] = ms / n
            tris = abi.scene_triangles(sc)
            accel = abi.Accel(tris)
            nodes, ntris = accel.info()
            accel.close()
            rays = live * 64
            row = {"frame": f"{W}x{H}", "raw": f"{W // 2}x{H // 2}", "detail": detail, "triangles": ntris, "nodes": nodes,
                   "rays": rays, "gtao_rt_main_ms": round(times["GTAO_rt_main"], 4),
                   "mrays_per_s": round(rays / (times["GTAO_rt_main"] * 1e-3) / 1e6, 1),
                   "gtao_compute_main_ms": round(times["GTAO_main"], 4), "reps": args.reps,
                   "nodes_per_wave": "not counted", "triangles_per_wave": "not counted"}
            print(json.dumps(row), flush=True)
            rows.append(row)
            frame.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/rt_ao_probe.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
