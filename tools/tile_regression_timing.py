#!/usr/bin/env python3
"""Times the tile plane regression (csrc/tile_regression.hip) with HIP events.

    python tools/tile_regression_timing.py [--out profiles/tile_regression.json] [--reps 20] [--inner 20]
                                           [--sizes 1920x1080,3840x2160,7680x4320]

At each full-resolution frame size, on the synthetic G-buffer's depth after the downsample (VKRH_STAGE_GBUFFER | DOWNSAMPLE of
the host frame: the pass reads mip 1):
  * vkr_tile_regression called directly into a (W / 16, H / 16) image, the reference's extent: time per call, the bytes the pass
    must move (4 B per half-resolution texel read, 16 B per tile written), the time those bytes take at the rate of the float4
    stream read (vkr_stream_read) measured in the same run, and the ratio of the two;
  * the task "SSSR_Tile_Regression" (VKRH_STAGE_TILE_REGRESSION) of the host frame on the same depth, device events around the
    task.
A run is --inner calls between one pair of events; reported per call: the median of --reps runs with min and max, the
candidates taking turns run by run.  The half-resolution depth of every size here (2 .. 33 MB) fits the last-level cache, so
repeated calls may read it from there: the floor is the HBM stream rate all the same, which makes the ratio a lower bound of
the distance to what the memory system allows.  No threshold (the pass has no predecessor): the numbers go into DESIGN.md
section 7.5."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _git_head():
    try:
        out = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        return out.stdout.strip() if out.returncode == 0 and out.stdout.strip() else "unknown (not a git checkout)"
    except OSError:
        return "unknown (no git)"


def _stats(times_ms):
    return {"median_ms": round(statistics.median(times_ms), 5), "min_ms": round(min(times_ms), 5), "max_ms": round(max(times_ms), 5), "runs": len(times_ms)}


def _timed(fn, inner):
    import torch

    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / inner


def pass_bytes(W, H):
    """(bytes read, bytes written) of the pass on a W x H frame: the half-resolution depth once, one RGBA32F texel per tile of
    the (W / 16, H / 16) image"""
    return (W // 2) * (H // 2) * 4, (W // 16) * (H // 16) * 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_regression.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080,3840x2160,7680x4320")
    ap.add_argument("--git-head", default=None, help="the head to record when the tree that runs is not a git checkout")
    args = ap.parse_args()
    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, host
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.images import ImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("tile_regression_timing: needs a GPU")
    lib = abi.product()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def row(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    # the float4 stream read of this run (bench.py measures the same): best of 4 over 2 GiB
    n = 2 << 30
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    src.random_(0, 255)
    sink = torch.zeros(4096, dtype=torch.float32, device="cuda")
    stream_gbs = 0.0
    for _ in range(4):
        ms = _timed(lambda: abi.check(lib.vkr_stream_read(src.data_ptr(), n, sink.data_ptr(), 4096, stream), lib), 1)
        stream_gbs = max(stream_gbs, n / (ms * 1e-3) / 1e9)
    del src
    row(measurement="stream_read", bytes=n, gb_per_s=round(stream_gbs, 1), note="float4 streaming read, best of 4")

    task = "SSSR_Tile_Regression"
    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        setup = FrameSetup(W, H)
        frame = host.HostFrame(setup, device="cuda")
        frame.run(host.STAGE_GBUFFER | host.STAGE_DOWNSAMPLE)
        torch.cuda.synchronize()
        depth = frame.image("depth", 1, 1)
        rt = frame.gtao_rt_params()
        push = abi.TileRegressionPush(rt.camera_to_world, *[float(v) for v in setup.fazz])
        out = ImageBuf(abi.FMT_RGBA32_SFLOAT, W // 16, H // 16, device="cuda")
        od = out.desc()

        def direct():
            abi.tile_regression(depth, od, push, stream)

        def staged():
            frame.run(host.STAGE_TILE_REGRESSION)

        for fn in (direct, staged):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t_direct, t_task = [], []
        for _ in range(args.reps):
            t_direct.append(_timed(direct, args.inner))
            frame.enable_task_timing(True, only=task)  # device events around the task alone: the recording on the host is not in the figure
            for _ in range(args.inner):
                staged()
            total_ms, launches = frame.collect_task_times()[task]
            t_task.append(total_ms / launches)
            frame.enable_task_timing(False)
        st = _stats(t_direct)
        read, written = pass_bytes(W, H)
        floor_ms = (read + written) / (stream_gbs * 1e9) * 1e3
        planes = out.raw(0)
        row(measurement="vkr_tile_regression", size=f"{W}x{H}", depth_view=f"{W // 2}x{H // 2}", tiles=f"{W // 16}x{H // 16}", bytes_read=read,
            bytes_written=written, floor_ms_at_stream_read=round(floor_ms, 5), ratio_to_floor=round(st["median_ms"] / floor_ms, 2),
            calls_per_run=args.inner, finite_planes=int(np.isfinite(planes[..., :3]).all(axis=-1).sum()), **st)
        row(measurement=f"task {task}", size=f"{W}x{H}", calls_per_run=args.inner, note="the frame stage: the same kernel behind AdvancedSSR::run_tile_regression_pass",
            **_stats(t_task))
        frame.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/tile_regression_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
