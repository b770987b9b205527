#!/usr/bin/env python3
"""Times the SSAO pass (csrc/ssao.hip) with HIP events.

    python tools/ssao_timing.py [--out profiles/ssao.json] [--reps 20] [--inner 10] [--sizes 1920x1080,3840x2160]

On the synthetic G-buffer's depth (VKRH_STAGE_GBUFFER of the host frame) at each size, with the 16 samples of the tests
(rng(11), one 16-byte slot each):
  * vkr_ssao called directly, output at the depth's extent: time per call, the algorithmic bytes (4 B read + 1 B written per
    pixel) over that time, and that rate as a fraction of the float4 stream read (vkr_stream_read) measured in the same run;
  * the tasks "SSAO" (VKRH_STAGE_SSAO) and "GTAO_main" (VKRH_STAGE_GTAO_MAIN_ONLY, the half-resolution horizon search the
    reference's frame uses for its ambient occlusion) of the host frame on the same G-buffer, device events around the task.
A run is --inner calls between one pair of events; reported per call: the median of --reps runs with min and max, the
candidates taking turns run by run.  No threshold: the numbers go into DESIGN.md section 7.4."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssao.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--git-head", default=None, help="the head to record when the tree that runs is not a git checkout")
    args = ap.parse_args()
    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, host
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.images import ImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("ssao_timing: needs a GPU")
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

    v = np.random.default_rng(11).normal(size=(16, 3))
    samples = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        setup = FrameSetup(W, H)
        frame = host.HostFrame(setup, device="cuda")
        frame.run(host.STAGE_LUT | host.STAGE_GBUFFER | host.STAGE_DOWNSAMPLE)
        frame.set_ssao_samples(samples, std140=1)
        torch.cuda.synchronize()
        depth = frame.image("depth", 0, 1)
        params = abi.ssao_params(setup.proj, *setup.fazz, samples)
        out = ImageBuf(abi.FMT_R8_UNORM, W, H, device="cuda")
        od = out.desc()

        def direct():
            abi.ssao(depth, params, od, stream)

        staged = {"SSAO": lambda: frame.run(host.STAGE_SSAO), "GTAO_main": lambda: frame.run(host.STAGE_GTAO_MAIN_ONLY)}
        for fn in [direct] + list(staged.values()):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t_direct, t_task = [], {k: [] for k in staged}
        for _ in range(args.reps):
            t_direct.append(_timed(direct, args.inner))
            for k, fn in staged.items():  # device events around the task alone: the recording on the host is not in the figure
                frame.enable_task_timing(True, only=k)
                for _ in range(args.inner):
                    fn()
                total_ms, launches = frame.collect_task_times()[k]
                t_task[k].append(total_ms / launches)
                frame.enable_task_timing(False)
        st = _stats(t_direct)
        nbytes = W * H * 5
        rate = nbytes / (st["median_ms"] * 1e-3) / 1e9
        codes = out.raw(0)[..., 0]
        row(measurement="vkr_ssao", size=f"{W}x{H}", algorithmic_bytes=nbytes, gb_per_s=round(rate, 1), fraction_of_stream_read=round(rate / stream_gbs, 4),
            depth_loads_per_pixel=34, calls_per_run=args.inner, distinct_codes=int(len(np.unique(codes))), **st)
        for k in staged:
            row(measurement=f"task {k}", size=f"{W}x{H}", calls_per_run=args.inner,
                note="half resolution, MIS, one slice" if k == "GTAO_main" else "the frame stage: the same kernel behind SSAOPass::draw", **_stats(t_task[k]))
        frame.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/ssao_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
