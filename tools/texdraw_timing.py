#!/usr/bin/env python3
"""Times the backbuffer texdraw pass (csrc/texdraw.hip) with HIP events and writes profiles/texdraw.json.

    bash tools/build_variants.sh texdraw.hip texdraw_lds "-DTEXDRAW_ENCODE_LDS"
    python tools/texdraw_timing.py [--out profiles/texdraw.json] [--reps 20] [--inner 10] [--sizes 3840x2160,1920x1080]
                                   [--lds-variant vk-renderer_amd/csrc/variants/texdraw_lds/libvkr_postfx.so]

At each size, RGBA16_SFLOAT source (halves in [0, 1)), source and destination of equal extent, the candidates taking turns run by
run in one process (the method of tools/transfer_timing.py):
  * texdraw_srgb        vkr_texdraw -> RGBA8_SRGB, the kernel as built: float_to_srgb8_fast (an estimate and one compare);
  * texdraw_srgb_lds    the same kernel built with -DTEXDRAW_ENCODE_LDS (float_to_srgb8_lds, the blit's search of eight dependent
                        LDS reads), loaded from the variant library beside the product; left out when that library is absent;
  * texdraw_unorm       vkr_texdraw -> RGBA8_UNORM: the pass without any sRGB encode;
  * blit_linear_srgb    vkr_blit_image LINEAR -> RGBA8_SRGB: what the pass has to beat;
  * blit_nearest_unorm  vkr_blit_image NEAREST -> RGBA8_UNORM: the floor of what this project moves for those bytes.
A run is --inner calls between one pair of events; reported per call: the median of --reps runs with min and max, the
algorithmic bytes (12 per pixel) over the median as a fraction of the float4 stream read (vkr_stream_read) of the same run.
"fast_encode_is_faster": the slowest run of texdraw_srgb is faster than the fastest run of texdraw_srgb_lds (the criterion of
DESIGN.md 7.3).  The two texdraw builds must leave the same bytes; the tool checks it.  Also: the task "BackbufSubpass" inside
a frame (VKRH_STAGE_BACKBUFFER after the chain; device events around the task).  The numbers go into DESIGN.md section 7.6."""
import argparse
import ctypes as C
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


def _alternating(fns, reps, inner):
    """{name: [ms per call, ...]}: the candidates take turns, run by run, after a warm-up of each"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(_timed(fn, inner))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texdraw.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--lds-variant", default=os.path.join(ROOT, "vk-renderer_amd", "csrc", "variants", "texdraw_lds", "libvkr_postfx.so"))
    ap.add_argument("--git-head", default=None, help="the head to record when the tree that runs is not a git checkout")
    args = ap.parse_args()
    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, host
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.images import ImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("texdraw_timing: needs a GPU")
    lib = abi.product()
    stream = torch.cuda.current_stream().cuda_stream
    variant = None
    if os.path.exists(args.lds_variant):
        variant = C.CDLL(args.lds_variant)
        variant.vkr_texdraw.argtypes = lib.vkr_texdraw.argtypes
        variant.vkr_texdraw.restype = C.c_int
        variant.vkr_last_error.restype = C.c_char_p
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
    if variant is None:
        row(measurement="note", note=f"no variant library at {os.path.relpath(args.lds_variant, ROOT)}: texdraw_srgb_lds is not measured")

    push = abi.texdraw_push(abi.TEXDRAW_SHOW_ALL)
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(7)
        half = ImageBuf(abi.FMT_RGBA16_SFLOAT, W, H, device="cuda")
        half.tensor.copy_(torch.from_numpy(rng.integers(0, 0x3C00, size=half.nbytes // 2, dtype=np.uint16).view(np.uint8)))  # halves in [0, 1)
        srgb = ImageBuf(abi.FMT_RGBA8_SRGB, W, H, device="cuda")
        srgb_lds = ImageBuf(abi.FMT_RGBA8_SRGB, W, H, device="cuda")
        unorm = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda")
        hd, sd, sld, ud = half.desc(), srgb.desc(), srgb_lds.desc(), unorm.desc()
        fns = {"texdraw_srgb": lambda: abi.texdraw(hd, sd, push, stream)}
        if variant is not None:
            fns["texdraw_srgb_lds"] = lambda: abi.check(variant.vkr_texdraw(C.byref(hd), C.byref(sld), C.byref(push), stream), variant)
        fns["texdraw_unorm"] = lambda: abi.texdraw(hd, ud, push, stream)
        fns["blit_linear_srgb"] = lambda: abi.blit_image(hd, sd, abi.FILTER_LINEAR, stream)
        fns["blit_nearest_unorm"] = lambda: abi.blit_image(hd, ud, abi.FILTER_NEAREST, stream)
        t = _alternating(fns, args.reps, args.inner)
        moved = W * H * (8 + 4)
        for k in fns:
            st = _stats(t[k])
            rate = moved / (st["median_ms"] * 1e-3) / 1e9
            row(measurement=k, size=f"{W}x{H}", src="RGBA16_SFLOAT", algorithmic_bytes=moved, gb_per_s=round(rate, 1),
                fraction_of_stream_read=round(rate / stream_gbs, 3), calls_per_run=args.inner, **st)
        if variant is not None:
            abi.texdraw(hd, sd, push, stream)
            abi.check(variant.vkr_texdraw(C.byref(hd), C.byref(sld), C.byref(push), stream), variant)
            torch.cuda.synchronize()
            same = bool(torch.equal(srgb.tensor, srgb_lds.tensor))
            row(measurement="fast_encode_vs_lds", size=f"{W}x{H}", same_bytes=same,
                fast_encode_is_faster=bool(max(t["texdraw_srgb"]) < min(t["texdraw_srgb_lds"])),
                fast_max_ms=round(max(t["texdraw_srgb"]), 5), lds_min_ms=round(min(t["texdraw_srgb_lds"]), 5))
            if not same:
                raise SystemExit("texdraw_timing: the two encodes left different bytes")
        del half, srgb, srgb_lds, unorm

        # the task inside a frame: the chain once, then the stage alone on the TAA output it left
        frame = host.HostFrame(FrameSetup(W, H), device="cuda")
        frame.run(host.STAGE_GBUFFER)
        frame.run(host.STAGE_LUT | host.STAGE_PREV_DEPTH)
        frame.run(host.STAGE_CHAIN | host.STAGE_BACKBUFFER)
        torch.cuda.synchronize()
        task, t_task = "BackbufSubpass", []
        for _ in range(args.reps):
            frame.enable_task_timing(True, only=task)  # device events around the task alone: the recording on the host is not in the figure
            for _ in range(args.inner):
                frame.run(host.STAGE_BACKBUFFER)
            total_ms, launches = frame.collect_task_times()[task]
            t_task.append(total_ms / launches)
            frame.enable_task_timing(False)
        row(measurement=f"task {task}", size=f"{W}x{H}", src="the TAA output", calls_per_run=args.inner,
            note="the frame stage: the same kernel behind add_backbuffer_subpass", **_stats(t_task))
        frame.close()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/texdraw_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "reps": args.reps,
                   "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
