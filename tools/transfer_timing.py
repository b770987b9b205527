#!/usr/bin/env python3
"""Times the image transfers (csrc/transfer.hip) with HIP events and writes profiles/transfer.json.

    python tools/transfer_timing.py [--out profiles/transfer.json] [--reps 20] [--inner 10]

  * vkr_gen_mipmaps of an RGBA8_SRGB image at 1024^2 and 4096^2 under both schedules (one launch per level / fused tiles), the
    two alternating run by run; beside it the only way to a device mip chain without the entry: scene.build_mips on the host
    plus the upload of every level (a host clock around work that ends in a synchronise);
  * vkr_blit_image 3840x2160 RGBA16_SFLOAT -> RGBA8_SRGB (LINEAR and NEAREST) and vkr_clear_image of a 3840x2160 D24_UNORM_S8
    image: time, algorithmic bytes (every source texel read once, every destination texel written once) over time, and that rate
    as a fraction of the float4 stream read (vkr_stream_read) measured in the same run;
  * the git head the numbers belong to.
A run is --inner calls between one pair of events; reported per call: the median of --reps runs with min and max.  No threshold:
the numbers go into DESIGN.md section 7.3 and decide the default schedule (DESIGN_EXPERIMENTS.md)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transfer.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--git-head", default=None, help="the head to record when the tree that runs is not a git checkout")
    ap.add_argument("--host-reps", type=int, default=20, help="runs of the host path (build_mips + upload)")
    args = ap.parse_args()
    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi
    from vk_renderer_amd import scene as scn
    from vk_renderer_amd.images import ImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("transfer_timing: needs a GPU")
    lib = abi.product()
    stream = torch.cuda.current_stream().cuda_stream
    before = lib.vkr_get_switches()
    both = abi.SWITCH_MIPS_PER_LEVEL | abi.SWITCH_MIPS_FUSED
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

    # ---- mip chain ----
    for size in (int(v) for v in args.sizes.split(",")):
        level0 = np.random.default_rng(size).integers(0, 256, size=(size, size, 4), dtype=np.uint8)
        mips = int(np.floor(np.log2(size))) + 1
        host_img = ImageBuf(abi.FMT_RGBA8_SRGB, size, size, mips)
        host_img.set_raw(level0, 0)
        img = ImageBuf(abi.FMT_RGBA8_SRGB, size, size, mips, device="cuda")
        img.upload(host_img.to_host())
        desc = img.desc()

        def chain(bit):
            def run():
                lib.vkr_set_switches((before & ~both) | bit)
                abi.gen_mipmaps(desc, stream)
            return run

        t = _alternating({"per_level": chain(abi.SWITCH_MIPS_PER_LEVEL), "fused": chain(abi.SWITCH_MIPS_FUSED)}, args.reps, args.inner)
        lib.vkr_set_switches(before)
        chain_bytes = sum(max(1, size >> m) ** 2 * 4 for m in range(mips)) + sum(max(1, size >> m) ** 2 * 4 for m in range(1, mips))
        launches = {"per_level": mips - 1, "fused": -(-(mips - 1) // 6)}
        for k in ("per_level", "fused"):
            st = _stats(t[k])
            row(measurement="gen_mipmaps", schedule=k, format="RGBA8_SRGB", size=f"{size}x{size}", levels=mips, launches=launches[k],
                algorithmic_bytes=chain_bytes, gb_per_s=round(chain_bytes / (st["median_ms"] * 1e-3) / 1e9, 1), calls_per_run=args.inner, **st)

        # the host path: build_mips + upload of every level
        def host_path():
            levels = scn.build_mips(level0)
            for m, lv in enumerate(levels):
                host_img.set_raw(lv, m)
            img.upload(host_img.to_host())
            torch.cuda.synchronize()

        host_path()
        times = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            host_path()
            times.append((time.perf_counter() - t0) * 1e3)
        st = _stats(times)
        fused_ms = statistics.median(t["fused"])
        row(measurement="gen_mipmaps_host_path", what="scene.build_mips (numpy) + upload of every level, host clock", size=f"{size}x{size}",
            ratio_to_fused=round(st["median_ms"] / fused_ms, 1), **st)
        del img

    # ---- blit and clear at 4K ----
    W, H = 3840, 2160
    rng = np.random.default_rng(7)
    half = ImageBuf(abi.FMT_RGBA16_SFLOAT, W, H, device="cuda")
    half.tensor.copy_(torch.from_numpy(rng.integers(0, 0x3C00, size=half.nbytes // 2, dtype=np.uint16).view(np.uint8)))  # halves in [0, 1)
    out = ImageBuf(abi.FMT_RGBA8_SRGB, W, H, device="cuda")
    hd, od = half.desc(), out.desc()
    t = _alternating({"linear": lambda: abi.blit_image(hd, od, abi.FILTER_LINEAR, stream), "nearest": lambda: abi.blit_image(hd, od, abi.FILTER_NEAREST, stream)},
                     args.reps, args.inner)
    blit_bytes = W * H * (8 + 4)
    for k in ("linear", "nearest"):
        st = _stats(t[k])
        rate = blit_bytes / (st["median_ms"] * 1e-3) / 1e9
        row(measurement="blit_image", filter=k, src="RGBA16_SFLOAT 3840x2160", dst="RGBA8_SRGB 3840x2160", algorithmic_bytes=blit_bytes,
            gb_per_s=round(rate, 1), fraction_of_stream_read=round(rate / stream_gbs, 3), calls_per_run=args.inner, **st)
    # the same bytes without the sRGB encode (a threshold search of 8 dependent LDS reads per channel): what the encode costs
    plain = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda")
    pd = plain.desc()
    t = _alternating({"linear": lambda: abi.blit_image(hd, pd, abi.FILTER_LINEAR, stream), "nearest": lambda: abi.blit_image(hd, pd, abi.FILTER_NEAREST, stream)},
                     args.reps, args.inner)
    for k in ("linear", "nearest"):
        st = _stats(t[k])
        rate = blit_bytes / (st["median_ms"] * 1e-3) / 1e9
        row(measurement="blit_image", filter=k, src="RGBA16_SFLOAT 3840x2160", dst="RGBA8_UNORM 3840x2160", algorithmic_bytes=blit_bytes,
            gb_per_s=round(rate, 1), fraction_of_stream_read=round(rate / stream_gbs, 3), calls_per_run=args.inner, **st)
    depth = ImageBuf(abi.FMT_D24_UNORM_S8, W, H, device="cuda")
    dd = depth.desc()
    t = _alternating({"clear": lambda: abi.clear_image(dd, depth=1.0, stream=stream)}, args.reps, args.inner)
    st = _stats(t["clear"])
    clear_bytes = W * H * 4
    rate = clear_bytes / (st["median_ms"] * 1e-3) / 1e9
    row(measurement="clear_image", image="D24_UNORM_S8 3840x2160", algorithmic_bytes=clear_bytes, gb_per_s=round(rate, 1),
        fraction_of_stream_read=round(rate / stream_gbs, 3), calls_per_run=args.inner, **st)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/transfer_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "reps": args.reps,
                   "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
