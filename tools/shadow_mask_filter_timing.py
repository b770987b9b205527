#!/usr/bin/env python3
"""Times the edge-aware filter of the shadow mask (csrc/shadow_mask_filter.hip) with HIP events, alone and behind the traced soft
mask it reconstructs, and measures what the pipeline buys: the error against a mask of 64 rays per pixel.

    python tools/shadow_mask_filter_timing.py [--out profiles/shadow_mask_filter.json] [--reps 20] [--inner 10]
                                              [--sizes 1920x1080,3840x2160] [--detail 64] [--build-variant]

On the procedural scene at --detail, rasterised by the host frame at each size, with the four lights of
tools/shadow_mask_rt_soft_timing.py at radius 0.5:
  * the filter alone for reach 4 (on the mask of S = 1, P = 4) and reach 2 (on the mask of S = 4, P = 2): the library's entry, and the
    library built with -DVKR_SHADOW_FILTER_EARLY_OUT=0 through tools/build_variants.sh (--build-variant builds it and exits: no GPU
    needed; without it the candidate is left out and the rows say so), run by run in turns.  The two must give the same bytes; the
    tool checks that.  The share of the 8 x 8 wave tiles whose window is flat (the waves that take the early-out) is computed here
    from the mask;
  * the pipelines soft(S = 1, P = 4) + filter(R = 4) and soft(S = 4, P = 2) + filter(R = 2), both calls between one pair of events,
    beside unfiltered soft(S = 16, P = 1), in turns in the same run;
  * the quality of those three: the mean and the 99th percentile of the absolute byte difference to unfiltered soft(S = 64, P = 1)
    over the penumbra (the channels of geometry pixels whose S = 64 value is neither 0 nor 255);
  * a sweep of the two thresholds of the accept test on the first pipeline at the first size: the pair with the smallest mean error.
A run is --inner calls between one pair of events; reported per call: the median of --reps runs with min and max.  No threshold
anywhere: the numbers go into DESIGN.md section 7.13."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "vk-renderer_amd", "csrc")
VARIANT = os.path.join(CSRC, "variants", "filter_no_early_out", "libvkr_postfx.so")

LIGHT_POS = (-1.85867, 5.81832, -0.247114)
RAYS = [LIGHT_POS + (1.0,), (3.0, 4.0, 2.0, 1.0), (1.5, 4.5, -1.5, 0.0), (-6.0, 9.0, 3.0, 0.0)]
RADIUS = 0.5
PIPELINES = [(1, 4, 4), (4, 2, 2)]  # (S, P, reach)
SWEEP_DOTS = (0.5, 0.8, 0.9, 0.95, 0.99)
SWEEP_PLANES = (0.002, 0.005, 0.01, 0.02, 0.05)


def build_variant():
    subprocess.check_call(["bash", os.path.join(ROOT, "tools", "build_variants.sh"), "shadow_mask_filter.hip", "filter_no_early_out",
                           "-DVKR_SHADOW_FILTER_EARLY_OUT=0"])
    return VARIANT


def load_variant(lib):
    """-> vkr_shadow_mask_filter of the library built without the early-out, or None"""
    if not os.path.exists(VARIANT):
        return None
    fn = C.CDLL(VARIANT).vkr_shadow_mask_filter
    fn.argtypes, fn.restype = lib.vkr_shadow_mask_filter.argtypes, C.c_int
    return fn


def flat_tile_share(mask, reach):
    """the share of the 8 x 8 tiles of `mask` (uint8 [h, w, 4]) whose window of reach - 1 texels around them, cut to the image, holds
    one single 32-bit value: the waves that take the early-out"""
    import numpy as np

    words = np.ascontiguousarray(mask).view(np.uint32)[..., 0]
    h, w = words.shape
    b = reach - 1
    ty, tx = (h + 7) // 8, (w + 7) // 8
    padded = np.pad(words, ((b, ty * 8 - h + b), (b, tx * 8 - w + b)), mode="edge")  # an edge value adds no new value to a window
    lo = hi = None
    for k in range(8 + 2 * b):  # columns of the window, per tile column
        col = padded[:, k::8][:, :tx]
        lo, hi = (col, col) if lo is None else (np.minimum(lo, col), np.maximum(hi, col))
    lo2 = hi2 = None
    for k in range(8 + 2 * b):
        rl, rh = lo[k::8][:ty], hi[k::8][:ty]
        lo2, hi2 = (rl, rh) if lo2 is None else (np.minimum(lo2, rl), np.maximum(hi2, rh))
    return float((lo2 == hi2).mean())


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shadow_mask_filter.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--detail", type=int, default=64)
    ap.add_argument("--build-variant", action="store_true", help="build the library without the early-out and exit (no GPU needed)")
    ap.add_argument("--git-head", default=None, help="the head to record when the tree that runs is not a git checkout")
    args = ap.parse_args()
    if args.build_variant:
        print("built", build_variant())
        return
    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, host
    from vk_renderer_amd import scene as scn
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.images import ImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("shadow_mask_filter_timing: needs a GPU")
    lib = abi.product()
    stream = torch.cuda.current_stream().cuda_stream
    no_early_out = load_variant(lib)
    rows = []

    def row(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    sc = scn.procedural_scene(detail=args.detail)
    accel = abi.Accel.from_scene(sc)
    nodes, tris = accel.info()
    for index, size in enumerate(args.sizes.split(",")):
        W, H = (int(x) for x in size.split("x"))
        setup = FrameSetup(W, H)
        frame = host.HostFrame(setup, device="cuda")
        frame.load_scene(sc)
        frame.run(host.STAGE_RASTER)
        torch.cuda.synchronize()
        depth, normal = frame.image("depth", 0, 1), frame.image("normal")
        geometry = (frame.download("depth").raw(0)[..., 0] & 0xFFFFFF) != 0xFFFFFF
        common = dict(size=f"{W}x{H}", detail=args.detail, triangles=tris, nodes=nodes, lights=len(RAYS), radius=RADIUS, calls_per_run=args.inner)
        rp = abi.shadow_rt_params(setup.inv_view, RAYS, *setup.fazz, normal_offset=abi.SHADOW_RT_NORMAL_OFFSET, tmin=abi.SHADOW_RT_TMIN)
        images = {k: ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda") for k in ("s1p4", "s4p2", "s16", "s64", "f4", "f2", "variant", "sweep")}
        descs = {k: v.desc() for k, v in images.items()}
        softs = {"s1p4": abi.shadow_rt_soft([RADIUS] * 4, 1, 4, device="cuda"), "s4p2": abi.shadow_rt_soft([RADIUS] * 4, 4, 2, device="cuda"),
                 "s16": abi.shadow_rt_soft([RADIUS] * 4, 16, 1, device="cuda"), "s64": abi.shadow_rt_soft([RADIUS] * 4, 64, 1, device="cuda")}

        def soft(key):
            return lambda: abi.check(lib.vkr_shadow_mask_rt_soft(C.byref(depth), C.byref(normal), accel.handle, C.byref(rp), C.byref(softs[key]),
                                                                 C.byref(descs[key]), stream), lib)

        def filt(fn, src, dst, reach, dot=abi.SHADOW_FILTER_NORMAL_MIN_DOT, plane=abi.SHADOW_FILTER_PLANE_TOLERANCE):
            fp = abi.shadow_filter_params(setup.inv_view, *setup.fazz, reach, dot, plane)
            return lambda: abi.check(fn(C.byref(depth), C.byref(normal), C.byref(descs[src]), C.byref(fp), C.byref(descs[dst]), stream), lib)

        for key in softs:
            soft(key)()
        torch.cuda.synchronize()
        truth = images["s64"].raw(0).astype(np.int32)
        penumbra = geometry[..., None] & (truth > 0) & (truth < 255)
        row(measurement="penumbra", **common, share_of_geometry_channels=round(float(penumbra.sum() / (4.0 * geometry.sum())), 5))

        def error(key):
            diff = np.abs(images[key].raw(0).astype(np.int32) - truth)[penumbra]
            return {"mean_abs_byte_error": round(float(diff.mean()), 3), "p99_abs_byte_error": float(np.percentile(diff, 99))}

        # ---- the filter alone, with and without the early-out
        for (S, P, reach), src, dst in zip(PIPELINES, ("s1p4", "s4p2"), ("f4", "f2")):
            cases = {"vkr_shadow_mask_filter": filt(lib.vkr_shadow_mask_filter, src, dst, reach)}
            if no_early_out is not None:
                cases["shadow_mask_filter without the early-out"] = filt(no_early_out, src, "variant", reach)
            for fn in cases.values():
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            same = bool(np.array_equal(images[dst].raw(0), images["variant"].raw(0))) if no_early_out is not None else None
            times = {k: [] for k in cases}
            for _ in range(args.reps):
                for k, fn in cases.items():
                    times[k].append(_timed(fn, args.inner))
            share = round(flat_tile_share(images[src].raw(0), reach), 5)
            for k in cases:
                row(measurement=k, reach=reach, mask=f"soft S {S} P {P}", **common, **_stats(times[k]), share_of_waves_that_take_the_early_out=share)
            row(measurement="with and without the early-out give the same bytes", reach=reach, size=f"{W}x{H}",
                value=same if same is not None else "variant without the early-out not built")
            if no_early_out is not None:
                assert same, "the early-out changed a byte"

        # ---- the pipelines beside the unfiltered mask of 16 rays
        def both(a, b):
            return lambda: (a(), b())

        cases = {"soft S 1 P 4 + filter R 4": both(soft("s1p4"), filt(lib.vkr_shadow_mask_filter, "s1p4", "f4", 4)),
                 "soft S 4 P 2 + filter R 2": both(soft("s4p2"), filt(lib.vkr_shadow_mask_filter, "s4p2", "f2", 2)),
                 "soft S 16 P 1, unfiltered": soft("s16"), "soft S 1 P 4, unfiltered": soft("s1p4"), "soft S 4 P 2, unfiltered": soft("s4p2")}
        for fn in cases.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(args.reps):
            for k, fn in cases.items():
                times[k].append(_timed(fn, args.inner))
        results = {"soft S 1 P 4 + filter R 4": "f4", "soft S 4 P 2 + filter R 2": "f2", "soft S 16 P 1, unfiltered": "s16",
                   "soft S 1 P 4, unfiltered": "s1p4", "soft S 4 P 2, unfiltered": "s4p2"}
        for k in cases:
            row(measurement=k, **common, **_stats(times[k]), **error(results[k]), thresholds=[abi.SHADOW_FILTER_NORMAL_MIN_DOT, abi.SHADOW_FILTER_PLANE_TOLERANCE])

        # ---- the thresholds
        if index == 0:
            best = None
            for dot in SWEEP_DOTS:
                for plane in SWEEP_PLANES:
                    filt(lib.vkr_shadow_mask_filter, "s1p4", "sweep", 4, dot, plane)()
                    torch.cuda.synchronize()
                    e = error("sweep")
                    row(measurement="threshold sweep, soft S 1 P 4 + filter R 4", size=f"{W}x{H}", normal_min_dot=dot, plane_tolerance=plane, **e)
                    if best is None or e["mean_abs_byte_error"] < best[0]:
                        best = (e["mean_abs_byte_error"], dot, plane)
            row(measurement="threshold sweep: smallest mean error", size=f"{W}x{H}", normal_min_dot=best[1], plane_tolerance=best[2], mean_abs_byte_error=best[0])
        frame.close()
    accel.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/shadow_mask_filter_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
