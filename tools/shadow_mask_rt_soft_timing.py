#!/usr/bin/env python3
"""Times the traced shadow mask with area lights (csrc/shadow_mask_rt_soft.hip) with HIP events, with and without the light-volume
cull, beside the hard entry.

    python tools/shadow_mask_rt_soft_timing.py [--out profiles/shadow_mask_rt_soft.json] [--reps 20] [--inner 10]
                                               [--sizes 1920x1080,3840x2160] [--details 16,64] [--samples 1,4,16] [--build-variant]

On the procedural scene at each detail, rasterised by the host frame at each size, for light 0 alone and for all four lights (the
lights of tools/shadow_mask_rt_timing.py), radius 0.5, a 4 x 4 tile of patterns, the candidates take turns run by run:
  * vkr_shadow_mask_rt: the unchanged hard entry, timed in the same run;
  * vkr_shadow_mask_rt_soft: the library's entry (no cull: csrc/shadow_mask_rt_soft.hip's default);
  * the same file built by this tool with -DVKR_SHADOW_RT_SOFT_CULL=1 (the light-volume cull) and =2 (the cull's report: no ray is
    walked, a channel reads 255 where the cull settles the pixel) under other entry names into csrc/build/ (--build-variant builds
    them and exits: no GPU needed; without them the candidates are left out and the rows say so).  Not entries of the product;
  * once per scene and size: vkr_shadow_mask_rt_soft at S = 1 with every radius 0, which runs the hard path, beside the hard entry.
A run is --inner calls between one pair of events; reported per call: the median of --reps runs with min and max, the ratio to
S x the hard entry's median, and from the report variant the share of geometry pixels, over the lights, that the cull settles
without a ray.  The variants with and without the cull must give the same bytes; the tool checks that.  No threshold anywhere: the
numbers go into DESIGN.md section 7.12."""
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
VARIANTS = {"cull": (1, os.path.join(CSRC, "build", "libvkr_shadow_rt_soft_cull.so")),
            "report": (2, os.path.join(CSRC, "build", "libvkr_shadow_rt_soft_report.so"))}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

LIGHT_POS = (-1.85867, 5.81832, -0.247114)
RAYS = [LIGHT_POS + (1.0,), (3.0, 4.0, 2.0, 1.0), (1.5, 4.5, -1.5, 0.0), (-6.0, 9.0, 3.0, 0.0)]
RADIUS = 0.5
PATTERN = 4


def build_variant(which):
    """csrc/shadow_mask_rt_soft.hip with another setting of the cull, with the flags of csrc/Makefile, linked against the product
    library; entries vkr_shadow_mask_rt_soft_<which> and vkr_shadow_mask_rt_soft_<which>_cutout"""
    mode, path = VARIANTS[which]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-DVKR_CONTRACT=2",
           "-fno-gpu-flush-denormals-to-zero", "-Wall", "-Wno-unused-function", f"-DVKR_SHADOW_RT_SOFT_CULL={mode}",
           f"-DVKR_SHADOW_RT_SOFT_ENTRY=vkr_shadow_mask_rt_soft_{which}", f"-DVKR_SHADOW_RT_SOFT_CUTOUT_ENTRY=vkr_shadow_mask_rt_soft_{which}_cutout",
           "-shared", "-o", path, os.path.join(CSRC, "shadow_mask_rt_soft.hip"), "-L" + CSRC, "-lvkr_postfx", "-Wl,-rpath," + CSRC]
    subprocess.check_call(cmd)
    return path


def load_variant(which, lib):
    """-> (opaque entry, cutout entry) of a built variant, or None"""
    path = VARIANTS[which][1]
    if not os.path.exists(path):
        return None
    so = C.CDLL(path)
    opaque, cutout = getattr(so, f"vkr_shadow_mask_rt_soft_{which}"), getattr(so, f"vkr_shadow_mask_rt_soft_{which}_cutout")
    opaque.argtypes, cutout.argtypes = lib.vkr_shadow_mask_rt_soft.argtypes, lib.vkr_shadow_mask_rt_soft_cutout.argtypes
    opaque.restype = cutout.restype = C.c_int
    return opaque, cutout


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shadow_mask_rt_soft.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--details", default="16,64")
    ap.add_argument("--samples", default="1,4,16")
    ap.add_argument("--build-variant", action="store_true", help="build the variants with the cull and with its report and exit (no GPU needed)")
    ap.add_argument("--git-head", default=None, help="the head to record when the tree that runs is not a git checkout")
    args = ap.parse_args()
    if args.build_variant:
        for which in VARIANTS:
            print("built", build_variant(which))
        return
    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, host
    from vk_renderer_amd import scene as scn
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.images import ImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("shadow_mask_rt_soft_timing: needs a GPU")
    lib = abi.product()
    stream = torch.cuda.current_stream().cuda_stream
    cull, report = load_variant("cull", lib), load_variant("report", lib)
    rows = []

    def row(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for detail in (int(x) for x in args.details.split(",")):
        sc = scn.procedural_scene(detail=detail)
        accel = abi.Accel.from_scene(sc)
        nodes, tris = accel.info()
        for size in args.sizes.split(","):
            W, H = (int(x) for x in size.split("x"))
            setup = FrameSetup(W, H)
            frame = host.HostFrame(setup, device="cuda")
            frame.load_scene(sc)
            frame.run(host.STAGE_RASTER)
            torch.cuda.synchronize()
            depth, normal = frame.image("depth", 0, 1), frame.image("normal")
            outs = {k: ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda") for k in ("hard", "soft", "cull", "report")}
            descs = {k: v.desc() for k, v in outs.items()}
            geometry = (frame.download("depth").raw(0)[..., 0] & 0xFFFFFF) != 0xFFFFFF
            common = dict(size=f"{W}x{H}", detail=detail, triangles=tris, nodes=nodes, calls_per_run=args.inner)

            def call(fn, rp, soft, key):
                return lambda: abi.check(fn(C.byref(depth), C.byref(normal), accel.handle, C.byref(rp), C.byref(soft), C.byref(descs[key]), stream), lib)

            for lights in (1, 4):
                rp = abi.shadow_rt_params(setup.inv_view, RAYS[:lights], *setup.fazz, normal_offset=abi.SHADOW_RT_NORMAL_OFFSET, tmin=abi.SHADOW_RT_TMIN)
                hard = lambda rp=rp: abi.check(lib.vkr_shadow_mask_rt(C.byref(depth), C.byref(normal), accel.handle, C.byref(rp), C.byref(descs["hard"]), stream), lib)  # noqa: E731
                for S in (int(x) for x in args.samples.split(",")):
                    soft = abi.shadow_rt_soft([RADIUS] * lights, S, PATTERN, device="cuda")
                    cases = {"vkr_shadow_mask_rt": hard, "vkr_shadow_mask_rt_soft (no cull)": call(lib.vkr_shadow_mask_rt_soft, rp, soft, "soft")}
                    if cull is not None:
                        cases["shadow_mask_rt_soft with the light-volume cull"] = call(cull[0], rp, soft, "cull")
                    if S == 1:
                        hard_path = abi.shadow_rt_soft([0.0] * lights, 1, PATTERN, device="cuda")
                        cases["vkr_shadow_mask_rt_soft, every radius 0 (the hard path)"] = call(lib.vkr_shadow_mask_rt_soft, rp, hard_path, "report")
                    for fn in cases.values():
                        for _ in range(2):
                            fn()
                    torch.cuda.synchronize()
                    if S == 1:
                        assert np.array_equal(outs["report"].raw(0), outs["hard"].raw(0)), "every radius 0 is not the hard entry"
                    times = {k: [] for k in cases}
                    for _ in range(args.reps):
                        for k, fn in cases.items():
                            times[k].append(_timed(fn, args.inner))
                    got = outs["soft"].raw(0)
                    same = bool(np.array_equal(got, outs["cull"].raw(0))) if cull is not None else None
                    settled = None
                    if report is not None:
                        call(report[0], rp, soft, "report")()
                        torch.cuda.synchronize()
                        rep = outs["report"].raw(0)[..., :lights][geometry]
                        assert np.isin(rep, (0, 255)).all(), "the report variant did not run its own kernel"
                        settled = round(float((rep == 255).mean()), 4)
                    hard_median = statistics.median(times["vkr_shadow_mask_rt"])
                    penumbra = round(float(((got[..., :lights][geometry] > 0) & (got[..., :lights][geometry] < 255)).mean()), 4)
                    for k in cases:
                        st = _stats(times[k])
                        row(measurement=k, lights=lights, samples=S, radius=RADIUS, pattern_side=PATTERN, **common, **st,
                            ratio_to_S_times_hard=round(st["median_ms"] / (S * hard_median), 4), share_settled_by_the_cull=settled,
                            share_in_penumbra=penumbra)
                    row(measurement="with and without the cull give the same bytes", lights=lights, samples=S, size=f"{W}x{H}", detail=detail,
                        value=same if same is not None else "variant with the cull not built")
                    if cull is not None:
                        assert same, "the cull changed a byte"
            frame.close()
        accel.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/shadow_mask_rt_soft_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
