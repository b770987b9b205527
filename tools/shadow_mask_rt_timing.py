#!/usr/bin/env python3
"""Times the ray-traced shadow mask (csrc/shadow_mask_rt.hip) with HIP events and measures the default ray offset.

    python tools/shadow_mask_rt_timing.py [--out profiles/shadow_mask_rt.json] [--reps 20] [--inner 10]
                                          [--sizes 1920x1080,3840x2160] [--details 16,64] [--build-variant]

On the procedural scene at each detail, rasterised by the host frame at each size, for 1 and 4 lights (light 0 is the point light
at the shading pass's LIGHT_POS, then a second point light and two directional ones), three candidates take turns run by run:
  * vkr_shadow_mask_rt: the shipped kernel, wave_any_hit_ray (segment box AND per-ray slab test);
  * the same kernel on wave_any_hit (segment box only): csrc/shadow_mask_rt.hip built a second time by this tool with
    -DVKR_SHADOW_RT_WALK=wave_any_hit under the entry name vkr_shadow_mask_rt_segbox into csrc/build/ (--build-variant builds it
    and exits: no GPU needed; without the library the candidate is left out and the rows say so).  Not an entry of the product;
  * vkr_shadow_mask at radius 1, bias 4096 codes, on 1024^2 maps of the same lights rendered by the same frame (for a
    directional light the map of the point light standing at the end of its vector: the lookup has no directional lights).
A run is --inner calls between one pair of events; reported per call: the median of --reps runs with min and max.  The two
traced candidates must give the same bytes (both are exact); the tool checks that.  For orientation: the share of non-sky pixels
on which light 0's channel agrees with vkr_shadow_mask at radius 0 and bias 4096.

The default offset: a single large floor facing the default light at the frame's default camera, no occluder,
so every non-sky pixel is lit; for normal_offset = 1e-6 .. 1e-1 and tmin = 0 the number of floor pixels that read 0 at 256 x 144
and 1920 x 1080.  No threshold anywhere: the numbers go into DESIGN.md section 7.8."""
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
VARIANT = os.path.join(CSRC, "build", "libvkr_shadow_rt_segbox.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

LIGHT_POS = (-1.85867, 5.81832, -0.247114)
RAYS = [LIGHT_POS + (1.0,), (3.0, 4.0, 2.0, 1.0), (1.5, 4.5, -1.5, 0.0), (-6.0, 9.0, 3.0, 0.0)]
CENTER = (0.0, 2.0, 1.0)
BIAS = 4096
MAP = 1024


def build_variant():
    """csrc/shadow_mask_rt.hip on the segment-box walk, with the flags of csrc/Makefile, linked against the product library"""
    os.makedirs(os.path.dirname(VARIANT), exist_ok=True)
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-DVKR_CONTRACT=2",
           "-fno-gpu-flush-denormals-to-zero", "-Wall", "-Wno-unused-function", "-DVKR_SHADOW_RT_WALK=wave_any_hit",
           "-DVKR_SHADOW_RT_ENTRY=vkr_shadow_mask_rt_segbox", "-shared", "-o", VARIANT, os.path.join(CSRC, "shadow_mask_rt.hip"),
           "-L" + CSRC, "-lvkr_postfx", "-Wl,-rpath," + CSRC]
    subprocess.check_call(cmd)
    return VARIANT


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


def plane_scene(scn, np):
    sc = scn.Scene()
    quad = sc.add_mesh(np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], np.float32), np.array([[0, 1, 0]] * 4, np.float32),
                       np.array([[0, 0], [8, 0], [8, 8], [0, 8]], np.float32), np.array([0, 2, 1, 0, 3, 2], np.uint32))
    sc.add_draw(sc.add_transform(np.array([[40, 0, 0, 0], [0, 1, 0, 0], [0, 0, 40, 30], [0, 0, 0, 1]], dtype=np.float32)), quad)
    return sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shadow_mask_rt.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--details", default="16,64")
    ap.add_argument("--build-variant", action="store_true", help="build the segment-box variant of the kernel and exit (no GPU needed)")
    ap.add_argument("--git-head", default=None, help="the head to record when the tree that runs is not a git checkout")
    args = ap.parse_args()
    if args.build_variant:
        print("built", build_variant())
        return
    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, camera, host
    from vk_renderer_amd import scene as scn
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.images import ImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("shadow_mask_rt_timing: needs a GPU")
    lib = abi.product()
    stream = torch.cuda.current_stream().cuda_stream
    segbox = None
    if os.path.exists(VARIANT):
        segbox = C.CDLL(VARIANT).vkr_shadow_mask_rt_segbox
        segbox.argtypes = lib.vkr_shadow_mask_rt.argtypes
        segbox.restype = C.c_int
    rows = []

    def row(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    # ---- the default offset: acne on the plane-only scene ----
    for W, H in ((256, 144), (1920, 1080)):
        frame = host.HostFrame(FrameSetup(W, H), device="cuda")
        frame.load_scene(plane_scene(scn, np))
        frame.run(host.STAGE_RASTER)
        torch.cuda.synchronize()
        geometry = (frame.download("depth").raw(0)[..., 0] & 0xFFFFFF) != 0xFFFFFF
        for exp in range(-6, 0):
            offset = float(f"1e{exp}")
            frame.set_shadow_rays([RAYS[0]], normal_offset=offset, tmin=0.0)
            frame.run(host.STAGE_SHADOW_MASK_RT)
            torch.cuda.synchronize()
            a = frame.download("shadow_mask").raw(0)[..., 0]
            row(measurement="plane-only acne", size=f"{W}x{H}", normal_offset=offset, tmin=0.0, floor_pixels=int(geometry.sum()),
                pixels_reading_0=int((a[geometry] == 0).sum()))
        frame.close()

    # ---- timings ----
    # the lookup's lights: the point lights look at CENTER; a directional light is stood in for by a point light at the end of its vector
    mvps = [camera.shadow_mvp(eye=tuple(r[:3]) if r[3] == 1.0 else tuple(c + v for c, v in zip(CENTER, r[:3])), center=CENTER) for r in RAYS]
    for detail in (int(x) for x in args.details.split(",")):
        sc = scn.procedural_scene(detail=detail)
        accel = abi.Accel.from_scene(sc)
        nodes, tris = accel.info()
        for size in args.sizes.split(","):
            W, H = (int(x) for x in size.split("x"))
            setup = FrameSetup(W, H)
            frame = host.HostFrame(setup, device="cuda")
            frame.load_scene(sc)
            frame.set_shadow_lights(mvps, MAP)
            frame.run(host.STAGE_RASTER | host.STAGE_SHADOW)
            torch.cuda.synchronize()
            depth, normal = frame.image("depth", 0, 1), frame.image("normal")
            layers = []
            for l in range(4):
                d = abi.VkrImg()
                frame._check(host.lib().vkrh_image_layer(frame.h, b"shadows", l, C.byref(d)))
                layers.append(d)
            layer_arr = (abi.VkrImg * 4)(*layers)
            outs = {k: ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda") for k in ("rt", "segbox", "map")}
            descs = {k: v.desc() for k, v in outs.items()}
            geometry = (frame.download("depth").raw(0)[..., 0] & 0xFFFFFF) != 0xFFFFFF
            for lights in (1, 4):
                rp = abi.shadow_rt_params(setup.inv_view, RAYS[:lights], *setup.fazz, normal_offset=abi.SHADOW_RT_NORMAL_OFFSET, tmin=abi.SHADOW_RT_TMIN)
                mp = abi.shadow_mask_params(setup.inv_view, mvps[:lights], *setup.fazz, radius=1, bias=BIAS)
                cases = {"vkr_shadow_mask_rt (per-ray cull)":
                         lambda rp=rp: abi.check(lib.vkr_shadow_mask_rt(C.byref(depth), C.byref(normal), accel.handle, C.byref(rp), C.byref(descs["rt"]), stream), lib)}
                if segbox is not None:
                    cases["shadow_mask_rt on the segment-box walk"] = \
                        lambda rp=rp: abi.check(segbox(C.byref(depth), C.byref(normal), accel.handle, C.byref(rp), C.byref(descs["segbox"]), stream), lib)
                cases["vkr_shadow_mask radius 1"] = \
                    lambda mp=mp: abi.check(lib.vkr_shadow_mask(C.byref(depth), layer_arr, C.byref(mp), C.byref(descs["map"]), stream), lib)
                for fn in cases.values():
                    for _ in range(2):
                        fn()
                torch.cuda.synchronize()
                times = {k: [] for k in cases}
                for _ in range(args.reps):
                    for k, fn in cases.items():
                        times[k].append(_timed(fn, args.inner))
                rt = outs["rt"].raw(0)
                same = bool(np.array_equal(rt, outs["segbox"].raw(0))) if segbox is not None else None
                for k in cases:
                    row(measurement=k, size=f"{W}x{H}", detail=detail, triangles=tris, nodes=nodes, lights=lights, calls_per_run=args.inner,
                        light0_share_shadowed=round(float((rt[..., 0][geometry] == 0).mean()), 4), **_stats(times[k]))
                row(measurement="the two walks give the same bytes", size=f"{W}x{H}", detail=detail, lights=lights,
                    value=same if same is not None else "segment-box variant not built")
                if segbox is not None:
                    assert same, "the two exact walks disagree"
            # orientation: light 0 against the lookup at radius 0
            mp = abi.shadow_mask_params(setup.inv_view, mvps[:1], *setup.fazz, radius=0, bias=BIAS)
            abi.check(lib.vkr_shadow_mask(C.byref(depth), layer_arr, C.byref(mp), C.byref(descs["map"]), stream), lib)
            torch.cuda.synchronize()
            agree = outs["rt"].raw(0)[..., 0][geometry] == outs["map"].raw(0)[..., 0][geometry]
            row(measurement="light 0 agrees with vkr_shadow_mask radius 0", size=f"{W}x{H}", detail=detail, bias=BIAS, map=f"{MAP}x{MAP}",
                non_sky_pixels=int(geometry.sum()), share=round(float(agree.mean()), 5))
            frame.close()
        accel.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/shadow_mask_rt_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
