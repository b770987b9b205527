#!/usr/bin/env python3
"""Times the shadow mask (csrc/shadow_mask.hip) and the two shading programs (csrc/shading.hip) with HIP events.

    python tools/shadow_mask_timing.py [--out profiles/shadow_mask.json] [--reps 20] [--inner 10] [--sizes 1920x1080,3840x2160]

On the procedural scene (cutout fence) rasterised by the host frame at each size, with 1024^2 shadow maps of lights A, B, C, A of
the tests rendered by VKRH_STAGE_SHADOW:
  * vkr_shadow_mask called directly for radius 0, 1, 2 and 1 and 4 lights (bias 4096 codes): time per call, the algorithmic
    bytes (4 B read + 4 B written per pixel; the map's texels are shared by neighbouring pixels and not counted) over that time,
    and that rate as a fraction of the float4 stream read (vkr_stream_read) measured in the same run; the share of light 0's
    channel that is 0 / 255 says what the kernel was looking at;
  * vkr_defered_shading and vkr_defered_shading_shadowed side by side on the images one full frame of the host frame left
    behind (the mask of radius 1, 1 light), and their ratio.
A run is --inner calls between one pair of events; reported per call: the median of --reps runs with min and max, the
candidates taking turns run by run.  No threshold: the numbers go into DESIGN.md section 7.7."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIGHTS = {  # eye -> center, as tests/shadow_light.py
    "A": ((-1.85867, 5.81832, -0.247114), (0.0, 2.0, 1.0)),
    "B": ((0.3, 0.4, 4.0), (0.0, 1.0, 8.0)),
    "C": ((-3.0, 2.5, 9.0), (1.0, 0.5, 3.0)),
}
BIAS = 4096
MAP = 1024


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shadow_mask.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--git-head", default=None, help="the head to record when the tree that runs is not a git checkout")
    args = ap.parse_args()
    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, camera, host
    from vk_renderer_amd import scene as scn
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.images import ImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("shadow_mask_timing: needs a GPU")
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

    mvps = [camera.shadow_mvp(eye=LIGHTS[k][0], center=LIGHTS[k][1]) for k in "ABCA"]
    sc = scn.procedural_scene(cutout=True)
    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        setup = FrameSetup(W, H)
        frame = host.HostFrame(setup, device="cuda")
        frame.load_scene(sc)
        frame.set_shadow_lights(mvps, MAP)
        frame.set_shadow_mask(bias=BIAS, radius=1)
        frame.run(host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH)
        frame.run(host.STAGE_RASTER | host.STAGE_SHADOW | host.STAGE_SHADOW_MASK | host.STAGE_CHAIN | host.STAGE_SHADING)
        torch.cuda.synchronize()
        depth = frame.image("depth", 0, 1)
        layers = []
        for l in range(4):
            d = abi.VkrImg()
            frame._check(host.lib().vkrh_image_layer(frame.h, b"shadows", l, C.byref(d)))
            layers.append(d)
        out = ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda")
        od = out.desc()

        cases = {}
        for lights in (1, 4):
            for radius in (0, 1, 2):
                p = abi.shadow_mask_params(setup.inv_view, mvps[:lights], *setup.fazz, radius=radius, bias=BIAS)
                cases[(lights, radius)] = (lambda p=p, lights=lights: abi.shadow_mask(depth, layers[:lights], p, od, stream))
        for fn in cases.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(args.reps):
            for k, fn in cases.items():
                times[k].append(_timed(fn, args.inner))
        nbytes = W * H * 8
        for (lights, radius), fn in cases.items():
            fn()
            torch.cuda.synchronize()
            a = out.raw(0)[..., 0]
            st = _stats(times[(lights, radius)])
            rate = nbytes / (st["median_ms"] * 1e-3) / 1e9
            row(measurement="vkr_shadow_mask", size=f"{W}x{H}", map=f"{MAP}x{MAP}", lights=lights, radius=radius, taps_per_light=(2 * radius + 1) ** 2, bias=BIAS,
                algorithmic_bytes=nbytes, gb_per_s=round(rate, 1), fraction_of_stream_read=round(rate / stream_gbs, 4), calls_per_run=args.inner,
                light0_share_shadowed=round(float((a == 0).mean()), 4), light0_share_lit=round(float((a == 255).mean()), 4), **st)

        # the two shading programs on the images of the frame above
        consts = abi.ShadingParams()
        consts.inverse_camera = abi.Mat4.from_np(setup.inv_view)
        consts.camera = abi.Mat4.from_np(setup.view)
        consts.shadow_mvp = abi.Mat4.from_np(mvps[0])
        consts.fovy, consts.aspect, consts.znear, consts.zfar = [float(v) for v in setup.fazz]
        push = abi.ShadingPush((C.c_float * 2)(0.0, 1.0), 0)
        head = [frame.image(name) for name in ("albedo", "normal", "material", "depth")]
        tail = [frame.image(name) for name in ("acc_ao", "brdf", "blurred")]
        mask = frame.image("shadow_mask")
        color = ImageBuf(abi.FMT_RGBA8_SRGB, W, H, device="cuda")
        cd = color.desc()
        refs = [C.byref(v) for v in head + [consts] + tail]

        def plain():
            abi.check(lib.vkr_defered_shading(*refs, C.byref(cd), C.byref(push), stream), lib)

        def shadowed():
            abi.defered_shading_shadowed(*head, consts, *tail, mask, cd, push, stream)

        shading = {"vkr_defered_shading": plain, "vkr_defered_shading_shadowed": shadowed}
        for fn in shading.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        st_times = {k: [] for k in shading}
        for _ in range(args.reps):
            for k, fn in shading.items():
                st_times[k].append(_timed(fn, args.inner))
        st = {k: _stats(v) for k, v in st_times.items()}
        for k in shading:
            row(measurement=k, size=f"{W}x{H}", calls_per_run=args.inner, **st[k])
        row(measurement="shadowed / plain shading", size=f"{W}x{H}",
            ratio_of_medians=round(st["vkr_defered_shading_shadowed"]["median_ms"] / st["vkr_defered_shading"]["median_ms"], 4))
        frame.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/shadow_mask_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
