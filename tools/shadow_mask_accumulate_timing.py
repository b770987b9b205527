#!/usr/bin/env python3
"""Times the temporal accumulation of the shadow mask (csrc/shadow_mask_accumulate.hip) with HIP events beside its bandwidth floor,
and measures what it buys: the error against a mask of 64 rays per pixel, frame after frame.

    python tools/shadow_mask_accumulate_timing.py [--out profiles/shadow_mask_accumulate.json] [--reps 20] [--inner 10]
                                                  [--size 3840x2160] [--quality-size 1920x1080] [--detail 64] [--build-variant]

On the procedural scene at --detail, rasterised by the host frame, with the four lights of tools/shadow_mask_filter_timing.py at
radius 0.5:
  * time, at --size: the pass alone on the rasterised G-buffer with prev_depth = depth, a history in every texel and (a) zero
    velocity, (b) a whole-frame pan of 3.5 texels, (c) reset = 1 (no gather); the same for the library built with
    -DVKR_SHADOW_ACCUM_PLAIN_DIVIDE=1 through tools/build_variants.sh (--build-variant builds it and exits: no GPU needed; without it
    the rows say so), run by run in turns, with a byte comparison of the two; and, in the same run, vkr_stream_read over the pass's
    byte count (29 B read and 13 B written per pixel): the bandwidth floor the ratio is taken against;
  * quality, at --quality-size with a static camera: the mean absolute byte error over the penumbra (the channels of geometry pixels
    whose 64-ray value is neither 0 nor 255) of soft(S 1, P 4) + filter(R 4); of soft(S 1, P 4 with the table of frame k of 8) +
    accumulation (max_count 8 and 32) with and without the filter after 1, 4, 8 and 32 frames; and of soft(S 16, P 1) alone;
  * the same chain under a camera that pans about --pan-pixels texels a frame (the frame rasterises every frame and swaps its depths;
    the 64-ray mask is traced again per measured frame): what the disocclusion resets cost, and the share of geometry pixels with a
    valid history.
A timed run is --inner calls between one pair of events; reported per call: the median of --reps runs with min and max.  No threshold
anywhere: the numbers go into DESIGN.md section 7.16."""
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
VARIANT = os.path.join(CSRC, "variants", "accum_plain_divide", "libvkr_postfx.so")

LIGHT_POS = (-1.85867, 5.81832, -0.247114)
RAYS = [LIGHT_POS + (1.0,), (3.0, 4.0, 2.0, 1.0), (1.5, 4.5, -1.5, 0.0), (-6.0, 9.0, 3.0, 0.0)]
RADIUS = 0.5
S, P, REACH, PATTERN_FRAMES = 1, 4, 4, 8
MAX_COUNTS = (8, 32)
AFTER = (1, 4, 8, 32)
BYTES_READ, BYTES_WRITTEN = 4 + 4 + 4 + 4 + 4 + 8 + 1, 8 + 1 + 4


def build_variant():
    subprocess.check_call(["bash", os.path.join(ROOT, "tools", "build_variants.sh"), "shadow_mask_accumulate.hip", "accum_plain_divide",
                           "-DVKR_SHADOW_ACCUM_PLAIN_DIVIDE=1"])
    return VARIANT


def load_variant(lib):
    """-> vkr_shadow_mask_accumulate of the library built with the plain divide, or None"""
    if not os.path.exists(VARIANT):
        return None
    fn = C.CDLL(VARIANT).vkr_shadow_mask_accumulate
    fn.argtypes, fn.restype = lib.vkr_shadow_mask_accumulate.argtypes, C.c_int
    return fn


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shadow_mask_accumulate.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--quality-size", default="1920x1080")
    ap.add_argument("--detail", type=int, default=64)
    ap.add_argument("--pan-pixels", type=float, default=4.0)
    ap.add_argument("--build-variant", action="store_true", help="build the library with the plain divide and exit (no GPU needed)")
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
        raise SystemExit("shadow_mask_accumulate_timing: needs a GPU")
    lib = abi.product()
    stream = torch.cuda.current_stream().cuda_stream
    plain_divide = load_variant(lib)
    rows = []

    def row(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    sc = scn.procedural_scene(detail=args.detail)
    accel = abi.Accel.from_scene(sc)

    def still(W, H, eye=(0.0, 1.0, -1.0)):
        return FrameSetup(W, H, eye=eye, prev_delta=(0.0, 0.0, 0.0), prev_yaw_delta=0.0)

    def accumulate(fn, depth, normal, velocity, prev_depth, mask, history, count, params, out_history, out_count, out_mask):
        abi.check(fn(C.byref(depth), C.byref(normal), C.byref(velocity), C.byref(prev_depth), C.byref(mask), C.byref(history), C.byref(count),
                     C.byref(params), C.byref(out_history), C.byref(out_count), C.byref(out_mask), stream), lib)

    # ---- time ---------------------------------------------------------------------------------------------------------------------
    W, H = (int(x) for x in args.size.split("x"))
    setup = still(W, H)
    frame = host.HostFrame(setup, device="cuda")
    frame.load_scene(sc)
    frame.run(host.STAGE_RASTER)
    torch.cuda.synchronize()
    depth, normal = frame.image("depth", 0, 1), frame.image("normal")
    geometry = (frame.download("depth").raw(0)[..., 0] & 0xFFFFFF) != 0xFFFFFF
    common = dict(size=f"{W}x{H}", detail=args.detail, calls_per_run=args.inner, geometry_share=round(float(geometry.mean()), 4))
    rng = np.random.default_rng(7)

    def image(fmt, arr=None):
        im = ImageBuf(fmt, W, H, device="cuda")
        if arr is not None:
            h = ImageBuf(fmt, W, H)
            h.set_raw(arr)
            im.upload(h.to_host())
        return im

    velocities = {"zero velocity": image(abi.FMT_RG16_SFLOAT),
                  "pan of 3.5 texels": image(abi.FMT_RG16_SFLOAT, np.broadcast_to(np.array([3.5 / W, 0.0], np.float16), (H, W, 2)))}
    mask = image(abi.FMT_RGBA8_UNORM, rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8))
    history = image(abi.FMT_RGBA16_UNORM, rng.integers(0, 65536, size=(H, W, 4), dtype=np.uint16))
    count = image(abi.FMT_R8_UNORM, np.full((H, W, 1), 5, np.uint8))
    outs = {k: (image(abi.FMT_RGBA16_UNORM), image(abi.FMT_R8_UNORM), image(abi.FMT_RGBA8_UNORM)) for k in ("library", "variant")}

    def call(fn, which, velocity, reset):
        p = abi.shadow_accum_params(setup.inv_view, setup.inv_view, *setup.fazz, max_count=8, reset=reset)
        oh, oc, om = (o.desc() for o in outs[which])
        return lambda: accumulate(fn, depth, normal, velocity.desc(), depth, mask.desc(), history.desc(), count.desc(), p, oh, oc, om)

    nbytes = (BYTES_READ + BYTES_WRITTEN) * W * H
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    sink = torch.zeros(4096, dtype=torch.float32, device="cuda")
    floor = lambda: abi.check(lib.vkr_stream_read(src.data_ptr(), nbytes, sink.data_ptr(), 4096, stream), lib)  # noqa: E731
    cases = {}
    for name, vel in velocities.items():
        cases[f"vkr_shadow_mask_accumulate, {name}"] = call(lib.vkr_shadow_mask_accumulate, "library", vel, False)
        if plain_divide is not None:
            cases[f"shadow_mask_accumulate with the plain divide, {name}"] = call(plain_divide, "variant", vel, False)
    cases["vkr_shadow_mask_accumulate, reset"] = call(lib.vkr_shadow_mask_accumulate, "library", velocities["zero velocity"], True)
    cases["vkr_stream_read of the pass's bytes"] = floor
    for fn in cases.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    if plain_divide is not None:
        for name, vel in velocities.items():
            call(lib.vkr_shadow_mask_accumulate, "library", vel, False)()
            call(plain_divide, "variant", vel, False)()
            torch.cuda.synchronize()
            same = all(bool(np.array_equal(a.raw(0), b.raw(0))) for a, b in zip(outs["library"], outs["variant"]))
            row(measurement="the two divisions give the same bytes", velocity=name, size=f"{W}x{H}", value=same)
            assert same, "the division changed a byte"
    else:
        row(measurement="the two divisions give the same bytes", size=f"{W}x{H}", value="variant with the plain divide not built")
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, fn in cases.items():
            times[k].append(_timed(fn, args.inner))
    floor_ms = statistics.median(times["vkr_stream_read of the pass's bytes"])
    for k in cases:
        st = _stats(times[k])
        row(measurement=k, **common, **st, bytes_per_pixel=BYTES_READ + BYTES_WRITTEN, gbytes_per_s=round(nbytes / st["median_ms"] / 1e6, 1),
            ratio_to_the_floor=round(st["median_ms"] / floor_ms, 3))
    frame.close()
    del src, outs, history, mask, count, velocities

    # ---- quality ------------------------------------------------------------------------------------------------------------------
    W, H = (int(x) for x in args.quality_size.split("x"))

    def rgba8():
        return ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda")

    tables = [abi.shadow_rt_soft([RADIUS] * 4, S, P, device="cuda", table=abi.shadow_disk_samples_frame(S, P, f, PATTERN_FRAMES)) for f in range(PATTERN_FRAMES)]
    fixed = abi.shadow_rt_soft([RADIUS] * 4, S, P, device="cuda")
    s16, s64 = abi.shadow_rt_soft([RADIUS] * 4, 16, 1, device="cuda"), abi.shadow_rt_soft([RADIUS] * 4, 64, 1, device="cuda")

    for motion, step in (("static camera", 0.0), (f"pan of about {args.pan_pixels:g} texels a frame", None)):
        frame = host.HostFrame(still(W, H), device="cuda")
        frame.load_scene(sc)
        if step is None:  # the world step that moves a point 3 units away by pan_pixels texels
            fovy, aspect = float(still(W, H).fazz[0]), float(still(W, H).fazz[1])
            step = args.pan_pixels * 3.0 * (2.0 * np.tan(fovy / 2) * aspect / W)
        mask_img, truth_img, filtered_img = rgba8(), rgba8(), rgba8()
        state = {mc: dict(history=[ImageBuf(abi.FMT_RGBA16_UNORM, W, H, device="cuda") for _ in range(2)],
                          count=[ImageBuf(abi.FMT_R8_UNORM, W, H, device="cuda") for _ in range(2)], out=rgba8()) for mc in MAX_COUNTS}
        prev_view, prev_inverse = None, None
        for k in range(max(AFTER)):
            eye = (step * k, 1.0, -1.0)
            setup = still(W, H, eye)
            frame.set_camera(setup.view, setup.view if prev_view is None else prev_view, setup.proj, setup.fazz)
            frame.run(host.STAGE_RASTER)
            depth, normal, velocity, prev_depth = frame.image("depth", 0, 1), frame.image("normal"), frame.image("velocity"), frame.image("prev_depth", 0, 1)
            rp = abi.shadow_rt_params(setup.inv_view, RAYS, *setup.fazz, normal_offset=abi.SHADOW_RT_NORMAL_OFFSET, tmin=abi.SHADOW_RT_TMIN)

            def soft(block, out):
                abi.check(lib.vkr_shadow_mask_rt_soft(C.byref(depth), C.byref(normal), accel.handle, C.byref(rp), C.byref(block), C.byref(out.desc()), stream), lib)

            def filt(source, out):
                fp = abi.shadow_filter_params(setup.inv_view, *setup.fazz, REACH)
                abi.check(lib.vkr_shadow_mask_filter(C.byref(depth), C.byref(normal), C.byref(source.desc()), C.byref(fp), C.byref(out.desc()), stream), lib)

            measured = (k + 1) in AFTER
            if measured:
                soft(s64, truth_img)
                torch.cuda.synchronize()
                truth = truth_img.raw(0).astype(np.int32)
                geometry = (frame.download("depth").raw(0)[..., 0] & 0xFFFFFF) != 0xFFFFFF
                penumbra = geometry[..., None] & (truth > 0) & (truth < 255)

                def error(im):
                    torch.cuda.synchronize()
                    diff = np.abs(im.raw(0).astype(np.int32) - truth)[penumbra]
                    return {"mean_abs_byte_error": round(float(diff.mean()), 3), "p99_abs_byte_error": float(np.percentile(diff, 99))}

                base = dict(size=f"{W}x{H}", camera=motion, frames=k + 1, penumbra_share_of_geometry_channels=round(float(penumbra.sum() / (4.0 * geometry.sum())), 5))
                if k == 0:
                    soft(fixed, mask_img)
                    row(measurement="soft S 1 P 4, unfiltered", **base, **error(mask_img))
                    filt(mask_img, filtered_img)
                    row(measurement="soft S 1 P 4 + filter R 4", **base, **error(filtered_img))
                    soft(s16, mask_img)
                    row(measurement="soft S 16 P 1, unfiltered", **base, **error(mask_img))
            soft(tables[k % PATTERN_FRAMES], mask_img)
            for mc in MAX_COUNTS:
                st = state[mc]
                p = abi.shadow_accum_params(setup.inv_view, setup.inv_view if prev_inverse is None else prev_inverse, *setup.fazz, max_count=mc, reset=(k == 0))
                accumulate(lib.vkr_shadow_mask_accumulate, depth, normal, velocity, prev_depth, mask_img.desc(), st["history"][0].desc(), st["count"][0].desc(), p,
                           st["history"][1].desc(), st["count"][1].desc(), st["out"].desc())
                st["history"].reverse()
                st["count"].reverse()
                if measured:
                    torch.cuda.synchronize()
                    kept = float((st["count"][0].raw(0)[..., 0][geometry] > 1).mean())
                    extra = dict(max_count=mc, pattern_frames=PATTERN_FRAMES, geometry_share_with_a_history=round(kept, 4))
                    row(measurement="soft S 1 P 4 + accumulation", **base, **extra, **error(st["out"]))
                    filt(st["out"], filtered_img)
                    row(measurement="soft S 1 P 4 + accumulation + filter R 4", **base, **extra, **error(filtered_img))
            torch.cuda.synchronize()
            frame.end_frame(True)
            prev_view, prev_inverse = setup.view, setup.inv_view
        frame.close()
    accel.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/shadow_mask_accumulate_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
