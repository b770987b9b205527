#!/usr/bin/env python3
"""Times the refit of the ray-query structure (csrc/accel_refit.hip) and the cost of the stale topology it leaves, with HIP events.

    python tools/accel_refit_timing.py [--out profiles/accel_refit.json] [--details 24,150] [--size 1920x1080] [--reps 9]

Per scene, procedural_scene(detail) (detail 24: 6916 triangles; detail 150: about 270k, Sponza-sized), two tables.

refit: vkr_scene_triangles and vkr_accel_refit on the scene with one sphere moved by its radius — each entry alone and both together,
per call, the median of --reps runs of `calls_per_run` calls between one pair of events, with the number of kernel launches a call
makes (from vkr_accel_refit_schedule: one over the records, one per level above the tail size, the tail; vkr_scene_triangles: one per
32 draws for the table and one for the triangles) — beside the only route to a moved scene there was before: vkr_accel_create on the
moved triangles (host build + synchronous upload), a host clock around the synchronous call.  The ratio is recorded, not asserted.
Per-kernel times inside one call are not measured here: they want a kernel trace in a run of its own.

stale topology: vkr_accel_closest on the frame's reflection rays (tools/reflections_rt_timing.py reflection_rays, half of --size)
and vkr_shadow_mask_rt at --size with one point light, on the REFITTED structure and on one freshly CREATED at the same pose, taking
turns run by run.  Poses: `small move` (one sphere moved by its radius; the G-buffer comes from the frame after
vkrh_set_draw_transforms), `cluster swap` (the two halves of the input exchange places: a neighbourhood of the mesh stays a
neighbourhood, only the upper levels stop fitting) and, at detail 24 only, `scramble` (a random permutation of the input: every leaf
holds triangles from all over the scene — the worst a topology can get; at 270k triangles a single call would run for seconds).
The geometry of the last two is the built scene's as a set, so their G-buffer is the unmoved frame's.  The tool checks what must hold
whatever the time: both structures give the same bytes.  No threshold anywhere: the numbers go into DESIGN.md section 7.14."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from reflections_rt_timing import _git_head, _stats, _timed, reflection_rays  # noqa: E402

LIGHT = (0.5, 2.5, 8.0, 1.0)
SPHERE_DRAW, SPHERE_RADIUS = 2, 0.9  # procedural_scene: the first sphere and its scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accel_refit.json"))
    ap.add_argument("--details", default="24,150")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--git-head", default=None, help="the head to record when the tree that runs is not a git checkout")
    args = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, host
    from vk_renderer_amd import scene as scn
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.images import ImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("accel_refit_timing: needs a GPU")
    stream = torch.cuda.current_stream().cuda_stream
    lib = abi.product()
    W, H = (int(x) for x in args.size.split("x"))
    refit_rows, stale_rows = [], []

    def emit(rows, **kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    def calls_per_run(fn):
        """enough calls that a run lasts about 20 ms, at most 50; 1 for a call of 20 ms or more"""
        for _ in range(2):
            fn()
        one = _timed(fn, 1)
        return max(1, min(50, int(20.0 / max(one, 1e-3))))

    def compare(cases, reps):
        inner = min(calls_per_run(fn) for fn in cases.values())
        times = {k: [] for k in cases}
        for _ in range(reps):
            for k, fn in cases.items():
                times[k].append(_timed(fn, inner))
        return {k: dict(_stats(v), calls_per_run=inner) for k, v in times.items()}

    for detail in (int(x) for x in args.details.split(",")):
        sc = scn.procedural_scene(detail=detail)
        tris = np.ascontiguousarray(abi.scene_triangles(sc), np.float32)
        n = len(tris)
        models = [np.array(sc.transforms[d["transform"]][0], np.float32) for d in sc.draws]
        moved_models = [m.copy() for m in models]
        moved_models[SPHERE_DRAW][0, 3] += np.float32(SPHERE_RADIUS)
        moved_sc = scn.procedural_scene(detail=detail)
        moved_sc.transforms = []
        for d, m in zip(moved_sc.draws, moved_models):
            d["transform"] = moved_sc.add_transform(m)
        small = np.ascontiguousarray(abi.scene_triangles(moved_sc), np.float32)
        common = dict(scene=f"procedural, detail {detail}", triangles=n)

        # ---- table 1: the refit against a new build ---------------------------------------------------------------------------------
        accel = abi.Accel(tris)
        nodes = accel.info()[0]
        sizes, tail = accel.refit_schedule()
        refit_launches = 1 + sum(1 for s in sizes if s > tail) + 1
        rs, keep = moved_sc.upload(device="cuda")
        table_launches = (rs.draw_count + 31) // 32 + 1
        out = torch.zeros((n, 9), dtype=torch.float32, device="cuda")
        nbytes = abi.scene_triangles_scratch_bytes(rs.draw_count)
        scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

        def scene_triangles():
            abi.check(lib.vkr_scene_triangles(C.byref(rs), out.data_ptr(), n, scratch.data_ptr(), nbytes, stream), lib)

        def refit():
            accel.refit(out, stream)

        def both():
            scene_triangles()
            refit()

        stats = compare({"vkr_scene_triangles": scene_triangles, "vkr_accel_refit": refit, "vkr_scene_triangles + vkr_accel_refit": both}, args.reps)
        assert out.cpu().numpy().reshape(-1, 3, 3).tobytes() == small.tobytes(), "vkr_scene_triangles and abi.scene_triangles differ"
        launches = {"vkr_scene_triangles": table_launches, "vkr_accel_refit": refit_launches, "vkr_scene_triangles + vkr_accel_refit": table_launches + refit_launches}
        for k, s in stats.items():
            emit(refit_rows, measurement=k, **common, nodes=nodes, levels=len(sizes), level_sizes_above_the_tail=[x for x in sizes if x > tail],
                 kernel_launches_per_call=launches[k], **s)
        build = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fresh = abi.Accel(small)
            build.append((time.perf_counter() - t0) * 1e3)
            fresh.close()
        total = stats["vkr_scene_triangles + vkr_accel_refit"]["median_ms"]
        emit(refit_rows, measurement="vkr_accel_create on the moved triangles (host build + upload, host clock)", **common, **_stats(build),
             ratio_to_scene_triangles_plus_refit=round(sorted(build)[1] / total, 1))

        # ---- table 2: what the stale topology costs the walks ----------------------------------------------------------------------
        setup = FrameSetup(W, H)
        frame = host.HostFrame(setup, device="cuda")
        frame.load_scene(sc)
        frame.run(host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH)
        rng = np.random.default_rng(7)
        half = n // 2
        poses = [("cluster swap", np.concatenate([tris[half:], tris[:half]]), False)]
        if n <= 20000:
            poses.append(("scramble", tris[rng.permutation(n)], False))
        poses.append(("small move", small, True))  # last: it moves the frame's draws
        for pose_name, pose, moves_frame in poses:
            if moves_frame:
                frame.set_draw_transforms(moved_models)
            frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE)
            torch.cuda.synchronize()
            verts = torch.from_numpy(np.ascontiguousarray(pose)).to("cuda")
            accel.refit(verts, stream)
            fresh = abi.Accel(pose)
            org, dirs, _ = reflection_rays(np, frame.download("depth").raw(1)[..., 0].astype(np.uint32), frame.download("dn").raw(0), setup,
                                           abi.SHADOW_RT_NORMAL_OFFSET)
            rays = len(org)
            to, td = torch.from_numpy(org).to("cuda"), torch.from_numpy(dirs).to("cuda")
            zfar = float(setup.fazz[3])
            hits = {k: torch.zeros((rays, 4), dtype=torch.int32, device="cuda") for k in ("refitted", "created")}
            stats = compare({"refitted": lambda: accel.closest(to, td, 0.0, zfar, hits["refitted"], stream),
                             "created": lambda: fresh.closest(to, td, 0.0, zfar, hits["created"], stream)}, args.reps)
            assert torch.equal(hits["refitted"], hits["created"]), "the refitted and the created structure answer differently"
            slow = stats["refitted"]["median_ms"] / stats["created"]["median_ms"]
            for k, s in stats.items():
                emit(stale_rows, measurement="vkr_accel_closest", pose=pose_name, structure=k, **common, rays=rays, refitted_over_created=round(slow, 3), **s)
            outs = {k: ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda") for k in ("refitted", "created")}
            sp = abi.shadow_rt_params(setup.inv_view, [LIGHT], *setup.fazz)
            depth0, normal0 = frame.image("depth", 0, 1), frame.image("normal")
            stats = compare({"refitted": lambda: abi.shadow_mask_rt(depth0, normal0, accel, sp, outs["refitted"].desc(), stream),
                             "created": lambda: abi.shadow_mask_rt(depth0, normal0, fresh, sp, outs["created"].desc(), stream)}, args.reps)
            assert np.array_equal(outs["refitted"].raw(0), outs["created"].raw(0)), "the refitted and the created structure give other masks"
            slow = stats["refitted"]["median_ms"] / stats["created"]["median_ms"]
            for k, s in stats.items():
                emit(stale_rows, measurement="vkr_shadow_mask_rt", pose=pose_name, structure=k, **common, size=f"{W}x{H}", refitted_over_created=round(slow, 3), **s)
            fresh.close()
        frame.close()
        accel.close()
        del keep
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/accel_refit_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(),
                   "refit": refit_rows, "stale_topology": stale_rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
