#!/usr/bin/env python3
"""Times the lit ray-traced reflections (csrc/reflections_rt_lit.hip) and the device-side normal table (csrc/scene_normals.hip) with
HIP events.

    python tools/reflections_rt_lit_timing.py [--out profiles/reflections_rt_lit_timing.json] [--reps 20] [--inner 10]
                                              [--size 3840x2160] [--detail 64]

On the procedural scene and on Suzanne (tools/reflections_rt_timing.py's placement), each rasterised by the host frame at --size, whose
half resolution (1920 x 1080 by default) is where the SSR images live:
  (a) vkr_reflections_rt beside vkr_reflections_rt_lit with 0, 1 and 4 lights (the lights of tests/test_reflections_rt_lit.py; 0: no
      light and ambient 1, the unlit image), called by hand on the frame's images, mode all;
  (b) vkr_scene_triangles beside vkr_scene_triangle_normals on the scene's draws.
A run is --inner calls between one pair of events; the candidates of one comparison take turns run by run; reported per call: the
median of --reps runs with min and max.  No threshold anywhere: the numbers go into DESIGN.md section 7.15."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from reflections_rt_timing import _git_head, _stats, _timed, suzanne_scene  # noqa: E402

LIGHTS = [(-1.85867, 5.81832, -0.247114, 1.0), (3.0, 4.0, -2.0, 0.0), (0.0, 0.25, 4.0, 1.0), (-6.0, 1.0, 3.0, 0.0)]
COLOURS = [(3.0, 2.5, 2.0), (0.30, 0.27, 0.22), (0.25, 0.35, 0.45), (0.12, 0.2, 0.16)]
AMBIENT = (0.1, 0.12, 0.14)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reflections_rt_lit_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--detail", type=int, default=64)
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
        raise SystemExit("reflections_rt_lit_timing: needs a GPU")
    lib = abi.product()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def row(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    def compare(cases):
        """the candidates take turns run by run: -> {name: stats}"""
        for fn in cases.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(args.reps):
            for k, fn in cases.items():
                times[k].append(_timed(fn, args.inner))
        return {k: _stats(v) for k, v in times.items()}

    W, H = (int(x) for x in args.size.split("x"))
    w2, h2 = W // 2, H // 2
    for name, sc in (("procedural", scn.procedural_scene(detail=args.detail)), ("suzanne", suzanne_scene(scn, np))):
        accel = abi.Accel.from_scene(sc)
        nodes, tris = accel.info()
        setup = FrameSetup(W, H)
        frame = host.HostFrame(setup, device="cuda")
        frame.load_scene(sc)
        frame.run(host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH)
        frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE)
        torch.cuda.synchronize()
        common = dict(scene=name, size=f"{W}x{H}", half=f"{w2}x{h2}", triangles=tris, nodes=nodes, calls_per_run=args.inner)
        rs, keep = sc.upload(device="cuda")
        att = torch.from_numpy(np.ascontiguousarray(abi.scene_triangle_attributes(sc)).view(np.uint8).copy()).to("cuda")
        nrm = torch.from_numpy(np.ascontiguousarray(abi.scene_triangle_normals(sc)).view(np.uint8).copy()).to("cuda")
        nbytes = abi.reflections_rt_scratch_bytes(rs.texture_count)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        outs = {k: ImageBuf(abi.FMT_RGBA8_UNORM, w2, h2, device="cuda") for k in ("unlit", 0, 1, 4)}
        depth, normal = frame.image("depth", 1, 1), frame.image("dn")
        params = abi.reflect_rt_params(setup.inv_view, *setup.fazz)
        blocks = {n: abi.reflect_lights(LIGHTS[:n], COLOURS[:n], AMBIENT if n else (1.0, 1.0, 1.0)) for n in (0, 1, 4)}

        def unlit():
            abi.reflections_rt(depth, normal, None, accel, att.data_ptr(), tris, rs.textures, rs.texture_count, params, outs["unlit"].desc(),
                               scratch.data_ptr(), nbytes, stream)

        def lit(n):
            return lambda: abi.reflections_rt_lit(depth, normal, None, accel, att.data_ptr(), tris, nrm.data_ptr(), tris, rs.textures, rs.texture_count, params,
                                                  blocks[n], outs[n].desc(), scratch.data_ptr(), nbytes, stream)

        cases = {"vkr_reflections_rt": unlit}
        cases.update({f"vkr_reflections_rt_lit, {n} lights": lit(n) for n in (0, 1, 4)})
        stats = compare(cases)
        base = stats["vkr_reflections_rt"]["median_ms"]
        for k, s in stats.items():
            row(measurement="(a) " + k, **common, **s, over_unlit=round(s["median_ms"] / base, 3))
        same = bool(np.array_equal(outs["unlit"].raw(0), outs[0].raw(0)))
        row(measurement="(a) no light and ambient 1 is the unlit image", scene=name, value=same)
        assert same, "the lit pass without lights differs from the unlit pass"
        # (b) the two device-side tables of the scene
        tri_out = torch.zeros((tris, 9), dtype=torch.float32, device="cuda")
        nrm_out = torch.zeros((tris, 12), dtype=torch.float32, device="cuda")
        sbytes = abi.scene_triangles_scratch_bytes(rs.draw_count)
        sscratch = torch.zeros(sbytes, dtype=torch.uint8, device="cuda")
        tables = {"vkr_scene_triangles": lambda: abi.check(lib.vkr_scene_triangles(C.byref(rs), tri_out.data_ptr(), tris, sscratch.data_ptr(), sbytes, stream), lib),
                  "vkr_scene_triangle_normals": lambda: abi.check(lib.vkr_scene_triangle_normals(C.byref(rs), nrm_out.data_ptr(), tris, sscratch.data_ptr(), sbytes, stream), lib)}
        for k, s in compare(tables).items():
            row(measurement="(b) " + k, **common, draws=int(rs.draw_count), **s)
        frame.close()
        accel.close()
        del keep
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/reflections_rt_lit_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
