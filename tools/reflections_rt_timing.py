#!/usr/bin/env python3
"""Times the closest-hit ray query (csrc/accel_closest.hip) and the ray-traced reflections (csrc/reflections_rt.hip) with HIP events.

    python tools/reflections_rt_timing.py [--out profiles/reflections_rt_timing.json] [--reps 20] [--inner 10] [--size 3840x2160]
                                          [--detail 64] [--build-variant]

On the procedural scene and on Suzanne (tests/golden/suzanne, stood over an untextured floor in front of the frame's camera), each
rasterised by the host frame at --size, whose half resolution is where the SSR images live:
  (a) vkr_accel_closest against vkr_accel_occluded on the frame's own reflection rays (one per half-resolution pixel that casts one,
      origins and unit mirror directions evaluated on the host from the frame's depth mip 1 and half-resolution normals, t in
      [0, zfar]): what the closest-hit walk costs over the any-hit walk; the tool checks that `index != miss` is the any-hit answer;
  (b) vkr_reflections_rt in both modes, called by hand on the frame's images, and the frame stages it replaces or complements:
      VKRH_STAGE_SSR_TRACE, VKRH_STAGE_SSR_RESOLVE (filter + blur), VKRH_STAGE_REFLECTIONS_RT in mode all (ReflectionsRT + blur)
      and in mode fill (trace + filter + ReflectionsRT + blur); a frame stage's time includes the recording of its tasks;
  (c) vkr_accel_closest against the same entry on the child-ordering walk (wave_closest_hit_ordered): csrc/accel_closest.hip built
      a second time by this tool with -DVKR_CLOSEST_WALK=wave_closest_hit_ordered under the entry name vkr_accel_closest_ordered
      into csrc/build/ (--build-variant builds it and exits: no GPU needed; without the library the candidate is left out and the
      rows say so).  Not an entry of the product.  The two walks must give the same bytes; the tool checks that;
  (d) the share of half-resolution pixels that fill mode traces (geometry whose screen-space ray is invalid).
A run is --inner calls between one pair of events; the candidates of one comparison take turns run by run; reported per call: the
median of --reps runs with min and max.  No threshold anywhere: the numbers go into DESIGN.md section 7.9."""
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
VARIANT = os.path.join(CSRC, "build", "libvkr_closest_ordered.so")
SUZANNE = os.path.join(ROOT, "tests", "golden", "suzanne", "Suzanne.gltf")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_variant():
    """csrc/accel_closest.hip on the child-ordering walk, with the flags of csrc/Makefile, linked against the product library"""
    os.makedirs(os.path.dirname(VARIANT), exist_ok=True)
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-DVKR_CONTRACT=2",
           "-fno-gpu-flush-denormals-to-zero", "-Wall", "-Wno-unused-function", "-DVKR_CLOSEST_WALK=wave_closest_hit_ordered",
           "-DVKR_CLOSEST_ENTRY=vkr_accel_closest_ordered", "-DVKR_CLOSEST_KERNEL=k_accel_closest_ordered", "-shared", "-o", VARIANT,
           os.path.join(CSRC, "accel_closest.hip"), "-L" + CSRC, "-lvkr_postfx", "-Wl,-rpath," + CSRC]
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


def suzanne_scene(scn, np):
    """Suzanne in front of the frame's camera over an untextured floor and before an untextured wall"""
    sc = scn.load_gltf(SUZANNE)
    place = np.array([[1, 0, 0, 0], [0, 1, 0, 1.3], [0, 0, 1, 3.0], [0, 0, 0, 1]], np.float32)
    moved = []
    for m, _ in sc.transforms:
        model = (place @ np.asarray(m, np.float32)).astype(np.float32)
        moved.append((model, np.linalg.inv(model.astype(np.float64)).T.astype(np.float32)))
    sc.transforms = moved
    quad = sc.add_mesh(np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], np.float32), np.array([[0, 1, 0]] * 4, np.float32),
                       np.array([[0, 0], [8, 0], [8, 8], [0, 8]], np.float32), np.array([0, 2, 1, 0, 3, 2], np.uint32))
    sc.add_draw(sc.add_transform(np.array([[14, 0, 0, 0], [0, 1, 0, 0], [0, 0, 14, 8], [0, 0, 0, 1]], dtype=np.float32)), quad)
    sc.add_draw(sc.add_transform(np.array([[12, 0, 0, 0], [0, 0, -7, 3.5], [0, 1, 0, 14], [0, 0, 0, 1]], dtype=np.float32)), quad)
    return sc


def reflection_rays(np, depth_words, normal_codes, setup, normal_offset):
    """the pass's rays (DESIGN_NUMERICS.md, Reflections, ray traced) in plain float32 numpy: -> (origins, directions, cast [h, w]).
    For timing: not the bit-exact restatement (that is tests/reflections_rt_reference.py)."""
    F = np.float32
    h, w = depth_words.shape
    gy, gx = np.mgrid[0:h, 0:w]
    ux, uy = ((gx + F(0.5)) / F(w)).astype(F), ((gy + F(0.5)) / F(h)).astype(F)
    d = ((depth_words & 0xFFFFFF).astype(np.float64) / 16777215.0).astype(F)
    fovy, aspect, n_, f_ = (F(v) for v in setup.fazz)
    tg = F(np.tan(float(fovy) / 2.0))
    with np.errstate(all="ignore"):
        z = (n_ * f_) / (d * (f_ - n_) - f_)
        vx, vy = -(F(2) * ux - F(1)) * (z * aspect * tg), -(F(2) * uy - F(1)) * (z * tg)
        M = np.asarray(setup.inv_view, F)
        world = np.stack([M[r, 0] * vx + M[r, 1] * vy + M[r, 2] * z + M[r, 3] for r in range(3)], -1).astype(F)
        e = (normal_codes.astype(np.float64) / 65535.0).astype(F) * F(2) - F(1)
        nz = F(1) - np.abs(e[..., 0]) - np.abs(e[..., 1])
        sgn = lambda k: np.where(k >= 0, F(1), F(-1)).astype(F)  # noqa: E731
        nx = np.where(nz < 0, (F(1) - np.abs(e[..., 1])) * sgn(e[..., 0]), e[..., 0])
        ny = np.where(nz < 0, (F(1) - np.abs(e[..., 0])) * sgn(e[..., 1]), e[..., 1])
        n = np.stack([nx, ny, nz], -1).astype(F)
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        view = world - M[:3, 3]
        r = view - F(2) * (n * view).sum(-1, keepdims=True) * n
        r /= np.linalg.norm(r, axis=-1, keepdims=True)
        cast = (d < F(1)) & ((n * r).sum(-1) > 0)
    origin = (world + F(normal_offset) * n).astype(F)
    return np.ascontiguousarray(origin[cast]), np.ascontiguousarray(r[cast].astype(F)), cast


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reflections_rt_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--detail", type=int, default=64)
    ap.add_argument("--build-variant", action="store_true", help="build the child-ordering variant of vkr_accel_closest and exit (no GPU needed)")
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
        raise SystemExit("reflections_rt_timing: needs a GPU")
    lib = abi.product()
    stream = torch.cuda.current_stream().cuda_stream
    ordered = None
    if os.path.exists(VARIANT):
        ordered = C.CDLL(VARIANT).vkr_accel_closest_ordered
        ordered.argtypes = lib.vkr_accel_closest.argtypes
        ordered.restype = C.c_int
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
        frame.pin_randoms(0.25, 3, 5)
        frame.run(host.STAGE_SSR_TRACE | host.STAGE_SSR_RESOLVE)
        torch.cuda.synchronize()
        common = dict(scene=name, size=f"{W}x{H}", half=f"{w2}x{h2}", triangles=tris, nodes=nodes, calls_per_run=args.inner)
        depth_words = frame.download("depth").raw(1)[..., 0].astype(np.uint32)
        normal_codes = frame.download("dn").raw(0)
        rays_w = frame.download("rays").raw(0)[..., 3]
        org, dirs, cast = reflection_rays(np, depth_words, normal_codes, setup, abi.SHADOW_RT_NORMAL_OFFSET)
        geometry = (depth_words & 0xFFFFFF) != 0xFFFFFF
        fill_traced = cast & (rays_w == 65535)
        # (d)
        row(measurement="(d) share of half-resolution pixels that fill mode traces", **common, pixels=int(cast.size), geometry=int(geometry.sum()),
            cast_in_mode_all=int(cast.sum()), invalid_screen_space_rays=int((geometry & (rays_w == 65535)).sum()), traced_in_mode_fill=int(fill_traced.sum()),
            share_of_all_pixels=round(float(fill_traced.mean()), 5), share_of_geometry=round(float(fill_traced.sum() / max(1, geometry.sum())), 5))
        # (a) and (c): the ray-level entries on the frame's rays
        n = len(org)
        to, td = torch.from_numpy(org).to("cuda"), torch.from_numpy(dirs).to("cuda")
        zfar = float(setup.fazz[3])
        hits = {k: torch.zeros((n, 4), dtype=torch.int32, device="cuda") for k in ("closest", "ordered")}
        occ = torch.zeros(n, dtype=torch.int32, device="cuda")
        cases = {"vkr_accel_occluded (any hit)": lambda: accel.occluded(to, td, 0.0, zfar, occ, stream),
                 "vkr_accel_closest": lambda: accel.closest(to, td, 0.0, zfar, hits["closest"], stream)}
        if ordered is not None:
            cases["vkr_accel_closest on the child-ordering walk"] = \
                lambda: abi.check(ordered(accel.handle, to.data_ptr(), td.data_ptr(), 0.0, zfar, n, hits["ordered"].data_ptr(), stream), lib)
        stats = compare(cases)
        got = hits["closest"].cpu().numpy().view(np.uint32)
        hit = got[:, 3] != 0xFFFFFFFF
        assert np.array_equal(hit, occ.cpu().numpy().astype(bool)), "closest and any hit disagree on whether a ray hits"
        for k, s in stats.items():
            row(measurement=("(c) " if "ordering" in k else "(a) ") + k, **common, rays=n, share_hit=round(float(hit.mean()), 4), **s)
        same = bool(np.array_equal(got, hits["ordered"].cpu().numpy().view(np.uint32))) if ordered is not None else None
        row(measurement="(c) the two walks give the same bytes", scene=name, value=same if same is not None else "child-ordering variant not built")
        if ordered is not None:
            assert same, "the two exact walks disagree"
        # (b) the pass by hand, both modes, on the frame's images
        rs, keep = sc.upload(device="cuda")
        att = torch.from_numpy(np.ascontiguousarray(abi.scene_triangle_attributes(sc)).view(np.uint8).copy()).to("cuda")
        nbytes = abi.reflections_rt_scratch_bytes(rs.texture_count)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        outs = {k: ImageBuf(abi.FMT_RGBA8_UNORM, w2, h2, device="cuda") for k in ("all", "fill")}
        images = dict(depth=frame.image("depth", 1, 1), normal=frame.image("dn"), rays=frame.image("rays"))

        def by_hand(fill):
            p = abi.reflect_rt_params(setup.inv_view, *setup.fazz, fill_misses=fill)
            abi.reflections_rt(images["depth"], images["normal"], images["rays"] if fill else None, accel, att.data_ptr(), tris, rs.textures,
                               rs.texture_count, p, outs["fill" if fill else "all"].desc(), scratch.data_ptr(), nbytes, stream)

        for k, s in compare({"vkr_reflections_rt, all": lambda: by_hand(False), "vkr_reflections_rt, fill misses": lambda: by_hand(True)}).items():
            row(measurement="(b) " + k, **common, **s)
        # (b) the frame stages
        def stage(mask, fill=None):
            if fill is not None:
                frame.set_reflection_rays(fill_misses=fill)
            return lambda: frame.run(mask)

        stages = {"VKRH_STAGE_SSR_TRACE": stage(host.STAGE_SSR_TRACE), "VKRH_STAGE_SSR_RESOLVE (filter + blur)": stage(host.STAGE_SSR_RESOLVE)}
        for k, s in compare(stages).items():
            row(measurement="(b) frame: " + k, **common, **s)
        for label, fill in (("VKRH_STAGE_REFLECTIONS_RT, all (ReflectionsRT + blur)", False), ("VKRH_STAGE_REFLECTIONS_RT, fill (trace + filter + ReflectionsRT + blur)", True)):
            for k, s in compare({label: stage(host.STAGE_REFLECTIONS_RT, fill)}).items():
                row(measurement="(b) frame: " + k, **common, **s)
        frame.close()
        accel.close()
        del keep
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/reflections_rt_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
