#!/usr/bin/env python3
"""Times the four entries that see alpha cutouts (csrc/accel_cutout.hip) beside their opaque siblings, with HIP events.

    python tools/ray_cutout_timing.py [--out profiles/ray_cutout_timing.json] [--reps 20] [--inner 10] [--size 3840x2160]

The method of tools/reflections_rt_timing.py: a run is --inner calls between one pair of events, the candidates of one comparison
take turns run by run, reported per call: the median of --reps runs with min and max.  Scenes, each rasterised by the host frame at
--size: the procedural scene WITH its fence (cutout=True) at detail 16 and 64, and Suzanne over an untextured floor and wall, whose
textures have no alpha-0 texel: abi.scene_opaque_texture_mask masks every one of them, so that row is the price of the filter when it
never fires.  Per scene:
  vkr_accel_occluded / _cutout and vkr_accel_closest / _cutout on the frame's own reflection rays (tools/reflections_rt_timing.py
  reflection_rays, t in [0, zfar]);
  vkr_shadow_mask_rt / _cutout on the frame's full-resolution depth and normal, one point light behind the fence;
  vkr_reflections_rt / _cutout, mode all, on the frame's half-resolution images.
The cutout entries get the scene's mask of textures without holes and alpha_lod 0.  The tool checks what must hold whatever the time:
the cutout any hit is `closest_cutout.index != miss`, a masked-opaque scene gives the opaque bytes, and every mask channel is at least
the opaque one.  No threshold anywhere: the numbers go into DESIGN.md section 7.11."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from reflections_rt_timing import _git_head, _stats, _timed, reflection_rays, suzanne_scene  # noqa: E402

LIGHT = (0.5, 2.5, 8.0, 1.0)  # behind the fence as the camera sees it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_cutout_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--git-head", default=None, help="the head to record when the tree that runs is not a git checkout")
    args = ap.parse_args()
    import numpy as np
    import torch

    import vk_renderer_amd  # noqa: F401
    from vk_renderer_amd import abi, host
    from vk_renderer_amd import scene as scn
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.images import ImageBuf

    if not torch.cuda.is_available():
        raise SystemExit("ray_cutout_timing: needs a GPU")
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def row(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    def compare(cases):
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
    scenes = (("procedural, fence, detail 16", scn.procedural_scene(detail=16, cutout=True)),
              ("procedural, fence, detail 64", scn.procedural_scene(detail=64, cutout=True)),
              ("suzanne (every texture masked opaque)", suzanne_scene(scn, np)))
    for name, sc in scenes:
        accel = abi.Accel.from_scene(sc)
        nodes, tris = accel.info()
        setup = FrameSetup(W, H)
        frame = host.HostFrame(setup, device="cuda")
        frame.load_scene(sc)
        frame.run(host.STAGE_LUT | host.STAGE_BRDF_LUT | host.STAGE_PREV_DEPTH)
        frame.run(host.STAGE_RASTER | host.STAGE_DOWNSAMPLE)
        torch.cuda.synchronize()
        mask = abi.scene_opaque_texture_mask(sc)
        all_masked = mask == (1 << len(sc.textures)) - 1
        cut = abi.ray_cutout(0, mask)
        common = dict(scene=name, size=f"{W}x{H}", triangles=tris, nodes=nodes, textures=len(sc.textures), opaque_texture_mask=mask,
                      calls_per_run=args.inner)
        rs, keep = sc.upload(device="cuda")
        att = torch.from_numpy(np.ascontiguousarray(abi.scene_triangle_attributes(sc)).view(np.uint8).copy()).to("cuda")
        nbytes = abi.accel_cutout_scratch_bytes(rs.texture_count)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        table = (att.data_ptr(), tris, rs.textures, rs.texture_count)
        # the ray-level entries on the frame's reflection rays
        org, dirs, _ = reflection_rays(np, frame.download("depth").raw(1)[..., 0].astype(np.uint32), frame.download("dn").raw(0), setup,
                                       abi.SHADOW_RT_NORMAL_OFFSET)
        n = len(org)
        to, td = torch.from_numpy(org).to("cuda"), torch.from_numpy(dirs).to("cuda")
        zfar = float(setup.fazz[3])
        hits = {k: torch.zeros((n, 4), dtype=torch.int32, device="cuda") for k in ("opaque", "cutout")}
        occ = {k: torch.zeros(n, dtype=torch.int32, device="cuda") for k in ("opaque", "cutout")}
        stats = compare({
            "vkr_accel_occluded": lambda: accel.occluded(to, td, 0.0, zfar, occ["opaque"], stream),
            "vkr_accel_occluded_cutout": lambda: abi.accel_occluded_cutout(accel, to, td, 0.0, zfar, *table, cut, occ["cutout"], scratch.data_ptr(), nbytes, stream),
            "vkr_accel_closest": lambda: accel.closest(to, td, 0.0, zfar, hits["opaque"], stream),
            "vkr_accel_closest_cutout": lambda: abi.accel_closest_cutout(accel, to, td, 0.0, zfar, *table, cut, hits["cutout"], scratch.data_ptr(), nbytes, stream)})
        got = {k: v.cpu().numpy().view(np.uint32) for k, v in hits.items()}
        any_hit = {k: v.cpu().numpy().astype(bool) for k, v in occ.items()}
        assert np.array_equal(got["cutout"][:, 3] != 0xFFFFFFFF, any_hit["cutout"]), "closest_cutout and occluded_cutout disagree on whether a ray hits"
        if all_masked:
            assert np.array_equal(got["cutout"], got["opaque"]) and np.array_equal(any_hit["cutout"], any_hit["opaque"]), "masked opaque, other bytes"
        changed = int((got["cutout"][:, 3] != got["opaque"][:, 3]).sum())
        for k, s in stats.items():
            row(measurement=k, **common, rays=n, rays_whose_closest_hit_changes=changed, **s)
        # the shadow mask at full resolution
        outs = {k: ImageBuf(abi.FMT_RGBA8_UNORM, W, H, device="cuda") for k in ("opaque", "cutout")}
        sp = abi.shadow_rt_params(setup.inv_view, [LIGHT], *setup.fazz)
        depth0, normal0 = frame.image("depth", 0, 1), frame.image("normal")
        stats = compare({
            "vkr_shadow_mask_rt": lambda: abi.shadow_mask_rt(depth0, normal0, accel, sp, outs["opaque"].desc(), stream),
            "vkr_shadow_mask_rt_cutout": lambda: abi.shadow_mask_rt_cutout(depth0, normal0, accel, *table, sp, cut, outs["cutout"].desc(), scratch.data_ptr(),
                                                                           nbytes, stream)})
        a, b = outs["opaque"].raw(0)[..., 0], outs["cutout"].raw(0)[..., 0]
        assert (b >= a).all(), "a mask channel is darker with cutouts"
        if all_masked:
            assert np.array_equal(a, b)
        for k, s in stats.items():
            row(measurement=k, **common, pixels=W * H, pixels_lit_through_holes=int(((b == 255) & (a == 0)).sum()), **s)
        # the reflections at half resolution, mode all
        routs = {k: ImageBuf(abi.FMT_RGBA8_UNORM, w2, h2, device="cuda") for k in ("opaque", "cutout")}
        rp = abi.reflect_rt_params(setup.inv_view, *setup.fazz)
        depth1, dn = frame.image("depth", 1, 1), frame.image("dn")
        stats = compare({
            "vkr_reflections_rt, all": lambda: abi.reflections_rt(depth1, dn, None, accel, *table, rp, routs["opaque"].desc(), scratch.data_ptr(), nbytes, stream),
            "vkr_reflections_rt_cutout, all": lambda: abi.reflections_rt_cutout(depth1, dn, None, accel, *table, rp, cut, routs["cutout"].desc(),
                                                                                scratch.data_ptr(), nbytes, stream)})
        a, b = routs["opaque"].raw(0), routs["cutout"].raw(0)
        if all_masked:
            assert np.array_equal(a, b)
        for k, s in stats.items():
            row(measurement=k, **common, pixels=w2 * h2, texels_that_change=int((a != b).any(axis=-1).sum()), **s)
        frame.close()
        accel.close()
        del keep
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/ray_cutout_timing.py", "device": torch.cuda.get_device_name(0), "git_head": args.git_head or _git_head(), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
