"""Deferred shading in the multi-GPU tiled frame (host/frame.cpp: TiledFrame::shaded_tail, vkrh_tiled_set_shading) on ONE GPU.

The expected image is the plain one-GPU frame in the reference's order (main.cpp:384-391): GTAO -> shading_pass.draw ->
taa_pass.run(color_out_tex), i.e. STAGE_BRDF_LUT once and STAGE_CHAIN | STAGE_SHADING per frame.  A shaded tiled frame must
reproduce it on every tile interior with 0 differing texels — the images of tests/test_tiled_native_gpu.py and color_out.

  * lockstep: in-process C++ ranks without a communicator, the wire played by copies (tiling.native_lockstep_frame, six phases)
  * real processes over tests/stub_rccl: the native step, one-frame order and two frames in flight
  * an emulated wire: the native step continues a lockstep run"""
import json
import os
import textwrap

import pytest

from test_native_wire_gpu import _launch, _stub, _workers_stderr
from test_tiled_native_gpu import OUTPUTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHADED_OUTPUTS = OUTPUTS + (("color_out", 0),)


def _plain(W, H, frames, device, shaded=True, names=SHADED_OUTPUTS + (("albedo", 0),), pin=False):
    from vk_renderer_amd import host
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.tiling import TiledFrame

    plain = TiledFrame(FrameSetup(W, H), 0, 1, 1, 1, device)
    plain.prepare()
    if shaded:
        plain.frame.run(host.STAGE_BRDF_LUT)
        plain.stage_plan = [host.STAGE_CHAIN | host.STAGE_SHADING]
    for _ in range(frames):
        if pin:
            plain.frame.pin_randoms(0.0, 0, 0)
        plain.step()
    plain.backend.sync()
    want = {n: plain.frame.download(n) for n, _ in names}
    plain.frame.close()
    return want


def _rows_differ(t, want, name, dv, lo, hi, want_is_window=False):
    """differing texels of image `name` on frame rows [lo, hi) (in texels of that image); `want` holds whole-frame images, or
    with want_is_window images of the same window as the rank's"""
    got = t.frame.download(name)
    ox, oy = got.origin
    a = got.raw(0)[lo - oy:hi - oy]
    w = want[name]
    b = w.raw(0)[lo - w.origin[1]:hi - w.origin[1]] if want_is_window else w.raw(0)[lo:hi]
    if name == "depth":
        a, b = a & 0xFFFFFF, b & 0xFFFFFF
    return int((a != b).any(axis=-1).sum())


def _interiors_differ(t, want, names=SHADED_OUTPUTS):
    bad = 0
    _, y0, _, th = t.tile
    for name, dv in names:
        n = _rows_differ(t, want, name, dv, y0 >> dv, (y0 + th) >> dv)
        print(f"[shaded] rank {t.rank} {name}: {n} differing texels")
        bad += n
    return bad


def _assert_plain_is_shaded(want):
    """not vacuous: the image the TAA resolves is not the albedo any more"""
    c, a = want["color_out"].raw(0), want["albedo"].raw(0)
    differ = int((c[..., :3] != a[..., :3]).any(axis=-1).sum())
    print(f"[shaded] plain frame: color_out differs from albedo on {differ} of {c.shape[0] * c.shape[1]} texels")
    assert 2 * differ > c.shape[0] * c.shape[1], "the plain frame's color_out is mostly its albedo: nothing was shaded"


CASES = [(2, 160, 4, 0, False, False), (3, 136, 3, 0, False, False), (4, 160, 4, 0, False, False),   # world 2, 3, 4
         (4, 160, 4, 1, False, False), (4, 160, 4, 2, False, False),                                  # the gather modes
         (4, 160, 4, 0, True, False), (3, 136, 3, 0, True, False),                                    # local rows first
         (4, 160, 4, 0, False, True), (3, 136, 3, 0, True, True), (2, 160, 4, 1, False, True)]       # every pass on its whole window


@pytest.mark.parametrize("world,tile_h,gather,mode,local_first,whole", CASES)
def test_shaded_ranks_in_lockstep_match_the_plain_shaded_frame(world, tile_h, gather, mode, local_first, whole, monkeypatch):
    import torch

    monkeypatch.setenv("VKR_TILED_WHOLE_WINDOW", "1" if whole else "0")
    monkeypatch.setenv("VKR_TILED_GATHER_MODE", str(mode))
    monkeypatch.setenv("VKR_TILED_LOCAL_FIRST", "1" if local_first else "0")

    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.tiling import TiledFrame, native_lockstep_frame

    W, H = 256, tile_h * world
    device = torch.device("cuda", 0)
    want = _plain(W, H, 3, device)
    _assert_plain_is_shaded(want)
    ranks = [TiledFrame(FrameSetup(W, H), r, world, 1, world, device, native=True, comm=None, shading=True) for r in range(world)]
    for t in ranks:
        assert t.native and t.gather_mips == gather and not t.frame.tiled_shading()
        t.prepare()
        assert t.frame.tiled_shading() and t.frame.tiled_local_first() == (local_first and mode == 0)
    for _ in range(3):
        native_lockstep_frame(ranks)
    for t in ranks:
        t.flush()
    torch.cuda.synchronize()
    bad = sum(_interiors_differ(t, want) for t in ranks)
    if mode != 1:
        assert all(t.frame.tiled_hit_errors() == 0 for t in ranks)
    # the frame really ended with the shading and the TAA, in one run
    assert ranks[0].frame.last_tasks()[-2:] == ["DeferedShading", "TAA"], ranks[0].frame.last_tasks()
    for t in ranks:
        t.frame.close()
    assert bad == 0


def test_shaded_taa_history_is_not_the_unshaded_one():
    import torch

    W, H = 256, 320
    device = torch.device("cuda", 0)
    shaded = _plain(W, H, 3, device)
    unshaded = _plain(W, H, 3, device, shaded=False, names=(("taa_hist", 0),))
    a, b = shaded["taa_hist"].raw(0), unshaded["taa_hist"].raw(0)
    differ = int((a != b).any(axis=-1).sum())
    print(f"[shaded] taa_hist: shaded and unshaded plain frames differ on {differ} of {W * H} texels")
    assert 2 * differ > W * H


def test_shaded_strips_of_different_heights():
    import torch

    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.tiling import TiledFrame, native_lockstep_frame

    bounds = [0, 96, 168, 304, 480]  # 168 = 8 * 21: depth mips 1..3 travel; half-res strip starts of both parities (48, 84, 152)
    world, W, H = len(bounds) - 1, 256, bounds[-1]
    device = torch.device("cuda", 0)
    want = _plain(W, H, 3, device)
    ranks = [TiledFrame(FrameSetup(W, H), r, world, 1, world, device, native=True, comm=None, row_bounds=bounds, shading=True) for r in range(world)]
    for r, t in enumerate(ranks):
        assert t.gather_mips == 3 and t.tile == (0, bounds[r], W, bounds[r + 1] - bounds[r])
        t.prepare()
    for _ in range(3):
        native_lockstep_frame(ranks)
    for t in ranks:
        t.flush()
    torch.cuda.synchronize()
    bad = sum(_interiors_differ(t, want) for t in ranks)
    for t in ranks:
        t.frame.close()
    assert bad == 0


def test_one_forced_rank_shaded():
    """one rank on the multi-GPU path (force_tiled): vkrh_tiled_step plays the six phases itself, the gathers are local copies"""
    import torch

    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.tiling import TiledFrame

    W, H = 512, 288
    device = torch.device("cuda", 0)
    want = _plain(W, H, 3, device)
    t = TiledFrame(FrameSetup(W, H), 0, 1, 1, 1, device, force_tiled=True, native=True, comm=None, shading=True)
    assert t.tiled and t.native
    t.prepare()
    assert t.frame.tiled_shading()
    for _ in range(3):
        t.step()
    t.flush()
    torch.cuda.synchronize()
    bad = _interiors_differ(t, want)
    t.frame.close()
    assert bad == 0


def test_python_wrapper_on_one_gpu_is_the_stage_plan():
    """TiledFrame(shading=True) on one untiled rank: the existing stage plan, the BRDF LUT run by prepare()"""
    import torch

    from vk_renderer_amd import host
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.tiling import TiledFrame

    W, H = 256, 320
    device = torch.device("cuda", 0)
    want = _plain(W, H, 2, device)
    t = TiledFrame(FrameSetup(W, H), 0, 1, 1, 1, device, shading=True)
    assert not t.tiled and t.stage_plan == [host.STAGE_CHAIN | host.STAGE_SHADING]
    t.prepare()
    for _ in range(2):
        t.step()
    t.backend.sync()
    bad = _interiors_differ(t, want)
    t.frame.close()
    assert bad == 0


def test_a_frame_whose_neighbour_rows_did_not_arrive_differs_beside_the_boundary():
    """The AO and SSR rows a strip's first and last rows are shaded from are the neighbours' CURRENT ones, moved in the same
    frame.  A harness that does not move them for one frame leaves last frame's rows in the receive buffers: color_out must then
    differ from the plain frame in the rows beside a strip boundary — and nowhere else in the strip.  Which rows those are
    follows from the footprint arithmetic of tests/test_tiled_shading.py (an even row 2k reads half-res rows k - 1 .. k + 1, an
    odd row 2k + 1 reads k .. k + 2): the even row y0 reads y0 / 2 - 1; the odd row y1 - 3 reads y1 / 2 through the lower tap
    of its (0|1, 1) picks, and y1 - 2 and y1 - 1 read y1 / 2 and y1 / 2 + 1.  One row at a strip's top, three at its bottom."""
    import torch

    from test_tiled_shading import _half_res_rows
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.tiling import TiledFrame, native_lockstep_frame

    world, W, th = 3, 256, 160
    H = th * world
    for y0 in range(th, H, th):  # every inner boundary: the strip rows whose footprint leaves the strip's own half-res rows
        above = [y for y in range(y0 - th, y0) if max(_half_res_rows(y, H)) >= y0 // 2]
        below = [y for y in range(y0, y0 + th) if min(_half_res_rows(y, H)) < y0 // 2]
        assert above == [y0 - 3, y0 - 2, y0 - 1] and below == [y0]
    device = torch.device("cuda", 0)
    want = _plain(W, H, 3, device)
    ranks = [TiledFrame(FrameSetup(W, H), r, world, 1, world, device, native=True, comm=None, shading=True) for r in range(world)]
    for t in ranks:
        t.prepare()
    native_lockstep_frame(ranks)
    native_lockstep_frame(ranks)
    native_lockstep_frame(ranks, skip_halos=(1, 2))
    for t in ranks:
        t.flush()
    torch.cuda.synchronize()
    beside = inside = 0
    for t in ranks:
        y0, y1 = t.tile[1], t.tile[1] + th
        top, bottom = (1 if t.rank > 0 else 0), (3 if t.rank + 1 < world else 0)
        got = t.frame.download("color_out")
        per_row = (got.raw(0)[y0 - got.origin[1]:y1 - got.origin[1]] != want["color_out"].raw(0)[y0:y1]).any(axis=-1).sum(axis=1).tolist()
        print(f"[shaded] rank {t.rank}: differing color_out texels by strip row {dict((y, n) for y, n in enumerate(per_row) if n)}")
        beside += sum(per_row[:top]) + sum(per_row[th - bottom:])
        inside += sum(per_row[top:th - bottom])
    for t in ranks:
        t.frame.close()
    print(f"[shaded] halo moves skipped for a frame: {beside} color_out texels differ beside the boundaries, {inside} elsewhere")
    assert beside >= 1
    assert inside == 0, "rows that read no neighbour row must not notice"


def test_gates():
    import torch

    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.tiling import TiledFrame, native_lockstep_frame

    world, W, th = 2, 256, 160
    H = th * world
    device = torch.device("cuda", 0)
    ranks = [TiledFrame(FrameSetup(W, H), r, world, 1, world, device, native=True, comm=None) for r in range(world)]
    for t in ranks:
        t.prepare()
        # shading off: phases are 0..4 (asked before anything is in flight: the refused call records nothing)
        with pytest.raises(RuntimeError, match=r"phases are 0\.\.4"):
            t.frame.tiled_phase(5)
        # the shading pass samples the BRDF LUT: it must have run
        with pytest.raises(RuntimeError, match="VKRH_STAGE_BRDF_LUT"):
            t.frame.tiled_set_shading(True)
        assert not t.frame.tiled_shading()
    from vk_renderer_amd import host

    native_lockstep_frame(ranks)  # leaves the three refreshes in flight
    for t in ranks:
        t.frame.run(host.STAGE_BRDF_LUT)
        with pytest.raises(RuntimeError, match="in flight"):
            t.frame.tiled_set_shading(True)
        assert not t.frame.tiled_shading()
    for t in ranks:
        t.flush()
        t.frame.tiled_set_shading(True)   # right after the flush: allowed
        assert t.frame.tiled_shading()
    native_lockstep_frame(ranks)          # six phases now; leaves the TAA refresh in flight
    for t in ranks:
        with pytest.raises(RuntimeError, match="in flight"):
            t.frame.tiled_set_shading(False)
        with pytest.raises(RuntimeError, match=r"phases are 0\.\.5"):
            t.frame.tiled_phase(6)
        t.flush()
        t.frame.tiled_set_shading(False)
        assert not t.frame.tiled_shading()
    native_lockstep_frame(ranks)          # five phases again
    for t in ranks:
        t.flush()
    torch.cuda.synchronize()
    for t in ranks:
        t.frame.close()
    # a halo below the reach of the pass (2 half-res rows): refused, with the bound in the message
    small = TiledFrame(FrameSetup(W, H), 0, world, 1, world, device, native=True, comm=None, halo=2, shading=True)
    assert small.gather_mips == 1
    with pytest.raises(RuntimeError, match="halo 2"):
        small.prepare()
    torch.cuda.synchronize()
    small.frame.close()


# ---- real processes over tests/stub_rccl -------------------------------------------------------------------------------------
WORKER = textwrap.dedent("""
    import json, os, sys
    sys.path.insert(0, %r)
    import numpy as np, torch, torch.distributed as dist
    import vk_renderer_amd
    from vk_renderer_amd import abi, host
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.tiling import TiledFrame
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    dist.init_process_group('gloo')
    def share(ident):
        box = [ident]; dist.broadcast_object_list(box, src=0); return box[0]
    def agree(ok):
        t = torch.tensor([1 if ok else 0], dtype=torch.int32); dist.all_reduce(t, op=dist.ReduceOp.MIN); return int(t.item()) == 1
    comm = abi.Comm(rank, world, share, agree)
    assert comm.self_check(device, agree), comm.self_check_error
    bounds = json.loads(os.environ['VKR_BOUNDS'])
    moving = os.environ['VKR_MOVING'] == '1'
    FRAMES = int(os.environ['VKR_FRAMES'])
    W, H = 256, bounds[-1]

    def camera(k):  # frame k looks from eye_k; its previous frame is camera k - 1
        return FrameSetup(W, H, eye=(0.03 * k, 1.0, -1.0 + 0.02 * k), yaw=90.0 + 0.3 * k, prev_delta=(-0.03, 0.0, -0.02), prev_yaw_delta=-0.3)

    def run(t, frames):
        for k in range(frames):
            if moving:
                s = camera(k)
                t.frame.set_camera(s.view, s.prev_view, s.proj, s.fazz)
                t.frame.run(host.STAGE_GBUFFER | host.STAGE_PREV_DEPTH)
            t.step()
        t.flush()
        t.backend.sync()

    equal = all(bounds[r + 1] - bounds[r] == bounds[1] for r in range(world))
    t = TiledFrame(FrameSetup(W, H), rank, world, 1, world, device, native=True, comm=comm, row_bounds=None if equal else bounds, shading=True)
    assert t.native and t.frame.tiled_handle
    t.prepare()
    assert t.frame.tiled_shading() and t.frame.tiled_pipelined() == (os.environ['VKR_TILED_PIPELINE'] == '1')
    run(t, FRAMES)
    # the plain shaded frame: main.cpp:384-391
    plain = TiledFrame(FrameSetup(W, H), 0, 1, 1, 1, device)
    plain.prepare()
    plain.frame.run(host.STAGE_BRDF_LUT)
    plain.stage_plan = [host.STAGE_CHAIN | host.STAGE_SHADING]
    run(plain, FRAMES)
    x0, y0, tw, th = t.tile
    bad = 0
    for name, dv in (('rays', 1), ('raw', 1), ('reflections', 1), ('filtered', 1), ('blurred_hist', 1), ('acc_hist', 1), ('taa_hist', 0), ('dn', 1), ('dv', 1),
                     ('color_out', 0)):
        got, want = t.frame.download(name), plain.frame.download(name)
        ox, oy = got.origin
        a = got.raw(0)[(y0 >> dv) - oy:(y0 >> dv) - oy + (th >> dv)]
        b = want.raw(0)[(y0 >> dv):(y0 >> dv) + (th >> dv)]
        d = (a != b).any(axis=-1)
        n = int(d.sum())
        if n:
            ys = np.flatnonzero(d.any(axis=1))
            print(f'rank {rank} {name}: {n} differing texels, tile rows {ys[0]}..{ys[-1]} of {th >> dv}')
        bad += n
    c, alb = plain.frame.download('color_out').raw(0), plain.frame.download('albedo').raw(0)
    if 2 * int((c[..., :3] != alb[..., :3]).any(axis=-1).sum()) <= W * H:
        print(f'rank {rank}: the plain frame was not shaded'); bad += 1
    errors = t.frame.tiled_hit_errors()
    if errors:
        print(f'rank {rank}: {errors} hit requests named texels their owner does not hold'); bad += 1
    if t.frame.last_tasks()[-2:] != ['DeferedShading', 'TAA']:
        print(f'rank {rank}: the frame did not end with shading + TAA: {t.frame.last_tasks()}'); bad += 1
    print(f'[shaded wire] rank {rank}: {bad} problems, hit rounds {t.frame.tiled_hit_rounds()}')
    dist.barrier()
    torch.cuda.synchronize()
    t.frame.close(); plain.frame.close()
    comm.close()
    dist.destroy_process_group()
    sys.exit(1 if bad else 0)
""") % ROOT


@pytest.mark.parametrize("bounds,moving,frames,pipelined", [
    ([0, 160, 320], False, 3, False),          # 2 ranks, one-frame order
    ([0, 160, 320], True, 4, False),           # ... the camera moving every frame
    ([0, 160, 320], False, 4, True),           # 2 ranks, two frames in flight (static: the next frame's G-buffer is resident)
    ([0, 96, 168, 304, 480], False, 3, False),  # 4 ranks, strips of different heights
])
def test_shaded_native_frame_between_real_processes(bounds, moving, frames, pipelined, tmp_path):
    world = len(bounds) - 1
    assert world <= 4
    script = tmp_path / "shaded_worker.py"
    script.write_text(WORKER)
    log = tmp_path / "wire.log"
    env = dict(os.environ, VKR_RCCL_LIBRARY=_stub(), VKR_STUB_RCCL_LOG=str(log), VKR_STUB_RCCL_TIMEOUT_S="120", VKR_BOUNDS=json.dumps(bounds),
               VKR_MOVING="1" if moving else "0", VKR_FRAMES=str(frames), HSA_ENABLE_IPC_MODE_LEGACY="0",
               VKR_TILED_PIPELINE="1" if pipelined else "0", VKR_TILED_LOCAL_FIRST="0")
    for name in ("VKR_GATHER_V_BROADCAST", "VKR_HIT_CAP_PERCENT", "VKR_TILED_GATHER_MODE", "VKR_TILED_ALBEDO_GATHER", "VKR_TILED_WHOLE_WINDOW"):
        env.pop(name, None)
    rc, out, err = _launch(world, [str(script)], env, timeout=420)
    print(out[-3000:])
    assert rc == 0, out[-3000:] + "\n--- the ranks' own stderr ---\n" + _workers_stderr(err)


# ---- the native step on an emulated wire -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
def test_shaded_native_step_on_an_emulated_wire_equals_the_lockstep_result(pipelined, monkeypatch):
    """The pattern of test_native_frame_on_an_emulated_wire_receives_what_its_peers_would_send, shaded: three ranks in lockstep
    (randoms pinned), then every rank NATIVELY on an emulated communicator that holds the exchange stream and moves nothing.
      * what has no history (rays, raw, reflections, filtered) is the plain frame's on every interior, bit for bit;
      * color_out and the TAA history equal those of ranks that simply went on in lockstep for the same number of frames — on
        the strip rows that the stale receive buffers cannot reach: an emulated exchange delivers the rows of the LAST lockstep
        frame, and the histories carry them inwards by at most the blur's 11 half-res texels a frame; 3 frames x 22 rows and
        the 2 half-res rows of the shading footprint stay within 72 rows of an inner strip boundary."""
    import torch

    monkeypatch.setenv("VKR_TILED_PIPELINE", "1" if pipelined else "0")
    monkeypatch.setenv("VKR_TILED_LOCAL_FIRST", "0")
    monkeypatch.delenv("VKR_TILED_GATHER_MODE", raising=False)
    monkeypatch.delenv("VKR_TILED_WHOLE_WINDOW", raising=False)

    from vk_renderer_amd import abi
    from vk_renderer_amd.camera import FrameSetup
    from vk_renderer_amd.tiling import TiledFrame, native_lockstep_frame

    world, W, th, margin = 3, 256, 192, 72
    H = th * world
    device = torch.device("cuda", 0)
    names = (("rays", 1), ("raw", 1), ("reflections", 1), ("filtered", 1))
    want = _plain(W, H, 3, device, names=names + (("color_out", 0), ("albedo", 0)), pin=True)
    _assert_plain_is_shaded(want)

    def lockstep_ranks(frames, last_in_capacities):
        ranks = [TiledFrame(FrameSetup(W, H), r, world, 1, world, device, native=True, comm=None, shading=True) for r in range(world)]
        for t in ranks:
            t.prepare()
        for k in range(frames):
            for t in ranks:
                t.frame.pin_randoms(0.0, 0, 0)
            native_lockstep_frame(ranks, hit_in_capacities=last_in_capacities and k == frames - 1)
        return ranks

    # the continuation in lockstep: six frames
    ref = lockstep_ranks(6, False)
    for t in ref:
        t.flush()
    torch.cuda.synchronize()
    held = []
    for t in ref:
        held.append({n: t.frame.download(n) for n in ("color_out", "taa_hist")})
        t.frame.close()

    ranks = lockstep_ranks(3, True)
    counts = ranks[0].hit_matrix
    assert sum(counts) > 0
    bad = compared = 0
    for r, t in enumerate(ranks):
        comm = abi.Comm.emulated(r, world, 60.0, 5.0)
        assert t.frame.tiled_pipelined() == pipelined and t.frame.tiled_shading()
        t.frame.tiled_emulate_wire(comm.handle, counts)
        for _ in range(3):
            t.frame.pin_randoms(0.0, 0, 0)
            t.frame.tiled_step()
        t.frame.tiled_flush()
        torch.cuda.synchronize()
        assert t.frame.tiled_hit_errors() == 0
        assert t.frame.tiled_hit_rounds() == (3, 0, 0), "every round must go out on the seeded capacities, none repeated"
        assert t.frame.last_tasks()[-2:] == ["DeferedShading", "TAA"]
        bad += _interiors_differ(t, want, names)
        y0, y1 = t.tile[1], t.tile[1] + th
        lo, hi = y0 + (margin if r > 0 else 0), y1 - (margin if r + 1 < world else 0)
        for name in ("color_out", "taa_hist"):
            n = _rows_differ(t, held[r], name, 0, lo, hi, want_is_window=True)
            print(f"[shaded] rank {r} {name} rows {lo}..{hi}: {n} texels differ from the lockstep continuation")
            bad += n
            compared += hi - lo
        t.frame.close()
        comm.close()
    assert compared >= 2 * (2 * (th - margin) + (th - 2 * margin))
    assert bad == 0
