"""The cameras of tests/camera_cases.py on the CPU, the oracle alone.

- A default FrameSetup is what it was before it took a lens and an attitude as keywords, to the byte.
- Every camera input of every pass is observable: replaced by the frozen camera's value (a scalar, a whole matrix, one entry at a
  time) or with its 3x3 block transposed, the pass's reference (the oracle, or the numpy restatement of a pass that has one)
  leaves the pass's own rule on at least one case at 70x38.  What no case makes observable is listed: in UNREAD what the pass
  does not read, in NOT_SHOWN what it reads into something no case can show; DESIGN_NUMERICS.md "Cameras" has both tables.
- No case stands on a knife edge of the reference: with one of fovy, aspect, znear, zfar moved to the next float32, the oracle
  stays within the cap plus four times what the frozen camera does, outside the texels of sky_half for the AO accumulation.
- The C++ host mirror derives the same matrices from vkrh_set_camera as FrameSetup does, bit for bit, under every case."""
import ctypes as C
import math

import numpy as np
import pytest

from vk_renderer_amd import camera
from vk_renderer_amd.camera import FrameSetup

import camera_cases as cc
from parity import mismatches

MATRICES = ("view", "prev_view", "proj", "mvp", "prev_mvp", "inv_view", "prev_inv_view", "normal_mat", "prev_normal_mat")


# ---- the default setup ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(70, 38), (206, 226), (640, 360), (3840, 2160)])
@pytest.mark.parametrize("kw", [{}, dict(eye=(0.3, 1.4, -0.2), yaw=75.0, prev_delta=(-0.03, 0.01, 0.02), prev_yaw_delta=-0.4)], ids=["frozen", "moved"])
def test_default_setup_is_what_it_was(size, kw):
    """the formulas of FrameSetup before the keywords, inline"""
    w, h = size
    eye, yaw = kw.get("eye", (0.0, 1.0, -1.0)), kw.get("yaw", 90.0)
    prev_delta, prev_yaw_delta = kw.get("prev_delta", (0.02, 0.0, 0.01)), kw.get("prev_yaw_delta", 0.2)
    f32 = lambda m: np.asarray(m, dtype=np.float32).astype(np.float64)
    aspect = float(w) / float(h)
    want = {}
    want["proj"] = f32(camera.perspective_rh_zo(math.radians(60.0), aspect, 0.05, 80.0))
    want["view"] = f32(camera.camera_view(eye, yaw))
    want["prev_view"] = f32(camera.camera_view(tuple(e + d for e, d in zip(eye, prev_delta)), yaw + prev_yaw_delta))
    want["mvp"] = f32(want["proj"] @ want["view"])
    want["prev_mvp"] = f32(want["proj"] @ want["prev_view"])
    want["inv_view"] = f32(np.linalg.inv(want["view"]))
    want["prev_inv_view"] = f32(np.linalg.inv(want["prev_view"]))
    want["normal_mat"] = want["inv_view"].T
    want["prev_normal_mat"] = want["prev_inv_view"].T
    got = FrameSetup(w, h, **kw)
    for name in MATRICES:
        g = np.ascontiguousarray(getattr(got, name))
        assert g.dtype == np.float64 and g.tobytes() == np.ascontiguousarray(want[name]).tobytes(), name
    fazz = (np.float32(math.radians(60.0)), np.float32(aspect), np.float32(0.05), np.float32(80.0))
    assert len(got.fazz) == 4 and all(type(a) is np.float32 and a.tobytes() == b.tobytes() for a, b in zip(got.fazz, fazz))
    assert got.aspect == aspect and (camera.FOVY, camera.ZNEAR, camera.ZFAR) == (math.radians(60.0), 0.05, 80.0)


def test_keywords():
    """roll is a rotation about the view axis on top of camera_view; the deltas move the previous frame only; aspect None is W / H"""
    s = FrameSetup(70, 38, pitch=-35.0, roll=30.0, prev_pitch_delta=1.5, prev_roll_delta=-2.0, fovy=1.0, znear=0.2, zfar=300.0, aspect=1.6)
    f32 = lambda m: np.asarray(m, dtype=np.float32).astype(np.float64)

    def rz(deg):
        c, sn = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        return np.array([[c, -sn, 0, 0], [sn, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)

    assert np.array_equal(s.view, f32(rz(30.0) @ camera.camera_view((0.0, 1.0, -1.0), 90.0, -35.0)))
    assert np.array_equal(s.prev_view, f32(rz(28.0) @ camera.camera_view((0.02, 1.0, -0.99), 90.2, -33.5)))
    assert np.array_equal(s.proj, f32(camera.perspective_rh_zo(1.0, 1.6, 0.2, 300.0)))
    assert [float(v) for v in s.fazz] == [float(np.float32(v)) for v in (1.0, 1.6, 0.2, 300.0)]
    assert FrameSetup(70, 38, fovy=1.0).aspect == 70.0 / 38.0
    # a rolled view is still a rigid motion: its inverse is its transpose and the eye
    r = s.view[:3, :3]
    assert np.allclose(r @ r.T, np.eye(3), atol=1e-6) and np.allclose(s.inv_view[:3, 3], (0.0, 1.0, -1.0), atol=1e-6)
    with pytest.raises(TypeError):
        FrameSetup(70, 38, 0, 1, (0.0, 1.0, -1.0), 90.0, (0.02, 0.0, 0.01), 0.2, "flat", 1.0)  # the lens is keyword-only


def test_cases():
    assert list(cc.CASES) == ["pitch_down", "pitch_down_roll", "pitch_up", "roll_90", "narrow", "wide", "anamorphic", "deep_range", "far_small",
                              "near_small", "prev_pitch", "all_moved", "yaw_eye"]
    with pytest.raises(TypeError):
        cc.CASES["pitch_up"]["pitch"] = 0.0
    with pytest.raises(TypeError):
        cc.CASES["level"] = {}
    for name in cc.CASES:
        cc.setup(name, cc.SMALL)
    # pitch_up: about half of the frame is sky
    assert 0.35 < float(cc.record("pitch_up", cc.SMALL).sky.mean()) < 0.65
    # the frozen view is zeros and +-1 (to 1e-16); a pitched and rolled one has neither
    assert np.isin(np.abs(np.round(cc.setup("default", cc.SMALL).view[:3, :3], 12)), (0.0, 1.0)).all()
    assert (np.abs(cc.setup("yaw_eye", cc.SMALL).view[:3, :3]) > 0.1).all()


def test_extent_names_its_case_to_caches_and_comparisons():
    """camera_cases.Extent: unpacks and indexes as the size, is a key of its own per case, and equals no bare size, so a kit's
    `size == (64, 36)` content assertion written for the frozen camera does not fire under another"""
    import functools

    e = cc.Extent((64, 36), "pitch_up")
    w, h = e
    assert (w, h, e[0], e[1], len(e)) == (64, 36, 64, 36, 2)
    assert e != (64, 36) and (64, 36) != e and not e == (64, 36) and e == cc.Extent((64, 36), "pitch_up") and e != cc.Extent((64, 36), "wide")
    seen = []

    @functools.lru_cache(maxsize=None)
    def kit(size):
        seen.append(size)
        return len(seen)

    assert len({kit((64, 36)), kit(e), kit(cc.Extent((64, 36), "wide")), kit(cc.Extent((64, 36), "pitch_up"))}) == 3
    assert cc.frame_setup(e, 64, 36).view.tobytes() == cc.setup("pitch_up", (64, 36)).view.tobytes()
    assert cc.frame_setup((64, 36), 64, 36).view.tobytes() == FrameSetup(64, 36).view.tobytes()


# ---- what a step is held to ------------------------------------------------------------------------------------------------------------
def outside(step, results, skip=None):
    """{output: texels outside the step's own rule}: differing texels of an integer output, texels outside tests/parity.py
    otherwise; skip: {output: [h, w] bool} of texels left out"""
    counts = {}
    for out, (img, want) in results.items():
        n = 0
        host = img.to_host()
        for mip in range(img.mips):
            if step.is_exact(out):
                bad = (cc.bits(img, mip, host) != cc.bits(img, mip, want)).any(axis=-1)
            else:
                bad = mismatches(img.format, img.decode(mip, host), img.decode(mip, want))
            if skip is not None and out in skip and mip == 0:
                bad = bad & ~skip[out]
            n += int(bad.sum())
        counts[out] = n
    return counts


def leaves_the_rule(step, results):
    counts = outside(step, results)
    return any(n > (0 if step.is_exact(out) else cc.cap(results[out][0].width * results[out][0].height)) for out, n in counts.items())


# ---- every camera input is observable ----------------------------------------------------------------------------------------------------
SCALARS = ("fovy", "aspect", "znear", "zfar")
_LENS = SCALARS
# what each step hands its pass of the setup (vk-renderer_amd/chain.py, camera.py)
INPUTS = {
    "synth": ("inv_view", "prev_inv_view", "mvp", "prev_mvp") + _LENS,
    "downsample": (),
    "ssr_trace": ("normal_mat",) + _LENS,
    "ssr_filter": ("normal_mat",) + _LENS,
    "ssr_blur": ("inv_view", "prev_inv_view") + _LENS,
    "gtao_main": ("normal_mat",) + _LENS,
    "gtao_filter": ("znear", "zfar"),
    "gtao_accumulate": ("inv_view", "prev_inv_view", "mvp") + _LENS,
    "taa": ("inv_view", "prev_inv_view") + _LENS,
    "gtao_graphics": ("normal_mat",) + _LENS,
    "gtao_deinterleaved": ("normal_mat",) + _LENS,
    "screen_trace": ("normal_mat",) + _LENS,
    "screen_trace_filter": ("znear", "zfar"),
    "screen_trace_accumulate": _LENS,
    "ssr_simple": ("normal_mat",) + _LENS,
    "shading": ("inv_view", "view") + _LENS,
    "shading_show_ao": ("inv_view", "view") + _LENS,
    "trace_indirect": ("normal_mat",) + _LENS,
    "gtao_main_no_mis": ("normal_mat",) + _LENS,
    "gtao_reproject": _LENS,
}
ORDER = ("all_moved", "yaw_eye", "pitch_down_roll", "prev_pitch", "pitch_up", "roll_90", "deep_range", "near_small", "far_small", "anamorphic", "narrow", "wide",
         "pitch_down")


def mutations(name):
    """-> [(label, mutate(setup, default setup))] of input `name`"""
    if name in SCALARS:
        k = SCALARS.index(name)

        def scalar(st, df):
            st.fazz = tuple(df.fazz[i] if i == k else v for i, v in enumerate(st.fazz))
        return [("default", scalar)]

    def whole(st, df):
        setattr(st, name, getattr(df, name).copy())

    def transposed(st, df):
        m = getattr(st, name).copy()
        m[:3, :3] = m[:3, :3].T.copy()
        setattr(st, name, m)

    out = [("default", whole), ("3x3 transposed", transposed)]
    setups = [cc.setup(c, cc.SMALL) for c in cc.CASES]
    df = cc.setup("default", cc.SMALL)
    for i in range(4):
        for j in range(4):
            if all(getattr(s, name)[i, j] == getattr(df, name)[i, j] for s in setups):
                continue  # the entry is the frozen camera's under every case

            def entry(st, df, i=i, j=j):
                m = getattr(st, name).copy()
                m[i, j] = getattr(df, name)[i, j]
                setattr(st, name, m)
            out.append((f"[{i}][{j}]", entry))
    return out


# (step, input, mutation; "*": every one) that no case makes observable, and why: the pass does not read it, or reads it into
# nothing that it stores (DESIGN_NUMERICS.md "Cameras" has the same table)
_DIRECTION = "the normal matrix turns a direction (w = 0): its fourth row (maths convention) meets the zero"
UNREAD = {
    **{(s, "normal_mat", f"[3][{j}]"): _DIRECTION for s, names in INPUTS.items() if "normal_mat" in names for j in range(3)},
    ("gtao_accumulate", "inv_view", "*"): "accum.comp reprojects with prev_inverse_camera and mvp alone: inverse_camera is declared and never used",
    ("shading", "view", "*"): "defered_shading/shader.frag declares `camera` and reads inverse_camera alone",
    ("shading_show_ao", "*", "*"): "show_ao stores the upsampled occlusion: nothing the camera enters is stored",
    ("synth", "mvp", "[2][*]"): "the generator takes the velocity from clip x, y and w: the z row of mvp is not read",
    ("synth", "prev_mvp", "[2][*]"): "as mvp: the z row is not read",
    ("screen_trace_accumulate", "fovy", "*"): "accumulate.comp compares view z alone, which fovy and aspect do not enter",
    ("screen_trace_accumulate", "aspect", "*"): "as fovy",
    ("gtao_reproject", "fovy", "*"): "reproject.comp (STATIC_REPROJECT) compares view z alone, which fovy and aspect do not enter",
    ("gtao_reproject", "aspect", "*"): "as fovy",
}
# read by the pass, and still shown by no case: said apart from UNREAD, because a wrong kernel could hide here
NOT_SHOWN = {
    ("gtao_deinterleaved", "normal_mat", "[2][0]"): "with the reference's literal dispatch the pass samples the top-left quarter of an 8 x 4 depth layer at "
                                                     "70x38, one surface, and writes 45 texels: the entry moves fewer than two of them out of tolerance; the "
                                                     "same code (gtao_camera_space_v2) shows the entry in gtao_graphics",
}


def _listed(key):
    step, name, label = key
    row = label[:3] + "[*]" if label.startswith("[") else None
    return any(k in UNREAD or k in NOT_SHOWN for k in (key, (step, name, "*"), (step, "*", "*"), (step, name, row)))


def _observable(step, name, label, mutate, chains):
    df = cc.setup("default", cc.SMALL)
    for case in ORDER:
        rec = cc.record(case, cc.SMALL)
        st = rec.setup()
        before = {n: np.array(getattr(st, n)) for n in MATRICES}
        fazz = st.fazz
        mutate(st, df)
        if st.fazz == fazz and all(np.array_equal(before[n], getattr(st, n)) for n in MATRICES):
            continue  # this case holds the frozen camera's value there
        if case not in chains:
            chains[case] = rec.chain("oracle")
        chains[case].setup = st
        if leaves_the_rule(step, rec.run(chains[case], step)):
            return case
    return None


@pytest.fixture(scope="module")
def observability(oracle_lib):
    """{(step, input, mutation): the first case under which the oracle shows it, or None}"""
    table, chains = {}, {}
    for step_name, names in INPUTS.items():
        for name in names:
            for label, mutate in mutations(name):
                table[(step_name, name, label)] = _observable(cc.STEPS[step_name], name, label, mutate, chains)
    return table


def test_every_step_is_listed():
    assert set(INPUTS) == set(cc.STEPS)


def test_every_camera_input_is_observable(observability):
    unseen = {k for k, case in observability.items() if case is None}
    listed = {k for k in observability if _listed(k)}
    for k in sorted(unseen - listed):
        print("[camera] not observable under any case:", k)
    for k in sorted(listed - unseen):
        print("[camera] listed as unread, but observable under", observability[k], ":", k)
    assert unseen == listed
    used = sorted({case for case in observability.values() if case is not None})
    print(f"[camera] {len(observability)} mutated inputs: {len(observability) - len(unseen)} shown by {used}, {len(unseen)} listed as unread")
    # every row of the list is about something the steps are handed
    for step, name, label in list(UNREAD) + list(NOT_SHOWN):
        assert any(k[0] == step and name in ("*", k[1]) for k in observability), (step, name, label)


# ---- the same for the passes with exact restatements ---------------------------------------------------------------------------------------
# ssao, tile_regression, gtao_rt_main, trace_probe, the shadow masks and the traced reflections have no oracle entry: their
# references are the numpy restatements, on the G-buffer kits tests/test_camera_cases_gpu.py runs the kernels on (the procedural
# scene through the oracle's rasteriser under the case's camera).  Same mutations; the rule of these passes is any differing byte.
HALF = (cc.SMALL[0] // 2, cc.SMALL[1] // 2)
_WORLD = ("inv_view",) + _LENS
RESTATED_INPUTS = {
    "ssao": ("proj",) + _LENS, "tile_regression": _WORLD, "gtao_rt_main": _WORLD, "trace_probe": _WORLD, "shadow_mask": _WORLD,
    "shadow_mask_rt": _WORLD, "shadow_mask_rt_cutout": _WORLD, "shadow_mask_rt_soft": _WORLD, "shadow_mask_filter": _WORLD,
    "reflections_rt": _WORLD, "reflections_rt_cutout": _WORLD,
}


def restated(pass_name, case):
    """-> f(setup) -> the bytes the restatement of `pass_name` stores on the kit's rasterised G-buffer under `case`, the camera
    handed to the pass being `setup`'s"""
    import probe_reference as probe_ref
    import shadow_light as sl
    import shadow_mask_reference as mask_ref
    import side_pass_content as sp
    import ssao_reference as ssao_ref
    import test_ray_cutout_passes_gpu as cutout
    import test_reflections_rt_gpu as mirror
    import test_shadow_mask_filter_gpu as filt
    import test_shadow_mask_gpu as mask_gpu
    import test_shadow_mask_rt_gpu as hard
    import test_shadow_mask_rt_soft_gpu as soft
    import tile_regression_reference as tile_ref
    import gtao_rt_reference as gtao_ref

    full, half = cc.Extent(cc.SMALL, case), cc.Extent(HALF, case)
    ar = sp.arith()
    lens = lambda st: [float(v) for v in st.fazz]
    if pass_name == "ssao":
        words = sp.inputs("ssao", "raster", full)[0]
        return lambda st: ssao_ref.ssao(ar, words, st.proj, *st.fazz, sp.ssao_samples("fixed"), *cc.SMALL)[0]
    if pass_name == "tile_regression":
        words = sp.inputs("tile_regression", "raster", half, 1)[0]
        return lambda st: tile_ref.tile_regression(ar, words, st.inv_view, *lens(st), *tile_ref.tiles_of(*HALF))
    if pass_name == "gtao_rt_main":
        words, codes = sp.inputs("gtao_rt", "raster", half, 1)[:2]
        return lambda st: gtao_ref.gtao_rt(ar, words, codes, (st.inv_view, *lens(st)), 0.3, sp.ao_directions(), sp.ao_triangles("scene"), *HALF)
    if pass_name == "trace_probe":
        words, codes = sp.inputs("trace_probe", "raster", full)[:2]
        colour, depth = sp.probes("room", 4, 16)
        return lambda st: probe_ref.trace_probe(ar, words, codes, probe_ref.ProbeArrays(colour, depth), st.inv_view, sp.PMIN, sp.PMAX, 4, *lens(st), *cc.SMALL)[0]
    if pass_name == "shadow_mask":  # the maps of lights A, B, C by the oracle's rasteriser (tests/shadow_light.py), 128^2
        words = cutout._inputs("raster", full)[0]
        mvps = [sl.mvp(k) for k in "ABC"]
        maps = _shadow_maps()
        return lambda st: mask_ref.shadow_mask(mask_gpu._arith(), words, maps, st.inv_view, mvps, *st.fazz, 1, mask_gpu.RASTER_BIAS)
    if pass_name == "shadow_mask_rt":
        words, codes = hard._inputs("raster", full)[:2]
        return lambda st: hard.ref.shadow_mask_rt(hard._arith(), words, codes, st.inv_view, *st.fazz, list(hard.LIGHT_SETS[4]), hard.OFFSET, hard.TMIN, hard._scene()[1])
    if pass_name in ("shadow_mask_rt_cutout", "reflections_rt_cutout"):
        words, codes = cutout._inputs("raster", full)[:2]
        sc, tris, att, opaque = cutout._scene()
        if pass_name == "shadow_mask_rt_cutout":
            return lambda st: cutout.ref.shadow_mask_rt_cutout(cutout._arith(), words, codes, st.inv_view, *st.fazz, cutout.LIGHTS, cutout.OFFSET, cutout.TMIN,
                                                               tris, att, sc.textures, 0, opaque)
        before = np.full(words.shape + (4,), cutout.FILL, np.uint8)
        return lambda st: cutout.ref.reflections_rt_cutout(cutout._arith(), words, codes, None, st.inv_view, *st.fazz, cutout.OFFSET, cutout.TMIN,
                                                           float(st.fazz[3]), 0, 0, tris, att, sc.textures, before, 0, 0)[0]
    if pass_name == "shadow_mask_rt_soft":
        words, codes = soft._inputs("raster", full)[:2]
        lights, radii = soft.SETS["4"]
        return lambda st: soft.ref.shadow_mask_rt_soft(soft._arith(), words, codes, st.inv_view, *st.fazz, list(lights), soft.OFFSET, soft.TMIN,
                                                       soft._scene()[1], radii, soft._table(4, 2))
    if pass_name == "shadow_mask_filter":
        words, codes = filt._inputs("raster", full)[:2]
        mask = filt._random_mask(full, 3)
        return lambda st: filt.ref.shadow_mask_filter(filt._arith(), words, codes, mask, st.inv_view, *st.fazz, 3, *filt.THRESHOLDS)
    if pass_name == "reflections_rt":
        words, codes = mirror._inputs("raster", full)[:2]
        sc, tris, att, _ = mirror._scene()
        before = np.full(words.shape + (4,), mirror.FILL, np.uint8)
        return lambda st: mirror.ref.reflections_rt(mirror._arith(), words, codes, None, st.inv_view, *st.fazz, mirror.OFFSET, mirror.TMIN,
                                                    float(st.fazz[3]), 0, 0, tris, att, sc.textures, before)[0]
    raise KeyError(pass_name)


_MAPS = []


def _shadow_maps():
    if not _MAPS:
        import shadow_light as sl
        import test_ray_cutout_passes_gpu as cutout

        _MAPS.append(np.stack([sl.expected(cutout._scene()[0], sl.mvp(k), 128) for k in "ABC"]))
    return _MAPS[0]


# what no case shows of these passes, and why (DESIGN_NUMERICS.md "Cameras"): nothing is unread; read and not shown:
_CANCELS = ("the filter takes world positions only in the difference W_tap - W_pixel of its plane test (and view z for the tolerance): the translation "
            "column cancels up to the rounding of W, which moves no tap across the tolerance on this content")
RESTATED_NOT_SHOWN = {("shadow_mask_filter", "inv_view", f"[{i}][3]"): _CANCELS for i in range(3)}


@pytest.fixture(scope="module")
def restated_observability(oracle_lib):
    """{(pass, input, mutation): the first case under which the restatement shows it, or None}; a mutation that changes nothing
    under any case (the transposed 3x3 block of a projection, which is diagonal) is no mutation and is left out"""
    df = cc.setup("default", cc.SMALL)
    table, calls, base = {}, {}, {}
    for pass_name, names in RESTATED_INPUTS.items():
        for name in names:
            for label, mutate in mutations(name):
                shown, applies = None, False
                for case in ORDER:
                    st = cc.setup(case, cc.SMALL)
                    before, fazz = {n: np.array(getattr(st, n)) for n in MATRICES}, st.fazz
                    mutate(st, df)
                    if st.fazz == fazz and all(np.array_equal(before[n], getattr(st, n)) for n in MATRICES):
                        continue
                    applies = True
                    if (pass_name, case) not in calls:
                        calls[(pass_name, case)] = restated(pass_name, case)
                        base[(pass_name, case)] = np.asarray(calls[(pass_name, case)](cc.setup(case, cc.SMALL))).tobytes()
                    if np.asarray(calls[(pass_name, case)](st)).tobytes() != base[(pass_name, case)]:
                        shown = case
                        break
                if applies:
                    table[(pass_name, name, label)] = shown
    return table


def test_every_restated_pass_is_listed():
    import inspect

    import test_camera_cases_gpu as gpu

    tests = {n[len("test_"):] for n, f in inspect.getmembers(gpu, inspect.isfunction) if n.startswith("test_")}
    ours = {"chain_stagewise", "side_rows_and_shading", "synth", "division_selftest_at_every_depth_range", "host_frame"}
    assert {p.replace("_cutout", "") for p in RESTATED_INPUTS} == tests - ours


def test_every_camera_input_of_the_restated_passes_is_observable(restated_observability):
    table = restated_observability
    unseen = {k for k, case in table.items() if case is None}
    listed = {k for k in table if k in RESTATED_NOT_SHOWN}
    for k in sorted(unseen - listed):
        print("[camera] not observable under any case:", k)
    for k in sorted(listed - unseen):
        print("[camera] listed as unread, but observable under", table[k], ":", k)
    used = sorted({case for case in table.values() if case is not None})
    print(f"[camera] restated passes: {len(table)} mutated inputs: {len(table) - len(unseen)} shown by {used}, {len(unseen)} listed as not shown")
    assert unseen == listed and len(listed) == len(RESTATED_NOT_SHOWN)


# ---- no case on a knife edge ---------------------------------------------------------------------------------------------------------------
def _static_class(step_name, out, mip):
    def skip(rec):
        pre = rec.pre[step_name]
        probe = rec.chain("oracle")
        edge = cc.nearly_static(probe.depth, probe.prev_depth, mip, pre["depth"], pre["prev_depth"])
        img = getattr(probe, out)
        return {out: edge[: img.height, : img.width]}
    return skip


# the texel classes on which a step's decision is ill-conditioned by construction, each a function of the step's inputs alone
SKIPPED = {
    "gtao_accumulate": lambda rec: {"acc_ao": rec.sky},
    "screen_trace_accumulate": _static_class("screen_trace_accumulate", "st_accumulated", 0),
    "gtao_reproject": _static_class("gtao_reproject", "ao_output", 1),
}


def nudged(rec, k):
    """the record's setup with scalar k of (fovy, aspect, znear, zfar) at the next float32 up"""
    st = rec.setup()
    st.fazz = tuple(np.nextafter(v, np.float32(np.inf), dtype=np.float32) if i == k else v for i, v in enumerate(st.fazz))
    return st


def nudge_counts(name, size):
    """{(step, output): (the most texels the oracle moves outside the rule when one camera scalar moves to the next float32, the
    image's texels)}, over the steps that take a scalar and store something under a tolerance, outside the classes of SKIPPED"""
    rec = cc.record(name, size)
    chain = rec.chain("oracle")
    worst = {}
    for k in range(4):
        chain.setup = nudged(rec, k)
        for step_name in rec.pre:
            step = cc.STEPS[step_name]
            if step.exact or not INPUTS[step_name]:
                continue
            skip = SKIPPED.get(step_name, lambda rec: None)(rec)
            results = rec.run(chain, step)
            for out, n in outside(step, results, skip).items():
                if not step.is_exact(out):
                    worst[(step_name, out)] = (max(worst.get((step_name, out), (0, 0))[0], n), results[out][0].width * results[out][0].height)
    return worst


@pytest.fixture(scope="module")
def nudges(oracle_lib):
    return {(name, size): nudge_counts(name, size) for size in cc.SIZES for name in ("default",) + tuple(cc.CASES)}


def test_no_case_stands_on_a_knife_edge(nudges):
    over = []
    for size in cc.SIZES:
        base = nudges[("default", size)]
        for name in cc.CASES:
            for (step, out), (n, texels) in nudges[(name, size)].items():
                allowed = cc.cap(texels) + 4 * base[(step, out)][0]
                if n:
                    print(f"[camera] nudge {name} {size[0]}x{size[1]} {step}:{out}: {n} of {texels} texels (default camera {base[(step, out)][0]}, allowed {allowed})")
                if n > allowed:
                    over.append((name, size, step, out, n, allowed))
    assert not over, over


def test_the_accumulation_flips_on_the_sky(oracle_lib):
    """Why sky_half is a class of its own: under pitch_up the oracle's gtao_accumulate moves a tenth of the image out of tolerance
    when one camera scalar moves by one float32, and every such texel has the sky's depth code at half resolution.  The
    reprojected ndc.z of a sky texel is 1 to a few ulps, so its linear depth is zfar or anything down to far below it, and
    depth_err = |prev_z - zfar| decides `depth_err < 0.2` (history kept or dropped) and, below 0.2, scales the kept sample count
    by clamp(1 - 0.1 vel - depth_err, 0.8, 1).  Most flipped texels therefore hold what the oracle stores with its history
    cleared or with it kept; the rest hold a sample count in between (printed)."""
    for size in cc.SIZES:
        rec = cc.record("pitch_up", size)
        chain = rec.chain("oracle")
        step = cc.STEPS["gtao_accumulate"]
        flipped, third = np.zeros_like(rec.sky), np.zeros_like(rec.sky)
        for k in range(4):
            chain.setup = nudged(rec, k)
            img, want = rec.run(chain, step)["acc_ao"]
            got = img.decode(0)
            bad = mismatches(img.format, got, img.decode(0, want))
            assert not (bad & ~rec.sky).any(), "the accumulation flips off the sky"
            flipped |= bad
            third |= bad & mismatches(img.format, got, img.decode(0, rec.acc_ao_cleared))
        print(f"[camera] pitch_up {size[0]}x{size[1]}: acc_ao flips under the nudge in {int(flipped.sum())} of {int(rec.sky.sum())} sky texels "
              f"({flipped.size} texels), {int(third.sum())} of them to neither the kept nor the cleared history")
        assert int(flipped.sum()) > 10 * cc.cap(flipped.size)


def test_the_static_reprojections_flip_where_the_depths_are_codes_apart(oracle_lib):
    """The class of SKIPPED for screen_trace_accumulate and gtao_reproject: the texels whose previous depth camera_cases moved by
    one or two codes.  Under deep_range (a D24 code is 1.2e-7 z^2 of linear depth, view z a few units, a float32 ulp of it
    2.4e-7) `delta < 1e-6` falls between differences four and five ulps long, and the oracle flips there under the nudge and
    nowhere else."""
    rec = cc.record("deep_range", cc.SMALL)
    chain = rec.chain("oracle")
    for step_name, out in (("screen_trace_accumulate", "st_accumulated"), ("gtao_reproject", "ao_output")):
        edge = SKIPPED[step_name](rec)[out]
        flipped = np.zeros_like(edge)
        for k in range(4):
            chain.setup = nudged(rec, k)
            img, want = rec.run(chain, cc.STEPS[step_name])[out]
            flipped |= mismatches(img.format, img.decode(0), img.decode(0, want))
        print(f"[camera] deep_range {step_name}: flips under the nudge in {int(flipped.sum())} texels, {int((flipped & edge).sum())} of them in the class of {int(edge.sum())}")
        assert flipped.any() and not (flipped & ~edge).any()


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------------
INVERSION = 2 * 2.0 ** -45  # twice the error of one float64 inversion of a view matrix (the test's docstring)
RESIDUE = 1e-9              # below it an entry of an inverse is what rounding left of an exact zero


def test_host_mirror_derives_the_same_matrices():
    """vkrh_set_camera with a case's view, prev_view and projection, then vkrh_camera_matrices: projection * view and projection *
    prev_view as the frame stores them for its passes, and the inverse(view) it hands the ray-traced stages (glm_compat.hpp:
    float64, rounded once); with prev_view given as the view, the inverse of that.  transpose(inverse(view)) moves no bit.

    The two products are FrameSetup's bits.  So is every entry of the inverses above RESIDUE in magnitude.  Below it they are
    not, and cannot be: FrameSetup inverts by LU (numpy.linalg.inv), the mirror by cofactors, and where an entry is zero in
    exact arithmetic, or the float32 rounding of the view's entries away from it, the two leave different residues: +0 against
    -0 under the frozen camera, 1.2707161e-24 against 1.2707160e-24 under pitch_down, -5.3606074e-12 against -5.3606078e-12 in
    a previous view.  Both are float64 inversions of a rigid motion with entries below 4 and a condition number below 20, so
    each is within 20 * 4 * 2^-52 < 2^-45 of the exact inverse: two residues may differ by INVERSION (+0 and -0 by nothing) and
    the one float32 step the rounding can add.  Neither side can follow the other: a default FrameSetup keeps its bytes, and an
    LU's residues are not the cofactors'.  Measured: 90 entries over the 14 cameras and both sizes, the largest 5.4e-12, none
    under a camera that rolls.  The frame lives on a malloc-backed allocator and launches nothing, as tests/test_host_mirror.py."""
    from vk_renderer_amd import host

    l = host.lib()
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    alloc = host._ALLOC(lambda n, u: libc.malloc(n))
    free = host._FREE(lambda p, u: libc.free(p))
    l.vkrh_set_allocator(alloc, free, None)

    def held(h, st, view):
        cam = host.HostCamera()
        cam.view, cam.prev_view, cam.projection = host._mat16(view), host._mat16(st.prev_view), host._mat16(st.proj)
        cam.fovy, cam.aspect, cam.znear, cam.zfar = [float(v) for v in st.fazz]
        assert l.vkrh_set_camera(h, C.byref(cam)) == 0, l.vkrh_last_error().decode()
        out = (C.c_float * 48)()
        assert l.vkrh_camera_matrices(h, out) == 0, l.vkrh_last_error().decode()
        return [np.ascontiguousarray(m.T) for m in np.array(out[:], dtype=np.float32).reshape(3, 4, 4)]

    count, largest, seen = 0, 0.0, set()
    try:
        for name in ("default",) + tuple(cc.CASES):
            for size in cc.SIZES:
                st = cc.setup(name, size)
                cfg = host.HostConfig(size[0], size[1], 0, 0, size[0], size[1], 0, None)
                h = l.vkrh_create(C.byref(cfg))
                assert h, l.vkrh_last_error().decode()
                try:
                    mvp, prev_mvp, inv_view = held(h, st, st.view)
                    prev_inv_view = held(h, st, st.prev_view)[2]
                finally:
                    l.vkrh_destroy(h)
                for m, have in (("mvp", mvp), ("prev_mvp", prev_mvp)):
                    want = np.asarray(getattr(st, m), dtype=np.float32)
                    assert have.tobytes() == want.tobytes(), f"{name} {size} {m}: the host mirror holds\n{have}\nFrameSetup\n{want}"
                for m, have in (("inv_view", inv_view), ("prev_inv_view", prev_inv_view)):
                    want = np.asarray(getattr(st, m), dtype=np.float32)
                    differ = (have.view(np.uint32) != want.view(np.uint32)) & ~((have == 0) & (want == 0))
                    big = np.abs(want) > RESIDUE
                    assert not (differ & big).any(), f"{name} {size} {m}: the host mirror derives\n{have}\nFrameSetup\n{want}"
                    gap = np.abs(have.astype(np.float64) - want.astype(np.float64))
                    assert (gap[~big] <= INVERSION + np.spacing(np.abs(want[~big]))).all(), f"{name} {size} {m}: a residue of {gap[~big].max()}"
                    assert (np.abs(have[~big]) <= RESIDUE).all()
                    signs = (have.view(np.uint32) != want.view(np.uint32)) & (have == 0) & (want == 0)
                    if differ.any() or signs.any():
                        seen.add(name)
                        count += int(differ.sum()) + int(signs.sum())
                        largest = max([largest] + np.abs(want[differ]).tolist())
    finally:
        l.vkrh_set_allocator(host._ALLOC(0), host._FREE(0), None)  # back to hipMalloc
    print(f"[camera] host mirror: entries of the two inverses whose bits are not FrameSetup's, over both sizes: {count} under {sorted(seen)}; "
          f"the largest of them {largest:.3e}")
    assert largest < 1e-11 and 0 < count <= 120
    assert not seen & {"pitch_down_roll", "roll_90", "all_moved", "yaw_eye"}, "a view that rolls has no exact zero to leave a residue of"
