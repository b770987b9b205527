"""Numpy restatement of vkr_shadow_mask_accumulate (csrc/shadow_mask_accumulate.hip; DESIGN_NUMERICS.md, Shadow mask, temporal
accumulation) — the checker of tests/test_shadow_mask_accumulate.py and tests/test_shadow_mask_accumulate_gpu.py.

Test infrastructure, like the oracle: the product package never imports it.  The surface point of a pixel is
tests/shadow_mask_rt_reference.py's pixel_surface, the arithmetic its Arith(contract), the view depth of a pixel
tests/shadow_mask_filter_reference.py's view_z; what is restated here is the pass: the reprojected texel, the six validity
conditions in their order, and the integer update.

`mutant` names one deliberate deviation from the rule (MUTANTS): tests/test_shadow_mask_accumulate.py asks that each of them
changes a byte on the constructed cases, so that no line of the rule goes unobserved."""
import numpy as np

from shadow_mask_filter_reference import view_z
from shadow_mask_rt_reference import Arith, F32, d24_to_float, pixel_surface  # noqa: F401

MUTANTS = ("round", "le_w", "count_g", "current_camera", "no_prev_sky", "bound_q", "256", "no_rounding", "truncated_mask", "cap_max_count")
VALID = 0  # `failed` of a pixel whose history is valid; otherwise the number 1..6 of the first condition that failed


def shadow_mask_accumulate(ar, depth_words, normal_codes, velocity, prev_depth_words, mask, history, history_count, inverse_camera,
                           prev_inverse_camera, fovy, aspect, znear, zfar, max_count, plane_tolerance, reset, mutant=None):
    """the whole pass -> (out_history uint16 [h, w, 4], out_count uint8 [h, w], out_mask uint8 [h, w, 4], failed uint8 [h, w]).
    depth_words, prev_depth_words: raw D24S8 texels [h, w]; normal_codes: raw RG16_UNORM texels [h, w, 2]; velocity: float16
    [h, w, 2]; mask: uint8 [h, w, 4]; history: uint16 [h, w, 4]; history_count: uint8 [h, w]; the matrices 4x4, maths convention."""
    assert mutant is None or mutant in MUTANTS, mutant
    h, w = depth_words.shape
    mask = np.asarray(mask, np.uint8).reshape(h, w, 4)
    history = np.asarray(history, np.uint16).reshape(h, w, 4)
    history_count = np.asarray(history_count, np.uint8).reshape(h, w)
    camera = (fovy, aspect, znear, zfar)
    sky, world, normal, _ = pixel_surface(ar, depth_words, normal_codes, inverse_camera, *camera, 0.0)
    # W' per texel of the previous frame: a value per texel, the same whichever pixel lands on it
    prev_sky, prev_world, _, _ = pixel_surface(ar, prev_depth_words, normal_codes, inverse_camera if mutant == "current_camera" else prev_inverse_camera,
                                               *camera, 0.0)
    gy, gx = np.mgrid[0:h, 0:w]
    wf, hf = F32(w), F32(h)
    vel = np.asarray(velocity, np.float16).reshape(h, w, 2).astype(F32)  # fp16 -> fp32 is exact
    with np.errstate(all="ignore"):
        uvx = ((gx.astype(F32) + F32(0.5)) / wf).astype(F32)
        uvy = ((gy.astype(F32) + F32(0.5)) / hf).astype(F32)
        fx = ((uvx + vel[..., 0]).astype(F32) * wf).astype(F32)
        fy = ((uvy + vel[..., 1]).astype(F32) * hf).astype(F32)
        if mutant == "le_w":
            inside = (fx >= 0) & (fx <= wf) & (fy >= 0) & (fy <= hf)
        else:
            inside = (fx >= 0) & (fx < wf) & (fy >= 0) & (fy < hf)  # a compare with a NaN is false
        qfx, qfy = (np.rint(fx), np.rint(fy)) if mutant == "round" else (np.floor(fx), np.floor(fy))
    if mutant in ("round", "le_w"):  # a mutant may point one texel outside: it reads the border texel
        qfx, qfy = np.minimum(qfx, wf - 1), np.minimum(qfy, hf - 1)
    qx = np.where(inside, qfx, 0).astype(np.int64)
    qy = np.where(inside, qfy, 0).astype(np.int64)
    n = (history_count if mutant == "count_g" else history_count[qy, qx]).astype(np.uint32)
    with np.errstate(all="ignore"):
        diff = (prev_world[qy, qx] - world).astype(F32)  # three subtractions, previous minus current
        pdot = ar.dot(normal, diff)
        z = view_z(ar, prev_depth_words, znear, zfar)[qy, qx] if mutant == "bound_q" else view_z(ar, depth_words, znear, zfar)
        bound = (F32(plane_tolerance) * np.abs(z)).astype(F32)
        on_plane = np.abs(pdot) <= bound  # a NaN: invalid
    conditions = [np.full((h, w), not reset), ~sky, inside, n >= 1, np.ones((h, w), bool) if mutant == "no_prev_sky" else ~prev_sky[qy, qx], on_plane]
    failed = np.zeros((h, w), np.uint8)
    for number, ok in reversed(list(enumerate(conditions, start=1))):
        failed = np.where(ok, failed, number).astype(np.uint8)
    valid = failed == VALID

    cap = np.uint32(max_count if mutant == "cap_max_count" else max_count - 1)
    n1 = np.where(valid, np.minimum(n, cap) + np.uint32(1), np.uint32(1)).astype(np.uint32)
    scale = np.uint32(256 if mutant == "256" else 257)
    H = history[qy, qx].astype(np.uint32)
    m = mask.astype(np.uint32)
    half = np.zeros_like(n1) if mutant == "no_rounding" else n1 >> np.uint32(1)
    new = (H * (n1 - np.uint32(1))[..., None] + scale * m + half[..., None]) // n1[..., None]
    new = np.where(valid[..., None], new, scale * m).astype(np.uint32)
    assert (new <= 65535).all()
    out = (np.uint32(255) * new + np.uint32(0 if mutant == "truncated_mask" else 32767)) // np.uint32(65535)
    return new.astype(np.uint16), n1.astype(np.uint8), out.astype(np.uint8), failed
