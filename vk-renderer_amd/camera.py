"""Camera / projection conventions of the reference and the frozen synthetic frame setup.

Reference: scene/camera.hpp:14-39 (yaw/pitch camera, world-up (0,-1,0), glm::lookAt),
main.cpp:293-294 (eye (0,1,-1), glm::perspective(60 deg, W/H, 0.05, 80), RH, depth 0..1
because of GLM_FORCE_DEPTH_ZERO_TO_ONE, camera.hpp:4-5), main.cpp:368-373 (normal_mat).
glm is not vendored in the reference, so these matrices are restated from glm's published
formulas, computed in float64 and rounded to float32: the kernels take them as data.
"""
import ctypes as C
import math

import numpy as np

from . import abi

FOVY = math.radians(60.0)
ZNEAR, ZFAR = 0.05, 80.0
SEED = 0x5EED0001


def perspective_rh_zo(fovy, aspect, znear, zfar):
    t = math.tan(fovy / 2.0)
    m = np.zeros((4, 4), dtype=np.float64)
    m[0, 0] = 1.0 / (aspect * t)
    m[1, 1] = 1.0 / t
    m[2, 2] = zfar / (znear - zfar)
    m[3, 2] = -1.0
    m[2, 3] = -(zfar * znear) / (zfar - znear)
    return m


def look_at_rh(eye, center, up):
    eye, center, up = (np.asarray(v, dtype=np.float64) for v in (eye, center, up))
    f = center - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4, dtype=np.float64)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[0, 3], m[1, 3], m[2, 3] = -s.dot(eye), -u.dot(eye), f.dot(eye)
    return m


def camera_view(pos, yaw_deg=90.0, pitch_deg=0.0, world_up=(0.0, -1.0, 0.0)):
    """scene/camera.hpp:26-39"""
    yaw, pitch = math.radians(yaw_deg), math.radians(pitch_deg)
    f = np.array([math.cos(yaw) * math.cos(pitch), math.sin(pitch), math.sin(yaw) * math.cos(pitch)])
    f /= np.linalg.norm(f)
    right = np.cross(f, np.asarray(world_up, dtype=np.float64))
    right /= np.linalg.norm(right)
    up = np.cross(right, f)
    up /= np.linalg.norm(up)
    pos = np.asarray(pos, dtype=np.float64)
    return look_at_rh(pos, pos + f, up)


def rolled_view(pos, yaw_deg=90.0, pitch_deg=0.0, roll_deg=0.0):
    """Rz(roll) * camera_view(pos, yaw, pitch): the camera turned about its own view axis.  roll 0 is camera_view itself, to the
    bit (the product with the identity would turn its -0.0 entries into +0.0)."""
    v = camera_view(pos, yaw_deg, pitch_deg)
    if roll_deg == 0.0:
        return v
    c, s = math.cos(math.radians(roll_deg)), math.sin(math.radians(roll_deg))
    r = np.eye(4, dtype=np.float64)
    r[0, 0], r[0, 1], r[1, 0], r[1, 1] = c, -s, s, c
    return r @ v


LIGHT_POS = (-1.85867, 5.81832, -0.247114)  # main.cpp:295; LIGHT_POS of defered_shading/shader.frag


def _f32(v):
    return float(np.float32(v))


def look_at(eye, center, up):
    """glm::lookAt (RH) as a 4x4 float32 array (maths convention: m[row, column]): the components of eye, center and up rounded to
    float32, every entry evaluated in float64 — plain scalar arithmetic in one fixed order, so that the C++ host mirror
    (host/frame.cpp) reproduces it bit for bit — and rounded once."""
    e, c, u = ([_f32(x) for x in v] for v in (eye, center, up))
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def unit(a):
        n = math.sqrt(dot(a, a))
        return [a[0] / n, a[1] / n, a[2] / n]

    f = unit([c[0] - e[0], c[1] - e[1], c[2] - e[2]])
    s = unit(cross(f, u))
    t = cross(s, f)
    m = np.zeros((4, 4), dtype=np.float64)
    m[0, :3], m[1, :3], m[2, :3] = s, t, [-f[0], -f[1], -f[2]]
    m[0, 3], m[1, 3], m[2, 3], m[3, 3] = -dot(s, e), -dot(t, e), dot(f, e), 1.0
    return m.astype(np.float32)


def shadow_mvp(eye=LIGHT_POS, center=(0.0, 2.0, 1.0), up=(0.0, -1.0, 0.0), fovy_deg=90.0, near=0.05, far=80.0):
    """The light matrix of the shadow pass, perspective(radians(fovy), 1, near, far) * lookAt(eye, center, up) (main.cpp:295 with
    the defaults), under this module's rule: fovy (in radians), near, far and the vectors rounded to float32, the two factors
    evaluated in float64 and rounded to float32, their product evaluated in float64 and rounded once.  Bit-equal to the default
    light of the host frame (vkrh_shadow_lights).  -> 4x4 float32, maths convention."""
    fovy = _f32(np.float32(fovy_deg) * np.float32(0.01745329251994329576923690768489))
    p = perspective_rh_zo(fovy, 1.0, _f32(near), _f32(far)).astype(np.float32)
    v = look_at(eye, center, up)
    out = np.zeros((4, 4), dtype=np.float32)
    for r in range(4):
        for c in range(4):
            acc = 0.0
            for k in range(4):
                acc += float(p[r, k]) * float(v[k, c])
            out[r, c] = np.float32(acc)
    return out


class FrameSetup:
    """All per-frame uniforms of the frozen benchmark frame: current camera at
    (0,1,-1) yaw 90; previous frame = eye + (0.02,0,0.01), yaw + 0.2 deg; jitter 0;
    angle_offset = 60/360, weight_ratio 1, max_roughness 1, render_flags 7, accumulate 1."""

    def __init__(self, width, height, frame_random=0, use_mis=1, eye=(0.0, 1.0, -1.0), yaw=90.0,
                 prev_delta=(0.02, 0.0, 0.01), prev_yaw_delta=0.2, material="flat", *, fovy=FOVY, znear=ZNEAR, zfar=ZFAR,
                 pitch=0.0, roll=0.0, aspect=None, prev_pitch_delta=0.0, prev_roll_delta=0.0):
        """fovy in radians; yaw, pitch, roll and their previous-frame deltas in degrees.  view = Rz(roll) * camera_view(eye, yaw,
        pitch): the roll turns the picture about the view axis.  aspect None: width / height."""
        self.width, self.height = width, height
        # "flat": one roughness per object (the frozen scene of SURVEY 8(d)); "textured": per-texel roughness
        # (VKR_SYNTH_TEXTURED_ROUGHNESS, include/vkr_postfx.h)
        if material not in ("flat", "textured"):
            raise ValueError(f"material {material!r}: 'flat' or 'textured'")
        self.material = material
        self.synth_flags = abi.SYNTH_TEXTURED_ROUGHNESS if material == "textured" else 0
        self.aspect = float(width) / float(height) if aspect is None else float(aspect)
        # glm computes in float32; here every *input* matrix is rounded to float32 first and every
        # derived matrix is evaluated in float64 from those and rounded once (host/glm_compat.hpp does
        # the same), so the Python and the C++ host layers hand bit-identical uniforms to the kernels (the inverses up to the
        # entries that are zero in exact arithmetic, where LU and cofactors leave different residues: tests/test_camera_cases.py).
        f32 = lambda m: np.asarray(m, dtype=np.float32).astype(np.float64)
        self.proj = f32(perspective_rh_zo(fovy, self.aspect, znear, zfar))
        self.view = f32(rolled_view(eye, yaw, pitch, roll))
        peye = tuple(e + d for e, d in zip(eye, prev_delta))
        self.prev_view = f32(rolled_view(peye, yaw + prev_yaw_delta, pitch + prev_pitch_delta, roll + prev_roll_delta))
        self.mvp = f32(self.proj @ self.view)
        self.prev_mvp = f32(self.proj @ self.prev_view)
        self.inv_view = f32(np.linalg.inv(self.view))
        self.prev_inv_view = f32(np.linalg.inv(self.prev_view))
        self.normal_mat = self.inv_view.T  # transpose(inverse(view)), main.cpp:368
        self.prev_normal_mat = self.prev_inv_view.T
        self.frame_random = frame_random
        self.use_mis = use_mis
        self.fazz = (np.float32(fovy), np.float32(self.aspect), np.float32(znear), np.float32(zfar))

    def _fazz4(self):
        return (C.c_float * 4)(*[float(v) for v in self.fazz])

    def synth(self, prev=False, depth_only=False):
        p = abi.SynthParams()
        if prev:  # the previous frame's own G-buffer (only its depth is consumed)
            p.camera_to_world = abi.Mat4.from_np(self.prev_inv_view)
            p.mvp = abi.Mat4.from_np(self.prev_mvp)
            p.prev_mvp = abi.Mat4.from_np(self.prev_mvp)
        else:
            p.camera_to_world = abi.Mat4.from_np(self.inv_view)
            p.mvp = abi.Mat4.from_np(self.mvp)
            p.prev_mvp = abi.Mat4.from_np(self.prev_mvp)
        p.fovy, p.aspect, p.znear, p.zfar = [float(v) for v in self.fazz]
        p.seed = SEED
        p.flags = abi.SYNTH_DEPTH_ONLY if depth_only else self.synth_flags
        return p

    def gtao_params(self):
        p = abi.GtaoParams()
        p.normal_mat = abi.Mat4.from_np(self.normal_mat)
        p.fovy, p.aspect, p.znear, p.zfar = [float(v) for v in self.fazz]
        return p

    def gtao_push(self, angle_offset=60.0 / 360.0, weight_ratio=1.0, two_directions=0, reflections_only=0):
        return abi.GtaoPush(angle_offset, weight_ratio, self.use_mis, two_directions, reflections_only)

    def gtao_filter_push(self):
        return abi.GtaoFilterPush(float(self.fazz[2]), float(self.fazz[3]))

    def gtao_accum_params(self):
        p = abi.GtaoAccumParams()
        p.inverse_camera = abi.Mat4.from_np(self.inv_view)
        p.prev_inverse_camera = abi.Mat4.from_np(self.prev_inv_view)
        p.mvp = abi.Mat4.from_np(self.mvp)
        p.fovy_aspect_znear_zfar = self._fazz4()
        return p

    def trace_params(self, frame_random=None):
        p = abi.TraceParams()
        p.normal_mat = abi.Mat4.from_np(self.normal_mat)
        p.frame_random = self.frame_random if frame_random is None else frame_random
        p.fovy, p.aspect, p.znear, p.zfar = [float(v) for v in self.fazz]
        return p

    def reproject_params(self):
        p = abi.ReprojectParams()
        p.inverse_camera = abi.Mat4.from_np(self.inv_view)
        p.prev_inverse_camera = abi.Mat4.from_np(self.prev_inv_view)
        p.fovy_aspect_znear_zfar = self._fazz4()
        return p
