"""The multi-frame scene of the temporal anti-aliasing tests: the lit Cornell fixture under a camera that translates and turns
between frames, the reference chain of one frame up to the resolve's inputs (oracle -> visibility -> G-buffer -> lighting), and the
CONDITION that the chain's path bytes must meet so that a run cannot pass by leaving a rule out.  Shared by the CPU test of the
condition in tests/test_taa_ref.py and by tests/test_gpu_taa.py."""
import math

import numpy as np

import gbuffer_ref as GR
import lighting_ref as LR
import taa_ref as TR
import visibility_ref as VR
from suite_support import halves_to_words
from toyrenderer_amd import interop as I
from toyrenderer_amd import synth
from toyrenderer_amd import taa as T
from visibility_scenes import consts

F = np.float32
RENDER = (160, 90)
FRAMES = 6
LIGHT = ((0.3, -0.8, -0.52), 3.0)
SETTINGS = dict(min_blend=0.1, max_sample_count=64, jitter=True)
START = (0.0, 0.0, -3.2)                           # from the fixture's camera to the box's opening: geometry on every border of the image
STEP = (0.05, 0.015, -0.04)                        # the eye's translation per frame
YAW_STEP = math.radians(2.5)                       # and its turn about the world's up axis
FIRST = 3                                          # the path's step at frame 0: turned far enough that the walls' edges cross the image


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz)


def camera_at(camera, f):
    """(eye, orientation) of frame f."""
    f += FIRST
    eye = tuple(float(p) + o + f * s for p, o, s in zip(camera.position, START, STEP))
    yaw = (0.0, math.sin(0.5 * f * YAW_STEP), 0.0, math.cos(0.5 * f * YAW_STEP))
    return eye, _quat_mul(yaw, tuple(float(x) for x in camera.orientation))


def view_at(camera, f, render=RENDER):
    """The unjittered View of frame f: prevWorldToView is frame f - 1's (frame 0: its own)."""
    P = synth.perspective_rh_reverse_z_infinite(camera.yfov, render[0] / render[1], camera.znear)
    V = synth.world_to_view(*camera_at(camera, f))
    prev = synth.world_to_view(*camera_at(camera, max(f - 1, 0)))
    return synth.View(V, prev, P, float(np.float32(camera.znear)), *render)


def lighting_consts(view, eye, light=LIGHT):
    """DeferredLightingConsts as FrameDriver fills them for a frame without SSAO, debug view or DDGI."""
    k = np.zeros(1, I.DeferredLightingConsts)
    k["m_ClipToWorld"] = I.clip_to_world(view.worldToView, view.viewToClip)
    k["m_CameraOrigin"] = eye
    k["m_DirectionalLightVector"], k["m_DirectionalLightStrength"] = light
    k["m_LightingOutputResolution"] = (view.renderW, view.renderH)
    return k


def frame_inputs(oracle, vr, gr, lr, sc, geo_v, view, prev_world_to_clip, mats, lk, flags=7):
    """(depth, motion words, LightingOutput words) of one frame under the jittered `view` whose m_PrevWorldToClip is given."""
    W, H = view.renderW, view.renderH
    ref = oracle.frame(sc, view.as_dict(), oracle.HzbTexture(*view.hzb_dims), np.zeros((H, W), F), cullingFlags=flags, record_capacity=4096,
                       raster=(I.world_to_clip(view.worldToView, view.viewToClip), *geo_v))
    k = consts(view)
    k["m_PrevWorldToClip"] = prev_world_to_clip
    geo = VR.Geometry(sc, *geo_v)
    vis, depth = VR.frame_visibility(vr, k, geo, ref, W, H)
    g, m = GR.frame_gbuffer(gr, k, geo, ref, vis, mats, 0)
    motion = halves_to_words(VR.to_half_bits(m))
    return depth, motion, LR.lighting(lr, lk, g, depth, motion=motion)


def leaving(path):
    """Texels whose history position is outside the image in a frame without a reset: no fetch happened."""
    return (path & (TR.VALID | TR.WEIGHTS)) == 0


def check_condition(paths):
    """Every frame after the first has texels with valid history, texels reset by leaving the screen, texels changed by the clamp
    and texels whose dilation moved off-centre, each at least 0.5 % of the image, and fractional bilinear weights."""
    for f, path in enumerate(paths):
        if f == 0:
            assert not np.any(path & (TR.VALID | TR.WEIGHTS)), "the first frame resets"
            continue
        least = 0.005 * path.size
        counts = dict(valid=np.count_nonzero(path & TR.VALID), leaving=np.count_nonzero(leaving(path)), clamped=np.count_nonzero(path & TR.CLAMPED),
                      dilated=np.count_nonzero(path & TR.DILATED), fractional=np.count_nonzero((path & TR.WEIGHTS) == TR.WEIGHTS))
        for name, n in counts.items():
            assert n >= least, (f, name, n, least, counts)
