"""Host side of temporal anti-aliasing: the jitter sequence of Graphic::ComputeCurrentJitterOffset (Graphic.cpp:949-998), the
jittered projection of View::Update (Scene.cpp:127-131), the settings and the TAAConsts of "taa_CS_TemporalResolve"
(csrc/k_taa.hip).  One definition for FrameDriver and the tests; csrc/host does the same float operations."""
import dataclasses

import numpy as np

from . import interop as I

F = np.float32
PHASE_COUNT = 8                                   # GetJitterPhaseCount: uint(8 * (displayWidth / renderWidth)^2) with render = display
DEFAULTS = dict(min_blend=0.1, max_sample_count=64.0, jitter=True)


def check_settings(s) -> dict:
    unknown = set(s) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"taa: unknown settings {sorted(unknown)}; known: {sorted(DEFAULTS)}")
    out = dict(min_blend=float(s.get("min_blend", DEFAULTS["min_blend"])), max_sample_count=float(s.get("max_sample_count", DEFAULTS["max_sample_count"])),
               jitter=bool(s.get("jitter", DEFAULTS["jitter"])))
    if not (0.0 <= out["min_blend"] <= 1.0):
        raise ValueError(f"taa: min_blend = {out['min_blend']} is outside [0, 1]")
    if not (1.0 <= out["max_sample_count"] <= 65504.0):
        raise ValueError(f"taa: max_sample_count = {out['max_sample_count']} is outside [1, 65504]: the count is stored as a binary16")
    return out


def van_der_corput(base: int, index: int) -> np.float32:
    """Graphic.cpp:980-992, in float as written."""
    ret, denominator = F(0.0), F(base)
    while index > 0:
        ret = F(ret + F(F(index % base) / denominator))
        index //= base
        denominator = F(denominator * F(base))
    return ret


def jitter_offset(frame_counter: int):
    """The Halton branch of Graphic::ComputeCurrentJitterOffset: (x, y) in [-0.5, 0.5), in pixels."""
    index = int(frame_counter) % PHASE_COUNT + 1
    return F(van_der_corput(2, index) - F(0.5)), F(van_der_corput(3, index) - F(0.5))


def jittered_view_to_clip(view_to_clip, jitter, W: int, H: int) -> np.ndarray:
    """m_ViewToClip *= CreateTranslation(2 jx / W, -2 jy / H, 0) (Scene.cpp:127-131), with interop.world_to_clip's float32 product."""
    T = np.eye(4, dtype=F)
    T[3, 0] = F(F(F(2.0) * F(jitter[0])) / F(W))
    T[3, 1] = F(F(F(-2.0) * F(jitter[1])) / F(H))
    return I.world_to_clip(view_to_clip, T)


def begin_frame(view, frame_counter: int, settings: dict, last):
    """View::Update for one frame of a sequence (Scene.cpp:113-133).  last: what the previous frame returned as its fourth value, or
    None on the first frame.  Returns (the jittered View, (current, previous) jitter in pixels, m_PrevWorldToClip, last for the
    next frame).  On the first frame the previous jitter and m_PrevWorldToClip are this frame's."""
    current = jitter_offset(frame_counter) if settings["jitter"] else (F(0.0), F(0.0))
    jittered = dataclasses.replace(view, viewToClip=jittered_view_to_clip(view.viewToClip, current, view.renderW, view.renderH))
    world_to_clip = I.world_to_clip(jittered.worldToView, jittered.viewToClip)
    previous, prev_world_to_clip = last if last is not None else (current, world_to_clip)
    return jittered, (current, previous), prev_world_to_clip, (current, world_to_clip)


def jitter_delta(current, previous):
    """m_JitterDelta: the previous minus the current jitter offset in pixels, in binary32 (TAAConsts and SigmaConsts carry it)."""
    return (F(F(previous[0]) - F(current[0])), F(F(previous[1]) - F(current[1])))


def consts(W: int, H: int, settings: dict, current, previous, reset: bool) -> np.ndarray:
    k = np.zeros(1, I.TAAConsts)
    k["m_OutputDims"] = (W, H)
    k["m_JitterDelta"] = jitter_delta(current, previous)
    k["m_MinBlend"] = settings["min_blend"]
    k["m_MaxSampleCount"] = settings["max_sample_count"]
    k["m_bResetHistory"] = int(bool(reset))
    return k
