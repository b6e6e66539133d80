"""Host side of temporal anti-aliasing: the jitter sequence of Graphic::ComputeCurrentJitterOffset (Graphic.cpp:949-998), the
jittered projection of View::Update (Scene.cpp:127-131), the settings and the TAAConsts of "taa_CS_TemporalResolve"
(csrc/k_taa.hip).  One definition for FrameDriver and the tests; csrc/host does the same float operations."""
import dataclasses

import numpy as np

from . import interop as I
from . import rhi
from .rhi import PUSH, SAMPLER, TEX_SRV, TEX_UAV

F = np.float32
PHASE_COUNT = 8                                   # GetJitterPhaseCount: uint(8 * (displayWidth / renderWidth)^2) with render = display
DEFAULTS = dict(min_blend=0.1, max_sample_count=64.0, jitter=True)
TAA_OFF = "temporal anti-aliasing is off (taa=None)"


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


class TemporalAAPass:
    """taa: None (the default) changes nothing.  A dict of settings (needs post=True): min_blend (0.1), max_sample_count (64) and
    jitter (True): temporal anti-aliasing, the place of the reference's TAARenderer (csrc/k_taa.hip, taa.py).  Every record() is
    then one frame of a sequence: the jitter is Graphic::ComputeCurrentJitterOffset's Halton offset of self.frame_counter
    ((0, 0) with jitter=False), the frame's projection is view.viewToClip times the pixel offset matrix (Scene.cpp:127-131), and
    that jittered projection is what the cull, the rasters, the resolve, AO, the shadows, lighting, the sky and the probe draw
    see; m_PrevWorldToClip is the previous record()'s jittered world-to-clip (this frame's on the first record), as
    View::Update keeps it.  One "taa_CS_TemporalResolve" dispatch behind the exposure passes and in front of
    "postprocess_PS_PostProcess" reads LightingOutput, self.depth, self.motion and the history written by the previous
    record(), and writes the other of the two self.taa_history textures (RGBA16_FLOAT) and self.anti_aliased_output
    (R11G11B10_FLOAT), which the post pass then reads in the place of LightingOutput; bloom and the histogram keep reading
    LightingOutput.  The first record() and the one after reset_taa() run with m_bResetHistory = 1.  self.taa_consts holds
    the TAAConsts of the last record(), self.taa_written the index of the history texture it wrote, self.taa_jitter its (current, previous) offsets in pixels, self.taa_view the jittered
    View it rendered with and self.taa_prev_world_to_clip its m_PrevWorldToClip; download_anti_aliased_output() and
    download_taa_history() (the texture written last) read the results back."""
    taa = taa_consts = taa_jitter = taa_view = taa_prev_world_to_clip = taa_history = anti_aliased_output = _taa_last = None
    _taa_reset, taa_written = True, 1

    def _check_taa(self, taa, post):
        if taa is not None:
            if not post:
                raise ValueError("taa=... needs post=True: the post pass is what reads the anti-aliased output")
            self.taa = check_settings(taa)

    def _create_taa(self):                           # TAARenderer::Initialize (TAARenderer.cpp:263-271) + the two histories of the resolve
        dev, W, H = self.dev, self.view.renderW, self.view.renderH
        if self.taa is not None:
            self.taa_history = [self._own(dev.create_texture(W, H, 1, rhi.FORMAT_RGBA16_FLOAT, f"TAA History {i}")) for i in (0, 1)]
            self.anti_aliased_output = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_R11G11B10_FLOAT, "Anti-Aliased Lighting Output"))

    # ---- TAARenderer::Render's place (TAARenderer.cpp:273-275 for the inputs; the resolve is csrc/k_taa.hip) ---------------------
    def _taa_begin(self):
        """The frame's jitter, its jittered View and m_PrevWorldToClip (View::Update, Scene.cpp:113-133)."""
        self.taa_view, self.taa_jitter, self.taa_prev_world_to_clip, self._taa_last = begin_frame(self.view, self.frame_counter, self.taa, self._taa_last)
        return self.taa_view

    def _taa_resolve(self, cl):
        v = self.view
        self.taa_consts = consts(v.renderW, v.renderH, self.taa, *self.taa_jitter, self._taa_reset)
        read, write = self.taa_history[self.taa_written], self.taa_history[1 - self.taa_written]
        cl.dispatch("taa_CS_TemporalResolve",
                    [PUSH(0), TEX_SRV(0, self.lighting_output), TEX_SRV(1, self.depth), TEX_SRV(2, self.motion), TEX_SRV(3, read), TEX_UAV(0, write, 0),
                     TEX_UAV(1, self.anti_aliased_output, 0), SAMPLER(0)], I.groups8(v.renderW, v.renderH), push=self.taa_consts)
        self.taa_written, self._taa_reset = 1 - self.taa_written, False

    def reset_taa(self):
        """The next record() runs the resolve with m_bResetHistory = 1: every texel starts again from its current colour."""
        if self.taa is None:
            raise ValueError("reset_taa: " + TAA_OFF)
        self._taa_reset = True

    def download_anti_aliased_output(self) -> np.ndarray:
        """The words of AntiAliasedLightingOutput, (H, W) uint32."""
        return self._download("download_anti_aliased_output", self.taa, TAA_OFF, lambda: self.anti_aliased_output.download_mip(0))

    def download_taa_history(self) -> np.ndarray:
        """The history texture written last, (H, W, 4) float16: xyz the colour, w the accumulated sample count."""
        return self._download("download_taa_history", self.taa, TAA_OFF, lambda: self.taa_history[self.taa_written].download_mip(0))
