"""Host side of the ambient occlusion pass (AmbientOcclusionRenderer.cpp, extern/xegtao/XeGTAO.h): the settings, GTAOUpdateConstants
and the push constants of "ambientocclusion_CS_XeGTAO_*" (csrc/k_ambientocclusion.hip).  Every operation is a float32 operation in
the reference's order, so that this file and csrc/host/AmbientOcclusionRenderer.cpp hand the GPU the same 96 bytes."""
from __future__ import annotations

import numpy as np

from . import interop as I
from . import rhi
from .rhi import CB, PUSH, SAMPLER, TEX_SRV, TEX_UAV

F = np.float32
# AmbientOcclusionRenderer::Initialize sets quality 3 (Ultra) and 3 denoise passes; the rest are GTAOSettings' defaults
DEFAULTS = dict(quality=3, denoise_passes=3, radius=0.5, falloff_range=0.615, final_value_power=2.2, depth_mip_sampling_offset=3.3)
RADIUS_MULTIPLIER, SAMPLE_DISTRIBUTION_POWER, THIN_OCCLUDER_COMPENSATION = F(1.457), F(2.0), F(0.0)    # carried, compiled in by the passes
DEPTH_MIP_LEVELS = 5
QUALITY = ((1, 2), (2, 2), (3, 3), (9, 2))          # (slices, steps per slice) of Low, Medium, High, Ultra


def check_settings(ao) -> dict:
    """The dict FrameDriver(ao=...) takes, completed with DEFAULTS; ValueError for a bad one."""
    if not isinstance(ao, dict):
        raise ValueError("ao: needs a dict of settings (quality, denoise_passes, radius, falloff_range, final_value_power, depth_mip_sampling_offset)")
    unknown = set(ao) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"ao: unknown settings {sorted(unknown)}")
    s = {**DEFAULTS, **ao}
    for key in ("quality", "denoise_passes"):
        if isinstance(s[key], bool) or int(s[key]) != s[key] or not 0 <= int(s[key]) <= 3:
            raise ValueError(f"ao: {key} = {s[key]!r}: needs an integer in 0..3")
        s[key] = int(s[key])
    if not (np.isfinite(s["radius"]) and s["radius"] >= 0.0):
        raise ValueError(f"ao: radius = {s['radius']!r}: needs a finite radius >= 0")
    for key in ("falloff_range", "final_value_power", "depth_mip_sampling_offset"):
        if not np.isfinite(s[key]):
            raise ValueError(f"ao: {key} = {s[key]!r}: needs a finite value")
    return s


def update_constants(width: int, height: int, settings: dict, view_to_clip, frame_counter: int) -> np.ndarray:
    """XeGTAO::GTAOUpdateConstants (XeGTAO.h:164-198) with rowMajor = true; frame_counter is what the renderer passes,
    g_Graphic.m_FrameCounter % 256."""
    P = np.asarray(view_to_clip, F).reshape(4, 4)
    k = np.zeros(1, I.GTAOConstants)
    px, py = F(1.0) / F(width), F(1.0) / F(height)
    k["ViewportSize"] = (width, height)
    k["ViewportPixelSize"] = (px, py)
    mul, add = F(-P[3, 2]), F(P[2, 2])
    if F(mul * add) < 0:                              # the handedness flip
        add = F(-add)
    k["DepthUnpackConsts"] = (mul, add)
    with np.errstate(all="ignore"):
        tan_y, tan_x = F(1.0) / P[1, 1], F(1.0) / P[0, 0]
    k["CameraTanHalfFOV"] = (tan_x, tan_y)
    ndc_mul = (F(tan_x * F(2.0)), F(tan_y * F(-2.0)))
    k["NDCToViewMul"] = ndc_mul
    k["NDCToViewAdd"] = (F(tan_x * F(-1.0)), F(tan_y * F(1.0)))
    k["NDCToViewMul_x_PixelSize"] = (F(ndc_mul[0] * px), F(ndc_mul[1] * py))
    k["EffectRadius"] = F(settings["radius"])
    k["EffectFalloffRange"] = F(settings["falloff_range"])
    k["DenoiseBlurBeta"] = F(1e4) if settings["denoise_passes"] == 0 else F(1.2)
    k["RadiusMultiplier"] = RADIUS_MULTIPLIER
    k["SampleDistributionPower"] = SAMPLE_DISTRIBUTION_POWER
    k["ThinOccluderCompensation"] = THIN_OCCLUDER_COMPENSATION
    k["FinalValuePower"] = F(settings["final_value_power"])
    k["DepthMIPSamplingOffset"] = F(settings["depth_mip_sampling_offset"])
    k["NoiseIndex"] = int(frame_counter) % 64 if settings["denoise_passes"] > 0 else 0
    return k


def main_pass_constants(world_to_view, quality: int) -> np.ndarray:
    """XeGTAOMainPassConstantBuffer: m_WorldToView with its translation row zeroed, and the quality level."""
    k = np.zeros(1, I.XeGTAOMainPassConstantBuffer)
    m = np.array(world_to_view, F).reshape(4, 4)
    m[3, :3] = 0.0
    k["m_WorldToViewNoTranslate"] = m
    k["m_Quality"] = quality
    return k


def denoise_constants(final_apply: bool) -> np.ndarray:
    k = np.zeros(1, I.XeGTAODenoiseConstants)
    k["m_FinalApply"] = int(final_apply)
    return k


class AmbientOcclusionPass:
    """ao: None (the default) changes nothing.  A dict of settings, any of quality (0..3: Low, Medium, High, Ultra), denoise_passes
    (0..3), radius, falloff_range, final_value_power, depth_mip_sampling_offset (the reference's defaults: 3, 3, 0.5, 0.615, 2.2,
    3.3; needs gbuffer=True, which lighting implies; not together with an external ssao=): AmbientOcclusionRenderer
    (AmbientOcclusionRenderer.cpp, XeGTAO).  The driver owns the working depth chain (R16_FLOAT, 5 mips), the working AO term
    (R8_UINT), the edges (R8_UNORM) and self.ssao_texture (R8_UINT); after the G-buffer resolve and in front of the lighting
    dispatch it records "ambientocclusion_CS_XeGTAO_PrefilterDepths", "ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0"
    and max(1, denoise_passes) "ambientocclusion_CS_XeGTAO_Denoise" dispatches ping-ponging between the working term and
    self.ssao_texture, the last with m_FinalApply = 1; as in the reference, with 2 passes the finally-applied image lands in
    the working term and self.ssao_texture holds the first pass's output.  With lighting the texture is the lighting pass's
    t3 and m_SSAOEnabled is 1; debug view 9 shows it, and the non-debug pass multiplies the DDGI ambient term by it: with
    ddgi= the texture changes LightingOutput, without it (no ambient term) it does not.  self.frame_counter (0; the caller may set it
    before record()) feeds NoiseIndex as g_Graphic.m_FrameCounter % 256 does; self.gtao_consts holds the 96-byte GTAOConstants
    of the last record(); download_ssao() reads self.ssao_texture back."""
    ao = gtao_consts = ao_depth = ao_working = ao_edges = ssao_texture = None

    def _check_ao(self, ao, gbuffer, ssao):
        if ao is not None:
            if not gbuffer:
                raise ValueError("ao=... needs gbuffer=True (or lighting=True): the main pass reads the normals of GBufferA")
            if ssao is not None:
                raise ValueError("ao=... together with an external ssao= texture: the driver generates the texture itself")
            self.ao = check_settings(ao)

    def _create_ao(self):                            # AmbientOcclusionRenderer::Setup (AmbientOcclusionRenderer.cpp:85-127)
        dev, W, H = self.dev, self.view.renderW, self.view.renderH
        if self.ao is not None:
            self.ao_depth = self._own(dev.create_texture(W, H, DEPTH_MIP_LEVELS, rhi.FORMAT_R16_FLOAT, "XeGTAO Working Depth Buffer"))
            self.ssao_texture = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_R8_UINT, "SSAO Buffer"))
            self.ao_working = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_R8_UINT, "Working SSAO Texture"))
            self.ao_edges = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_R8_UNORM, "Working Edges Texture"))
            self.ssao = self.ssao_texture            # what the lighting pass binds as t3

    # ---- AmbientOcclusionRenderer::Render (AmbientOcclusionRenderer.cpp:129-248) ------------------------------------------
    def _ambient_occlusion(self, cl):
        v, W, H = self.view, self.view.renderW, self.view.renderH
        self.gtao_consts = update_constants(W, H, self.ao, v.viewToClip, int(self.frame_counter) % 256)
        cb = cl.constant_buffer(self.gtao_consts, "GTAOConstants")
        cl.dispatch("ambientocclusion_CS_XeGTAO_PrefilterDepths",
                    [CB(0, cb), TEX_SRV(0, self.depth), *[TEX_UAV(m, self.ao_depth, m) for m in range(DEPTH_MIP_LEVELS)], SAMPLER(0)],
                    ((W + 15) // 16, (H + 15) // 16, 1))
        cl.dispatch("ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0",
                    [CB(0, cb), PUSH(1), TEX_SRV(0, self.ao_depth), TEX_SRV(2, self.gbufferA), TEX_UAV(0, self.ao_working, 0), TEX_UAV(1, self.ao_edges, 0), SAMPLER(0)],
                    I.groups8(W, H), push=main_pass_constants(v.worldToView, self.ao["quality"]))
        ping_pong = [self.ao_working, self.ssao_texture]
        passes = max(1, self.ao["denoise_passes"])   # without denoising one last pass still writes the term into the output texture
        for i in range(passes):
            cl.dispatch("ambientocclusion_CS_XeGTAO_Denoise",
                        [CB(0, cb), PUSH(1), TEX_SRV(0, ping_pong[0]), TEX_SRV(1, self.ao_edges), TEX_UAV(0, ping_pong[1], 0), SAMPLER(0)],
                        ((W + 15) // 16, (H + 7) // 8, 1), push=denoise_constants(i == passes - 1))
            ping_pong.reverse()

    def download_ssao(self) -> np.ndarray:
        """The bytes of the generated SSAO texture, (H, W) uint8."""
        return self._download("download_ssao", self.ssao_texture, "AO generation is off (ao=None)", lambda: self.ssao_texture.download_mip(0))
