"""Host side of the ambient occlusion pass (AmbientOcclusionRenderer.cpp, extern/xegtao/XeGTAO.h): the settings, GTAOUpdateConstants
and the push constants of "ambientocclusion_CS_XeGTAO_*" (csrc/k_ambientocclusion.hip).  Every operation is a float32 operation in
the reference's order, so that this file and csrc/host/AmbientOcclusionRenderer.cpp hand the GPU the same 96 bytes."""
from __future__ import annotations

import numpy as np

from . import interop as I

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
