// direct_light.hip.h -- EvaluateDirectionalLight with DefaultLitBxDF (lightingcommon.hlsli) for the passes that light a surface
// point from the directional light: the lighting pass (k_deferredlighting.hip, which states the convention: "PS_Main",
// "EnvBRDFApprox" and "exp2" there) with the camera as viewer, and the probe trace (k_giprobetrace.hip) with the probe as viewer.
// tests/lighting_ref.c restates it word for word (lr_lit).
#pragma once

#include "cull_math.hip.h"
#include "gbuffer_unpack.hip.h"
#include "screen_pass.hip.h"

namespace dl
{

// exp2 for x <= 0; coefficients and error analysis: tests/lighting_ref.c (kExp2CeilC)
__device__ __forceinline__ float exp2Soft(float x)
{
#ifdef TR_LIGHTING_EXPERIMENT_HW_EXP2          // negative control only (profiles/lighting/): the hardware's v_exp_f32
    return __builtin_amdgcn_exp2f(x);
#else
    const float i = __builtin_ceilf(x), f = x - i;
    float p = 0x1.7b4b46p-17f;
    p = cm::fma_(p, f, 0x1.383ffcp-13f);
    p = cm::fma_(p, f, 0x1.5ca2c2p-10f);
    p = cm::fma_(p, f, 0x1.3b20d4p-7f);
    p = cm::fma_(p, f, 0x1.c6b024p-5f);
    p = cm::fma_(p, f, 0x1.ebfbdep-3f);
    p = cm::fma_(p, f, 0x1.62e430p-1f);
    p = cm::fma_(p, f, 1.0f);
    return __builtin_ldexpf(p, (int)i);
#endif
}

// The surface `p` at `world` seen from `viewer`, lit along L (as given, not normalised) with `strength`, times `shadow`, plus the
// surface's emissive.
__device__ __forceinline__ cm::F3 litSurface(const gbuf::GBufferParams& p, cm::F3 viewer, cm::F3 world, cm::F3 L, float strength, float shadow)
{
    const float oneMinusMetal = 1.0f - p.metallic, dielectric = 0.08f * 0.5f;
    const cm::F3 diffuse = { p.albedo.x * oneMinusMetal, p.albedo.y * oneMinusMetal, p.albedo.z * oneMinusMetal };
    const cm::F3 f0 = { dielectric + p.metallic * (p.albedo.x - dielectric), dielectric + p.metallic * (p.albedo.y - dielectric), dielectric + p.metallic * (p.albedo.z - dielectric) };
    const cm::F3 V = gbuf::normalize_({ viewer.x - world.x, viewer.y - world.y, viewer.z - world.z });
    const cm::F3 H = gbuf::normalize_({ V.x + L.x, V.y + L.y, V.z + L.z });
    const float NdotV = sp::saturate_(__builtin_fabsf(cm::dot3(p.normal, V)) + 1e-5f), NdotL = sp::saturate_(cm::dot3(p.normal, L));
    const float NdotH = sp::saturate_(cm::dot3(p.normal, H)), VdotH = sp::saturate_(cm::dot3(V, H));
    const float al = p.roughness * p.roughness, a2 = cm::min_(cm::max_(al * al, 0.0001f), 1.0f);
    const float d = (NdotH * a2 - NdotH) * NdotH + 1.0f;                                            // D_GGX
    const float D = cm::div_(a2, (0x1.921fb6p+1f * d) * d);
    const float smithV = NdotL * (NdotV * (1.0f - a2) + a2), smithL = NdotV * (NdotL * (1.0f - a2) + a2);   // Vis_SmithJointApprox
    const float Vis = 0.5f * cm::div_(1.0f, smithV + smithL);
    const float x = 1.0f - VdotH, xx = x * x, Fc = (xx * xx) * x;                                   // F_Schlick
    const float DVis = D * Vis;
    const float r = p.roughness;                                                                    // EnvBRDFApprox
    const float rx = r * -1.0f + 1.0f, ry = r * -0.0275f + 0.0425f, rz = r * -0.572f + 1.04f, rw = r * 0.022f + -0.04f;
    const float a004 = cm::min_(rx * rx, exp2Soft(-9.28f * NdotV)) * rx + ry;
    const float A = -1.04f * a004 + rz, B = 1.04f * a004 + rw;
    const float kInvPi = 0x1.45f306p-2f;
    auto channel = [&](float diff, float f0c, float emissive) {
        const float F = Fc + (1.0f - Fc) * f0c;
        const float spec = DVis * F + (f0c * A + B);
        return (((diff * kInvPi + spec) * NdotL) * strength) * shadow + emissive;
    };
    return { channel(diffuse.x, f0.x, p.emissive.x), channel(diffuse.y, f0.y, p.emissive.y), channel(diffuse.z, f0.z, p.emissive.z) };
}

} // namespace dl
