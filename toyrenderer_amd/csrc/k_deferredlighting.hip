// k_deferredlighting.hip -- "deferredlighting_PS_Main" and "deferredlighting_PS_Main_Debug": the reference's full-screen pass
// after GBufferRenderer (source/DeferredLightingRenderer.cpp, source/shaders/deferredlighting.hlsl; EvaluateDirectionalLight,
// DefaultLitBxDF and UnpackGBuffer of lightingcommon.hlsli), WITHOUT DDGI and with the shadow mask as an input: the directional
// light and the debug views, closed arithmetic on GBufferA, depth, the motion target, the SSAO and the shadow-mask texels.
// DDGI ambient is out of scope; the sky is k_sky.hip's, the SSAO texture k_ambientocclusion.hip's, the shadow mask
// k_shadowmask.hip's.
//
// WHICH PIXELS: the reference draws where the stencil equals the opaque bit.  The stand-in: a pixel is written iff its depth
// word is > 0.0f (NaN, +-0 and negative depths are skipped); every other texel of u0 keeps what it held.
//
// CONVENTION (parity unpinned; restated in tests/lighting_ref.c and DESIGN.md 3).  The shared part (binary32 rules, saturate, lerp,
// dot3, inUV, UVToClipXY, worldPosition) is stated in screen_pass.hip.h.  Here:
//   normalize(v) = v / sqrt(dot3(v, v)); rcp(x) = 1.0f / x;
//   UnpackGBuffer: RGBA8 (float)byte * (1.0f / 255.0f), unorm16 (float)u * (1.0f / 65535.0f), one multiply by the rounded
//             constant each; UnpackOctadehron f = f * 2 - 1, z = (1 - |fx|) - |fy|, t = saturate(-z), x += (x >= 0 ? -t : t),
//             y likewise, then normalize; UnpackR9G9B9E5 ldexp(mantissa, E - 24), exact;
//   PS_Main: ComputeDiffuseColor albedo * (1 - metallic); ComputeF0 lerp(0.08f * 0.5f, albedo, metallic); V = normalize(origin -
//             worldPosition), L = the light vector as given (not normalised), H = normalize(V + L); NdotV = saturate(|N.V| + 1e-5f),
//             NdotL, NdotH, VdotH saturated; a = r * r, a2 = fmin(fmax(a * a, 0.0001f), 1); D_GGX a2 / ((pi * d) * d) with
//             d = (NdotH * a2 - NdotH) * NdotH + 1; Vis_SmithJointApprox 0.5f * rcp(NdotL * (NdotV * (1 - a2) + a2) +
//             NdotV * (NdotL * (1 - a2) + a2)); F_Schlick Fc + (1 - Fc) * f0, Fc = ((x * x) * (x * x)) * x, x = 1 - VdotH;
//             specular = (D * Vis) * F + EnvBRDFApprox; rgb = (((diffuse * (1 / pi) + specular) * NdotL) * lightStrength) * shadow
//             + emissive; shadow = (float)byte / 255.0f of the R8_UNORM texel at the pixel (a point sample at inUV at equal
//             resolution; unbound: 1.0f);
//   EnvBRDFApprox: r4 = r * (-1, -0.0275f, -0.572f, 0.022f) + (1, 0.0425f, 1.04f, -0.04f); a004 = fmin(r4.x * r4.x,
//             exp2(-9.28f * NdotV)) * r4.x + r4.y; AB = (-1.04f, 1.04f) * a004 + r4.zw; f0 * AB.x + AB.y;
//   exp2:     v_exp_f32 is good to 1 ulp only and cannot be restated on a CPU, so it is software, for x <= 0: i = ceil(x),
//             f = x - i in (-1, 0], a degree-7 Horner polynomial in fma, then ldexp(p, i).  ceil, not floor: with floor f = x + 1
//             is inexact for -1 < x < 0; with ceil f is exact everywhere (|x| < 1: f = x; else x and i are multiples of ulp(x)
//             and |f| < 1).  Coefficients and the error analysis (truncation 0.112 * 2^-25, Horner 2.3304 * 2^-25, bound
//             2.46 * 2^-25 times 2^i) are in tests/lighting_ref.c next to the same numbers; measured maximum in DESIGN.md 9;
//   PS_Main_Debug: shadowFactor = fmax(0.05f, shadow); mode 1 dot3(N, L) * shadowFactor (may be negative: stored as 0); 2, 3
//             seed = uint(debugValue * 255.0f), three successive QuickRandomFloat; 4 albedo; 5 normal; 6 emissive; 7 metallic;
//             8 roughness; 9 (float)ssao / 255.0f (unbound: 255); 11 shadowFactor; 12 kLODColors[uint(debugValue * 255.0f)], an
//             index >= 8 gives (0, 0, 0) (the reference reads past its table there); 13 (motion.x / (float)W, motion.y / (float)H,
//             0); any other mode (0, 0, 0).  Mode 10 (Ambient) needs the DDGI volume and is refused at record time;
//   store:    R11G11B10_FLOAT as in r11g11b10.hip.h; alpha is dropped.
//
// KERNEL: one thread per pixel, no LDS.  The depth word is read first and a skipped pixel ends there (sky costs 4 B); a lit
// pixel then reads GBufferA in one 16-byte load and the shadow byte, and stores 4 B: about 25 B against 17 correctly rounded
// divisions and 3 square roots, so the arithmetic is the cost, as in k_gbuffer.hip.  The tile is screen_pass.hip.h's.
//
// MEASURED (tools/lighting_cost.py, generated city of 2251 instances at 3840x2160, 8.29 M lit pixels, shadow mask bound, builds
// alternated three times on one MI355X; profiles/lighting/): this kernel 103.0 us (spread 0.5), 99.4 us in a kernel trace of its
// own; its 207 MB alone would stream in 32.0 us at the box's 6.48 TB/s, and a build that only loads and stores takes 38.5 us.  A
// build with approximate division and square root takes 56.0 us: the correctly rounded operations, which the bit-exact bar needs,
// are 47 us of the 64 us of arithmetic.  The 16 x 4 wave mapping (TR_LIGHTING_TILE_W=16) measures 102.9 us, equal within the
// spread, so the 64 x 1 row stays.  The debug entry in view 4: 47.6 us.  Code object: PS_Main 27 VGPRs, _Debug 22 VGPRs, 8 waves
// per SIMD, no scratch, no LDS (-Rpass-analysis=kernel-resource-usage).
#include "cull_math.hip.h"
#include "gbuffer_unpack.hip.h"
#include "r11g11b10.hip.h"
#include "screen_pass.hip.h"

namespace
{

using namespace interop;
using namespace gbuf;

#ifndef TR_LIGHTING_TILE_W
#define TR_LIGHTING_TILE_W sp::kTileW          // the shared tile; 16 gives the G-buffer resolve's 16 x 4 wave (tools/lighting_cost.py measures both)
#endif
constexpr uint32_t kTileW = TR_LIGHTING_TILE_W, kTileH = sp::kBlock / kTileW;
static_assert(kTileW * kTileH == sp::kBlock && (kTileW == sp::kTileW || kTileW == 16), "tile shape");

struct LightingArgs
{
    DeferredLightingConsts k;
    const uint4* gbufferA;                     // RGBA32_UINT
    const uint32_t* motion;                    // RG16_FLOAT (debug only)
    const float* depth;                        // R32_FLOAT
    const uint8_t* ssao;                       // R8_UINT or nullptr (255)
    const uint8_t* shadow;                     // R8_UNORM or nullptr (1.0)
    uint32_t* out;                             // R11G11B10_FLOAT
};

// exp2 for x <= 0; coefficients and error analysis: tests/lighting_ref.c (kExp2C)
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

__device__ __forceinline__ float quickRandomFloat(uint32_t& seed)                                  // random.hlsli:7-11
{
    seed = 1664525u * seed + 1013904223u;
    return (float)(seed & 0x00FFFFFFu) / 16777216.0f;
}

__device__ __forceinline__ cm::F3 litPixel(const LightingArgs& a, const GBufferParams& p, uint32_t px, uint32_t py, float depth, float shadow)
{
    const DeferredLightingConsts& k = a.k;
    const cm::F3 world = sp::worldPosition(k.m_ClipToWorld, px, py, k.m_LightingOutputResolution.x, k.m_LightingOutputResolution.y, depth);
    const float oneMinusMetal = 1.0f - p.metallic, dielectric = 0.08f * 0.5f;
    const cm::F3 diffuse = { p.albedo.x * oneMinusMetal, p.albedo.y * oneMinusMetal, p.albedo.z * oneMinusMetal };
    const cm::F3 f0 = { dielectric + p.metallic * (p.albedo.x - dielectric), dielectric + p.metallic * (p.albedo.y - dielectric), dielectric + p.metallic * (p.albedo.z - dielectric) };
    const cm::F3 V = normalize_({ k.m_CameraOrigin[0] - world.x, k.m_CameraOrigin[1] - world.y, k.m_CameraOrigin[2] - world.z });
    const cm::F3 L = { k.m_DirectionalLightVector[0], k.m_DirectionalLightVector[1], k.m_DirectionalLightVector[2] };
    const cm::F3 H = normalize_({ V.x + L.x, V.y + L.y, V.z + L.z });
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
    const float strength = k.m_DirectionalLightStrength, kInvPi = 0x1.45f306p-2f;
    auto channel = [&](float diff, float f0c, float emissive) {
        const float F = Fc + (1.0f - Fc) * f0c;
        const float spec = DVis * F + (f0c * A + B);
        return (((diff * kInvPi + spec) * NdotL) * strength) * shadow + emissive;
    };
    return { channel(diffuse.x, f0.x, p.emissive.x), channel(diffuse.y, f0.y, p.emissive.y), channel(diffuse.z, f0.z, p.emissive.z) };
}

__device__ __forceinline__ cm::F3 debugPixel(const LightingArgs& a, const GBufferParams& p, uint64_t i, float shadow)
{
    const DeferredLightingConsts& k = a.k;
    const float shadowFactor = cm::max_(0.05f, shadow);
    switch (k.m_DebugMode) {
    case kDeferredLightingDebugMode_LightingOnly: {
        const float v = cm::dot3(p.normal, { k.m_DirectionalLightVector[0], k.m_DirectionalLightVector[1], k.m_DirectionalLightVector[2] }) * shadowFactor;
        return { v, v, v }; }
    case kDeferredLightingDebugMode_ColorizeInstances: case kDeferredLightingDebugMode_ColorizeMeshlets: {
        uint32_t seed = (uint32_t)(p.debugValue * 255.0f);
        const float r = quickRandomFloat(seed), g = quickRandomFloat(seed), b = quickRandomFloat(seed);
        return { r, g, b }; }
    case kDeferredLightingDebugMode_Albedo: return p.albedo;
    case kDeferredLightingDebugMode_Normal: return p.normal;
    case kDeferredLightingDebugMode_Emissive: return p.emissive;
    case kDeferredLightingDebugMode_Metalness: return { p.metallic, p.metallic, p.metallic };
    case kDeferredLightingDebugMode_Roughness: return { p.roughness, p.roughness, p.roughness };
    case kDeferredLightingDebugMode_AmbientOcclusion: {
        const float v = cm::div_((float)(a.ssao ? (uint32_t)a.ssao[i] : 255u), 255.0f);
        return { v, v, v }; }
    case kDeferredLightingDebugMode_ShadowMask: return { shadowFactor, shadowFactor, shadowFactor };
    case kDeferredLightingDebugMode_MeshLOD: {
        const uint32_t lod = (uint32_t)(p.debugValue * 255.0f);                                     // kLODColors, restated: LOD 0 red .. LOD 7 purple
        if (lod >= 8u) return { 0.0f, 0.0f, 0.0f };
        const float r = lod <= 2u ? 1.0f : (lod == 3u || lod == 7u) ? 0.5f : 0.0f;
        const float g = (lod >= 2u && lod <= 4u) ? 1.0f : (lod == 1u || lod == 5u) ? 0.5f : 0.0f;
        const float b = lod >= 5u ? 1.0f : 0.0f;
        return { r, g, b }; }
    case kDeferredLightingDebugMode_MotionVectors: {
        const uint32_t m = a.motion[i];
        return { cm::div_((float)sp::halfOf(m), (float)k.m_LightingOutputResolution.x), cm::div_((float)sp::halfOf(m >> 16), (float)k.m_LightingOutputResolution.y), 0.0f }; }
    default: return { 0.0f, 0.0f, 0.0f };
    }
}

template <bool DEBUG>
__global__ __launch_bounds__(sp::kBlock) void lightingKernel(LightingArgs a)
{
    const uint32_t W = a.k.m_LightingOutputResolution.x, H = a.k.m_LightingOutputResolution.y;
    const sp::Pixel at = sp::pixel<kTileW, kTileH>();
    if (!at.inside(W, H)) return;
    const uint64_t i = at.index(W);
    const float depth = a.depth[i];
    if (!(depth > 0.0f)) return;                                                                   // the stencil stand-in: sky costs 4 B
    const uint4 g = a.gbufferA[i];
    const float shadow = a.shadow ? cm::div_((float)a.shadow[i], 255.0f) : 1.0f;
#ifdef TR_LIGHTING_EXPERIMENT_STORE_ONLY        // attribution only (profiles/lighting/): the pass's bytes without its arithmetic
    a.out[i] = g.x ^ g.y ^ g.z ^ g.w ^ __builtin_bit_cast(uint32_t, shadow);
#else
    const GBufferParams p = unpackGBuffer(g);
    const cm::F3 rgb = DEBUG ? debugPixel(a, p, i, shadow) : litPixel(a, p, at.x, at.y, depth, shadow);
#ifdef TR_LIGHTING_EXPERIMENT_TRUNC_STORE       // negative control only (profiles/lighting/): truncation instead of round to nearest even
    auto trunc = [](float v, uint32_t mbits) {
        const uint32_t u = __builtin_bit_cast(uint32_t, v), top = (31u << mbits) - 1u;
        if (u >> 31 || u < 0x38800000u) return 0u;
        const uint32_t q = (u - (112u << 23)) >> (23u - mbits);
        return q < top ? q : top; };
    a.out[i] = trunc(rgb.x, 6) | trunc(rgb.y, 6) << 11 | trunc(rgb.z, 5) << 22;
#else
    a.out[i] = trhip::packR11G11B10(rgb.x, rgb.y, rgb.z);
#endif
#endif
}

// Records either entry: validates the bindings and emits one direct dispatch.
template <bool DEBUG>
int recordLighting(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const DeferredLightingConsts* k = (const DeferredLightingConsts*)ctx.constants(0, sizeof(DeferredLightingConsts));
    TRHIP_REQUIRE(k, "%s: constant buffer b0 (DeferredLightingConsts, 112 bytes) missing", name);
    TRHIP_REQUIRE(!k->m_bRTDDGIEnabled, "%s: m_bRTDDGIEnabled is set: DDGI ambient is not built", name);
    TRHIP_REQUIRE(k->m_DebugMode != kDeferredLightingDebugMode_Ambient, "%s: m_DebugMode 10 (Ambient) needs the DDGI volume, which is not built", name);
    const uint32_t W = k->m_LightingOutputResolution.x, H = k->m_LightingOutputResolution.y;
    TRHIP_REQUIRE(W && H, "%s: m_LightingOutputResolution %ux%u is empty", name, W, H);
    if (const int rc = sp::requireCover(ctx, sp::kGroupSide, sp::kGroupSide, W, H)) return rc;
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_RGBA32_UINT, "Texture_SRV t0 = the RGBA32_UINT GBufferA", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 1, TRHIP_FORMAT_RG16_FLOAT, "Texture_SRV t1 = the RG16_FLOAT GBufferMotion", DEBUG, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 2, TRHIP_FORMAT_R32_FLOAT, "Texture_SRV t2 = the R32_FLOAT depth buffer", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 3, TRHIP_FORMAT_R8_UINT, "Texture_SRV t3 = the R8_UINT SSAO texture", false, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 4, TRHIP_FORMAT_R8_UNORM, "Texture_SRV t4 = the R8_UNORM shadow mask", false, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_R11G11B10_FLOAT, "Texture_UAV u0 = the R11G11B10_FLOAT LightingOutput, mip 0", true, sp::kOneMipAt0 } };
    trhip_texture_t* tex[6];
    if (const int rc = sp::bindTextures(ctx, want, tex, W, H, "m_LightingOutputResolution")) return rc;
    LightingArgs a = sp::zeroed<LightingArgs>();
    a.k = *k;
    a.gbufferA = (const uint4*)tex[0]->ptr;
    a.motion = tex[1] ? (const uint32_t*)tex[1]->ptr : nullptr;
    a.depth = (const float*)tex[2]->ptr;
    a.ssao = tex[3] ? (const uint8_t*)tex[3]->ptr : nullptr;
    a.shadow = tex[4] ? (const uint8_t*)tex[4]->ptr : nullptr;
    a.out = (uint32_t*)tex[5]->ptr;
    sp::launch(ctx, lightingKernel<DEBUG>, DEBUG ? "lightingKernel<debug>" : "lightingKernel<lit>", sp::tiles(W, H, kTileW, kTileH), dim3(kTileW, kTileH), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("deferredlighting_PS_Main", recordLighting<false>, 0);
trhip::ShaderRegistrar r1("deferredlighting_PS_Main_Debug", recordLighting<true>, 0);

} // namespace
