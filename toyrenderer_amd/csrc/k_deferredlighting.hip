// k_deferredlighting.hip -- "deferredlighting_PS_Main" and "deferredlighting_PS_Main_Debug": the reference's full-screen pass
// after GBufferRenderer (source/DeferredLightingRenderer.cpp, source/shaders/deferredlighting.hlsl; EvaluateDirectionalLight,
// DefaultLitBxDF and UnpackGBuffer of lightingcommon.hlsli), with the shadow mask and the DDGI probe volume as inputs: the
// directional light, the DDGI ambient term and the debug views, closed arithmetic on GBufferA, depth, the motion target, the SSAO
// and the shadow-mask texels, plus the probe lookups of ddgi_irradiance.hip.h.  The volume is an input here: supplied, or filled
// by k_giprobetrace.hip and k_giprobeblend.hip in front of this pass.  The sky is k_sky.hip's, the SSAO texture k_ambientocclusion.hip's, the shadow mask
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
//   (PS_Main's directional light, EnvBRDFApprox and exp2 below are written in direct_light.hip.h, which the probe trace shares.)
//   exp2:     v_exp_f32 is good to 1 ulp only and cannot be restated on a CPU, so it is software, for x <= 0: i = ceil(x),
//             f = x - i in (-1, 0], a degree-7 Horner polynomial in fma, then ldexp(p, i).  ceil, not floor: with floor f = x + 1
//             is inexact for -1 < x < 0; with ceil f is exact everywhere (|x| < 1: f = x; else x and i are multiples of ulp(x)
//             and |f| < 1).  Coefficients and the error analysis (truncation 0.112 * 2^-25, Horner 2.3304 * 2^-25, bound
//             2.46 * 2^-25 times 2^i) are in tests/lighting_ref.c next to the same numbers; measured maximum in DESIGN.md 9;
//   PS_Main_Debug: shadowFactor = fmax(0.05f, shadow); mode 1 dot3(N, L) * shadowFactor (may be negative: stored as 0); 2, 3
//             seed = uint(debugValue * 255.0f), three successive QuickRandomFloat; 4 albedo; 5 normal; 6 emissive; 7 metallic;
//             8 roughness; 9 (float)ssao / 255.0f (unbound: 255); 11 shadowFactor; 12 kLODColors[uint(debugValue * 255.0f)], an
//             index >= 8 gives (0, 0, 0) (the reference reads past its table there); 13 (motion.x / (float)W, motion.y / (float)H,
//             0); any other mode (0, 0, 0).  Mode 10 (Ambient) needs the DDGI volume and is refused at record time without it;
//   DDGI:     (m_bRTDDGIEnabled in PS_Main, mode 10 in _Debug; the <*, ddgi> instantiations) irr = ddgi::irradiance(worldPosition,
//             N, m_CameraOrigin), stated in ddgi_irradiance.hip.h and restated in tests/ddgi_ref.c.  PS_Main: ambient = (albedo *
//             (1 / pi)) * irr per channel (albedo as unpacked, not times 1 - metallic: Diffuse_Lambert(m_Albedo)), then, when
//             m_SSAOEnabled, ambient * ((float)ssao / 255.0f) (unbound: 255); rgb = the directional light's rgb (emissive
//             included) + ambient.  Mode 10 stores irr itself;
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
// per SIMD, no scratch, no LDS (-Rpass-analysis=kernel-resource-usage).  The two DDGI instantiations (the 8 probe lookups of
// ddgi_irradiance.hip.h): <lit, ddgi> 73 VGPRs, 6 waves per SIMD; <debug, ddgi> 71 VGPRs, 7 waves per SIMD; no scratch, no LDS.
// MEASURED with DDGI (tools/ddgi_cost.py, the same city and call shape, a 26 x 14 x 37 volume, 17.3 MB of probe textures;
// profiles/ddgi/): <lit, ddgi> 1060.7 us (spread 8.7) against 100.7 us (spread 1.2) for <lit> in the same call and 101.3 us (spread
// 1.3) for the parent commit's <lit>: the query's about 200 correctly rounded divisions per lit pixel (12 per probe decode UNORM10
// texels) against the directional light's 17 are the cost; the probe textures stay in L2.
#include <type_traits>

#include "cull_math.hip.h"
#include "ddgi_irradiance.hip.h"
#include "direct_light.hip.h"
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

struct LightingDdgiArgs                        // the <*, ddgi> instantiations: the two plain ones keep LightingArgs, byte for byte
{
    LightingArgs base;
    ddgi::Textures probes;
};

__device__ __forceinline__ float quickRandomFloat(uint32_t& seed)                                  // random.hlsli:7-11
{
    seed = 1664525u * seed + 1013904223u;
    return (float)(seed & 0x00FFFFFFu) / 16777216.0f;
}

// EvaluateDirectionalLight with the camera as viewer: direct_light.hip.h, which the probe trace shares.
__device__ __forceinline__ cm::F3 litPixel(const LightingArgs& a, const GBufferParams& p, uint32_t px, uint32_t py, float depth, float shadow)
{
    const DeferredLightingConsts& k = a.k;
    const cm::F3 world = sp::worldPosition(k.m_ClipToWorld, px, py, k.m_LightingOutputResolution.x, k.m_LightingOutputResolution.y, depth);
    return dl::litSurface(p, { k.m_CameraOrigin[0], k.m_CameraOrigin[1], k.m_CameraOrigin[2] }, world,
                          { k.m_DirectionalLightVector[0], k.m_DirectionalLightVector[1], k.m_DirectionalLightVector[2] }, k.m_DirectionalLightStrength, shadow);
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

__device__ __forceinline__ const LightingArgs& plain(const LightingArgs& a) { return a; }
__device__ __forceinline__ const LightingArgs& plain(const LightingDdgiArgs& a) { return a.base; }

template <bool DEBUG, bool DDGI = false>
__global__ __launch_bounds__(sp::kBlock) void lightingKernel(std::conditional_t<DDGI, LightingDdgiArgs, LightingArgs> args)
{
    const LightingArgs& a = plain(args);
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
    cm::F3 rgb = DEBUG ? debugPixel(a, p, i, shadow) : litPixel(a, p, at.x, at.y, depth, shadow);
    if constexpr (DDGI) {
        const cm::F3 world = sp::worldPosition(a.k.m_ClipToWorld, at.x, at.y, W, H, depth);
        const cm::F3 irr = ddgi::irradiance(args.probes, world, p.normal, { a.k.m_CameraOrigin[0], a.k.m_CameraOrigin[1], a.k.m_CameraOrigin[2] });
        if (DEBUG) {
            rgb = irr;                                                                             // mode 10, the only one recorded with <debug, ddgi>
        } else {
            const float kInvPi = 0x1.45f306p-2f;
            cm::F3 ambient = { (p.albedo.x * kInvPi) * irr.x, (p.albedo.y * kInvPi) * irr.y, (p.albedo.z * kInvPi) * irr.z };
            if (a.k.m_SSAOEnabled) {
                const float ao = cm::div_((float)(a.ssao ? (uint32_t)a.ssao[i] : 255u), 255.0f);
                ambient = { ambient.x * ao, ambient.y * ao, ambient.z * ao };
            }
            rgb = { rgb.x + ambient.x, rgb.y + ambient.y, rgb.z + ambient.z };
        }
    }
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

// The DDGI bindings of either entry: t5 the descriptor, t6..t8 the probe textures, and the descriptor's host copy behind the
// DeferredLightingConsts in b0.  Everything the kernel's addressing rests on is checked here, against the host copy.
struct DdgiTexture { uint32_t slot, format, texelsPerProbe; const char* what; };
constexpr DdgiTexture kDdgiTextures[3] = { { 6, TRHIP_FORMAT_RGBA16_FLOAT, 1, "Texture_SRV t6 = the RGBA16_FLOAT array of probe data" },
                                           { 7, TRHIP_FORMAT_R10G10B10A2_UNORM, kDDGIIrradianceInteriorTexels + 2, "Texture_SRV t7 = the R10G10B10A2_UNORM array of probe irradiance" },
                                           { 8, TRHIP_FORMAT_RG16_FLOAT, kDDGIDistanceInteriorTexels + 2, "Texture_SRV t8 = the RG16_FLOAT array of probe distance" } };

int requireDdgi(const trhip::DispatchCtx& ctx, const char* why)
{
    const char* name = ctx.shaderName;
    const uint8_t* block = (const uint8_t*)ctx.constants(0, sizeof(DeferredLightingConsts) + sizeof(DDGIVolumeDesc));
    trhip_buffer_t* descBuffer = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 5);
    bool all = block && descBuffer;
    for (const DdgiTexture& w : kDdgiTextures) all = all && ctx.texture(TRHIP_BIND_TEXTURE_SRV, w.slot);
    TRHIP_REQUIRE(all, "%s: %s needs the DDGI volume: t5 (the 64-byte DDGIVolumeDesc), t6 (probe data), t7 (probe irradiance), t8 (probe distance) and "
                       "the descriptor's host copy behind the DeferredLightingConsts in b0 (176 bytes); not all of them are bound", name, why);
    TRHIP_REQUIRE(descBuffer->byteSize >= sizeof(DDGIVolumeDesc), "%s: t5 holds %llu bytes, the DDGIVolumeDesc is 64", name, (unsigned long long)descBuffer->byteSize);
    DDGIVolumeDesc D;
    memcpy(&D, block + sizeof(DeferredLightingConsts), sizeof D);
    for (int a = 0; a < 3; ++a) {
        TRHIP_REQUIRE(D.probeCounts[a] >= 1 && D.probeCounts[a] <= (int)kDDGIMaxProbeCount, "%s: DDGIVolumeDesc probeCounts[%d] = %d, not in 1..1024", name, a, D.probeCounts[a]);
        TRHIP_REQUIRE(D.probeSpacing[a] > 0.0f && D.probeSpacing[a] <= 3.402823466e38f, "%s: DDGIVolumeDesc probeSpacing[%d] = %g is not positive and finite", name, a, (double)D.probeSpacing[a]);
    }
    TRHIP_REQUIRE(D.numIrradianceInteriorTexels == kDDGIIrradianceInteriorTexels && D.numDistanceInteriorTexels == kDDGIDistanceInteriorTexels,
                  "%s: DDGIVolumeDesc interior texel counts %u and %u; the probe tiles have 6 (irradiance) and 14 (distance)", name, D.numIrradianceInteriorTexels, D.numDistanceInteriorTexels);
    for (const DdgiTexture& w : kDdgiTextures) {
        const trhip_texture_t* t = ctx.texture(TRHIP_BIND_TEXTURE_SRV, w.slot);
        TRHIP_REQUIRE(t->format == w.format, "%s: needs %s", name, w.what);
        TRHIP_REQUIRE(t->arraySize != 0, "%s: needs %s; the texture bound is not an array texture", name, w.what);
        const uint32_t tw = (uint32_t)D.probeCounts[0] * w.texelsPerProbe, th = (uint32_t)D.probeCounts[2] * w.texelsPerProbe;
        TRHIP_REQUIRE(t->width == tw && t->height == th && t->arraySize == (uint32_t)D.probeCounts[1], "%s: %s is %ux%u with %u slices; probeCounts (%d, %d, %d) need %ux%u with %d slices", name, w.what,
                      t->width, t->height, t->arraySize, D.probeCounts[0], D.probeCounts[1], D.probeCounts[2], tw, th, D.probeCounts[1]);
    }
    return TRHIP_OK;
}

void bindDdgi(const trhip::DispatchCtx& ctx, ddgi::Textures& p)
{
    const trhip_texture_t* data = ctx.texture(TRHIP_BIND_TEXTURE_SRV, 6), * irr = ctx.texture(TRHIP_BIND_TEXTURE_SRV, 7), * dist = ctx.texture(TRHIP_BIND_TEXTURE_SRV, 8);
    p.desc = (const DDGIVolumeDesc*)ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 5)->ptr;
    p.data = (const uint2*)data->ptr; p.irradiance = (const uint32_t*)irr->ptr; p.distance = (const uint32_t*)dist->ptr;
    p.dataW = data->width; p.dataH = data->height; p.irrW = irr->width; p.irrH = irr->height; p.distW = dist->width; p.distH = dist->height;
    p.slices = data->arraySize;
    p.dataPitch = (uint32_t)(data->slicePitch / data->texelBytes); p.irrPitch = (uint32_t)(irr->slicePitch / irr->texelBytes); p.distPitch = (uint32_t)(dist->slicePitch / dist->texelBytes);
}

// Records either entry: validates the bindings and emits one direct dispatch.
template <bool DEBUG>
int recordLighting(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const DeferredLightingConsts* k = (const DeferredLightingConsts*)ctx.constants(0, sizeof(DeferredLightingConsts));
    TRHIP_REQUIRE(k, "%s: constant buffer b0 (DeferredLightingConsts, 112 bytes) missing", name);
    // The flag or mode 10 at either entry needs the whole volume bound and valid; PS_Main then evaluates it with the flag, _Debug
    // in mode 10.  With neither, t5..t8 are accepted and ignored.
    const bool ambientView = k->m_DebugMode == kDeferredLightingDebugMode_Ambient;
    if (k->m_bRTDDGIEnabled || ambientView)
        if (const int rc = requireDdgi(ctx, k->m_bRTDDGIEnabled ? "m_bRTDDGIEnabled is set and" : "m_DebugMode 10 (Ambient)")) return rc;
    const bool wantDdgi = DEBUG ? ambientView : k->m_bRTDDGIEnabled != 0;
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
    if (wantDdgi) {
        LightingDdgiArgs d = sp::zeroed<LightingDdgiArgs>();
        d.base = a;
        bindDdgi(ctx, d.probes);
        sp::launch(ctx, lightingKernel<DEBUG, true>, DEBUG ? "lightingKernel<debug, ddgi>" : "lightingKernel<lit, ddgi>", sp::tiles(W, H, kTileW, kTileH), dim3(kTileW, kTileH), d);
        return TRHIP_OK;
    }
    sp::launch(ctx, lightingKernel<DEBUG>, DEBUG ? "lightingKernel<debug>" : "lightingKernel<lit>", sp::tiles(W, H, kTileW, kTileH), dim3(kTileW, kTileH), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("deferredlighting_PS_Main", recordLighting<false>, 0);
trhip::ShaderRegistrar r1("deferredlighting_PS_Main_Debug", recordLighting<true>, 0);

} // namespace
