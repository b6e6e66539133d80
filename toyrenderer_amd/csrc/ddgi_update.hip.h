// ddgi_update.hip.h -- what "giprobetrace_CS_ProbeTrace" (k_giprobetrace.hip), the two "ProbeBlendingCS_DDGIProbeBlendingCS"
// passes (k_giprobeblend.hip) and the three placement passes (k_giprobeplacement.hip) share: the constant block, a probe's
// coordinates and position, a ray's direction (of the 256 and of the 32 fixed ones), the octahedral decode, and the record-time
// checks of the block, of the probe textures and of the fixed-ray distances (the scene's buffers: rw::bindScene).  The RTXGI SDK is not part of this project; this is
// the project's own statement of the published update (Majercik et al., JCGT 2019) and tests/ddgi_update_ref.c restates it word
// for word.  The query's conventions (ddgi_irradiance.hip.h) hold here too: binary32, no contraction, fma only in dot3 and the
// polynomials, / and sqrt correctly rounded.
//
//   probe     index p = (y * counts.z + z) * counts.x + x (ddgi.Volume.probe_positions_and_states' order); its data texel is (x, z) of
//             slice y, its tiles start at texel (x * N, z * N) of slice y;
//   position  ((spacing * (float)c) - ext) + origin, + data.xyz * spacing with flags bit 0: the query's probePos;
//   direction of ray i of kDDGIRaysPerProbe = 256 (spherical Fibonacci): f = (float)i * 0.618034f; phi = RN(2 pi) * (f - floor(f));
//             c = 1.0f - (float)(2 * i + 1) / 256.0f; s = sqrt(saturate(1.0f - c * c)); d = (cosSoft(phi) * s, sinSoft(phi) * s, c);
//             rotated = (dot3(row0, d), dot3(row1, d), dot3(row2, d)) with the rows of DDGIUpdateConsts::rayRotation; the direction
//             is normalize(rotated) = rotated / sqrt(dot3(rotated, rotated));
//   octDecode(o): v = (o.x, o.y, (1 - |o.x|) - |o.y|); v.z < 0: v.x = (1 - |o.y|) * s(o.x), v.y = (1 - |o.x|) * s(o.y), s(x) = x >= 0 ?
//             1 : -1; normalize(v).  The inverse of ddgi::oct.  Interior texel i of n (6 or 14) has o = (float)(2 * i + 1) / (float)n - 1.
#pragma once

#include "cull_math.hip.h"
#include "ddgi_irradiance.hip.h"
#include "ray_walk.hip.h"
#include "screen_pass.hip.h"
#include "soft_math.hip.h"

namespace ddgiu
{

// b0 of the three passes: the update's constants and the host copy of the volume's descriptor behind them.
struct Block
{
    interop::DDGIUpdateConsts k;
    interop::DDGIVolumeDesc D;
};
static_assert(sizeof(Block) == 160, "b0 of the DDGI update passes");

struct I3 { int x, y, z; };

__device__ __forceinline__ I3 probeCoords(uint32_t probe, const interop::DDGIVolumeDesc& D)
{
    const uint32_t cx = (uint32_t)D.probeCounts[0], cz = (uint32_t)D.probeCounts[2];
    return { (int)(probe % cx), (int)(probe / (cx * cz)), (int)((probe / cx) % cz) };
}

__device__ __forceinline__ cm::F3 probePosition(const interop::DDGIVolumeDesc& D, I3 c, uint2 data)
{
    const cm::F3 spacing = { D.probeSpacing[0], D.probeSpacing[1], D.probeSpacing[2] };
    const cm::F3 ext = { (spacing.x * (float)(D.probeCounts[0] - 1)) * 0.5f, (spacing.y * (float)(D.probeCounts[1] - 1)) * 0.5f, (spacing.z * (float)(D.probeCounts[2] - 1)) * 0.5f };
    cm::F3 p = { (spacing.x * (float)c.x - ext.x) + D.origin[0], (spacing.y * (float)c.y - ext.y) + D.origin[1], (spacing.z * (float)c.z - ext.z) + D.origin[2] };
    if (D.flags & interop::kDDGIFlag_Relocation) {
        p.x = p.x + (float)sp::halfOf(data.x) * spacing.x;
        p.y = p.y + (float)sp::halfOf(data.x >> 16) * spacing.y;
        p.z = p.z + (float)sp::halfOf(data.y) * spacing.z;
    }
    return p;
}

__device__ __forceinline__ bool inactive(const interop::DDGIVolumeDesc& D, uint2 data)
{
    return (D.flags & interop::kDDGIFlag_Classification) && (float)sp::halfOf(data.y >> 16) == 1.0f;
}

__device__ __forceinline__ cm::F3 rayDirection(uint32_t i, const interop::DDGIUpdateConsts& k)
{
    const float f = (float)i * 0.618034f, phi = 0x1.921fb6p+2f * (f - __builtin_floorf(f));
    const float c = 1.0f - cm::div_((float)(2u * i + 1u), (float)interop::kDDGIRaysPerProbe), s = cm::sqrt_(sp::saturate_(1.0f - c * c));
    const cm::F3 d = { softmath::cosSoft(phi) * s, softmath::sinSoft(phi) * s, c };
    const cm::F3 r = { cm::dot3({ k.rayRotation[0][0], k.rayRotation[0][1], k.rayRotation[0][2] }, d), cm::dot3({ k.rayRotation[1][0], k.rayRotation[1][1], k.rayRotation[1][2] }, d),
                       cm::dot3({ k.rayRotation[2][0], k.rayRotation[2][1], k.rayRotation[2][2] }, d) };
    return ddgi::normalize(r);
}

// Fixed ray i of kDDGIFixedRays = 32, the rays of relocation and classification (k_giprobeplacement.hip): rayDirection's formula
// with 32 in place of 256 and no rotation (d itself is normalised, not its product with a matrix).
__device__ __forceinline__ cm::F3 fixedRayDirection(uint32_t i)
{
    const float f = (float)i * 0.618034f, phi = 0x1.921fb6p+2f * (f - __builtin_floorf(f));
    const float c = 1.0f - cm::div_((float)(2u * i + 1u), (float)interop::kDDGIFixedRays), s = cm::sqrt_(sp::saturate_(1.0f - c * c));
    const cm::F3 d = { softmath::cosSoft(phi) * s, softmath::sinSoft(phi) * s, c };
    return ddgi::normalize(d);
}

__device__ __forceinline__ cm::F3 octDecode(float ox, float oy)
{
    cm::F3 v = { ox, oy, (1.0f - __builtin_fabsf(ox)) - __builtin_fabsf(oy) };
    if (v.z < 0.0f) {
        v.x = (1.0f - __builtin_fabsf(oy)) * (ox >= 0.0f ? 1.0f : -1.0f);
        v.y = (1.0f - __builtin_fabsf(ox)) * (oy >= 0.0f ? 1.0f : -1.0f);
    }
    return ddgi::normalize(v);
}

// ---- record side -------------------------------------------------------------------------------------------------------------
// The descriptor's host copy, checked as the lighting pass checks its own, wherever a pass keeps it (the probe visualisation's passes,
// k_giprobedraw.hip, have blocks of their own).
inline int requireDesc(const char* name, const interop::DDGIVolumeDesc& D)
{
    for (int a = 0; a < 3; ++a) {
        TRHIP_REQUIRE(D.probeCounts[a] >= 1 && D.probeCounts[a] <= (int)interop::kDDGIMaxProbeCount, "%s: DDGIVolumeDesc probeCounts[%d] = %d, not in 1..1024", name, a, D.probeCounts[a]);
        TRHIP_REQUIRE(D.probeSpacing[a] > 0.0f && D.probeSpacing[a] <= 3.402823466e38f, "%s: DDGIVolumeDesc probeSpacing[%d] = %g is not positive and finite", name, a, (double)D.probeSpacing[a]);
    }
    TRHIP_REQUIRE(D.numIrradianceInteriorTexels == interop::kDDGIIrradianceInteriorTexels && D.numDistanceInteriorTexels == interop::kDDGIDistanceInteriorTexels,
                  "%s: DDGIVolumeDesc interior texel counts %u and %u; the probe tiles have 6 (irradiance) and 14 (distance)", name, D.numIrradianceInteriorTexels, D.numDistanceInteriorTexels);
    TRHIP_REQUIRE((uint64_t)D.probeCounts[0] * (uint64_t)D.probeCounts[1] * (uint64_t)D.probeCounts[2] <= (1u << 22), "%s: %d x %d x %d probes; the update takes at most 2^22", name,
                  D.probeCounts[0], D.probeCounts[1], D.probeCounts[2]);
    return TRHIP_OK;
}

// b0: the 160-byte block
inline int requireBlock(const trhip::DispatchCtx& ctx, Block& out)
{
    const char* name = ctx.shaderName;
    const void* block = ctx.constants(0, sizeof(Block));
    TRHIP_REQUIRE(block, "%s: constant buffer b0 (the 96-byte DDGIUpdateConsts and the 64-byte DDGIVolumeDesc behind it, 160 bytes) missing or short", name);
    memcpy(&out, block, sizeof out);
    return requireDesc(name, out.D);
}

inline uint32_t numProbes(const interop::DDGIVolumeDesc& D) { return (uint32_t)D.probeCounts[0] * (uint32_t)D.probeCounts[1] * (uint32_t)D.probeCounts[2]; }

// One probe texture: bound, of the format, an array of probeCounts.y slices of probeCounts.x * n by probeCounts.z * n texels, and
// created with the UAV bit where the pass writes it.
inline int requireProbeTexture(const trhip::DispatchCtx& ctx, uint32_t type, uint32_t slot, uint32_t format, uint32_t texelsPerProbe, const char* what,
                               const interop::DDGIVolumeDesc& D, trhip_texture_t*& out)
{
    const char* name = ctx.shaderName;
    trhip_texture_t* t = out = ctx.texture(type, slot);
    TRHIP_REQUIRE(t && t->format == format, "%s: needs %s", name, what);
    TRHIP_REQUIRE(t->arraySize != 0, "%s: needs %s; the texture bound is not an array texture", name, what);
    const uint32_t tw = (uint32_t)D.probeCounts[0] * texelsPerProbe, th = (uint32_t)D.probeCounts[2] * texelsPerProbe;
    TRHIP_REQUIRE(t->width == tw && t->height == th && t->arraySize == (uint32_t)D.probeCounts[1], "%s: %s is %ux%u with %u slices; probeCounts (%d, %d, %d) need %ux%u with %d slices", name, what,
                  t->width, t->height, t->arraySize, D.probeCounts[0], D.probeCounts[1], D.probeCounts[2], tw, th, D.probeCounts[1]);
    TRHIP_REQUIRE(type != TRHIP_BIND_TEXTURE_UAV || t->isUAV, "%s: %s was created without the UAV bit; the pass writes it", name, what);
    return TRHIP_OK;
}

// The scene and its acceleration structure in the probe trace's slots: t4 the TLAS nodes, t5 instances, t6 vertices, t7 materials
// (asked for only where the pass shades its hits), t8 indices, t9 mesh data, t10 TLAS instances, t11 BLAS headers, t12 BLAS nodes,
// t13 triangle order: rw::bindScene's slot table.
constexpr uint32_t kSceneSlots[10] = { 4, 5, 6, 7, 8, 9, 10, 11, 12, 13 };

// ---- what the three placement passes share (k_giprobeplacement.hip) --------------------------------------------------------------
// u0 of all three: the fixed-ray distances, float[numProbes * 32]
inline int requireFixedRayDistances(const trhip::DispatchCtx& ctx, uint32_t probes, float*& out)
{
    const char* name = ctx.shaderName;
    trhip_buffer_t* d = ctx.buffer(TRHIP_BIND_STRUCTURED_UAV, 0);
    TRHIP_REQUIRE(d, "%s: needs StructuredBuffer_UAV u0 = the fixed-ray distances, float[numProbes * 32]", name);
    TRHIP_REQUIRE(d->byteSize == (uint64_t)probes * interop::kDDGIFixedRays * sizeof(float), "%s: the fixed-ray distances at u0 hold %llu bytes; %u probes of 32 floats are %llu", name,
                  (unsigned long long)d->byteSize, probes, (unsigned long long)probes * interop::kDDGIFixedRays * sizeof(float));
    out = (float*)d->ptr;
    return TRHIP_OK;
}

// A direct dispatch of (ceil(threads / perGroup), 1, 1) groups
inline int requireLinearDispatch(const trhip::DispatchCtx& ctx, uint64_t threads, uint32_t perGroup, const char* what)
{
    const uint32_t groups = (uint32_t)((threads + perGroup - 1) / perGroup);
    TRHIP_REQUIRE(!ctx.indirect && ctx.gx == groups && ctx.gy == 1 && ctx.gz == 1, "%s: needs a direct dispatch of (%s, 1, 1) = (%u, 1, 1) groups", ctx.shaderName, what, groups);
    return TRHIP_OK;
}

} // namespace ddgiu
