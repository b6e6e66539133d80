// gbuffer_unpack.hip.h -- UnpackGBuffer (lightingcommon.hlsli:36-51) for the passes that read GBufferA: the lighting pass
// (k_deferredlighting.hip, which states UnpackGBuffer's convention) and the shadow mask's trace (k_shadowmask.hip, which reads the normal).
#pragma once

#include "screen_pass.hip.h"

namespace gbuf
{

__device__ __forceinline__ cm::F3 normalize_(cm::F3 v)
{
    const float len = cm::sqrt_(cm::dot3(v, v));
    return { cm::div_(v.x, len), cm::div_(v.y, len), cm::div_(v.z, len) };
}

__device__ __forceinline__ float unorm8(uint32_t byte) { return (float)byte * (1.0f / 255.0f); }
__device__ __forceinline__ float unorm16(uint32_t u) { return (float)u * (1.0f / 65535.0f); }

struct GBufferParams { cm::F3 albedo; float debugValue; cm::F3 normal, emissive; float roughness, metallic; };

__device__ __forceinline__ GBufferParams unpackGBuffer(uint4 g)                                    // lightingcommon.hlsli:36-51
{
    GBufferParams p;
    p.albedo = { unorm8(g.x & 0xFFu), unorm8((g.x >> 8) & 0xFFu), unorm8((g.x >> 16) & 0xFFu) };
    p.debugValue = unorm8(g.x >> 24);
    const float fx = unorm16(g.y & 0xFFFFu) * 2.0f - 1.0f, fy = unorm16(g.y >> 16) * 2.0f - 1.0f;   // packunpack.hlsli:17-26
    cm::F3 n = { fx, fy, (1.0f - __builtin_fabsf(fx)) - __builtin_fabsf(fy) };
    const float t = sp::saturate_(-n.z);
    n.x += n.x >= 0.0f ? -t : t;
    n.y += n.y >= 0.0f ? -t : t;
    p.normal = normalize_(n);
    const int e = (int)(g.z >> 27) - 24;                                                           // packunpack.hlsli:247-251
    p.emissive = { __builtin_ldexpf((float)(g.z & 0x1FFu), e), __builtin_ldexpf((float)((g.z >> 9) & 0x1FFu), e), __builtin_ldexpf((float)((g.z >> 18) & 0x1FFu), e) };
    p.roughness = unorm8(g.w & 0xFFu);
    p.metallic = unorm8((g.w >> 8) & 0xFFu);
    return p;
}

} // namespace gbuf
