// visibility_resolve.hip.h -- the one resolve from the visibility buffer, shared by "basepass_PS_Main_motion"
// (k_motion.hip: the motion target alone) and "basepass_PS_Main_GBuffer" (k_gbuffer.hip: GBufferA and the motion
// target, the two render targets of the reference's PS_Main_GBuffer, basepass.hlsl:231-253).  The texel decode, the
// fetch chain with its bounds checks, the vertex arithmetic and the edge function are the raster's own (mesh_stage.hip.h);
// the checks only a resolve needs, the interpolation and the motion words exist once, here; the G-buffer half is compiled
// in by the template argument only.
//
// CONVENTION of the G-buffer half (parity unpinned; restated in tests/gbuffer_ref.c).  With q_i = e_i / w_i
// and s = (q0 + q1) + q2 of the motion resolve:
//   N_i     = normalize(mul(unpack(m_PackedNormal), adjugate(World3x3)))  (basepass.hlsl:162-167): R10G10B10A2 with x in
//             bits 20-29, y 10-19, z 0-9, (float)q / 1023.0f (unorm10: the same value), then * 2.0f, then - 1.0f; adjugate rows cross(r1, r2),
//             cross(r2, r0), cross(r0, r1) as cm::cross3; the row-vector product as cm::mulVec; v / sqrt(dot3(v, v));
//   normal  = fma(q2, N2, fma(q1, N1, q0 * N0)) / s per component, NOT renormalised (the reference does not);
//   albedo  = m_ConstAlbedo.rgb, emissive = m_ConstEmissive, roughness = 1, metallic = 0 (Q13: m_ConstRoughness and
//             m_ConstMetallic are never read by the reference's shader); texture flags are ignored, the upload paths
//             refuse them; ALPHA_MASK_MODE's discard is not modelled here: the ALPHA_MASK_MODE=1 rasters (k_raster.hip) apply it, and a
//             discarded sample never becomes a texel;
//   x = PackRGBA8(albedo, debugValue), y = PackUnorm2x16(PackOctadehron(normal)), z = PackR9G9B9E5(emissive),
//   w = PackRGBA8(1, 0, 0, 0) = 0xFF  (lightingcommon.hlsli:28-34), saturate(x) = fmin(fmax(x, 0), 1) (a NaN gives 0),
//             uint(x) truncates, round = round half to even;
//   debugValue by m_DebugMode: 2 QuickRandomFloat(m_InstanceConstIdx), 3 QuickRandomFloat(m_MeshletGroupOffset + lane),
//             12 (float)m_MeshLOD / 255.0f, else 0.
//
// CONVENTION of the TEXTURED instantiation (a texture table bound at t19; parity unpinned; restated in
// tests/material_textures_ref.c).  GetCommonGBufferParams (lightingcommon.hlsli:435-493) as written:
//   uv, wp  = m_TexCoord (half2 -> float, exact) and mul(pos, World), interpolated as the normal: fma(q2, a2, fma(q1, a1, q0 * a0)) / s;
//   ddx,ddy = the same interpolation of the SAME triangle with the edge functions re-evaluated at (cx + 1, cy) and at (cx, cy + 1)
//             (the triangle's plane extended), minus the centre value: what a pixel quad lying inside one triangle yields.  A
//             DEVIATION at triangle borders, where hardware differentiates across the helper lanes of the quad;
//   samples = SampleMaterialValue of each slot flagged in m_MaterialFlags (material_textures.hip.h states the sampler);
//   albedo  = m_ConstAlbedo * sample, roughness = mr.g, metallic = mr.b (defaults (0, 1, 0, 0) when unflagged), emissive =
//             m_ConstEmissive * sample.rgb, w = PackRGBA8(roughness, metallic, 0, 0);
//   normal  = with a normal map: TwoChannelNormalX2 (toyrenderer_common.hlsli:226-231: xy = 2.0f * n.xy - 1.0f, z = sqrt(1.0f -
//             fma(y, y, x * x)), a NaN z is kept), CalculateTBNWithoutTangent (:235-247) from ddx / ddy of wp and uv (cm::cross3, the
//             float2 x float2x3 product fma(b, r1, a * r0), normalize = v / sqrt(dot3)), mul(unpackedNormal, TBN) as cm::mulVec, then
//             normalize, on the interpolated, not renormalised geometric normal;
//   bounds  = a flagged slot whose m_DescriptorIndex is at or past the table's count, names an empty entry or an entry of another
//             format ends the pixel untouched in both targets, like every other broken chain here.
// Without a table recordResolve launches resolveKernel<GBUFFER> exactly as before: no word and no cost of a texture-free frame moves.
#pragma once

#include "material_textures.hip.h"
#include "mesh_stage.hip.h"
#include "screen_pass.hip.h"

#include <type_traits>

namespace vres
{

using namespace mesh;

constexpr uint32_t kTileW = 16, kTileH = 16;   // one workgroup per 16x16 pixels: a wave covers 16x4 neighbouring pixels
constexpr uint32_t kBlock = kTileW * kTileH;
constexpr uint32_t kTexturedWaves = 4;          // waves per SIMD of the TEXTURED instantiation: 128 VGPRs (k_gbuffer.hip)

struct ResolveArgs
{
    BasePassConstants k;
    Geometry geo;
    const MeshletAmplificationData* records[4]; uint32_t recordCapacity[4];
    const uint32_t* lists[4]; uint32_t listCapacity[4];
    const unsigned long long* vis;                               // RG32_UINT as u64
    uint32_t* motion;                                            // RG16_FLOAT: x in the low half, y in the high half
    const char* materials; uint32_t numMaterials;                // MaterialData, the first 32 bytes are read (G-buffer only)
    uint4* gbufferA;                                             // RGBA32_UINT (G-buffer only)
    uint32_t width, height;
};

// The TEXTURED instantiation's arguments: + the texture table bound at t19 and the device's sRGB table.
struct TexturedArgs : ResolveArgs
{
    const mtex::TableEntry* table; uint32_t tableCount;
    const float* srgb;                                           // 256 floats (trhip_device_t::srgbTable)
};

// ---- the pack functions of GBufferA (packunpack.hlsli, lightingcommon.hlsli:28-34, random.hlsli:7-11) ----------------
using sp::saturate_;
__device__ __forceinline__ uint32_t bitsOf(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ float floatOf(uint32_t u) { return __builtin_bit_cast(float, u); }

__device__ __forceinline__ uint32_t packRGBA8(float r, float g, float b, float a)                 // packunpack.hlsli:96-103
{
    return (uint32_t)(saturate_(r) * 255.0f) | (uint32_t)(saturate_(g) * 255.0f) << 8 | (uint32_t)(saturate_(b) * 255.0f) << 16 |
           (uint32_t)(saturate_(a) * 255.0f) << 24;
}

__device__ __forceinline__ uint32_t packOctUnorm2x16(cm::F3 n)                                    // packunpack.hlsli:4-15, 28-32
{
    const float l1 = (__builtin_fabsf(n.x) + __builtin_fabsf(n.y)) + __builtin_fabsf(n.z);
    const float x = n.x / l1, y = n.y / l1, z = n.z / l1;
    float ox = x, oy = y;
    if (!(z >= 0.0f)) {                                                                              // the lower hemisphere folds over
        ox = (1.0f - __builtin_fabsf(y)) * (x >= 0.0f ? 1.0f : -1.0f);
        oy = (1.0f - __builtin_fabsf(x)) * (y >= 0.0f ? 1.0f : -1.0f);
    }
    ox = ox * 0.5f + 0.5f;
    oy = oy * 0.5f + 0.5f;
    const uint32_t ux = (uint32_t)__builtin_rintf(saturate_(ox) * 65535.0f), uy = (uint32_t)__builtin_rintf(saturate_(oy) * 65535.0f);
    return ux | uy << 16;
}

__device__ __forceinline__ uint32_t packR9G9B9E5(float r, float g, float b)                       // packunpack.hlsli:221-245
{
    const float kMaxVal = floatOf(0x477F8000u), kMinVal = floatOf(0x37800000u);                   // 1.FF x 2^15, 1.00 x 2^-16
    r = cm::min_(cm::max_(r, 0.0f), kMaxVal);
    g = cm::min_(cm::max_(g, 0.0f), kMaxVal);
    b = cm::min_(cm::max_(b, 0.0f), kMaxVal);
    const float maxChannel = cm::max_(cm::max_(kMinVal, r), cm::max_(g, b));
    const float bias = floatOf((bitsOf(maxChannel) + 0x07804000u) & 0x7F800000u);                // the largest exponent + 15, no mantissa
    const uint32_t R = bitsOf(r + bias), G = bitsOf(g + bias), B = bitsOf(b + bias);              // the add rounds the channel into the low 9 bits
    const uint32_t E = (bitsOf(bias) << 4) + 0x10000000u;
    return E | B << 18 | G << 9 | (R & 0x1FFu);
}

__device__ __forceinline__ float quickRandomFloat(uint32_t seed)                                  // random.hlsli:7-11
{
    seed = 1664525u * seed + 1013904223u;
    return (float)(seed & 0x00FFFFFFu) / 16777216.0f;
}

// (float)q / 1023.0f for q in [0, 1023] without the division: the product with RN(1/1023) and one residual correction give
// the correctly rounded quotient for all 1024 inputs (restated and checked exhaustively in tests/test_gbuffer_ref.py).
__device__ __forceinline__ float unorm10(uint32_t q)
{
    const float rc = 0x1.00401p-10f, x = (float)q;
    const float q0 = x * rc;
    return cm::fma_(cm::fma_(-q0, 1023.0f, x), rc, q0);
}

__device__ __forceinline__ cm::F3 unpackNormal(uint32_t packed)                                   // packunpack.hlsli:135-157 (.xyz)
{
    const float x = unorm10((packed >> 20) & 0x3FFu), y = unorm10((packed >> 10) & 0x3FFu), z = unorm10(packed & 0x3FFu);
    return { x * 2.0f - 1.0f, y * 2.0f - 1.0f, z * 2.0f - 1.0f };
}

__device__ __forceinline__ cm::F3 normalize3(cm::F3 v)
{
    const float len = cm::sqrt_(cm::dot3(v, v));
    return { v.x / len, v.y / len, v.z / len };
}

// STREAMED: the maps of slot `s`, which samples table entry `t` (material_textures.hip.h).  false: an index that is not 0xFFFFFFFF and
// names no map of a texture like `t`: past the table, empty, another format or size, or `t` is not streamable.  The sizes checked
// here are what keeps every map access inside its allocation.
__device__ __forceinline__ bool streamOf(const TexturedArgs& a, const TextureData& s, const mtex::TableEntry& t, mtex::Stream& st)
{
    st = { nullptr, nullptr, t.pad[0], t.pad[1], 0u };
    const uint32_t mm = s.m_MinMapTextureDescriptorIndex, fb = s.m_FeedbackTextureDescriptorIndex;
    if (mm == 0xFFFFFFFFu && fb == 0xFFFFFFFFu) return true;
    if (!st.shiftX || !st.shiftY) return false;
    const uint32_t rw = t.width >> st.shiftX, rh = t.height >> st.shiftY;
    st.regionsX = rw;
    if (mm != 0xFFFFFFFFu) {
        if (mm >= a.tableCount) return false;
        const mtex::TableEntry& m = a.table[mm];
        if (!m.base || m.format != TRHIP_FORMAT_R8_UINT || m.width != rw || m.height != rh) return false;
        st.minMip = reinterpret_cast<const uint8_t*>(m.base);
    }
    if (fb != 0xFFFFFFFFu) {
        if (fb >= a.tableCount) return false;
        const mtex::TableEntry& m = a.table[fb];
        if (!m.base || m.format != TRHIP_SAMPLER_FEEDBACK_FORMAT || m.width != rw || m.height != rh || m.pad[0] != st.shiftX || m.pad[1] != st.shiftY) return false;
        if (a.k.m_bWriteSamplerFeedback) st.feedback = const_cast<uint32_t*>(m.base);
    }
    return true;
}

// TEXTURED (with GBUFFER only): GetCommonGBufferParams with its four material textures; see the CONVENTION above.
// STREAMED (with TEXTURED only): + the min-mip clamp, the feedback marks and the min-mip colours (material_textures.hip.h, "texture
// streaming"); recorded only when the table holds a map, so the other two instantiations are what they were.
template <bool GBUFFER, bool TEXTURED = false, bool STREAMED = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(TEXTURED ? kTexturedWaves : GBUFFER ? 8 : 1, TEXTURED ? kTexturedWaves : 8)))
void resolveKernel(std::conditional_t<TEXTURED, TexturedArgs, ResolveArgs> a)
{
    static_assert(GBUFFER || !TEXTURED, "the motion resolve samples nothing");
    static_assert(TEXTURED || !STREAMED, "streaming is the textured resolve's");
    const float* tables = nullptr;
    if constexpr (TEXTURED) {                                                            // before anyone leaves: a barrier inside
        __shared__ float lds[mtex::kLdsFloats];
        mtex::stageTables(lds, a.srgb, threadIdx.y * kTileW + threadIdx.x);
        tables = lds;
    }
    const float halfW = 0.5f * (float)a.width, halfH = 0.5f * (float)a.height;
    const sp::Pixel at = sp::pixel<kTileW, kTileH>();
    if (!at.inside(a.width, a.height)) return;
    const uint32_t px = at.x, py = at.y;
    const uint64_t i = at.index(a.width);
    const unsigned long long texel = a.vis[i];
    if (!texel) return;
    const VisTexel id = unpackVisibility((uint32_t)texel);
    if (id.listPosition >= a.listCapacity[id.slot]) return;
    withMeshlet(a.lists[id.slot][id.listPosition], a.records[id.slot], a.recordCapacity[id.slot], a.geo, [&](const Meshlet& ml) {   // a return below leaves the pixel as it is
        const BasePassInstanceConstants& inst = *ml.inst;
        if ((GBUFFER && inst.m_MaterialDataIdx >= a.numMaterials) || id.triangle >= ml.nt) return;
        const uint32_t packed = a.geo.triangles[ml.trianglesAt + id.triangle];
        const uint32_t idx[3] = { packed & 0xFFu, (packed >> 8) & 0xFFu, (packed >> 16) & 0xFFu };
        if (idx[0] >= ml.nv || idx[1] >= ml.nv || idx[2] >= ml.nv) return;
        const mtex::TableEntry* tex[4] = { nullptr, nullptr, nullptr, nullptr };         // albedo, normal, metallic-roughness, emissive
        if constexpr (TEXTURED) {
            const MaterialData& m = *reinterpret_cast<const MaterialData*>(a.materials + (uint64_t)inst.m_MaterialDataIdx * sizeof(MaterialData));
            const TextureData* slots = &m.m_AlbedoTexture;
            for (int c = 0; c < 4; ++c) {
                if (!(m.m_MaterialFlags & (1u << c))) continue;
                const uint32_t d = slots[c].m_DescriptorIndex;
                if (d >= a.tableCount || !mtex::sampled(a.table[d])) return;             // past the table, empty, another format
                tex[c] = a.table + d;
                if constexpr (STREAMED) {
                    mtex::Stream st;
                    if (!streamOf(a, slots[c], a.table[d], st)) return;                  // a map index that names no map of this texture
                }
            }
        }
        const cm::M43 Wm = cm::loadM43(inst.m_WorldMatrix), Pm = cm::loadM43(inst.m_PrevWorldMatrix);
        const cm::M43 clipXYZ = cm::loadM43(a.k.m_WorldToClip);
        float sx[3], sy[3], w[3];
        cm::F3 prev[3];
        uint32_t packedNormal[3];
        uint32_t texCoord[3];                                                            // TEXTURED: m_TexCoord, half2
        cm::F3 wpos[3];                                                                  // TEXTURED: mul(pos, World)
        bool ok = true;
        for (int j = 0; j < 3; ++j) {
            const uint32_t vid = a.geo.vertexIds[ml.vertexIdsAt + idx[j]];
            if (vid >= a.geo.numVertices) { ok = false; break; }
            const RawVertexFormat& vtx = vertexAt(a.geo, vid);
            const cm::F3 pos = { vtx.m_Position[0], vtx.m_Position[1], vtx.m_Position[2] };
            if (GBUFFER) packedNormal[j] = vtx.m_PackedNormal;
            if constexpr (TEXTURED) {
                texCoord[j] = *reinterpret_cast<const uint32_t*>(vtx.m_TexCoord);
                wpos[j] = cm::mulPoint(pos, Wm);
            }
            const ScreenVertex sv = toScreen(pos, Wm, clipXYZ, a.k.m_WorldToClip, halfW, halfH);
            w[j] = sv.w; sx[j] = sv.sx; sy[j] = sv.sy;
            prev[j] = cm::mulPoint(pos, Pm);
        }
        if (!ok) return;
        const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
        const float area = edgeFn(sx[0], sy[0], sx[1], sy[1], sx[2], sy[2]);
        const float sgn = area < 0.0f ? -1.0f : 1.0f;
        const float e0 = sgn * edgeFn(sx[1], sy[1], sx[2], sy[2], cx, cy), e1 = sgn * edgeFn(sx[2], sy[2], sx[0], sy[0], cx, cy), e2 = sgn * edgeFn(sx[0], sy[0], sx[1], sy[1], cx, cy);
        const float q0 = e0 / w[0], q1 = e1 / w[1], q2 = e2 / w[2];
        const float s = (q0 + q1) + q2;
        const float P[3] = { cm::fma_(q2, prev[2].x, cm::fma_(q1, prev[1].x, q0 * prev[0].x)) / s,
                             cm::fma_(q2, prev[2].y, cm::fma_(q1, prev[1].y, q0 * prev[0].y)) / s,
                             cm::fma_(q2, prev[2].z, cm::fma_(q1, prev[1].z, q0 * prev[0].z)) / s };
        float clip[4];
        for (int j = 0; j < 4; ++j)
            clip[j] = cm::fma_(P[2], a.k.m_PrevWorldToClip.m[2][j], cm::fma_(P[1], a.k.m_PrevWorldToClip.m[1][j], P[0] * a.k.m_PrevWorldToClip.m[0][j])) + a.k.m_PrevWorldToClip.m[3][j];
        float mx = 0.0f, my = 0.0f;
        if (clip[3] > 0.0f) {                                                            // basepass.hlsl:230-237
            const float ux = (clip[0] / clip[3]) * 0.5f + 0.5f, uy = (clip[1] / clip[3]) * -0.5f + 0.5f;
            mx = ux * (float)a.width - cx;
            my = uy * (float)a.height - cy;
        }
        a.motion[i] = sp::halfBits(mx) | sp::halfBits(my) << 16;                            // SV_Target1
        if (GBUFFER) {                                                                   // SV_Target0
            const cm::F3 adj0 = cm::cross3(Wm.r1, Wm.r2), adj1 = cm::cross3(Wm.r2, Wm.r0), adj2 = cm::cross3(Wm.r0, Wm.r1);   // MakeAdjugateMatrix
            cm::F3 N[3];
            for (int j = 0; j < 3; ++j) {                                                // basepass.hlsl:162-167
                const cm::F3 n = cm::mulVec(unpackNormal(packedNormal[j]), adj0, adj1, adj2);
                const float len = cm::sqrt_(cm::dot3(n, n));
                N[j] = { n.x / len, n.y / len, n.z / len };
            }
            const cm::F3 normal = { cm::fma_(q2, N[2].x, cm::fma_(q1, N[1].x, q0 * N[0].x)) / s,
                                    cm::fma_(q2, N[2].y, cm::fma_(q1, N[1].y, q0 * N[0].y)) / s,
                                    cm::fma_(q2, N[2].z, cm::fma_(q1, N[1].z, q0 * N[0].z)) / s };
            float debugValue = 0.0f;                                                     // basepass.hlsl:238-249
            if (a.k.m_DebugMode == kDeferredLightingDebugMode_ColorizeInstances) debugValue = quickRandomFloat(ml.rec.m_InstanceConstIdx);
            else if (a.k.m_DebugMode == kDeferredLightingDebugMode_ColorizeMeshlets) debugValue = quickRandomFloat(ml.rec.m_MeshletGroupOffset + ml.lane);
            else if (a.k.m_DebugMode == kDeferredLightingDebugMode_MeshLOD) debugValue = (float)ml.rec.m_MeshLOD / 255.0f;
            const float* mat = reinterpret_cast<const float*>(a.materials + (uint64_t)inst.m_MaterialDataIdx * sizeof(MaterialData));   // albedo rgb(a), emissive rgb
            uint4 out;
            if constexpr (TEXTURED) {
                // uv at the centre, at (cx + 1, cy) and at (cx, cy + 1): the same triangle, its plane extended
                const float ex0 = sgn * edgeFn(sx[1], sy[1], sx[2], sy[2], cx + 1.0f, cy), ex1 = sgn * edgeFn(sx[2], sy[2], sx[0], sy[0], cx + 1.0f, cy), ex2 = sgn * edgeFn(sx[0], sy[0], sx[1], sy[1], cx + 1.0f, cy);
                const float ey0 = sgn * edgeFn(sx[1], sy[1], sx[2], sy[2], cx, cy + 1.0f), ey1 = sgn * edgeFn(sx[2], sy[2], sx[0], sy[0], cx, cy + 1.0f), ey2 = sgn * edgeFn(sx[0], sy[0], sx[1], sy[1], cx, cy + 1.0f);
                const float qx0 = ex0 / w[0], qx1 = ex1 / w[1], qx2 = ex2 / w[2], qy0 = ey0 / w[0], qy1 = ey1 / w[1], qy2 = ey2 / w[2];
                const float sX = (qx0 + qx1) + qx2, sY = (qy0 + qy1) + qy2;
                const float u0 = (float)sp::halfOf(texCoord[0]), u1 = (float)sp::halfOf(texCoord[1]), u2 = (float)sp::halfOf(texCoord[2]);
                const float v0 = (float)sp::halfOf(texCoord[0] >> 16), v1 = (float)sp::halfOf(texCoord[1] >> 16), v2 = (float)sp::halfOf(texCoord[2] >> 16);
                const float u = cm::fma_(q2, u2, cm::fma_(q1, u1, q0 * u0)) / s, v = cm::fma_(q2, v2, cm::fma_(q1, v1, q0 * v0)) / s;
                const float dudx = cm::fma_(qx2, u2, cm::fma_(qx1, u1, qx0 * u0)) / sX - u, dvdx = cm::fma_(qx2, v2, cm::fma_(qx1, v1, qx0 * v0)) / sX - v;
                const float dudy = cm::fma_(qy2, u2, cm::fma_(qy1, u1, qy0 * u0)) / sY - u, dvdy = cm::fma_(qy2, v2, cm::fma_(qy1, v1, qy0 * v0)) / sY - v;
                const MaterialData& m = *reinterpret_cast<const MaterialData*>(mat);
                const TextureData* slots = &m.m_AlbedoTexture;
                cm::F3 albedo = { 1.0f, 1.0f, 1.0f }, mr = { 0.0f, 1.0f, 0.0f }, emissive = { 1.0f, 1.0f, 1.0f }, shaded = normal;
                // SampleMaterialValue of slot c; STREAMED: through the slot's maps (checked above), the albedo slot's min-mip colour if asked for
                // (STREAMED: the four samples are taken by one rolled loop, so that the sampler with its marks exists once in the code object.
                // streamOf runs again here, its result known to be true from the check above: the kernel sits at its 128-VGPR bound, and
                // holding 4 x 5 words of Stream across the interpolation costs more than two loads of a line the check just touched.)
                cm::F3 streamed0 = albedo, streamed1 = albedo, streamed2 = albedo, streamed3 = albedo;
                if constexpr (STREAMED) {
#pragma unroll 1
                    for (int c = 0; c < 4; ++c) {
                        const mtex::TableEntry* t = c == 0 ? tex[0] : c == 1 ? tex[1] : c == 2 ? tex[2] : tex[3];
                        if (!t) continue;
                        mtex::Stream st;
                        streamOf(a, slots[c], *t, st);
                        uint32_t minMip;
                        cm::F3 value = mtex::sampleStreamed(*t, st, tables, slots[c].m_IsWrapSampler != 0u, u, v, dudx, dvdx, dudy, dvdy, minMip);
                        if (c == 0 && a.k.m_bVisualizeMinMipTilesOnAlbedoOutput && st.minMip) value = mtex::mipColour(minMip);
                        if (c == 0) streamed0 = value; else if (c == 1) streamed1 = value; else if (c == 2) streamed2 = value; else streamed3 = value;
                    }
                }
                auto sampleSlot = [&](int c) {
                    if constexpr (STREAMED) return c == 0 ? streamed0 : c == 1 ? streamed1 : c == 2 ? streamed2 : streamed3;
                    else return mtex::sample(*tex[c], tables, slots[c].m_IsWrapSampler != 0u, u, v, dudx, dvdx, dudy, dvdy);
                };
                if (tex[0]) albedo = sampleSlot(0);
                if (tex[1]) {
                    const cm::F3 ns = sampleSlot(1);
                    const float nx = 2.0f * ns.x - 1.0f, ny = 2.0f * ns.y - 1.0f;                   // TwoChannelNormalX2
                    const cm::F3 unpacked = { nx, ny, cm::sqrt_(1.0f - cm::fma_(ny, ny, nx * nx)) };
                    cm::F3 pc, pxx, pyy;                                                             // the world position at the three points
                    pc = { cm::fma_(q2, wpos[2].x, cm::fma_(q1, wpos[1].x, q0 * wpos[0].x)) / s, cm::fma_(q2, wpos[2].y, cm::fma_(q1, wpos[1].y, q0 * wpos[0].y)) / s, cm::fma_(q2, wpos[2].z, cm::fma_(q1, wpos[1].z, q0 * wpos[0].z)) / s };
                    pxx = { cm::fma_(qx2, wpos[2].x, cm::fma_(qx1, wpos[1].x, qx0 * wpos[0].x)) / sX, cm::fma_(qx2, wpos[2].y, cm::fma_(qx1, wpos[1].y, qx0 * wpos[0].y)) / sX, cm::fma_(qx2, wpos[2].z, cm::fma_(qx1, wpos[1].z, qx0 * wpos[0].z)) / sX };
                    pyy = { cm::fma_(qy2, wpos[2].x, cm::fma_(qy1, wpos[1].x, qy0 * wpos[0].x)) / sY, cm::fma_(qy2, wpos[2].y, cm::fma_(qy1, wpos[1].y, qy0 * wpos[0].y)) / sY, cm::fma_(qy2, wpos[2].z, cm::fma_(qy1, wpos[1].z, qy0 * wpos[0].z)) / sY };
                    const cm::F3 dp1 = { pxx.x - pc.x, pxx.y - pc.y, pxx.z - pc.z }, dp2 = { pyy.x - pc.x, pyy.y - pc.y, pyy.z - pc.z };
                    const cm::F3 m2 = cm::cross3(dp1, dp2), inv0 = cm::cross3(dp2, m2), inv1 = cm::cross3(m2, dp1);   // CalculateTBNWithoutTangent
                    const cm::F3 t = normalize3({ cm::fma_(dudy, inv1.x, dudx * inv0.x), cm::fma_(dudy, inv1.y, dudx * inv0.y), cm::fma_(dudy, inv1.z, dudx * inv0.z) });
                    const cm::F3 b = normalize3({ cm::fma_(dvdy, inv1.x, dvdx * inv0.x), cm::fma_(dvdy, inv1.y, dvdx * inv0.y), cm::fma_(dvdy, inv1.z, dvdx * inv0.z) });
                    shaded = normalize3(cm::mulVec(unpacked, t, b, normal));
                }
                if (tex[2]) mr = sampleSlot(2);
                if (tex[3]) emissive = sampleSlot(3);
                out.x = packRGBA8(mat[0] * albedo.x, mat[1] * albedo.y, mat[2] * albedo.z, debugValue);
                out.y = packOctUnorm2x16(shaded);
                out.z = packR9G9B9E5(mat[4] * emissive.x, mat[5] * emissive.y, mat[6] * emissive.z);
                out.w = packRGBA8(mr.y, mr.z, 0.0f, 0.0f);                               // roughness = mr.g, metallic = mr.b
            } else {
                out.x = packRGBA8(mat[0], mat[1], mat[2], debugValue);
                out.y = packOctUnorm2x16(normal);
                out.z = packR9G9B9E5(mat[4], mat[5], mat[6]);
                out.w = packRGBA8(1.0f, 0.0f, 0.0f, 0.0f);                               // roughness 1, metallic 0 (Q13)
            }
            a.gbufferA[i] = out;                                                         // one 16-byte store per lane
        }
    });                                                                              // withMeshlet: nothing may follow, a chain out of bounds ends the pixel too
}

// Records the resolve: validates the bindings and emits one direct dispatch.  GBUFFER: + t3 materials, u0 = GBufferA
// (RGBA32_UINT), the motion target at u1; otherwise the motion target at u0.
template <bool GBUFFER>
int recordResolve(trhip::DispatchCtx& ctx)
{
    const BasePassConstants* k = (const BasePassConstants*)ctx.constants(0, sizeof(BasePassConstants));
    TRHIP_REQUIRE(k, "%s: constant buffer b0 (BasePassConstants, 256 bytes) missing", ctx.shaderName);
    TexturedArgs a = sp::zeroed<TexturedArgs>();                                                                  // ResolveArgs + the table; sliced when none is bound
    a.k = *k;
    if (const int rc = bindGeometry(ctx, a.geo)) return rc;
    trhip_buffer_t* records[4];
    trhip_buffer_t* lists[4];
    for (uint32_t s = 0; s < 4; ++s) {
        records[s] = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 10 + s);
        lists[s] = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 14 + s);
        TRHIP_REQUIRE(records[s] && lists[s], "%s: needs the records of all four pass slots at t10..t13 and their visible lists at t14..t17 (slot %u missing)", ctx.shaderName, s);
    }
    trhip_texture_t* vis = ctx.texture(TRHIP_BIND_TEXTURE_SRV, 18);
    uint32_t mip = 0;
    trhip_texture_t* motion = ctx.texture(TRHIP_BIND_TEXTURE_UAV, GBUFFER ? 1 : 0, &mip);
    TRHIP_REQUIRE(vis && vis->format == TRHIP_FORMAT_RG32_UINT, "%s: needs Texture_SRV t18 = the RG32_UINT visibility buffer", ctx.shaderName);
    TRHIP_REQUIRE(motion && mip == 0 && motion->format == TRHIP_FORMAT_RG16_FLOAT, "%s: needs Texture_UAV u%u = the RG16_FLOAT motion target, mip 0", ctx.shaderName, GBUFFER ? 1u : 0u);
    const uint32_t W = k->m_OutputResolution.x, H = k->m_OutputResolution.y;
    TRHIP_REQUIRE(vis->width == W && vis->height == H && motion->width == W && motion->height == H,
                  "%s: visibility buffer %ux%u and motion target %ux%u must both be m_OutputResolution %ux%u", ctx.shaderName, vis->width, vis->height, motion->width, motion->height, W, H);
    trhip_buffer_t* materials = nullptr;
    trhip_texture_t* gbufferA = nullptr;
    if (GBUFFER) {
        materials = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 3);
        TRHIP_REQUIRE(materials, "%s: needs SRV t3 = the MaterialData buffer (124-byte stride)", ctx.shaderName);
        uint32_t gmip = 0;
        gbufferA = ctx.texture(TRHIP_BIND_TEXTURE_UAV, 0, &gmip);
        TRHIP_REQUIRE(gbufferA && gmip == 0 && gbufferA->format == TRHIP_FORMAT_RGBA32_UINT, "%s: needs Texture_UAV u0 = the RGBA32_UINT GBufferA, mip 0", ctx.shaderName);
        TRHIP_REQUIRE(gbufferA->width == W && gbufferA->height == H, "%s: GBufferA %ux%u must be m_OutputResolution %ux%u", ctx.shaderName, gbufferA->width, gbufferA->height, W, H);
    }
    if (const int rc = sp::requireCover(ctx, sp::kGroupSide, sp::kGroupSide, W, H)) return rc;
    for (uint32_t s = 0; s < 4; ++s) {
        a.records[s] = (const MeshletAmplificationData*)records[s]->ptr;
        a.recordCapacity[s] = elements32(records[s], sizeof(MeshletAmplificationData));
        a.lists[s] = (const uint32_t*)lists[s]->ptr;
        a.listCapacity[s] = elements32(lists[s], 4);
    }
    a.vis = (const unsigned long long*)vis->ptr;
    a.motion = (uint32_t*)motion->ptr;
    if (GBUFFER) {
        a.materials = (const char*)materials->ptr;
        a.numMaterials = elements32(materials, sizeof(MaterialData));
        a.gbufferA = (uint4*)gbufferA->ptr;
    }
    a.width = W; a.height = H;
    const dim3 grid = sp::tiles(W, H, kTileW, kTileH);
    if constexpr (GBUFFER) {
        if (trhip_texture_table_t* table = ctx.textureTable(19)) {                   // t19: the TEXTURED instantiation
            for (size_t d = 0; d < table->slots.size(); ++d)
                TRHIP_REQUIRE(!table->slots[d] || !table->slots[d]->isUAV, "%s: the texture table at t19 holds '%s' at index %zu, created with the UAV or render-target bit: a sampled texture is read only",
                              ctx.shaderName, table->slots[d]->name.c_str(), d);
            TRHIP_REQUIRE(table->entries.ptr && ctx.cl->dev->srgbTable.ptr, "%s: the texture table at t19 has no device data", ctx.shaderName);
            a.table = (const mtex::TableEntry*)table->entries.ptr;
            a.tableCount = (uint32_t)table->slots.size();
            a.srgb = (const float*)ctx.cl->dev->srgbTable.ptr;
            // An R8_UINT or feedback entry selects the STREAMED instantiation.  The table cannot tell a min-mip map from another R8_UINT
            // texture, so any R8_UINT entry selects it: harmless (materials that name no map get the textured kernel's words), if surprising.
            if (table->streamEntries) {
                ctx.emit("streamed", [a, grid](hipStream_t s) {
                    TRHIP_LAUNCH((resolveKernel<true, true, true>), grid, dim3(kTileW, kTileH), 0, s, a);
                    return trhip::launchStatus("resolveKernel<gbuffer, textured, streamed>"); });
                return TRHIP_OK;
            }
            ctx.emit("textured", [a, grid](hipStream_t s) {
                TRHIP_LAUNCH((resolveKernel<true, true>), grid, dim3(kTileW, kTileH), 0, s, a);
                return trhip::launchStatus("resolveKernel<gbuffer, textured>"); });
            return TRHIP_OK;
        }
    }
    const ResolveArgs plain = a;
    ctx.emit("main", [plain, grid](hipStream_t s) {
        TRHIP_LAUNCH(resolveKernel<GBUFFER>, grid, dim3(kTileW, kTileH), 0, s, plain);
        return trhip::launchStatus(GBUFFER ? "resolveKernel<gbuffer>" : "resolveKernel<motion>"); });
    return TRHIP_OK;
}

} // namespace vres
