// k_giprobetrace.hip -- "giprobetrace_CS_ProbeTrace": the first pass of GIRenderer::RenderDDGI (source/GIRenderer.cpp,
// source/shaders/giprobetrace.hlsl:23-148): 256 rays from every probe of the DDGI volume through the scene's acceleration
// structure, each lit by the directional light, the surface's emissive and the volume's own irradiance of the update before.  The two
// blend passes (k_giprobeblend.hip) fold the records into the probe textures.  The RTXGI SDK is not part of this project; the ray
// directions and the record layout are the project's own (ddgi_update.hip.h), and tests/ddgi_update_ref.c is the definition.
//
// BINDINGS.  b0 ddgiu::Block (DDGIUpdateConsts, then the DDGIVolumeDesc's host copy; 160 bytes); the reference's registers: t0 the
// 64-byte DDGIVolumeDesc, t1 the RGBA16_FLOAT array of probe data, t2 the R10G10B10A2_UNORM irradiance array, t3 the RG16_FLOAT
// distance array, t4 the TLAS nodes, t5 instances, t6 vertices, t7 materials, t8 indices, t9 mesh data; the structure's other
// buffers: t10 TLAS instances, t11 BLAS headers, t12 BLAS nodes, t13 triangle order; u0 the ray records, a structured buffer
// float4[numProbes * 256] (the reference's RGBA32F texture array holds the same words).  Samplers are accepted and ignored.  A
// direct dispatch of (256 / 64, probeCounts.x * probeCounts.z, probeCounts.y) groups of 64 threads.
//
// CONVENTION (binary32, no contraction, fma only where written, / and sqrt correctly rounded).  Per (ray i, probe p):
//   probe     position and state as ddgi_update.hip.h has them; with flags bit 1 a probe whose data.w == 1.0f traces nothing and its
//             256 records keep what they held (the 32 fixed rays that can wake it are a pass of their own, k_giprobeplacement.hip);
//   ray       origin the probe, direction ddgiu::rayDirection(i), TMin 0, TMax probeMaxRayDistance; rw::closestHit (ray_walk.hip.h);
//   miss      record (1, 1, 1, 1e27f) (giprobetrace.hlsl:67: the sky's radiance is the reference's own TODO);
//   back face record (0, 0, 0, -0.2f * t);
//   front face: b0 = (1.0f - b1) - b2; position and normal InterpolateVertex's (raytracingcommon.hlsli:24-36): ((0 + v0 * b0) + v1 * b1)
//             + v2 * b2 per component, not fused; the normal's components unpacked as (float)q / 1023.0f * 2 - 1 (x in bits 20-29);
//             world = the position through the instance's m_WorldMatrix: fma(p.z, w[2][j], fma(p.y, w[1][j], p.x * w[0][j])) + w[3][j];
//             QUIRK 1: the normal stays in OBJECT space and is not normalised, as the reference passes it (raytracingcommon.hlsli:197);
//             material: albedo m_ConstAlbedo.rgb, emissive m_ConstEmissive, roughness 1, metallic 0 (what GetCommonGBufferParams gives
//             without textures; a textured material is traced with these constants: DEVIATION);
//             shadow ray: QUIRK 2: from the PROBE (giprobetrace.hlsl:107), direction the light vector, TMin 0, TMax 1e10f; every
//             candidate commits, so it is occluded iff rw::closestHit finds anything;
//             rgb = dl::litSurface(surface, viewer = the probe, world, L, strength, shadow = occluded ? 0.0f : 1.0f) (direct_light.hip.h:
//             the lighting pass's directional light, emissive included) + (fmin(albedo, 0.9f) * RN(1 / pi)) * irr per channel,
//             irr = ddgi::irradiance(world, normal, cameraOrigin = the probe) on the textures as the update before left them;
//             record (saturate(rgb), t).
//
// KERNEL.  One thread per (ray, probe); a wave is 64 consecutive rays of one probe, so its lanes start at one point and fan out.
// The walk, the triangle test and the triangle fetch are ray_walk.hip.h's (rw::walk, whose visitor closestHit is; the hit's
// attributes are read through rw::fetchTri): no stack, no LDS, no per-lane array.  UNTUNED, as the sun's trace is: correctness came
// first.  closestHit does not prune against the best hit, front-face rays walk the structure twice (the shadow ray: a closest hit
// too, not an any-hit ray) and then run the query's eight probe lookups.  Code object (-Rpass-analysis=kernel-resource-usage): 79
// VGPRs, occupancy 6 waves per SIMD, 41 spilled scalar registers, no scratch, no LDS.  MEASURED (tools/ddgi_update_cost.py, the
// generated city of 2251 instances, 13 468 probes = 3.45 M rays, one MI355X; profiles/ray_walk/README.md): 61.8 ms per update, next
// to 0.10 and 0.49 ms for the two blends.
#include "ddgi_irradiance.hip.h"
#include "ddgi_update.hip.h"
#include "direct_light.hip.h"
#include "ray_walk.hip.h"

namespace
{

using namespace interop;
using cm::F3;

constexpr uint32_t kWave = 64;                 // [numthreads(kNumThreadsPerWave, 1, 1)]

struct ProbeTraceArgs
{
    ddgiu::Block b;
    rw::SceneArgs scene;
    ddgi::Textures probes;                     // t0..t3
    float4* rays;                              // u0
    uint32_t numProbes;
};

__device__ __forceinline__ F3 unpackNormal(uint32_t packed)                                        // packunpack.hlsli:135-157 (.xyz)
{
    const float x = cm::div_((float)((packed >> 20) & 0x3FFu), 1023.0f), y = cm::div_((float)((packed >> 10) & 0x3FFu), 1023.0f), z = cm::div_((float)(packed & 0x3FFu), 1023.0f);
    return { x * 2.0f - 1.0f, y * 2.0f - 1.0f, z * 2.0f - 1.0f };
}

__device__ __forceinline__ float bary(float v0, float v1, float v2, float b0, float b1, float b2) { return ((0.0f + v0 * b0) + v1 * b1) + v2 * b2; }

__global__ __launch_bounds__(kWave) void probeTraceKernel(ProbeTraceArgs a)
{
    const DDGIVolumeDesc& D = a.b.D;
    const DDGIUpdateConsts& k = a.b.k;
    const uint32_t probe = blockIdx.x / (kDDGIRaysPerProbe / kWave), ray = (blockIdx.x % (kDDGIRaysPerProbe / kWave)) * kWave + threadIdx.x;
    if (probe >= a.numProbes) return;
    const ddgiu::I3 c = ddgiu::probeCoords(probe, D);
    const uint2 data = a.probes.data[(uint64_t)c.y * a.probes.dataPitch + (uint32_t)c.z * a.probes.dataW + (uint32_t)c.x];
    if (ddgiu::inactive(D, data)) return;
    const F3 origin = ddgiu::probePosition(D, c, data), dir = ddgiu::rayDirection(ray, k);
    float4* out = a.rays + (uint64_t)probe * kDDGIRaysPerProbe + ray;
    const rw::Hit hit = rw::closestHit(a.scene, origin, dir, 0.0f, k.probeMaxRayDistance);
    if (hit.inst == 0xFFFFFFFFu) { *out = make_float4(1.0f, 1.0f, 1.0f, 1e27f); return; }
    if (!hit.front) { *out = make_float4(0.0f, 0.0f, 0.0f, -0.2f * hit.t); return; }

    // the hit's attributes: closestHit's visitor passed this (mesh, triangle) through the same rw::fetchTri on the same buffers, so
    // the fetch cannot answer false here and the return below is never taken (tests/ddgi_update_ref.c says the same of its refetch)
    const BasePassInstanceConstants& inst = a.scene.instances[hit.inst];
    rw::Tri T;
    if (!rw::fetchTri(a.scene, reinterpret_cast<const MeshData*>(a.scene.meshes + (uint64_t)inst.m_MeshDataIdx * sizeof(MeshData)), hit.tri, T)) return;
    const F3* v = T.v;
    F3 n[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) n[j] = unpackNormal(*reinterpret_cast<const uint32_t*>(a.scene.vertices + T.i[j] * sizeof(RawVertexFormat) + offsetof(RawVertexFormat, m_PackedNormal)));
    const float b1 = hit.b1, b2 = hit.b2, b0 = (1.0f - b1) - b2;
    const F3 p = { bary(v[0].x, v[1].x, v[2].x, b0, b1, b2), bary(v[0].y, v[1].y, v[2].y, b0, b1, b2), bary(v[0].z, v[1].z, v[2].z, b0, b1, b2) };
    gbuf::GBufferParams s;
    s.normal = { bary(n[0].x, n[1].x, n[2].x, b0, b1, b2), bary(n[0].y, n[1].y, n[2].y, b0, b1, b2), bary(n[0].z, n[1].z, n[2].z, b0, b1, b2) };
    const float* w = &inst.m_WorldMatrix.m[0][0];
    const F3 world = { cm::fma_(p.z, w[8], cm::fma_(p.y, w[4], p.x * w[0])) + w[12], cm::fma_(p.z, w[9], cm::fma_(p.y, w[5], p.x * w[1])) + w[13],
                       cm::fma_(p.z, w[10], cm::fma_(p.y, w[6], p.x * w[2])) + w[14] };
    s.albedo = { 0.0f, 0.0f, 0.0f }; s.emissive = { 0.0f, 0.0f, 0.0f };
    if (inst.m_MaterialDataIdx < a.scene.numMaterials) {                                           // a material index past the buffer: black
        const MaterialData* m = reinterpret_cast<const MaterialData*>(a.scene.materials + (uint64_t)inst.m_MaterialDataIdx * sizeof(MaterialData));
        s.albedo = { m->m_ConstAlbedo.x, m->m_ConstAlbedo.y, m->m_ConstAlbedo.z };
        s.emissive = { m->m_ConstEmissive[0], m->m_ConstEmissive[1], m->m_ConstEmissive[2] };
    }
    s.debugValue = 0.0f; s.roughness = 1.0f; s.metallic = 0.0f;

    const F3 L = { k.m_DirectionalLightVector[0], k.m_DirectionalLightVector[1], k.m_DirectionalLightVector[2] };
    const bool occluded = rw::closestHit(a.scene, origin, L, 0.0f, 1e10f).inst != 0xFFFFFFFFu;
    const F3 lit = dl::litSurface(s, origin, world, L, k.m_DirectionalLightStrength, occluded ? 0.0f : 1.0f);
    const F3 irr = ddgi::irradiance(a.probes, world, s.normal, origin);
    const float kInvPi = 0x1.45f306p-2f;
    const F3 rgb = { lit.x + (cm::min_(s.albedo.x, 0.9f) * kInvPi) * irr.x, lit.y + (cm::min_(s.albedo.y, 0.9f) * kInvPi) * irr.y, lit.z + (cm::min_(s.albedo.z, 0.9f) * kInvPi) * irr.z };
    *out = make_float4(sp::saturate_(rgb.x), sp::saturate_(rgb.y), sp::saturate_(rgb.z), hit.t);
}

int recordProbeTrace(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    ProbeTraceArgs a = sp::zeroed<ProbeTraceArgs>();
    if (const int rc = ddgiu::requireBlock(ctx, a.b)) return rc;
    const DDGIVolumeDesc& D = a.b.D;
    const uint32_t probes = a.numProbes = ddgiu::numProbes(D);
    TRHIP_REQUIRE(!ctx.indirect && ctx.gx == kDDGIRaysPerProbe / kWave && ctx.gy == (uint32_t)D.probeCounts[0] * (uint32_t)D.probeCounts[2] && ctx.gz == (uint32_t)D.probeCounts[1],
                  "%s: needs a direct dispatch of (256 / 64, probeCounts.x * probeCounts.z, probeCounts.y) = (4, %u, %d) groups of 64 threads", name,
                  (uint32_t)D.probeCounts[0] * (uint32_t)D.probeCounts[2], D.probeCounts[1]);
    trhip_buffer_t* descBuffer = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 0);
    TRHIP_REQUIRE(descBuffer && descBuffer->byteSize >= sizeof(DDGIVolumeDesc), "%s: needs StructuredBuffer_SRV t0 = the 64-byte DDGIVolumeDesc", name);
    trhip_texture_t *data, *irr, *dist;
    if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_SRV, 1, TRHIP_FORMAT_RGBA16_FLOAT, 1, "Texture_SRV t1 = the RGBA16_FLOAT array of probe data", D, data)) return rc;
    if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_SRV, 2, TRHIP_FORMAT_R10G10B10A2_UNORM, kDDGIIrradianceInteriorTexels + 2,
                                                  "Texture_SRV t2 = the R10G10B10A2_UNORM array of probe irradiance", D, irr)) return rc;
    if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_SRV, 3, TRHIP_FORMAT_RG16_FLOAT, kDDGIDistanceInteriorTexels + 2,
                                                  "Texture_SRV t3 = the RG16_FLOAT array of probe distance", D, dist)) return rc;
    trhip_buffer_t* rays = ctx.buffer(TRHIP_BIND_STRUCTURED_UAV, 0);
    TRHIP_REQUIRE(rays, "%s: needs StructuredBuffer_UAV u0 = the ray records, float4[numProbes * 256]", name);
    TRHIP_REQUIRE(rays->byteSize == (uint64_t)probes * kDDGIRaysPerProbe * sizeof(float4), "%s: the ray records at u0 hold %llu bytes; %u probes of 256 float4 records are %llu", name,
                  (unsigned long long)rays->byteSize, probes, (unsigned long long)probes * kDDGIRaysPerProbe * sizeof(float4));
    if (const int rc = rw::bindScene(ctx, ddgiu::kSceneSlots, true, a.scene)) return rc;
    ddgi::Textures& p = a.probes;
    p.desc = (const DDGIVolumeDesc*)descBuffer->ptr;
    p.data = (const uint2*)data->ptr; p.irradiance = (const uint32_t*)irr->ptr; p.distance = (const uint32_t*)dist->ptr;
    p.dataW = data->width; p.dataH = data->height; p.irrW = irr->width; p.irrH = irr->height; p.distW = dist->width; p.distH = dist->height;
    p.slices = data->arraySize;
    p.dataPitch = (uint32_t)(data->slicePitch / data->texelBytes); p.irrPitch = (uint32_t)(irr->slicePitch / irr->texelBytes); p.distPitch = (uint32_t)(dist->slicePitch / dist->texelBytes);
    a.rays = (float4*)rays->ptr;
    sp::launch(ctx, probeTraceKernel, "probeTraceKernel", dim3(probes * (kDDGIRaysPerProbe / kWave)), dim3(kWave), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("giprobetrace_CS_ProbeTrace", recordProbeTrace, 0);

} // namespace
