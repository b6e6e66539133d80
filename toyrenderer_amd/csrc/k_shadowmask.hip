// k_shadowmask.hip -- "shadowmask_CS_ShadowMask": ShadowMaskRenderer::TraceShadows without denoising (source/ShadowMaskRenderer.cpp
// :253-305, source/shaders/shadowmask.hlsl CS_ShadowMask): one ray per pixel towards the sun through the scene's acceleration
// structure; and "raytracing_CS_RefitTLAS", this build's stand-in for buildTopLevelAccelStructFromBuffer (BasePassRenderers.cpp
// :159-160): the per-frame refit of that structure's top level.  The structure is the project's own (include/trhip.h,
// "acceleration structure"; built on the host by accel_build.cpp).  With m_bDoDenoising != 0 the trace writes the
// penumbra texture that the shadow denoiser reads (k_sigma.hip: DenoiseShadows' place), and "shadowmask_CS_PackNormalAndRoughness"
// (shadowmask.hlsl:147-167) is here too: push constants or b0 PackNormalAndRoughnessConsts (8 bytes), t2 GBufferA, u0
// R10G10B10A2_UNORM, groups of 8 x 8.
//
// BINDINGS of the trace: b0 ShadowMaskConsts (112 bytes), t0 R32_FLOAT depth, t1 the TLAS nodes, t2 GBufferA, t3 instances, t4
// vertices, t5 materials, t6 indices, t7 mesh data, t8 RGBA8_UNORM 128 x 128 blue noise, u0 R8_UNORM mask, u1 R16_FLOAT linear view
// depth; the structure's other buffers: t9 TLAS instances, t10 BLAS headers, t11 BLAS nodes, t12 triangle order; t19 the texture table (optional: see
// `alpha` below).  Samplers are accepted and ignored.  Of the refit: push constants RefitTLASConstants (12 bytes), t0 instances, t1 BLAS headers, t2 BLAS nodes,
// t3 level offsets, t4 level nodes, u0 the TLAS nodes, u1 the TLAS instances.
//
// CONVENTION (tests/shadowmask_ref.c is the definition; the walk, the two tests and the triangle fetch are stated once on the device,
// in ray_walk.hip.h, and occluded() below is a visitor of rw::walk).  IEEE binary32, no contraction, fma only where written, / and
// sqrt correctly rounded:
//   worldPosition, dot3 as screen_pass.hip.h states them; UnpackGBuffer's normal, normalize as k_deferredlighting.hip (gbuffer_unpack.hip.h);
//   noise = (float)byte / 255.0f of the blue noise texel's R and G at (px % 128, py % 128), + m_NoisePhase, fmod(x, 1) = x - trunc(x);
//   MapToCone / CreateTangentVectors as the HLSL with softmath::cosSoft / sinSoft, RN(pi / 4) and RN(pi / 2), cross as cm::cross3,
//             (n + u.x * t0) + u.y * t1; the direction is its normalize; origin = worldPosition + normal * m_RayStartOffset;
//             TMin = m_RayStartOffset, TMax = 1e10f;
//   the walk: rw::walk (ray_walk.hip.h states its rules: skip links, index checks, flags, the move to object space once per instance);
//             objectFromWorld: cofactors / determinant in the order written there;
//   triTest:  the watertight test of Woop, Benthin and Wald in binary32 without the double fallback; two-sided; hit iff
//             TMin < t < TMax.  A candidate on a ForceNonOpaque instance counts iff m_ConstAlbedo.w >= m_AlphaCutoff of the
//             candidate's instance's material (the reference reads Committed* there: shadowmask.hlsl:113-116);
//   alpha:    without a table at t19 that is the whole rule and the kernel of before is launched unchanged.  With one, the TEXTURED
//             instantiation ("#textured" in the profile): a candidate whose material has MaterialFlag_UseAlbedoTexture counts iff
//             m_ConstAlbedo.w * alphaLevel0(uv) >= m_AlphaCutoff (tests/alpha_test_ref.c; see commits()).  Any-hit over independent
//             per-candidate tests stays order-independent, so "equals brute force over every triangle" still holds;
//   boxHit:   conservative: per axis a direction component without a finite reciprocal asks lo <= origin <= hi only (the default
//             light (0, -1, 0) makes every ray axis-parallel, Cornell's walls are boxes of no thickness: no inf * 0 here); else
//             the slab's interval with both ends moved outward by 2^-18 of themselves; node boxes are padded by the builder (2^-16
//             of the mesh's largest |coordinate|) and by the refit (2^-12 of the leaf's largest |coordinate|).  Any-hit over all
//             triangles is order-independent, so the mask equals brute force for any tree as long as boxHit never rejects what
//             triTest accepts: tests/test_shadowmask_ref.py walks the same arrays on the CPU and allows no differing texel;
//   output:   depth == 0.0f: u1 = 0x7BFF, u0 untouched; else u0 = occluded ? 0 : 255, u1 = binary16 RNE of
//             length(worldPosition - m_CameraPosition) (a NaN is stored as 0x7E00);
//   penumbra: m_bDoDenoising != 0 (tests/sigma_ref.c is the definition): u0 must be an R16_FLOAT texture, the R8_UNORM mask is refused.
//             u0 = SIGMA_FrontEnd_PackPenumbra(occluded ? t : kFP16Max, m_TanSunAngularRadius), which NRD's absent header leaves to this
//             project: no occluder 0x7BFF (65504), else binary16 of min(0.5f * (t * m_TanSunAngularRadius), 32768.0f); u1 and far
//             texels as above.  DEVIATION: the reference traces with ACCEPT_FIRST_HIT_AND_END_SEARCH and packs CommittedRayT() of
//             whichever hit came first (its own comment quotes NVIDIA: wrong, long distances); here t is that of the CLOSEST
//             committing candidate: closestCommit(), the third visitor of rw::walk, hands the best t so far to triTest as tmax,
//             runs commits() on what it accepts and never stops.  Only t leaves it: no tie rule, and it equals brute force for any
//             tree.  Profile labels "#penumbra" and "#textured_penumbra"; the two kernels of before keep name, arguments and label;
//   pack:     x, y = the octahedral encoding of UnpackGBuffer's normal (packOctUnorm2x16's mapping with cm::div_) before any 16-bit
//             store, z = roughness, w = 0, each (uint)rint(saturate(v) * 1023.0f) as k_giprobeblend.hip stores UNORM10; every texel.
//
// KERNEL: one thread per pixel, a workgroup is one wave covering the reference's 8 x 8 tile, so the 64 rays of a wave start next
// to each other.  NO STACK: the nodes are in depth-first preorder with skip links (trhip.h), the walk is `hit an inner box ->
// i + 1, else -> skip`, so there is no per-lane array, nothing to overflow, no LDS and no scratch; a link that does not move
// forward ends the walk (a corrupt buffer cannot spin).  Runtime-chosen vector components go through sel() (selects), not through
// an indexed array.  Every index read on the device is checked against its buffer before it is followed.  A wave walks until its
// last lane is done, and lanes that disagree on a box serialise both sides.  MEASURED (tools/shadowmask_cost.py, the generated city
// of 2251 instances at 3840x2160, one MI355X; profiles/ray_walk/README.md): the trace 1.77 ms with hard and 3.51 ms with soft shadows
// next to a lighting pass of 0.10 ms, the refit 35 us.  Untuned: correctness came first.  The TEXTURED instantiation
// (tools/alpha_test_cost.py, the same city with 225 alpha-masked, textured instances): 2.38 ms beside 1.80 ms hard, 4.81 beside 3.55 ms
// soft; 69 VGPRs instead of 58, no scratch.  The penumbra instantiations (-Rpass-analysis=kernel-resource-usage): 56 and 69 VGPRs, the
// pack kernel 23, none with scratch or LDS.  MEASURED (tools/sigma_cost.py, the same city, soft, both traces alternated in one session; profiles/sigma/):
// the penumbra trace 46453 us (spread 71) beside the any-hit trace's 3516 us (6): 13.2 times.  On that scene every ray is occluded:
// the any-hit walk ends at its first committing candidate, the closest-commit walk visits every box the ray's line touches, because
// rw::walk does not prune against the best t so far (ray_walk.hip.h).  Untuned; off by default.
#include "cull_math.hip.h"
#include "gbuffer_unpack.hip.h"
#include "material_textures.hip.h"
#include "ray_walk.hip.h"
#include "screen_pass.hip.h"
#include "soft_math.hip.h"

#include <type_traits>

namespace
{

using namespace interop;
using cm::F3;
using namespace rw;                            // Ray, walk, fetchTri, triTest, bindScene, SceneArgs: ray_walk.hip.h

constexpr uint32_t kTileSide = 8;               // [numthreads(8, 8, 1)]
constexpr uint32_t kRefitBlock = 64;
constexpr float kTlasPad = 0x1p-12f;

struct TraceTargets
{
    ShadowMaskConsts k;
    const float* depth;                        // R32_FLOAT
    const uint4* gbufferA;                     // RGBA32_UINT
    const uint32_t* noise;                     // RGBA8_UNORM, 128 x 128
    uint8_t* mask;                             // R8_UNORM
    uint16_t* lvd;                             // R16_FLOAT
};
struct TraceArgs : TraceTargets, SceneArgs {}; // the members in the order they always had: the scene's pointers follow the targets

// The TEXTURED instantiation's arguments: + the texture table bound at t19.
struct TexturedTraceArgs : TraceArgs
{
    const mtex::TableEntry* table; uint32_t tableCount;
};

// rows r0 r1 r2 r3 of p_object = (p_world, 1) * M, from the rows of m_WorldMatrix
__device__ __forceinline__ void objectFromWorld(const float* w, float* out)
{
    const F3 a = { w[0], w[1], w[2] }, b = { w[4], w[5], w[6] }, c = { w[8], w[9], w[10] }, t = { w[12], w[13], w[14] };
    const float c00 = b.y * c.z - b.z * c.y, c01 = b.z * c.x - b.x * c.z, c02 = b.x * c.y - b.y * c.x;
    const float det = (a.x * c00 + a.y * c01) + a.z * c02;
    float inv[3][3];
    inv[0][0] = cm::div_(c00, det); inv[1][0] = cm::div_(c01, det); inv[2][0] = cm::div_(c02, det);
    inv[0][1] = cm::div_(a.z * c.y - a.y * c.z, det); inv[1][1] = cm::div_(a.x * c.z - a.z * c.x, det); inv[2][1] = cm::div_(a.y * c.x - a.x * c.y, det);
    inv[0][2] = cm::div_(a.y * b.z - a.z * b.y, det); inv[1][2] = cm::div_(a.z * b.x - a.x * b.z, det); inv[2][2] = cm::div_(a.x * b.y - a.y * b.x, det);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[3 * i + j] = inv[i][j];
#pragma unroll
    for (int j = 0; j < 3; ++j) out[9 + j] = -((t.x * inv[0][j] + t.y * inv[1][j]) + t.z * inv[2][j]);
}

// ---- "raytracing_CS_RefitTLAS" --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRefitBlock) void refitLeavesKernel(const BasePassInstanceConstants* __restrict__ instances, uint32_t numInstances,
                                                                 const trhip_blas_header* __restrict__ headers, uint32_t numMeshes,
                                                                 const trhip_accel_node* __restrict__ blasNodes, uint32_t numBlasNodes,
                                                                 trhip_accel_node* nodes, uint32_t numNodes, trhip_tlas_instance* records)
{
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= numInstances) return;
    const uint32_t flags = records[i].flags, leafNode = records[i].leaf_node;
    if (!flags || leafNode >= numNodes) return;
    float w[16];
    const float4* src = reinterpret_cast<const float4*>(&instances[i].m_WorldMatrix);
#pragma unroll
    for (int r = 0; r < 4; ++r) { const float4 v = src[r]; w[4 * r] = v.x; w[4 * r + 1] = v.y; w[4 * r + 2] = v.z; w[4 * r + 3] = v.w; }
    float m[12];
    objectFromWorld(w, m);
#pragma unroll
    for (int j = 0; j < 12; ++j) records[i].object_from_world[j] = m[j];
    const uint32_t mesh = instances[i].m_MeshDataIdx;
    float lo[3] = { kFloatMax, kFloatMax, kFloatMax }, hi[3] = { -kFloatMax, -kFloatMax, -kFloatMax };
    if (mesh < numMeshes && headers[mesh].num_nodes && headers[mesh].node_offset < numBlasNodes) {
        const trhip_accel_node root = blasNodes[headers[mesh].node_offset];
        float largest = 0.0f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const F3 p = { c & 1 ? root.hi[0] : root.lo[0], c & 2 ? root.hi[1] : root.lo[1], c & 4 ? root.hi[2] : root.lo[2] };
            const float q[3] = { cm::fma_(p.z, w[8], cm::fma_(p.y, w[4], p.x * w[0])) + w[12], cm::fma_(p.z, w[9], cm::fma_(p.y, w[5], p.x * w[1])) + w[13],
                                 cm::fma_(p.z, w[10], cm::fma_(p.y, w[6], p.x * w[2])) + w[14] };
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = cm::min_(lo[a], q[a]); hi[a] = cm::max_(hi[a], q[a]); largest = cm::max_(largest, __builtin_fabsf(q[a])); }
        }
        const float pad = kTlasPad * largest;
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = lo[a] - pad; hi[a] = hi[a] + pad; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { nodes[leafNode].lo[a] = lo[a]; nodes[leafNode].hi[a] = hi[a]; }
}

// One workgroup: the inner boxes height by height, children before parents.  A tree of n leaves has n - 1 inner nodes in at most
// 56 heights; the barrier between two heights also orders this group's stores to global memory before its next loads.
constexpr uint32_t kInnerBlock = 256;
__global__ __launch_bounds__(kInnerBlock) void refitInnerKernel(const uint32_t* __restrict__ levelOffsets, const uint32_t* __restrict__ levelNodes, uint32_t numLevels,
                                                                uint32_t numLevelNodes, trhip_accel_node* nodes, uint32_t numNodes)
{
    for (uint32_t l = 0; l < numLevels; ++l) {
        const uint32_t begin = levelOffsets[l], end = levelOffsets[l + 1] < numLevelNodes ? levelOffsets[l + 1] : numLevelNodes;
        for (uint32_t k = begin + threadIdx.x; k < end; k += kInnerBlock) {
            const uint32_t n = levelNodes[k];
            if (n >= numNodes || n + 1 >= numNodes) continue;
            const uint32_t right = nodes[n + 1].skip;
            if (right >= numNodes) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                nodes[n].lo[a] = cm::min_(nodes[n + 1].lo[a], nodes[right].lo[a]);
                nodes[n].hi[a] = cm::max_(nodes[n + 1].hi[a], nodes[right].hi[a]);
            }
        }
        __syncthreads();
    }
}

int recordRefit(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const RefitTLASConstants* k = (const RefitTLASConstants*)ctx.constants(0, sizeof(RefitTLASConstants));
    TRHIP_REQUIRE(k, "%s: push constants (RefitTLASConstants, 12 bytes) missing or of another size", name);
    TRHIP_REQUIRE(!ctx.indirect, "%s: needs a direct dispatch of 64-thread groups", name);
    trhip_buffer_t* instances = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 0);
    trhip_buffer_t* headers = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 1);
    trhip_buffer_t* blasNodes = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 2);
    trhip_buffer_t* levelOffsets = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 3);
    trhip_buffer_t* levelNodes = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 4);
    trhip_buffer_t* nodes = ctx.buffer(TRHIP_BIND_STRUCTURED_UAV, 0);
    trhip_buffer_t* records = ctx.buffer(TRHIP_BIND_STRUCTURED_UAV, 1);
    TRHIP_REQUIRE(instances && headers && blasNodes && levelOffsets && levelNodes && nodes && records,
                  "%s: needs SRVs t0 (instances), t1 (BLAS headers), t2 (BLAS nodes), t3 (level offsets), t4 (level nodes) and UAVs u0 (TLAS nodes), u1 (TLAS instances)", name);
    const uint32_t n = k->m_NumInstances;
    TRHIP_REQUIRE((uint64_t)n * sizeof(BasePassInstanceConstants) <= instances->byteSize, "%s: %u instances exceed the instance buffer", name, n);
    TRHIP_REQUIRE((uint64_t)n * sizeof(trhip_tlas_instance) <= records->byteSize, "%s: %u instances exceed the TLAS instance buffer", name, n);
    TRHIP_REQUIRE((uint64_t)k->m_NumNodes * sizeof(trhip_accel_node) <= nodes->byteSize, "%s: %u nodes exceed the TLAS node buffer", name, k->m_NumNodes);
    TRHIP_REQUIRE(((uint64_t)k->m_NumLevels + 1) * 4 <= levelOffsets->byteSize, "%s: %u levels exceed the level offset buffer", name, k->m_NumLevels);
    TRHIP_REQUIRE((uint64_t)ctx.gx * kRefitBlock >= n, "%s: a direct dispatch of 64-thread groups covering %u instances", name, n);
    if (!n || !k->m_NumNodes) return TRHIP_OK;
    const RefitTLASConstants kk = *k;
    const BasePassInstanceConstants* ip = (const BasePassInstanceConstants*)instances->ptr;
    const trhip_blas_header* hp = (const trhip_blas_header*)headers->ptr;
    const trhip_accel_node* bp = (const trhip_accel_node*)blasNodes->ptr;
    const uint32_t numMeshes = (uint32_t)(headers->byteSize / sizeof(trhip_blas_header)), numBlasNodes = (uint32_t)(blasNodes->byteSize / sizeof(trhip_accel_node));
    const uint32_t* lo = (const uint32_t*)levelOffsets->ptr; const uint32_t* ln = (const uint32_t*)levelNodes->ptr;
    const uint32_t numLevelNodes = (uint32_t)(levelNodes->byteSize / 4);
    trhip_accel_node* np = (trhip_accel_node*)nodes->ptr;
    trhip_tlas_instance* rp = (trhip_tlas_instance*)records->ptr;
    ctx.emit("main", [=](hipStream_t s) {
        TRHIP_LAUNCH(refitLeavesKernel, dim3((kk.m_NumInstances + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, s, ip, kk.m_NumInstances, hp, numMeshes, bp, numBlasNodes,
                     np, kk.m_NumNodes, rp);
        if (kk.m_NumLevels)
            TRHIP_LAUNCH(refitInnerKernel, dim3(1), dim3(kInnerBlock), 0, s, lo, ln, kk.m_NumLevels, numLevelNodes, np, kk.m_NumNodes);
        return trhip::launchStatus("refitTLAS"); });
    return TRHIP_OK;
}

// ---- the ray of one pixel -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fmod1(float x) { return x - __builtin_truncf(x); }

__device__ __forceinline__ F3 mapToCone(float sx, float sy, F3 n, float radius)                     // shadowmask.hlsl:24-63
{
    const float ox = 2.0f * sx - 1.0f, oy = 2.0f * sy - 1.0f;
    if (ox == 0.0f && oy == 0.0f) return n;
    float theta, r;
    if (__builtin_fabsf(ox) > __builtin_fabsf(oy)) { r = ox; theta = 0x1.921fb6p-1f * cm::div_(oy, ox); }
    else { r = oy; theta = 0x1.921fb6p+0f * (1.0f - 0.5f * cm::div_(ox, oy)); }
    const float ux = (radius * r) * softmath::cosSoft(theta), uy = (radius * r) * softmath::sinSoft(theta);
    const bool zUp = __builtin_fabsf(n.z) < 0.99999f;
    const F3 up = { zUp ? 0.0f : 1.0f, 0.0f, zUp ? 1.0f : 0.0f };
    const F3 t0 = gbuf::normalize_(cm::cross3(up, n)), t1 = cm::cross3(n, t0);
    return { (n.x + ux * t0.x) + uy * t1.x, (n.y + ux * t0.y) + uy * t1.y, (n.z + ux * t0.z) + uy * t1.z };
}

// A candidate: the triangle's texture coordinates (packed half2) and the hit's barycentrics.  TEXTURED only.
struct Candidate { uint32_t tc[3]; float b1, b2; };

// the candidate counts: ForceOpaque always, ForceNonOpaque by the alpha test of its instance's material (GetCommonGBufferParams
// without textures).  TEXTURED (tests/alpha_test_ref.c: at_commits): a material with MaterialFlag_UseAlbedoTexture counts iff
// m_ConstAlbedo.w * alphaLevel0(uv) >= m_AlphaCutoff, uv as InterpolateVertex (raytracingcommon.hlsli:24-36, :189) has it:
// b0 = (1.0f - b1) - b2, uv = ((0 + uv0 * b0) + uv1 * b1) + uv2 * b2, not fused.  DEVIATION: the reference calls Sample in a
// compute shader, where the derivatives come from unrelated neighbouring rays; this build reads mip 0.  A descriptor index past
// the table, an empty entry or one of another format: the candidate does not count.
template <bool TEXTURED, typename Args>
__device__ __forceinline__ bool commits(const Args& a, uint32_t inst, uint32_t flags, const Candidate& c)
{
    if (flags != kTLASInstanceForceNonOpaque) return true;
    const uint32_t mat = a.instances[inst].m_MaterialDataIdx;
    if (mat >= a.numMaterials) return false;
    const MaterialData* m = reinterpret_cast<const MaterialData*>(a.materials + (uint64_t)mat * sizeof(MaterialData));
    if constexpr (TEXTURED) {
        if (m->m_MaterialFlags & MaterialFlag_UseAlbedoTexture) {
            const uint32_t d = m->m_AlbedoTexture.m_DescriptorIndex;
            if (d >= a.tableCount || !mtex::sampled(a.table[d])) return false;
            const float b0 = (1.0f - c.b1) - c.b2;
            const float u = ((0.0f + (float)sp::halfOf(c.tc[0]) * b0) + (float)sp::halfOf(c.tc[1]) * c.b1) + (float)sp::halfOf(c.tc[2]) * c.b2;
            const float v = ((0.0f + (float)sp::halfOf(c.tc[0] >> 16) * b0) + (float)sp::halfOf(c.tc[1] >> 16) * c.b1) + (float)sp::halfOf(c.tc[2] >> 16) * c.b2;
            return m->m_ConstAlbedo.w * mtex::alphaLevel0(a.table[d], m->m_AlbedoTexture.m_IsWrapSampler != 0u, u, v) >= m->m_AlphaCutoff;
        }
    }
    return m->m_ConstAlbedo.w >= m->m_AlphaCutoff;
}

template <bool TEXTURED>
__device__ __forceinline__ bool meshTriHit(const TraceArgs& a, const MeshData* md, uint32_t tri, const Ray& r, float tmin, float tmax, Candidate& c, float& t)
{
    Tri T;
    TriHit h;
    if (!fetchTri(a, md, tri, T) || !triTest(T.v[0], T.v[1], T.v[2], r, tmin, tmax, h)) return false;
    t = h.t;
    if constexpr (TEXTURED) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c.tc[k] = *reinterpret_cast<const uint32_t*>(a.vertices + T.i[k] * sizeof(RawVertexFormat) + offsetof(RawVertexFormat, m_TexCoord));
        c.b1 = h.b1; c.b2 = h.b2;
    }
    return true;
}

// The any-hit visitor of rw::walk (tests/shadowmask_ref.c: occluded_walk): the first candidate that is hit and counts ends the walk.
template <bool TEXTURED, typename Args>
__device__ bool occluded(const Args& a, F3 o, F3 d, float tmin, float tmax)
{
    return walk(a, o, d, [&](uint32_t inst, uint32_t flags, const MeshData* md, uint32_t tri, const Ray& r) {
        Candidate c;
        float t;
        return meshTriHit<TEXTURED>(a, md, tri, r, tmin, tmax, c, t) && commits<TEXTURED>(a, inst, flags, c); });
}

// TEXTURED: a texture table is bound at t19 and alpha-mask candidates read their albedo texture's alpha (commits).
template <bool TEXTURED>
__global__ __launch_bounds__(kTileSide * kTileSide) void shadowMaskKernel(std::conditional_t<TEXTURED, TexturedTraceArgs, TraceArgs> a)
{
    const ShadowMaskConsts& k = a.k;
    const uint32_t W = k.m_OutputResolution.x, H = k.m_OutputResolution.y;
    const sp::Pixel at = sp::pixel<kTileSide, kTileSide>();
    if (!at.inside(W, H)) return;
    const uint32_t px = at.x, py = at.y;
    const uint64_t i = at.index(W);
    const float depth = a.depth[i];
    if (depth == 0.0f) { a.lvd[i] = 0x7BFFu; return; }                                             // kFarDepth: u1 = kFP16Max, u0 untouched
    // sp::worldPosition's operations written out: through the call the compiler resolves this kernel's arguments differently, spills
    // 45 scalar registers instead of 10, and the trace measured 1 % slower (profiles/shadowmask/README.md).  Keep the two alike.
    const float u = cm::div_((float)px + 0.5f, (float)W), v = cm::div_((float)py + 0.5f, (float)H);
    const float cx = u * 2.0f + -1.0f, cy = v * -2.0f + 1.0f;                                      // UVToClipXY
    float h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        h[j] = cm::fma_(depth, k.m_ClipToWorld.m[2][j], cm::fma_(cy, k.m_ClipToWorld.m[1][j], cx * k.m_ClipToWorld.m[0][j])) + k.m_ClipToWorld.m[3][j];
    const F3 wp = { cm::div_(h[0], h[3]), cm::div_(h[1], h[3]), cm::div_(h[2], h[3]) };
    const F3 n = gbuf::unpackGBuffer(a.gbufferA[i]).normal;
    const uint32_t texel = a.noise[(py % kBlueNoiseSize) * kBlueNoiseSize + (px % kBlueNoiseSize)];
    const float sx = fmod1(cm::div_((float)(texel & 0xFFu), 255.0f) + k.m_NoisePhase), sy = fmod1(cm::div_((float)((texel >> 8) & 0xFFu), 255.0f) + k.m_NoisePhase);
    const F3 light = { k.m_DirectionalLightDirection[0], k.m_DirectionalLightDirection[1], k.m_DirectionalLightDirection[2] };
    const F3 d = gbuf::normalize_(mapToCone(sx, sy, light, k.m_TanSunAngularRadius));
    const F3 o = { wp.x + n.x * k.m_RayStartOffset, wp.y + n.y * k.m_RayStartOffset, wp.z + n.z * k.m_RayStartOffset };
    const bool occ = occluded<TEXTURED>(a, o, d, k.m_RayStartOffset, 1e10f);
    a.mask[i] = occ ? 0u : 255u;
    const F3 toCamera = { wp.x - k.m_CameraPosition[0], wp.y - k.m_CameraPosition[1], wp.z - k.m_CameraPosition[2] };
    const float len = cm::sqrt_(cm::dot3(toCamera, toCamera));
    a.lvd[i] = sp::halfBits(len);
}

// The closest-commit visitor of rw::walk (tests/sigma_ref.c: closest_commit_walk): every candidate that triTest accepts below the best t
// so far and that commits() replaces it; the walk is never stopped.  Only t leaves, so no tie rule is needed and the answer is
// brute force's minimum whatever the tree.  Returns tmax when nothing commits.
template <bool TEXTURED, typename Args>
__device__ float closestCommit(const Args& a, F3 o, F3 d, float tmin, float tmax)
{
    float best = tmax;
    walk(a, o, d, [&](uint32_t inst, uint32_t flags, const MeshData* md, uint32_t tri, const Ray& r) {
        Candidate c;
        float t;
        if (meshTriHit<TEXTURED>(a, md, tri, r, tmin, best, c, t) && commits<TEXTURED>(a, inst, flags, c)) best = t;
        return false; });
    return best;
}

// m_bDoDenoising != 0: u0 (a.mask) is the R16_FLOAT penumbra texture.  The texel's ray is shadowMaskKernel's, statement for statement,
// and written out for the reason given there: with the ray in one shared __forceinline__ function the compiler spills 40 and 53 scalar
// registers in the two mask kernels instead of 4 and 18, and 11 and 27 in these two instead of 0 and 2 (-Rpass-analysis=kernel-
// resource-usage).  Keep the two alike.  The candidate's test IS shared: meshTriHit hands back t.
template <bool TEXTURED>
__global__ __launch_bounds__(kTileSide * kTileSide) void shadowPenumbraKernel(std::conditional_t<TEXTURED, TexturedTraceArgs, TraceArgs> a)
{
    const ShadowMaskConsts& k = a.k;
    const uint32_t W = k.m_OutputResolution.x, H = k.m_OutputResolution.y;
    const sp::Pixel at = sp::pixel<kTileSide, kTileSide>();
    if (!at.inside(W, H)) return;
    const uint32_t px = at.x, py = at.y;
    const uint64_t i = at.index(W);
    const float depth = a.depth[i];
    if (depth == 0.0f) { a.lvd[i] = 0x7BFFu; return; }
    const float u = cm::div_((float)px + 0.5f, (float)W), v = cm::div_((float)py + 0.5f, (float)H);
    const float cx = u * 2.0f + -1.0f, cy = v * -2.0f + 1.0f;
    float h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        h[j] = cm::fma_(depth, k.m_ClipToWorld.m[2][j], cm::fma_(cy, k.m_ClipToWorld.m[1][j], cx * k.m_ClipToWorld.m[0][j])) + k.m_ClipToWorld.m[3][j];
    const F3 wp = { cm::div_(h[0], h[3]), cm::div_(h[1], h[3]), cm::div_(h[2], h[3]) };
    const F3 n = gbuf::unpackGBuffer(a.gbufferA[i]).normal;
    const uint32_t texel = a.noise[(py % kBlueNoiseSize) * kBlueNoiseSize + (px % kBlueNoiseSize)];
    const float sx = fmod1(cm::div_((float)(texel & 0xFFu), 255.0f) + k.m_NoisePhase), sy = fmod1(cm::div_((float)((texel >> 8) & 0xFFu), 255.0f) + k.m_NoisePhase);
    const F3 light = { k.m_DirectionalLightDirection[0], k.m_DirectionalLightDirection[1], k.m_DirectionalLightDirection[2] };
    const F3 d = gbuf::normalize_(mapToCone(sx, sy, light, k.m_TanSunAngularRadius));
    const F3 o = { wp.x + n.x * k.m_RayStartOffset, wp.y + n.y * k.m_RayStartOffset, wp.z + n.z * k.m_RayStartOffset };
    const float tmax = 1e10f;
#ifdef TR_SIGMA_MUTATE_FIRST_HIT               // negative control only (profiles/sigma/mutations.txt): the first committing candidate's t, as the reference takes it
    float t = tmax;
    walk(a, o, d, [&](uint32_t inst, uint32_t flags, const MeshData* md, uint32_t tri, const Ray& r) {
        Candidate c;
        return meshTriHit<TEXTURED>(a, md, tri, r, k.m_RayStartOffset, tmax, c, t) && commits<TEXTURED>(a, inst, flags, c); }) || (t = tmax);
#else
    const float t = closestCommit<TEXTURED>(a, o, d, k.m_RayStartOffset, tmax);
#endif
    // SIGMA_FrontEnd_PackPenumbra as this project fixes it: no occluder 65504, else min(0.5f * (t * tan), 32768)
    reinterpret_cast<uint16_t*>(a.mask)[i] = (uint16_t)(t < tmax ? sp::halfBits(cm::min_(0.5f * (t * k.m_TanSunAngularRadius), 32768.0f)) : 0x7BFFu);
    const F3 toCamera = { wp.x - k.m_CameraPosition[0], wp.y - k.m_CameraPosition[1], wp.z - k.m_CameraPosition[2] };
    a.lvd[i] = sp::halfBits(cm::sqrt_(cm::dot3(toCamera, toCamera)));
}

int recordShadowMask(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const ShadowMaskConsts* k = (const ShadowMaskConsts*)ctx.constants(0, sizeof(ShadowMaskConsts));
    TRHIP_REQUIRE(k, "%s: constant buffer b0 (ShadowMaskConsts, 112 bytes) missing or short", name);
    const bool penumbra = k->m_bDoDenoising != 0u;                                                  // u0 is then the R16_FLOAT penumbra texture (ShadowMaskRenderer.cpp:259)
    const uint32_t W = k->m_OutputResolution.x, H = k->m_OutputResolution.y;
    TRHIP_REQUIRE(W && H, "%s: m_OutputResolution %ux%u is empty", name, W, H);
    if (const int rc = sp::requireCover(ctx, kTileSide, kTileSide, W, H)) return rc;
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_R32_FLOAT, "Texture_SRV t0 = the R32_FLOAT depth buffer (one mip)", true, sp::kOneMipAt0 },
                                 { TRHIP_BIND_TEXTURE_SRV, 2, TRHIP_FORMAT_RGBA32_UINT, "Texture_SRV t2 = the RGBA32_UINT GBufferA (one mip)", true, sp::kOneMipAt0 },
                                 penumbra ? sp::Binding{ TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_R16_FLOAT, "Texture_UAV u0 = the R16_FLOAT shadow penumbra texture, which m_bDoDenoising != 0 writes in place of the mask (one mip)", true, sp::kOneMipAt0 }
                                          : sp::Binding{ TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_R8_UNORM, "Texture_UAV u0 = the R8_UNORM shadow mask (one mip)", true, sp::kOneMipAt0 },
                                 { TRHIP_BIND_TEXTURE_UAV, 1, TRHIP_FORMAT_R16_FLOAT, "Texture_UAV u1 = the R16_FLOAT linear view depth (one mip)", true, sp::kOneMipAt0 } };
    const sp::Binding wantNoise[] = { { TRHIP_BIND_TEXTURE_SRV, 8, TRHIP_FORMAT_RGBA8_UNORM, "Texture_SRV t8 = the RGBA8_UNORM 128x128 blue noise", true, sp::kOneMipAt0 } };
    trhip_texture_t *tex[4], *noise[1];
    if (const int rc = sp::bindTextures(ctx, want, tex, W, H, "m_OutputResolution")) return rc;
    if (const int rc = sp::bindTextures(ctx, wantNoise, noise, kBlueNoiseSize, kBlueNoiseSize, "the blue noise")) return rc;
    TRHIP_REQUIRE(tex[2] != tex[3], "%s: u0 and u1 are the same texture '%s'", name, tex[2]->name.c_str());
    TexturedTraceArgs a = sp::zeroed<TexturedTraceArgs>();                                          // TraceArgs + the table; sliced when none is bound
    if (const int rc = bindScene(ctx, { 1, 3, 4, 5, 6, 7, 9, 10, 11, 12 }, true, a)) return rc;
    a.k = *k;
    a.depth = (const float*)tex[0]->ptr; a.gbufferA = (const uint4*)tex[1]->ptr; a.mask = (uint8_t*)tex[2]->ptr; a.lvd = (uint16_t*)tex[3]->ptr;
    a.noise = (const uint32_t*)noise[0]->ptr;
    if (trhip_texture_table_t* table = ctx.textureTable(19)) {                                      // t19: the TEXTURED instantiation
        for (size_t d = 0; d < table->slots.size(); ++d)
            TRHIP_REQUIRE(!table->slots[d] || !table->slots[d]->isUAV, "%s: the texture table at t19 holds '%s' at index %zu, created with the UAV or render-target bit: a sampled texture is read only",
                          name, table->slots[d]->name.c_str(), d);
        TRHIP_REQUIRE(table->entries.ptr, "%s: the texture table at t19 has no device data", name);
        a.table = (const mtex::TableEntry*)table->entries.ptr;
        a.tableCount = (uint32_t)table->slots.size();
        if (penumbra)
            sp::launch(ctx, shadowPenumbraKernel<true>, "shadowPenumbraKernel<textured>", sp::tiles(W, H, kTileSide, kTileSide), dim3(kTileSide, kTileSide), a, "textured_penumbra");
        else
            sp::launch(ctx, shadowMaskKernel<true>, "shadowMaskKernel<textured>", sp::tiles(W, H, kTileSide, kTileSide), dim3(kTileSide, kTileSide), a, "textured");
        return TRHIP_OK;
    }
    const TraceArgs plain = a;
    if (penumbra) {
        sp::launch(ctx, shadowPenumbraKernel<false>, "shadowPenumbraKernel", sp::tiles(W, H, kTileSide, kTileSide), dim3(kTileSide, kTileSide), plain, "penumbra");
        return TRHIP_OK;
    }
    sp::launch(ctx, shadowMaskKernel<false>, "shadowMaskKernel", sp::tiles(W, H, kTileSide, kTileSide), dim3(kTileSide, kTileSide), plain);
    return TRHIP_OK;
}

// ---- "shadowmask_CS_PackNormalAndRoughness" (shadowmask.hlsl:147-167) -------------------------------------------------------------
struct PackArgs { const uint4* gbufferA; uint32_t* out; uint32_t W, H; };

__device__ __forceinline__ uint32_t unorm10(float v) { return (uint32_t)__builtin_rintf(sp::saturate_(v) * 1023.0f); }    // k_giprobeblend.hip's store rule

__global__ __launch_bounds__(sp::kBlock) void packNormalRoughnessKernel(PackArgs a)
{
    const sp::Pixel at = sp::pixel();
    if (!at.inside(a.W, a.H)) return;
    const uint64_t i = at.index(a.W);
    const gbuf::GBufferParams p = gbuf::unpackGBuffer(a.gbufferA[i]);
    const F3 n = p.normal;
    const float l1 = (__builtin_fabsf(n.x) + __builtin_fabsf(n.y)) + __builtin_fabsf(n.z);
    const float x = cm::div_(n.x, l1), y = cm::div_(n.y, l1), z = cm::div_(n.z, l1);
    float ox = x, oy = y;
    if (!(z >= 0.0f)) {                                                                              // the lower hemisphere folds over
        ox = (1.0f - __builtin_fabsf(y)) * (x >= 0.0f ? 1.0f : -1.0f);
        oy = (1.0f - __builtin_fabsf(x)) * (y >= 0.0f ? 1.0f : -1.0f);
    }
    a.out[i] = unorm10(ox * 0.5f + 0.5f) | unorm10(oy * 0.5f + 0.5f) << 10 | unorm10(p.roughness) << 20;      // w = 0
}

int recordPackNormalRoughness(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const PackNormalAndRoughnessConsts* k = (const PackNormalAndRoughnessConsts*)ctx.constants(0, sizeof(PackNormalAndRoughnessConsts));
    TRHIP_REQUIRE(k, "%s: b0 or push constants (PackNormalAndRoughnessConsts, 8 bytes) missing", name);
    const uint32_t W = k->m_OutputResolution.x, H = k->m_OutputResolution.y;
    TRHIP_REQUIRE(W && H, "%s: m_OutputResolution %ux%u is empty", name, W, H);
    if (const int rc = sp::requireCover(ctx, kTileSide, kTileSide, W, H)) return rc;
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 2, TRHIP_FORMAT_RGBA32_UINT, "Texture_SRV t2 = the RGBA32_UINT GBufferA (one mip)", true, sp::kOneMipAt0 },
                                 { TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_R10G10B10A2_UNORM, "Texture_UAV u0 = the R10G10B10A2_UNORM normal roughness texture (one mip)", true, sp::kOneMipAt0 } };
    trhip_texture_t* tex[2];
    if (const int rc = sp::bindTextures(ctx, want, tex, W, H, "m_OutputResolution")) return rc;
    const PackArgs a = { (const uint4*)tex[0]->ptr, (uint32_t*)tex[1]->ptr, W, H };
    sp::launch(ctx, packNormalRoughnessKernel, "packNormalRoughnessKernel", sp::tiles(W, H), dim3(sp::kTileW, sp::kTileH), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("shadowmask_CS_ShadowMask", recordShadowMask, 0);
trhip::ShaderRegistrar r1("raytracing_CS_RefitTLAS", recordRefit, 0);
trhip::ShaderRegistrar r2("shadowmask_CS_PackNormalAndRoughness", recordPackNormalRoughness, 0);

} // namespace
