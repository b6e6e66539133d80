// k_motion.hip -- "basepass_PS_Main_motion": the motion target (GBufferMotion, RG16_FLOAT) of the reference's base pass
// (source/shaders/basepass.hlsl:226-237 GetGBufferParams: prevClip = mul(float4(prevWorldPos, 1), m_PrevWorldToClip),
// motion = ClipXYToUV(prevClip.xy / prevClip.w) * m_OutputResolution - svPosition.xy, 0 when prevClip.w <= 0), resolved
// from the visibility buffer that "basepass_MS_Main_visibility" (k_raster.hip) wrote, in one direct dispatch after the
// base pass's last raster.
//
// CONVENTION (parity unpinned; restated in tests/visibility_ref.c): per pixel with a nonzero texel, decode slot, list
// position and triangle; recompute the three vertices' screen positions and clip w with the raster's exact operations and
// the edge functions at the pixel centre; interpolate prevWorld = mulPoint(position, m_PrevWorldMatrix) with perspective
// weights q_i = e_i / w_i, s = (q0 + q1) + q2, per component fma(q2, P2, fma(q1, P1, q0 * P0)) / s; prevClip = the
// 4-column chain of orc_raster_depth's mul_point4; ClipXYToUV = xy * (0.5, -0.5) + 0.5 as a multiply then an add.  Both
// components are stored as fp16, round to nearest even (a NaN as 0x7E00).  Pixels without a texel keep their value.
//
// Cost: meant to be bound by the 8-byte texel read plus a gather (list entry, record, instance, meshlet, triangle, three
// vertices) per covered pixel.  About 8.3 M pixels at 3840x2160 make roughly 100 MB, so a few tens of us were expected;
// tools/visibility_cost.py measured 134 us on a 2251-instance city at 3840x2160 with a 1-D grid-stride mapping: the
// per-pixel gather and the recomputation (~10 divisions) dominate, not the texel stream.  Now one workgroup per 16x16
// pixels (no 64-bit divide; a wave's 16x4 pixels mostly share a triangle, so its gathers hit the same lines): 104 us.  A per-wave
// triangle cache could go further; not done.
#include "cull_math.hip.h"
#include "trhip_internal.h"

using namespace interop;

namespace
{

constexpr uint32_t kTileW = 16, kTileH = 16;   // one workgroup per 16x16 pixels: a wave covers 16x4 neighbouring pixels
constexpr uint32_t kBlock = kTileW * kTileH;
constexpr uint32_t kGroupSide = 8;              // the reference entry's [numthreads(8, 8, 1)]: group counts cover the screen

struct MotionArgs
{
    BasePassConstants k;
    const BasePassInstanceConstants* instances; uint32_t numInstances;
    const MeshData* meshData; uint32_t numMeshes;
    const MeshletData* meshlets; uint64_t numMeshlets;
    const char* vertices; uint64_t numVertices;                 // RawVertexFormat, 20-byte stride
    const uint32_t* vertexIds; uint64_t numVertexIds;
    const uint32_t* triangles; uint64_t numTriangles;
    const MeshletAmplificationData* records[4]; uint32_t recordCapacity[4];
    const uint32_t* lists[4]; uint32_t listCapacity[4];
    const unsigned long long* vis;                               // RG32_UINT as u64
    uint32_t* motion;                                            // RG16_FLOAT: x in the low half, y in the high half
    uint32_t width, height;
};

__device__ __forceinline__ float edgeFn(float ax, float ay, float bx, float by, float px, float py)
{
    return cm::fma_(bx - ax, py - ay, -((by - ay) * (px - ax)));
}

__device__ __forceinline__ uint32_t toHalfBits(float f)
{
    if (f != f) return 0x7E00u;                                                          // one NaN
    const _Float16 h = (_Float16)f;                                                      // round to nearest even
    return (uint32_t)__builtin_bit_cast(uint16_t, h);
}

__global__ __launch_bounds__(kBlock) void motionKernel(MotionArgs a)
{
    const float halfW = 0.5f * (float)a.width, halfH = 0.5f * (float)a.height;
    const uint32_t px = blockIdx.x * kTileW + threadIdx.x, py = blockIdx.y * kTileH + threadIdx.y;
    if (px >= a.width || py >= a.height) return;
    const uint64_t i = (uint64_t)py * a.width + px;
    const unsigned long long texel = a.vis[i];
    if (!texel) return;
    const uint32_t payload = (uint32_t)texel;
    const uint32_t slot = payload >> 30, v = (payload >> 7) & 0x7FFFFFu, t = payload & 127u;
    if (v >= a.listCapacity[slot]) return;
    const uint32_t e = a.lists[slot][v], g = e >> 5, m = e & 31u;
    if (g >= a.recordCapacity[slot]) return;
    const MeshletAmplificationData rec = a.records[slot][g];
    if (rec.m_InstanceConstIdx >= a.numInstances) return;
    const BasePassInstanceConstants& inst = a.instances[rec.m_InstanceConstIdx];
    if (inst.m_MeshDataIdx >= a.numMeshes) return;
    const uint32_t lodIdx = rec.m_MeshLOD < kMaxNumMeshLODs ? rec.m_MeshLOD : kMaxNumMeshLODs - 1u;
    const MeshLODData lod = a.meshData[inst.m_MeshDataIdx].m_MeshLODDatas[lodIdx];
    const uint64_t mi = (uint64_t)lod.m_MeshletDataBufferIdx + rec.m_MeshletGroupOffset + m;
    if (mi >= a.numMeshlets) return;
    const MeshletData ml = a.meshlets[mi];
    uint32_t nv = ml.m_VertexAndTriangleCount & 0xFFu;
    const uint32_t nt = (ml.m_VertexAndTriangleCount >> 8) & 0xFFu;
    nv = nv < 64u ? nv : 64u;
    if (t >= nt || (uint64_t)ml.m_MeshletIndexIDsBufferIdx + nt > a.numTriangles || (uint64_t)ml.m_MeshletVertexIDsBufferIdx + nv > a.numVertexIds) return;
    const uint32_t packed = a.triangles[ml.m_MeshletIndexIDsBufferIdx + t];
    const uint32_t idx[3] = { packed & 0xFFu, (packed >> 8) & 0xFFu, (packed >> 16) & 0xFFu };
    if (idx[0] >= nv || idx[1] >= nv || idx[2] >= nv) return;
    const cm::M43 Wm = cm::loadM43(inst.m_WorldMatrix), Pm = cm::loadM43(inst.m_PrevWorldMatrix);
    const cm::M43 clipXYZ = cm::loadM43(a.k.m_WorldToClip);
    float sx[3], sy[3], w[3];
    cm::F3 prev[3];
    bool ok = true;
    for (int j = 0; j < 3; ++j) {                                                   // the raster's vertex arithmetic
        const uint32_t vid = a.vertexIds[ml.m_MeshletVertexIDsBufferIdx + idx[j]];
        if (vid >= a.numVertices) { ok = false; break; }
        const float* p = reinterpret_cast<const float*>(a.vertices + (uint64_t)vid * 20u);
        const cm::F3 pos = { p[0], p[1], p[2] };
        const cm::F3 wp = cm::mulPoint(pos, Wm);
        const cm::F3 c = cm::mulPoint(wp, clipXYZ);
        w[j] = cm::fma_(wp.z, a.k.m_WorldToClip.m[2][3], cm::fma_(wp.y, a.k.m_WorldToClip.m[1][3], wp.x * a.k.m_WorldToClip.m[0][3])) + a.k.m_WorldToClip.m[3][3];
        sx[j] = cm::fma_(c.x / w[j], halfW, halfW);
        sy[j] = cm::fma_(-(c.y / w[j]), halfH, halfH);
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
    a.motion[i] = toHalfBits(mx) | toHalfBits(my) << 16;
}

int recordMotion(trhip::DispatchCtx& ctx)
{
    const BasePassConstants* k = (const BasePassConstants*)ctx.constants(0, sizeof(BasePassConstants));
    TRHIP_REQUIRE(k, "%s: constant buffer b0 (BasePassConstants, 256 bytes) missing", ctx.shaderName);
    trhip_buffer_t* instances = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 0);
    trhip_buffer_t* vertices = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 1);
    trhip_buffer_t* meshData = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 2);
    trhip_buffer_t* meshlets = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 4);
    trhip_buffer_t* vids = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 5);
    trhip_buffer_t* tris = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 6);
    TRHIP_REQUIRE(instances && vertices && meshData && meshlets && vids && tris,
                  "%s: needs SRVs t0 (instances), t1 (vertices), t2 (mesh data), t4 (meshlets), t5 (meshlet vertex ids), t6 (meshlet triangles)", ctx.shaderName);
    trhip_buffer_t* records[4];
    trhip_buffer_t* lists[4];
    for (uint32_t s = 0; s < 4; ++s) {
        records[s] = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 10 + s);
        lists[s] = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 14 + s);
        TRHIP_REQUIRE(records[s] && lists[s], "%s: needs the records of all four pass slots at t10..t13 and their visible lists at t14..t17 (slot %u missing)", ctx.shaderName, s);
    }
    trhip_texture_t* vis = ctx.texture(TRHIP_BIND_TEXTURE_SRV, 18);
    uint32_t mip = 0;
    trhip_texture_t* motion = ctx.texture(TRHIP_BIND_TEXTURE_UAV, 0, &mip);
    TRHIP_REQUIRE(vis && vis->format == TRHIP_FORMAT_RG32_UINT, "%s: needs Texture_SRV t18 = the RG32_UINT visibility buffer", ctx.shaderName);
    TRHIP_REQUIRE(motion && mip == 0 && motion->format == TRHIP_FORMAT_RG16_FLOAT, "%s: needs Texture_UAV u0 = the RG16_FLOAT motion target, mip 0", ctx.shaderName);
    const uint32_t W = k->m_OutputResolution.x, H = k->m_OutputResolution.y;
    TRHIP_REQUIRE(vis->width == W && vis->height == H && motion->width == W && motion->height == H,
                  "%s: visibility buffer %ux%u and motion target %ux%u must both be m_OutputResolution %ux%u", ctx.shaderName, vis->width, vis->height, motion->width, motion->height, W, H);
    TRHIP_REQUIRE(!ctx.indirect && (uint64_t)ctx.gx * kGroupSide >= W && (uint64_t)ctx.gy * kGroupSide >= H,
                  "%s: a direct dispatch of 8x8-pixel groups covering %ux%u", ctx.shaderName, W, H);
    MotionArgs a;
    memset(&a, 0, sizeof a);
    a.k = *k;
    a.instances = (const BasePassInstanceConstants*)instances->ptr; a.numInstances = (uint32_t)std::min<uint64_t>(instances->byteSize / sizeof(BasePassInstanceConstants), 0xFFFFFFFFull);
    a.meshData = (const MeshData*)meshData->ptr; a.numMeshes = (uint32_t)std::min<uint64_t>(meshData->byteSize / sizeof(MeshData), 0xFFFFFFFFull);
    a.meshlets = (const MeshletData*)meshlets->ptr; a.numMeshlets = meshlets->byteSize / sizeof(MeshletData);
    a.vertices = (const char*)vertices->ptr; a.numVertices = vertices->byteSize / 20u;
    a.vertexIds = (const uint32_t*)vids->ptr; a.numVertexIds = vids->byteSize / 4;
    a.triangles = (const uint32_t*)tris->ptr; a.numTriangles = tris->byteSize / 4;
    for (uint32_t s = 0; s < 4; ++s) {
        a.records[s] = (const MeshletAmplificationData*)records[s]->ptr;
        a.recordCapacity[s] = (uint32_t)std::min<uint64_t>(records[s]->byteSize / sizeof(MeshletAmplificationData), 0xFFFFFFFFull);
        a.lists[s] = (const uint32_t*)lists[s]->ptr;
        a.listCapacity[s] = (uint32_t)std::min<uint64_t>(lists[s]->byteSize / 4, 0xFFFFFFFFull);
    }
    a.vis = (const unsigned long long*)vis->ptr;
    a.motion = (uint32_t*)motion->ptr;
    a.width = W; a.height = H;
    const dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH);
    ctx.emit("main", [a, grid](hipStream_t s) {
        TRHIP_LAUNCH(motionKernel, grid, dim3(kTileW, kTileH), 0, s, a);
        return trhip::launchStatus("motionKernel"); });
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("basepass_PS_Main_motion", recordMotion, 0);

} // namespace
