// mesh_stage.hip.h -- the one statement of the base pass's mesh stage, shared by the rasters (k_raster.hip) and the
// resolve from the visibility buffer (visibility_resolve.hip.h): which buffers hold the geometry and how a record binds
// them, how a visible-list entry leads to its meshlet, how a vertex gets to the screen, what the edge function is, and
// what a visibility texel means.  GBufferMotion and GBufferA are bit-exact because the resolve recomputes the winning
// triangle with the raster's operations; they are the raster's operations because both call these.
// Restated independently, on purpose, in oracle/tr_oracle.c and tests/ref_mesh_stage.h (for the C references of tests/).
#pragma once

#include "cull_math.hip.h"
#include "screen_pass.hip.h"
#include "trhip_internal.h"

namespace mesh
{

using namespace interop;

// ---- geometry: t0 instances, t1 vertices, t2 mesh data, t4 meshlets, t5 meshlet vertex ids, t6 meshlet triangles -----
// (BasePassRenderers.cpp:463-479).  Nested right after the constants in the kernels' argument blocks.
struct Geometry
{
    const BasePassInstanceConstants* instances; uint32_t numInstances;
    const MeshData* meshData; uint32_t numMeshes;
    const MeshletData* meshlets; uint64_t numMeshlets;
    const char* vertices; uint64_t numVertices;                 // RawVertexFormat
    const uint32_t* vertexIds; uint64_t numVertexIds;
    const uint32_t* triangles; uint64_t numTriangles;
};

// Elements of `stride` bytes in a buffer, saturated to 32 bits.
inline uint32_t elements32(const trhip_buffer_t* b, size_t stride) { return (uint32_t)std::min<uint64_t>(b->byteSize / stride, 0xFFFFFFFFull); }

inline int bindGeometry(const trhip::DispatchCtx& ctx, Geometry& g)
{
    trhip_buffer_t* instances = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 0);
    trhip_buffer_t* vertices = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 1);
    trhip_buffer_t* meshData = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 2);
    trhip_buffer_t* meshlets = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 4);
    trhip_buffer_t* vids = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 5);
    trhip_buffer_t* tris = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 6);
    TRHIP_REQUIRE(instances && vertices && meshData && meshlets && vids && tris,
                  "%s: needs SRVs t0 (instances), t1 (vertices), t2 (mesh data), t4 (meshlets), t5 (meshlet vertex ids), t6 (meshlet triangles)", ctx.shaderName);
    g.instances = (const BasePassInstanceConstants*)instances->ptr; g.numInstances = elements32(instances, sizeof(BasePassInstanceConstants));
    g.meshData = (const MeshData*)meshData->ptr; g.numMeshes = elements32(meshData, sizeof(MeshData));
    g.meshlets = (const MeshletData*)meshlets->ptr; g.numMeshlets = meshlets->byteSize / sizeof(MeshletData);
    g.vertices = (const char*)vertices->ptr; g.numVertices = vertices->byteSize / sizeof(RawVertexFormat);
    g.vertexIds = (const uint32_t*)vids->ptr; g.numVertexIds = vids->byteSize / 4;
    g.triangles = (const uint32_t*)tris->ptr; g.numTriangles = tris->byteSize / 4;
    return TRHIP_OK;
}

// ---- visible-list entry -> record -> instance -> LOD -> meshlet (basepass.hlsl:138-145) ----------------------------
struct Meshlet
{
    MeshletAmplificationData rec;
    const BasePassInstanceConstants* inst;
    uint32_t lane;                                               // the meshlet's index in its group of 32
    uint32_t vertexIdsAt, trianglesAt;                           // first element in Geometry::vertexIds / ::triangles
    uint32_t nv, nt;                                             // nv clamped to kMaxMeshletVertices
};

// Runs body(meshlet) unless an index on the way is out of bounds.  [vertexIdsAt, + nv) and [trianglesAt, + nt) are then in
// bounds; the vertex ids themselves are not checked (vertexAt's caller does).  A continuation, because a function that
// returns false and fills a struct costs the rasters registers or time (profiles/mesh_stage/README.md).
template <typename Body>
__device__ __forceinline__ void withMeshlet(uint32_t entry, const MeshletAmplificationData* records, uint32_t recordCapacity, const Geometry& g, Body body)
{
    const uint32_t group = entry >> 5, m = entry & 31u;
    if (group >= recordCapacity) return;
    const MeshletAmplificationData rec = records[group];
    if (rec.m_InstanceConstIdx >= g.numInstances) return;
    const BasePassInstanceConstants& inst = g.instances[rec.m_InstanceConstIdx];
    if (inst.m_MeshDataIdx >= g.numMeshes) return;
    const uint32_t lodIdx = rec.m_MeshLOD < kMaxNumMeshLODs ? rec.m_MeshLOD : kMaxNumMeshLODs - 1u;
    const MeshLODData lod = g.meshData[inst.m_MeshDataIdx].m_MeshLODDatas[lodIdx];
    const uint64_t mi = (uint64_t)lod.m_MeshletDataBufferIdx + rec.m_MeshletGroupOffset + m;
    if (mi >= g.numMeshlets) return;
    const MeshletData ml = g.meshlets[mi];
    uint32_t nv = ml.m_VertexAndTriangleCount & 0xFFu, nt = (ml.m_VertexAndTriangleCount >> 8) & 0xFFu;
    nv = nv < kMaxMeshletVertices ? nv : kMaxMeshletVertices;
    if ((uint64_t)ml.m_MeshletVertexIDsBufferIdx + nv > g.numVertexIds || (uint64_t)ml.m_MeshletIndexIDsBufferIdx + nt > g.numTriangles) return;
    body(Meshlet{ rec, &inst, m, ml.m_MeshletVertexIDsBufferIdx, ml.m_MeshletIndexIDsBufferIdx, nv, nt });
}

// vid < g.numVertices
__device__ __forceinline__ const RawVertexFormat& vertexAt(const Geometry& g, uint32_t vid) { return *reinterpret_cast<const RawVertexFormat*>(g.vertices + (uint64_t)vid * sizeof(RawVertexFormat)); }

// ---- object space -> screen (basepass.hlsl:149-158; the operations of orc_raster_depth, one for one) ----------------
struct ScreenVertex { float sx, sy, depth, w; };

// world space -> screen: toScreen behind its world transform (the probe spheres' vertices are made in world space, k_giprobedraw.hip)
__device__ __forceinline__ ScreenVertex worldToScreen(cm::F3 wp, const cm::M43& clipXYZ, const Matrix& worldToClip, float halfW, float halfH)
{
    const cm::F3 c = cm::mulPoint(wp, clipXYZ);
    const float w = cm::fma_(wp.z, worldToClip.m[2][3], cm::fma_(wp.y, worldToClip.m[1][3], wp.x * worldToClip.m[0][3])) + worldToClip.m[3][3];
    return { cm::fma_(c.x / w, halfW, halfW), cm::fma_(-(c.y / w), halfH, halfH), c.z / w, w };
}

__device__ __forceinline__ ScreenVertex toScreen(cm::F3 position, const cm::M43& world, const cm::M43& clipXYZ, const Matrix& worldToClip, float halfW, float halfH)
{
    return worldToScreen(cm::mulPoint(position, world), clipXYZ, worldToClip, halfW, halfH);
}

__device__ __forceinline__ float edgeFn(float ax, float ay, float bx, float by, float px, float py) { return cm::fma_(bx - ax, py - ay, -((by - ay) * (px - ax))); }

// One triangle over the pixels [bx0, bx1] x [by0, by1], `threads` lanes striding over them from `first`; every covered
// pixel that `keep(cx, cy, e0, e1, e2)` does not discard goes to `sink(px, py, depthBits)`.  The arithmetic of
// orc_raster_depth, operation for operation; keep is constant true in the rasters' plain instantiations.
template <typename Keep, typename Sink>
__device__ __forceinline__ void coverBox(float x0, float y0, float d0, float x1, float y1, float d1, float x2, float y2, float d2, float sgn,
                                         uint32_t bx0, uint32_t by0, uint32_t bw, uint32_t bh, uint32_t first, uint32_t threads, Keep keep, Sink sink)
{
    const uint64_t total = (uint64_t)bw * bh;
    for (uint64_t i = first; i < total; i += threads) {
        const uint32_t row = (uint32_t)(i / bw), col = (uint32_t)(i - (uint64_t)row * bw);
        const uint32_t px = bx0 + col, py = by0 + row;
        const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
        const float e0 = sgn * edgeFn(x1, y1, x2, y2, cx, cy), e1 = sgn * edgeFn(x2, y2, x0, y0, cx, cy), e2 = sgn * edgeFn(x0, y0, x1, y1, cx, cy);
        if (!(e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f)) continue;
        const float den = (e0 + e1) + e2;
        if (!(den > 0.0f)) continue;
        const float d = cm::fma_(e2, d2, cm::fma_(e1, d1, e0 * d0)) / den;
        if (d > 0.0f && keep(cx, cy, e0, e1, e2)) sink(px, py, __float_as_uint(d));       // GREATER test; NaN never passes
    }
}

// ---- m_TexCoord and its screen-space derivatives at one sample of a triangle (GetCommonGBufferParams' uv, ddx(uv), ddy(uv)) -----
// The formulas of the TEXTURED resolve (visibility_resolve.hip.h, which keeps its own copy beside the world position it
// interpolates through the same q: its registers are counted, k_gbuffer.hip), used by the rasters' alpha test (k_raster.hip).
// (x_i, y_i, w_i): the vertices' screen positions and clip w; tc_i: the packed half2 m_TexCoord (half -> float is exact); e_i: the
// sample's own signed edge values (e0 against the edge v1 v2, e1 against v2 v0, e2 against v0 v1).  q_i = e_i / w_i,
// s = (q0 + q1) + q2, uv = fma(q2, a2, fma(q1, a1, q0 * a0)) / s; ddx and ddy: the same triangle's plane re-evaluated at
// (cx + 1, cy) and at (cx, cy + 1), minus the centre value.
struct UvFootprint { float u, v, dudx, dvdx, dudy, dvdy; };

__device__ __forceinline__ UvFootprint uvFootprint(float x0, float y0, float x1, float y1, float x2, float y2, float sgn, float w0, float w1, float w2,
                                                   uint32_t tc0, uint32_t tc1, uint32_t tc2, float cx, float cy, float e0, float e1, float e2)
{
    const float q0 = e0 / w0, q1 = e1 / w1, q2 = e2 / w2;
    const float s = (q0 + q1) + q2;
    const float ex0 = sgn * edgeFn(x1, y1, x2, y2, cx + 1.0f, cy), ex1 = sgn * edgeFn(x2, y2, x0, y0, cx + 1.0f, cy), ex2 = sgn * edgeFn(x0, y0, x1, y1, cx + 1.0f, cy);
    const float ey0 = sgn * edgeFn(x1, y1, x2, y2, cx, cy + 1.0f), ey1 = sgn * edgeFn(x2, y2, x0, y0, cx, cy + 1.0f), ey2 = sgn * edgeFn(x0, y0, x1, y1, cx, cy + 1.0f);
    const float qx0 = ex0 / w0, qx1 = ex1 / w1, qx2 = ex2 / w2, qy0 = ey0 / w0, qy1 = ey1 / w1, qy2 = ey2 / w2;
    const float sX = (qx0 + qx1) + qx2, sY = (qy0 + qy1) + qy2;
    const float u0 = (float)sp::halfOf(tc0), u1 = (float)sp::halfOf(tc1), u2 = (float)sp::halfOf(tc2);
    const float v0 = (float)sp::halfOf(tc0 >> 16), v1 = (float)sp::halfOf(tc1 >> 16), v2 = (float)sp::halfOf(tc2 >> 16);
    const float u = cm::fma_(q2, u2, cm::fma_(q1, u1, q0 * u0)) / s, v = cm::fma_(q2, v2, cm::fma_(q1, v1, q0 * v0)) / s;
    return { u, v, cm::fma_(qx2, u2, cm::fma_(qx1, u1, qx0 * u0)) / sX - u, cm::fma_(qx2, v2, cm::fma_(qx1, v1, qx0 * v0)) / sX - v,
             cm::fma_(qy2, u2, cm::fma_(qy1, u1, qy0 * u0)) / sY - u, cm::fma_(qy2, v2, cm::fma_(qy1, v1, qy0 * v0)) / sY - v };
}

// ---- visibility texel: (depthBits << 32) | slot << 30 | listPosition << 7 | triangle ---------------------------------
constexpr uint32_t kVisTriangleBits = 7, kVisListBits = 23;
constexpr uint32_t kVisTriangles = 1u << kVisTriangleBits;       // triangle indices with a visibility texel
constexpr uint32_t kVisListCapacity = 1u << kVisListBits;        // list positions
static_assert(kVisTriangleBits + kVisListBits == 30, "two bits are left for the pass slot");

struct VisTexel { uint32_t slot, listPosition, triangle; };

__host__ __device__ __forceinline__ uint32_t visSlotBits(uint32_t slot) { return slot << (kVisTriangleBits + kVisListBits); }
__device__ __forceinline__ uint32_t packVisibility(uint32_t slotBits, uint32_t listPosition, uint32_t triangle) { return slotBits | listPosition << kVisTriangleBits | triangle; }
__device__ __forceinline__ VisTexel unpackVisibility(uint32_t payload)
{
    return { payload >> (kVisTriangleBits + kVisListBits), (payload >> kVisTriangleBits) & (kVisListCapacity - 1u), payload & (kVisTriangles - 1u) };
}

} // namespace mesh
