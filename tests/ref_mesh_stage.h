/* ref_mesh_stage.h -- the mesh stage as tests/visibility_ref.c, gbuffer_ref.c, material_textures_ref.c and alpha_test_ref.c
 * share it, stated ONCE: from a list entry or a visibility texel to the screen triangle, its coverage, its perspective weights
 * and its motion.  The CPU counterpart of csrc/mesh_stage.hip.h and csrc/visibility_resolve.hip.h, and independent of both.
 * Needs -I oracle for the buffer layouts of tr_oracle.h.
 *
 * It restates, operation for operation, the vertex and coverage arithmetic of the oracle's depth rasteriser (orc_raster_depth:
 * no near clipping, pixel-centre samples, inclusive edge functions on both windings, depth = one fma chain and one division)
 * and adds this build's conventions:
 *   texel   = (depthBits << 32) | passSlot << 30 | listPosition << 7 | triangle, max-merged per sample (depth > 0);
 *   TIE     = on equal depth the larger payload wins (a maximum of the u64, so independent of the draw order);
 *   triangles with index >= 128 write no texel;
 *   weights = e_i the edge function opposite vertex i times the sign of the triangle's area; q_i = e_i / w_i,
 *             s = (q0 + q1) + q2; interp(a) = fma(q2, a2, fma(q1, a1, q0 * a0)) / s;
 *   motion  = interp of prevWorld = mulPoint(position, m_PrevWorldMatrix); prevClip = 4-column chain with m_PrevWorldToClip;
 *             if prevClip.w > 0: (prevClip.xy / prevClip.w * (0.5, -0.5) + 0.5) * resolution - pixel centre (multiply, then
 *             add), else (0, 0).
 */
#ifndef TESTS_REF_MESH_STAGE_H
#define TESTS_REF_MESH_STAGE_H

#include "ref_base.h"
#include "tr_oracle.h"

typedef struct
{
    const OrcBasePassInstanceConstants* instances; const OrcMeshData* meshData; const OrcMeshletData* meshlets;
    const OrcRawVertexFormat* vertices; const uint32_t* vertexIds; const uint32_t* triangles;
} MsBuffers;

/* One triangle on the screen.  The raster fills everything but world and prev; the texel decode fills everything. */
typedef struct
{
    const OrcMeshletAmplificationData* rec; uint32_t lane;                   /* the record and the meshlet's lane in its group */
    const OrcBasePassInstanceConstants* inst;
    const OrcRawVertexFormat* vtx[3];
    float sx[3], sy[3], sd[3], w[3];                                         /* screen position, depth = z / w, clip w */
    float sgn;                                                               /* -1 when the screen area is negative, else 1 */
    float world[3][3], prev[3][3];                                           /* mulPoint(position, World), (position, PrevWorld) */
} MsTriangle;

static inline void mul_point3(const float p[3], const OrcMatrix* M, float o[3])
{
    for (int j = 0; j < 3; ++j) o[j] = fmaf(p[2], M->m[2][j], fmaf(p[1], M->m[1][j], p[0] * M->m[0][j])) + M->m[3][j];
}

static inline void mul_point_4(const float p[3], const OrcMatrix* M, float o[4])
{
    for (int j = 0; j < 4; ++j) o[j] = fmaf(p[2], M->m[2][j], fmaf(p[1], M->m[1][j], p[0] * M->m[0][j])) + M->m[3][j];
}

/* world position, screen position, depth and clip w of one vertex */
static inline void ms_project(const OrcBasePassConstants* k, const OrcMatrix* world, const float pos[3], float wp[3], float* sx, float* sy, float* sd, float* w)
{
    const float halfW = 0.5f * (float)k->m_OutputResolution[0], halfH = 0.5f * (float)k->m_OutputResolution[1];
    float c[4];
    mul_point3(pos, world, wp);
    mul_point_4(wp, &k->m_WorldToClip, c);
    *w = c[3];
    *sx = fmaf(c[0] / c[3], halfW, halfW);
    *sy = fmaf(-(c[1] / c[3]), halfH, halfH);
    *sd = c[2] / c[3];
}

/* the meshlet of lane `lane` of a record, nothing checked */
static inline const OrcMeshletData* ms_meshlet(const MsBuffers* b, const OrcMeshletAmplificationData* rec, uint32_t lane)
{
    const OrcBasePassInstanceConstants* inst = &b->instances[rec->m_InstanceConstIdx];
    const uint32_t lodIdx = rec->m_MeshLOD < ORC_MAX_LODS ? rec->m_MeshLOD : ORC_MAX_LODS - 1;
    const OrcMeshLODData* lod = &b->meshData[inst->m_MeshDataIdx].m_MeshLODDatas[lodIdx];
    return &b->meshlets[lod->m_MeshletDataBufferIdx + rec->m_MeshletGroupOffset + lane];
}

/* the screen area of the triangle, and its sign into T */
static inline float ms_area(MsTriangle* T)
{
    const float area = edge(T->sx[0], T->sy[0], T->sx[1], T->sy[1], T->sx[2], T->sy[2]);
    T->sgn = area < 0.0f ? -1.0f : 1.0f;
    return area;
}

static inline void ms_edges(const MsTriangle* T, float x, float y, float e[3])
{
    e[0] = T->sgn * edge(T->sx[1], T->sy[1], T->sx[2], T->sy[2], x, y);
    e[1] = T->sgn * edge(T->sx[2], T->sy[2], T->sx[0], T->sy[0], x, y);
    e[2] = T->sgn * edge(T->sx[0], T->sy[0], T->sx[1], T->sy[1], x, y);
}

/* q_i at (x, y), on the triangle's plane extended; returns s */
static inline float ms_weights(const MsTriangle* T, float x, float y, float q[3])
{
    float e[3];
    ms_edges(T, x, y, e);
    for (int j = 0; j < 3; ++j) q[j] = e[j] / T->w[j];
    return (q[0] + q[1]) + q[2];
}

static inline float ms_interp(const float q[3], float s, float a0, float a1, float a2) { return fmaf(q[2], a2, fmaf(q[1], a1, q[0] * a0)) / s; }

/* the motion (float, before the fp16 store) of the sample at (cx, cy) with weights q, s */
static inline void ms_motion(const OrcBasePassConstants* k, const MsTriangle* T, const float q[3], float s, float cx, float cy, float motion[2])
{
    float P[3], clip[4];
    for (int c = 0; c < 3; ++c) P[c] = ms_interp(q, s, T->prev[0][c], T->prev[1][c], T->prev[2][c]);
    mul_point_4(P, &k->m_PrevWorldToClip, clip);
    motion[0] = motion[1] = 0.0f;
    if (clip[3] > 0.0f) {
        const float ux = (clip[0] / clip[3]) * 0.5f + 0.5f, uy = (clip[1] / clip[3]) * -0.5f + 0.5f;
        motion[0] = ux * (float)k->m_OutputResolution[0] - cx;
        motion[1] = uy * (float)k->m_OutputResolution[1] - cy;
    }
}

/* The triangle a texel's payload names; records[s] / lists[s]: the four slots' buffers.
 * limits: NULL (nothing is checked), or numInstances, numMeshes, numMeshlets, numVertices, numVertexIds, numTriangles,
 *         numMaterials, recordCapacity[4], listCapacity[4] (15 values): 0 when the chain of indices leaves a buffer. */
static inline int ms_decode(const OrcBasePassConstants* k, const MsBuffers* b, const OrcMeshletAmplificationData* const* records, const uint32_t* const* lists,
                            const uint64_t* limits, uint32_t payload, MsTriangle* T)
{
    const uint32_t slot = payload >> 30, v = (payload >> 7) & 0x7FFFFFu, t = payload & 127u;
    if (limits && v >= limits[11 + slot]) return 0;
    const uint32_t e = lists[slot][v], g = e >> 5;
    if (limits && g >= limits[7 + slot]) return 0;
    T->rec = &records[slot][g];
    T->lane = e & 31u;
    if (limits && T->rec->m_InstanceConstIdx >= limits[0]) return 0;
    T->inst = &b->instances[T->rec->m_InstanceConstIdx];
    if (limits && (T->inst->m_MeshDataIdx >= limits[1] || T->inst->m_MaterialDataIdx >= limits[6])) return 0;
    if (limits) {
        const uint32_t lodIdx = T->rec->m_MeshLOD < ORC_MAX_LODS ? T->rec->m_MeshLOD : ORC_MAX_LODS - 1;
        if ((uint64_t)b->meshData[T->inst->m_MeshDataIdx].m_MeshLODDatas[lodIdx].m_MeshletDataBufferIdx + T->rec->m_MeshletGroupOffset + T->lane >= limits[2]) return 0;
    }
    const OrcMeshletData* ml = ms_meshlet(b, T->rec, T->lane);
    uint32_t nv = ml->m_VertexAndTriangleCount & 0xFFu;
    const uint32_t nt = (ml->m_VertexAndTriangleCount >> 8) & 0xFFu;
    if (nv > 64u) nv = 64u;
    if (limits && (t >= nt || (uint64_t)ml->m_MeshletIndexIDsBufferIdx + nt > limits[5] || (uint64_t)ml->m_MeshletVertexIDsBufferIdx + nv > limits[4])) return 0;
    const uint32_t packed = b->triangles[ml->m_MeshletIndexIDsBufferIdx + t];
    for (int j = 0; j < 3; ++j) {
        const uint32_t idx = (packed >> (8 * j)) & 0xFFu;
        if (limits && idx >= nv) return 0;
        const uint32_t vid = b->vertexIds[ml->m_MeshletVertexIDsBufferIdx + idx];
        if (limits && vid >= limits[3]) return 0;
        T->vtx[j] = &b->vertices[vid];
        ms_project(k, &T->inst->m_WorldMatrix, T->vtx[j]->m_Position, T->world[j], &T->sx[j], &T->sy[j], &T->sd[j], &T->w[j]);
        mul_point3(T->vtx[j]->m_Position, &T->inst->m_PrevWorldMatrix, T->prev[j]);
    }
    ms_area(T);
    return 1;
}

/* A covered sample (all three e_i >= 0, their sum > 0, depth > 0) of T at pixel centre (cx, cy) is merged iff keep answers
 * nonzero.  boxPixels: the pixels of the triangle's clamped bounding box. */
typedef int (*MsKeep)(void* ctx, const MsTriangle* T, float cx, float cy, uint64_t boxPixels);

/* Rasterises list entry v of pass slot `slot`: depth max-merged into depth[H*W] (as orc_raster_depth), texels max-merged into
 * vis[H*W].  keep: NULL keeps every covered sample. */
static inline void ms_raster_entry(const OrcBasePassConstants* k, const MsBuffers* b, const OrcMeshletAmplificationData* records, const uint32_t* list, uint32_t v,
                                   uint32_t slot, MsKeep keep, void* ctx, float* depth, uint64_t* vis)
{
    const uint32_t W = k->m_OutputResolution[0], H = k->m_OutputResolution[1];
    MsTriangle T;
    T.rec = &records[list[v] >> 5];
    T.lane = list[v] & 31u;
    T.inst = &b->instances[T.rec->m_InstanceConstIdx];
    const OrcMeshletData* ml = ms_meshlet(b, T.rec, T.lane);
    uint32_t nv = ml->m_VertexAndTriangleCount & 0xFFu;
    const uint32_t nt = (ml->m_VertexAndTriangleCount >> 8) & 0xFFu;
    if (nv > 64u) nv = 64u;
    const OrcRawVertexFormat* vtx[64];
    float sx[64], sy[64], sd[64], sw[64], wp[3];
    for (uint32_t i = 0; i < nv; ++i) {
        vtx[i] = &b->vertices[b->vertexIds[ml->m_MeshletVertexIDsBufferIdx + i]];
        ms_project(k, &T.inst->m_WorldMatrix, vtx[i]->m_Position, wp, &sx[i], &sy[i], &sd[i], &sw[i]);
    }
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t packed = b->triangles[ml->m_MeshletIndexIDsBufferIdx + t];
        const uint32_t idx[3] = { packed & 0xFFu, (packed >> 8) & 0xFFu, (packed >> 16) & 0xFFu };
        if (idx[0] >= nv || idx[1] >= nv || idx[2] >= nv) continue;
        for (int j = 0; j < 3; ++j) { T.vtx[j] = vtx[idx[j]]; T.sx[j] = sx[idx[j]]; T.sy[j] = sy[idx[j]]; T.sd[j] = sd[idx[j]]; T.w[j] = sw[idx[j]]; }
        if (!(T.w[0] > k->m_NearPlane && T.w[1] > k->m_NearPlane && T.w[2] > k->m_NearPlane)) continue;
        if (!(ms_area(&T) != 0.0f)) continue;
        const float minx = fminf(fminf(T.sx[0], T.sx[1]), T.sx[2]), maxx = fmaxf(fmaxf(T.sx[0], T.sx[1]), T.sx[2]);
        const float miny = fminf(fminf(T.sy[0], T.sy[1]), T.sy[2]), maxy = fmaxf(fmaxf(T.sy[0], T.sy[1]), T.sy[2]);
        if (!(maxx >= 0.0f && maxy >= 0.0f && minx <= (float)W && miny <= (float)H)) continue;
        const int x0 = (int)fmaxf(floorf(minx), 0.0f), x1 = (int)fminf(ceilf(maxx), (float)(W - 1));
        const int y0 = (int)fmaxf(floorf(miny), 0.0f), y1 = (int)fminf(ceilf(maxy), (float)(H - 1));
        if (x1 < x0 || y1 < y0) continue;
        const uint64_t boxPixels = (uint64_t)(x1 - x0 + 1) * (uint64_t)(y1 - y0 + 1);
        const uint64_t payload = (uint64_t)slot << 30 | (uint64_t)v << 7 | t;
        for (int py = y0; py <= y1; ++py)
            for (int px = x0; px <= x1; ++px) {
                const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
                float e[3];
                ms_edges(&T, cx, cy, e);
                if (!(e[0] >= 0.0f && e[1] >= 0.0f && e[2] >= 0.0f)) continue;
                const float den = (e[0] + e[1]) + e[2];
                if (!(den > 0.0f)) continue;
                const float d = fmaf(e[2], T.sd[2], fmaf(e[1], T.sd[1], e[0] * T.sd[0])) / den;
                if (!(d > 0.0f)) continue;
                if (keep && !keep(ctx, &T, cx, cy, boxPixels)) continue;
                const uint64_t i = (uint64_t)py * W + px;
                if (d > depth[i]) depth[i] = d;
                if (t < 128u) {
                    const uint64_t texel = (uint64_t)bits_of(d) << 32 | payload;
                    if (texel > vis[i]) vis[i] = texel;
                }
            }
    }
}

#endif
