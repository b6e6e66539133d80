/* visibility_ref.c -- test reference of the visibility buffer and the motion target (k_raster.hip
 * "basepass_MS_Main_visibility", k_motion.hip "basepass_PS_Main_motion").  Compiled by the tests themselves with
 * gcc -O2 -ffp-contract=off: only the fmaf calls written here fuse.
 *
 * Restates, operation for operation, the vertex and coverage arithmetic of the oracle's depth rasteriser
 * (orc_raster_depth: no near clipping, pixel-centre samples, inclusive edge functions on both windings, depth = one fma
 * chain and one division) and adds this build's conventions:
 *   texel   = (depthBits << 32) | passSlot << 30 | listPosition << 7 | triangle, max-merged per sample (depth > 0);
 *   TIE     = on equal depth the larger payload wins (a maximum of the u64, so independent of the draw order);
 *   triangles with index >= 128 write no texel;
 *   motion  = perspective-correct interpolation of prevWorld = mulPoint(position, m_PrevWorldMatrix) with q_i = e_i / w_i,
 *             s = (q0 + q1) + q2, fma(q2, P2, fma(q1, P1, q0 * P0)) / s; prevClip = 4-column chain with
 *             m_PrevWorldToClip; if prevClip.w > 0: (prevClip.xy / prevClip.w * (0.5, -0.5) + 0.5) * resolution - pixel
 *             centre (multiply, then add), else (0, 0).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "tr_oracle.h"

static void mul_point3(const float p[3], const OrcMatrix* M, float o[3])
{
    for (int j = 0; j < 3; ++j) o[j] = fmaf(p[2], M->m[2][j], fmaf(p[1], M->m[1][j], p[0] * M->m[0][j])) + M->m[3][j];
}

static void mul_point_4(const float p[3], const OrcMatrix* M, float o[4])
{
    for (int j = 0; j < 4; ++j) o[j] = fmaf(p[2], M->m[2][j], fmaf(p[1], M->m[1][j], p[0] * M->m[0][j])) + M->m[3][j];
}

static float edge(float ax, float ay, float bx, float by, float px, float py)
{
    return fmaf(bx - ax, py - ay, -((by - ay) * (px - ax)));
}

static uint32_t f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* screen position, depth and clip w of one vertex, as the raster computes them */
static void project(const OrcBasePassConstants* k, const OrcMatrix* world, const float pos[3], float* sx, float* sy, float* sd, float* w)
{
    const float halfW = 0.5f * (float)k->m_OutputResolution[0], halfH = 0.5f * (float)k->m_OutputResolution[1];
    float wp[3], c[4];
    mul_point3(pos, world, wp);
    mul_point_4(wp, &k->m_WorldToClip, c);
    *w = c[3];
    *sx = fmaf(c[0] / c[3], halfW, halfW);
    *sy = fmaf(-(c[1] / c[3]), halfH, halfH);
    *sd = c[2] / c[3];
}

static const OrcMeshletData* meshlet_of(const OrcBasePassInstanceConstants* instances, const OrcMeshData* meshData, const OrcMeshletData* meshlets,
                                        const OrcMeshletAmplificationData* rec, uint32_t lane)
{
    const OrcBasePassInstanceConstants* inst = &instances[rec->m_InstanceConstIdx];
    const uint32_t lodIdx = rec->m_MeshLOD < ORC_MAX_LODS ? rec->m_MeshLOD : ORC_MAX_LODS - 1;
    const OrcMeshLODData* lod = &meshData[inst->m_MeshDataIdx].m_MeshLODDatas[lodIdx];
    return &meshlets[lod->m_MeshletDataBufferIdx + rec->m_MeshletGroupOffset + lane];
}

/* Rasterises the listed meshlets of pass slot `slot`: depth max-merged into depth[H*W] (as orc_raster_depth), texels
 * max-merged into vis[H*W].  order: NULL or a permutation of [0, numVisible) to draw the list in. */
void vr_raster(const OrcBasePassConstants* k, const OrcBasePassInstanceConstants* instances, const OrcMeshData* meshData,
               const OrcMeshletData* meshlets, const OrcRawVertexFormat* vertices, const uint32_t* vertexIds, const uint32_t* triangles,
               const OrcMeshletAmplificationData* records, const uint32_t* list, uint32_t numVisible, const uint32_t* order, uint32_t slot,
               float* depth, uint64_t* vis)
{
    const uint32_t W = k->m_OutputResolution[0], H = k->m_OutputResolution[1];
    for (uint32_t n = 0; n < numVisible; ++n) {
        const uint32_t v = order ? order[n] : n;
        const OrcMeshletAmplificationData* rec = &records[list[v] >> 5];
        const OrcMeshletData* ml = meshlet_of(instances, meshData, meshlets, rec, list[v] & 31u);
        const OrcMatrix* world = &instances[rec->m_InstanceConstIdx].m_WorldMatrix;
        uint32_t nv = ml->m_VertexAndTriangleCount & 0xFFu;
        const uint32_t nt = (ml->m_VertexAndTriangleCount >> 8) & 0xFFu;
        if (nv > 64u) nv = 64u;
        float sx[64], sy[64], sd[64];
        int ok[64];
        for (uint32_t i = 0; i < nv; ++i) {
            float w;
            project(k, world, vertices[vertexIds[ml->m_MeshletVertexIDsBufferIdx + i]].m_Position, &sx[i], &sy[i], &sd[i], &w);
            ok[i] = w > k->m_NearPlane;
        }
        for (uint32_t t = 0; t < nt; ++t) {
            const uint32_t packed = triangles[ml->m_MeshletIndexIDsBufferIdx + t];
            const uint32_t a = packed & 0xFFu, b = (packed >> 8) & 0xFFu, c = (packed >> 16) & 0xFFu;
            if (a >= nv || b >= nv || c >= nv || !(ok[a] && ok[b] && ok[c])) continue;
            const float area = edge(sx[a], sy[a], sx[b], sy[b], sx[c], sy[c]);
            if (!(area != 0.0f)) continue;
            const float sgn = area < 0.0f ? -1.0f : 1.0f;
            const float minx = fminf(fminf(sx[a], sx[b]), sx[c]), maxx = fmaxf(fmaxf(sx[a], sx[b]), sx[c]);
            const float miny = fminf(fminf(sy[a], sy[b]), sy[c]), maxy = fmaxf(fmaxf(sy[a], sy[b]), sy[c]);
            if (!(maxx >= 0.0f && maxy >= 0.0f && minx <= (float)W && miny <= (float)H)) continue;
            const int x0 = (int)fmaxf(floorf(minx), 0.0f), x1 = (int)fminf(ceilf(maxx), (float)(W - 1));
            const int y0 = (int)fmaxf(floorf(miny), 0.0f), y1 = (int)fminf(ceilf(maxy), (float)(H - 1));
            const uint64_t payload = (uint64_t)slot << 30 | (uint64_t)v << 7 | t;
            for (int py = y0; py <= y1; ++py)
                for (int px = x0; px <= x1; ++px) {
                    const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
                    const float e0 = sgn * edge(sx[b], sy[b], sx[c], sy[c], cx, cy);
                    const float e1 = sgn * edge(sx[c], sy[c], sx[a], sy[a], cx, cy);
                    const float e2 = sgn * edge(sx[a], sy[a], sx[b], sy[b], cx, cy);
                    if (!(e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f)) continue;
                    const float den = (e0 + e1) + e2;
                    if (!(den > 0.0f)) continue;
                    const float d = fmaf(e2, sd[c], fmaf(e1, sd[b], e0 * sd[a])) / den;
                    if (!(d > 0.0f)) continue;
                    const uint64_t i = (uint64_t)py * W + px;
                    if (d > depth[i]) depth[i] = d;
                    if (t < 128u) {
                        const uint64_t texel = (uint64_t)f32_bits(d) << 32 | payload;
                        if (texel > vis[i]) vis[i] = texel;
                    }
                }
        }
    }
}

/* Motion (float, before the fp16 store) of every pixel with a nonzero texel; others are left as they are.  records[s] /
 * lists[s]: the four slots' buffers. */
void vr_motion(const OrcBasePassConstants* k, const OrcBasePassInstanceConstants* instances, const OrcMeshData* meshData,
               const OrcMeshletData* meshlets, const OrcRawVertexFormat* vertices, const uint32_t* vertexIds, const uint32_t* triangles,
               const OrcMeshletAmplificationData* const* records, const uint32_t* const* lists, const uint64_t* vis, float* motion)
{
    const uint32_t W = k->m_OutputResolution[0], H = k->m_OutputResolution[1];
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const uint64_t i = (uint64_t)py * W + px;
            if (!vis[i]) continue;
            const uint32_t payload = (uint32_t)vis[i];
            const uint32_t slot = payload >> 30, v = (payload >> 7) & 0x7FFFFFu, t = payload & 127u;
            const uint32_t e = lists[slot][v];
            const OrcMeshletAmplificationData* rec = &records[slot][e >> 5];
            const OrcMeshletData* ml = meshlet_of(instances, meshData, meshlets, rec, e & 31u);
            const OrcBasePassInstanceConstants* inst = &instances[rec->m_InstanceConstIdx];
            const uint32_t packed = triangles[ml->m_MeshletIndexIDsBufferIdx + t];
            const uint32_t idx[3] = { packed & 0xFFu, (packed >> 8) & 0xFFu, (packed >> 16) & 0xFFu };
            float sx[3], sy[3], sd[3], w[3], prev[3][3];
            for (int j = 0; j < 3; ++j) {
                const float* pos = vertices[vertexIds[ml->m_MeshletVertexIDsBufferIdx + idx[j]]].m_Position;
                project(k, &inst->m_WorldMatrix, pos, &sx[j], &sy[j], &sd[j], &w[j]);
                mul_point3(pos, &inst->m_PrevWorldMatrix, prev[j]);
            }
            const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
            const float area = edge(sx[0], sy[0], sx[1], sy[1], sx[2], sy[2]);
            const float sgn = area < 0.0f ? -1.0f : 1.0f;
            const float e0 = sgn * edge(sx[1], sy[1], sx[2], sy[2], cx, cy);
            const float e1 = sgn * edge(sx[2], sy[2], sx[0], sy[0], cx, cy);
            const float e2 = sgn * edge(sx[0], sy[0], sx[1], sy[1], cx, cy);
            const float q0 = e0 / w[0], q1 = e1 / w[1], q2 = e2 / w[2];
            const float s = (q0 + q1) + q2;
            float P[3], clip[4];
            for (int c = 0; c < 3; ++c) P[c] = fmaf(q2, prev[2][c], fmaf(q1, prev[1][c], q0 * prev[0][c])) / s;
            mul_point_4(P, &k->m_PrevWorldToClip, clip);
            float mx = 0.0f, my = 0.0f;
            if (clip[3] > 0.0f) {
                const float ux = (clip[0] / clip[3]) * 0.5f + 0.5f, uy = (clip[1] / clip[3]) * -0.5f + 0.5f;
                mx = ux * (float)W - cx;
                my = uy * (float)H - cy;
            }
            motion[2 * i] = mx;
            motion[2 * i + 1] = my;
        }
}
