/* gbuffer_ref.c -- test reference of GBufferA and the fused motion target (visibility_resolve.hip.h,
 * "basepass_PS_Main_GBuffer").  Compiled by the tests themselves with gcc -O2 -ffp-contract=off: only the fmaf calls
 * written here fuse.
 *
 * Restates the resolve of tests/visibility_ref.c (vr_motion: decode, vertex arithmetic, edge functions, q_i = e_i / w_i,
 * s = (q0 + q1) + q2, motion) and adds, per covered pixel:
 *   N_i    = normalize(mul(unpack(m_PackedNormal), adjugate(World3x3))): R10G10B10A2, x in bits 20-29, y 10-19, z 0-9,
 *            (float)q / 1023.0f, * 2.0f, - 1.0f; adjugate rows cross(r1, r2), cross(r2, r0), cross(r0, r1), each component
 *            fmaf(a, b, -(c * d)); the row-vector product as an fmaf chain; v / sqrtf(dot3(v, v));
 *   normal = fmaf(q2, N2, fmaf(q1, N1, q0 * N0)) / s, not renormalised;
 *   x = RGBA8(albedo.rgb, debugValue), y = unorm 2x16 of the octahedral normal, z = R9G9B9E5(emissive), w = 0xFF
 *            (roughness 1, metallic 0: the constants the reference's shader uses without a texture);
 *   saturate(x) = fminf(fmaxf(x, 0), 1) (a NaN gives 0), uint(x) truncates, round = rintf (half to even);
 *   debugValue by m_DebugMode: 2 QuickRandomFloat(instance), 3 QuickRandomFloat(m_MeshletGroupOffset + lane),
 *            12 (float)m_MeshLOD / 255.0f, else 0.
 * A pixel whose chain of indices leaves a buffer (the counts in `limits`) is left as it is in both outputs.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "tr_oracle.h"

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static float saturate(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

uint32_t gr_pack_rgba8(float r, float g, float b, float a)
{
    return (uint32_t)(saturate(r) * 255.0f) | (uint32_t)(saturate(g) * 255.0f) << 8 | (uint32_t)(saturate(b) * 255.0f) << 16 |
           (uint32_t)(saturate(a) * 255.0f) << 24;
}

uint32_t gr_pack_oct(float nx, float ny, float nz)
{
    const float l1 = (fabsf(nx) + fabsf(ny)) + fabsf(nz);
    const float x = nx / l1, y = ny / l1, z = nz / l1;
    float ox = x, oy = y;
    if (!(z >= 0.0f)) {
        ox = (1.0f - fabsf(y)) * (x >= 0.0f ? 1.0f : -1.0f);
        oy = (1.0f - fabsf(x)) * (y >= 0.0f ? 1.0f : -1.0f);
    }
    ox = ox * 0.5f + 0.5f;
    oy = oy * 0.5f + 0.5f;
    const uint32_t ux = (uint32_t)rintf(saturate(ox) * 65535.0f), uy = (uint32_t)rintf(saturate(oy) * 65535.0f);
    return ux | uy << 16;
}

uint32_t gr_pack_r9g9b9e5(float r, float g, float b)
{
    const float kMaxVal = float_of(0x477F8000u), kMinVal = float_of(0x37800000u);
    r = fminf(fmaxf(r, 0.0f), kMaxVal);
    g = fminf(fmaxf(g, 0.0f), kMaxVal);
    b = fminf(fmaxf(b, 0.0f), kMaxVal);
    const float maxChannel = fmaxf(fmaxf(kMinVal, r), fmaxf(g, b));
    const float bias = float_of((bits_of(maxChannel) + 0x07804000u) & 0x7F800000u);
    const uint32_t R = bits_of(r + bias), G = bits_of(g + bias), B = bits_of(b + bias);
    const uint32_t E = (bits_of(bias) << 4) + 0x10000000u;
    return E | B << 18 | G << 9 | (R & 0x1FFu);
}

float gr_quick_random_float(uint32_t seed)
{
    seed = 1664525u * seed + 1013904223u;
    return (float)(seed & 0x00FFFFFFu) / 16777216.0f;
}

float gr_mesh_lod_value(uint32_t lod) { return (float)lod / 255.0f; }

void gr_unpack_normal(uint32_t packed, float o[3])
{
    const float x = (float)((packed >> 20) & 0x3FFu) / 1023.0f, y = (float)((packed >> 10) & 0x3FFu) / 1023.0f, z = (float)(packed & 0x3FFu) / 1023.0f;
    o[0] = x * 2.0f - 1.0f; o[1] = y * 2.0f - 1.0f; o[2] = z * 2.0f - 1.0f;
}

/* array forms for the tests */
void gr_pack_rgba8_n(const float* rgba, uint64_t n, uint32_t* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gr_pack_rgba8(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]); }
void gr_pack_oct_n(const float* xyz, uint64_t n, uint32_t* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gr_pack_oct(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]); }
void gr_pack_r9g9b9e5_n(const float* rgb, uint64_t n, uint32_t* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gr_pack_r9g9b9e5(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]); }
void gr_quick_random_float_n(const uint32_t* seeds, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gr_quick_random_float(seeds[i]); }
void gr_mesh_lod_value_n(const uint32_t* lods, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gr_mesh_lod_value(lods[i]); }
void gr_unpack_normal_n(const uint32_t* words, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) gr_unpack_normal(words[i], out + 3 * i); }

static void cross3(const float a[3], const float b[3], float o[3])
{
    o[0] = fmaf(a[1], b[2], -(a[2] * b[1]));
    o[1] = fmaf(a[2], b[0], -(a[0] * b[2]));
    o[2] = fmaf(a[0], b[1], -(a[1] * b[0]));
}

/* normalize(mul(unpack(word), adjugate(World3x3))) */
void gr_vertex_normal(uint32_t word, const OrcMatrix* world, float o[3])
{
    float u[3], r0[3], r1[3], r2[3], n[3];
    gr_unpack_normal(word, u);
    cross3(world->m[1], world->m[2], r0);
    cross3(world->m[2], world->m[0], r1);
    cross3(world->m[0], world->m[1], r2);
    for (int j = 0; j < 3; ++j) n[j] = fmaf(u[2], r2[j], fmaf(u[1], r1[j], u[0] * r0[j]));
    const float len = sqrtf(fmaf(n[2], n[2], fmaf(n[1], n[1], n[0] * n[0])));
    for (int j = 0; j < 3; ++j) o[j] = n[j] / len;
}

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

/* MaterialData: 124-byte stride, floats 0-3 albedo, 4-6 emissive */
#define GR_MATERIAL_STRIDE 124u

/* limits: numInstances, numMeshes, numMeshlets, numVertices, numVertexIds, numTriangles, numMaterials,
 *         recordCapacity[4], listCapacity[4]  (15 values)
 * gbuffer: uint32[H*W*4]; motion: float[H*W*2] (before the fp16 store).  Pixels without a texel, or whose chain leaves a
 * buffer, are left as they are. */
void gr_gbuffer(const OrcBasePassConstants* k, const OrcBasePassInstanceConstants* instances, const OrcMeshData* meshData,
                const OrcMeshletData* meshlets, const OrcRawVertexFormat* vertices, const uint32_t* vertexIds, const uint32_t* triangles,
                const OrcMeshletAmplificationData* const* records, const uint32_t* const* lists, const uint64_t* vis,
                const unsigned char* materials, const uint64_t* limits, uint32_t* gbuffer, float* motion)
{
    const uint32_t W = k->m_OutputResolution[0], H = k->m_OutputResolution[1];
    const float halfW = 0.5f * (float)W, halfH = 0.5f * (float)H;
    const uint64_t numInstances = limits[0], numMeshes = limits[1], numMeshlets = limits[2], numVertices = limits[3],
                   numVertexIds = limits[4], numTriangles = limits[5], numMaterials = limits[6];
    const uint64_t* recordCapacity = limits + 7;
    const uint64_t* listCapacity = limits + 11;
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const uint64_t i = (uint64_t)py * W + px;
            if (!vis[i]) continue;
            const uint32_t payload = (uint32_t)vis[i];
            const uint32_t slot = payload >> 30, v = (payload >> 7) & 0x7FFFFFu, t = payload & 127u;
            if (v >= listCapacity[slot]) continue;
            const uint32_t e = lists[slot][v], g = e >> 5, lane = e & 31u;
            if (g >= recordCapacity[slot]) continue;
            const OrcMeshletAmplificationData* rec = &records[slot][g];
            if (rec->m_InstanceConstIdx >= numInstances) continue;
            const OrcBasePassInstanceConstants* inst = &instances[rec->m_InstanceConstIdx];
            if (inst->m_MeshDataIdx >= numMeshes || inst->m_MaterialDataIdx >= numMaterials) continue;
            const uint32_t lodIdx = rec->m_MeshLOD < ORC_MAX_LODS ? rec->m_MeshLOD : ORC_MAX_LODS - 1;
            const OrcMeshLODData* lod = &meshData[inst->m_MeshDataIdx].m_MeshLODDatas[lodIdx];
            const uint64_t mi = (uint64_t)lod->m_MeshletDataBufferIdx + rec->m_MeshletGroupOffset + lane;
            if (mi >= numMeshlets) continue;
            const OrcMeshletData* ml = &meshlets[mi];
            uint32_t nv = ml->m_VertexAndTriangleCount & 0xFFu;
            const uint32_t nt = (ml->m_VertexAndTriangleCount >> 8) & 0xFFu;
            if (nv > 64u) nv = 64u;
            if (t >= nt || (uint64_t)ml->m_MeshletIndexIDsBufferIdx + nt > numTriangles || (uint64_t)ml->m_MeshletVertexIDsBufferIdx + nv > numVertexIds) continue;
            const uint32_t packed = triangles[ml->m_MeshletIndexIDsBufferIdx + t];
            const uint32_t idx[3] = { packed & 0xFFu, (packed >> 8) & 0xFFu, (packed >> 16) & 0xFFu };
            if (idx[0] >= nv || idx[1] >= nv || idx[2] >= nv) continue;
            float sx[3], sy[3], w[3], prev[3][3], N[3][3];
            int ok = 1;
            for (int j = 0; j < 3; ++j) {
                const uint32_t vid = vertexIds[ml->m_MeshletVertexIDsBufferIdx + idx[j]];
                if (vid >= numVertices) { ok = 0; break; }
                const float* pos = vertices[vid].m_Position;
                float wp[3], c[4];
                mul_point3(pos, &inst->m_WorldMatrix, wp);
                mul_point_4(wp, &k->m_WorldToClip, c);
                w[j] = c[3];
                sx[j] = fmaf(c[0] / c[3], halfW, halfW);
                sy[j] = fmaf(-(c[1] / c[3]), halfH, halfH);
                mul_point3(pos, &inst->m_PrevWorldMatrix, prev[j]);
                gr_vertex_normal(vertices[vid].m_PackedNormal, &inst->m_WorldMatrix, N[j]);
            }
            if (!ok) continue;
            const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
            const float area = edge(sx[0], sy[0], sx[1], sy[1], sx[2], sy[2]);
            const float sgn = area < 0.0f ? -1.0f : 1.0f;
            const float e0 = sgn * edge(sx[1], sy[1], sx[2], sy[2], cx, cy);
            const float e1 = sgn * edge(sx[2], sy[2], sx[0], sy[0], cx, cy);
            const float e2 = sgn * edge(sx[0], sy[0], sx[1], sy[1], cx, cy);
            const float q0 = e0 / w[0], q1 = e1 / w[1], q2 = e2 / w[2];
            const float s = (q0 + q1) + q2;
            float P[3], clip[4], n[3];
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
            for (int c = 0; c < 3; ++c) n[c] = fmaf(q2, N[2][c], fmaf(q1, N[1][c], q0 * N[0][c])) / s;
            float debugValue = 0.0f;
            if (k->m_DebugMode == 2u) debugValue = gr_quick_random_float(rec->m_InstanceConstIdx);
            else if (k->m_DebugMode == 3u) debugValue = gr_quick_random_float(rec->m_MeshletGroupOffset + lane);
            else if (k->m_DebugMode == 12u) debugValue = gr_mesh_lod_value(rec->m_MeshLOD);
            float mat[7];
            memcpy(mat, materials + (uint64_t)inst->m_MaterialDataIdx * GR_MATERIAL_STRIDE, sizeof mat);
            gbuffer[4 * i] = gr_pack_rgba8(mat[0], mat[1], mat[2], debugValue);
            gbuffer[4 * i + 1] = gr_pack_oct(n[0], n[1], n[2]);
            gbuffer[4 * i + 2] = gr_pack_r9g9b9e5(mat[4], mat[5], mat[6]);
            gbuffer[4 * i + 3] = gr_pack_rgba8(1.0f, 0.0f, 0.0f, 0.0f);
        }
}
