/* gbuffer_ref.c -- test reference of GBufferA and the fused motion target (visibility_resolve.hip.h,
 * "basepass_PS_Main_GBuffer").  Compiled by the tests themselves with gcc -O2 -ffp-contract=off: only the fmaf calls
 * written here and in the headers fuse.
 *
 * The resolve is the checked texel decode, the weights at the pixel centre and the motion of tests/ref_mesh_stage.h; the packs,
 * the vertex normal and QuickRandomFloat are those of tests/ref_formats.h.  This file adds, per covered pixel:
 *   normal = interp(N_i) = fmaf(q2, N2, fmaf(q1, N1, q0 * N0)) / s of the vertices' world normals, not renormalised;
 *   x = RGBA8(albedo.rgb, debugValue), y = unorm 2x16 of the octahedral normal, z = R9G9B9E5(emissive), w = 0xFF
 *            (roughness 1, metallic 0: the constants the reference's shader uses without a texture);
 *   debugValue by m_DebugMode: 2 QuickRandomFloat(instance), 3 QuickRandomFloat(m_MeshletGroupOffset + lane),
 *            12 (float)m_MeshLOD / 255.0f, else 0.
 * A pixel whose chain of indices leaves a buffer (the counts in `limits`) is left as it is in both outputs.
 */
#include "ref_formats.h"
#include "ref_mesh_stage.h"

uint32_t gr_pack_rgba8(float r, float g, float b, float a) { return pack_rgba8(r, g, b, a); }
uint32_t gr_pack_oct(float nx, float ny, float nz) { return pack_oct(nx, ny, nz); }
uint32_t gr_pack_r9g9b9e5(float r, float g, float b) { return pack_r9g9b9e5(r, g, b); }
float gr_quick_random_float(uint32_t seed) { return quick_random_float(&seed); }
float gr_mesh_lod_value(uint32_t lod) { return (float)lod / 255.0f; }
void gr_unpack_normal(uint32_t packed, float o[3]) { unpack_normal10(packed, o); }
void gr_vertex_normal(uint32_t word, const OrcMatrix* world, float o[3]) { vertex_normal(word, world->m, o); }

/* array forms for the tests */
void gr_pack_rgba8_n(const float* rgba, uint64_t n, uint32_t* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gr_pack_rgba8(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]); }
void gr_pack_oct_n(const float* xyz, uint64_t n, uint32_t* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gr_pack_oct(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]); }
void gr_pack_r9g9b9e5_n(const float* rgb, uint64_t n, uint32_t* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gr_pack_r9g9b9e5(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]); }
void gr_quick_random_float_n(const uint32_t* seeds, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gr_quick_random_float(seeds[i]); }
void gr_mesh_lod_value_n(const uint32_t* lods, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gr_mesh_lod_value(lods[i]); }
void gr_unpack_normal_n(const uint32_t* words, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) gr_unpack_normal(words[i], out + 3 * i); }

/* MaterialData: 124-byte stride, floats 0-3 albedo, 4-6 emissive */
#define GR_MATERIAL_STRIDE 124u

/* limits: ms_decode's (15 values).
 * gbuffer: uint32[H*W*4]; motion: float[H*W*2] (before the fp16 store).  Pixels without a texel, or whose chain leaves a
 * buffer, are left as they are. */
void gr_gbuffer(const OrcBasePassConstants* k, const OrcBasePassInstanceConstants* instances, const OrcMeshData* meshData,
                const OrcMeshletData* meshlets, const OrcRawVertexFormat* vertices, const uint32_t* vertexIds, const uint32_t* triangles,
                const OrcMeshletAmplificationData* const* records, const uint32_t* const* lists, const uint64_t* vis,
                const unsigned char* materials, const uint64_t* limits, uint32_t* gbuffer, float* motion)
{
    const MsBuffers b = { instances, meshData, meshlets, vertices, vertexIds, triangles };
    const uint32_t W = k->m_OutputResolution[0], H = k->m_OutputResolution[1];
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const uint64_t i = (uint64_t)py * W + px;
            MsTriangle T;
            if (!vis[i] || !ms_decode(k, &b, records, lists, limits, (uint32_t)vis[i], &T)) continue;
            const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
            float q[3], N[3][3], n[3];
            const float s = ms_weights(&T, cx, cy, q);
            ms_motion(k, &T, q, s, cx, cy, motion + 2 * i);
            for (int j = 0; j < 3; ++j) vertex_normal(T.vtx[j]->m_PackedNormal, T.inst->m_WorldMatrix.m, N[j]);
            for (int c = 0; c < 3; ++c) n[c] = ms_interp(q, s, N[0][c], N[1][c], N[2][c]);
            float debugValue = 0.0f;
            if (k->m_DebugMode == 2u) debugValue = gr_quick_random_float(T.rec->m_InstanceConstIdx);
            else if (k->m_DebugMode == 3u) debugValue = gr_quick_random_float(T.rec->m_MeshletGroupOffset + T.lane);
            else if (k->m_DebugMode == 12u) debugValue = gr_mesh_lod_value(T.rec->m_MeshLOD);
            float mat[7];
            memcpy(mat, materials + (uint64_t)T.inst->m_MaterialDataIdx * GR_MATERIAL_STRIDE, sizeof mat);
            gbuffer[4 * i] = pack_rgba8(mat[0], mat[1], mat[2], debugValue);
            gbuffer[4 * i + 1] = pack_oct(n[0], n[1], n[2]);
            gbuffer[4 * i + 2] = pack_r9g9b9e5(mat[4], mat[5], mat[6]);
            gbuffer[4 * i + 3] = pack_rgba8(1.0f, 0.0f, 0.0f, 0.0f);
        }
}
