/* visibility_ref.c -- test reference of the visibility buffer and the motion target (k_raster.hip
 * "basepass_MS_Main_visibility", k_motion.hip "basepass_PS_Main_motion").  Compiled by the tests themselves with
 * gcc -O2 -ffp-contract=off: only the fmaf calls written here and in the headers fuse.
 *
 * Both passes are the mesh stage of tests/ref_mesh_stage.h, which states their arithmetic and conventions: vr_raster is its
 * raster with every covered sample kept, vr_motion its texel decode with nothing checked, its weights at the pixel centre and
 * its motion.
 */
#include "ref_mesh_stage.h"

/* Rasterises the listed meshlets of pass slot `slot`: depth max-merged into depth[H*W] (as orc_raster_depth), texels
 * max-merged into vis[H*W].  order: NULL or a permutation of [0, numVisible) to draw the list in. */
void vr_raster(const OrcBasePassConstants* k, const OrcBasePassInstanceConstants* instances, const OrcMeshData* meshData,
               const OrcMeshletData* meshlets, const OrcRawVertexFormat* vertices, const uint32_t* vertexIds, const uint32_t* triangles,
               const OrcMeshletAmplificationData* records, const uint32_t* list, uint32_t numVisible, const uint32_t* order, uint32_t slot,
               float* depth, uint64_t* vis)
{
    const MsBuffers b = { instances, meshData, meshlets, vertices, vertexIds, triangles };
    for (uint32_t n = 0; n < numVisible; ++n) ms_raster_entry(k, &b, records, list, order ? order[n] : n, slot, NULL, NULL, depth, vis);
}

/* Motion (float, before the fp16 store) of every pixel with a nonzero texel; others are left as they are.  records[s] /
 * lists[s]: the four slots' buffers. */
void vr_motion(const OrcBasePassConstants* k, const OrcBasePassInstanceConstants* instances, const OrcMeshData* meshData,
               const OrcMeshletData* meshlets, const OrcRawVertexFormat* vertices, const uint32_t* vertexIds, const uint32_t* triangles,
               const OrcMeshletAmplificationData* const* records, const uint32_t* const* lists, const uint64_t* vis, float* motion)
{
    const MsBuffers b = { instances, meshData, meshlets, vertices, vertexIds, triangles };
    const uint32_t W = k->m_OutputResolution[0], H = k->m_OutputResolution[1];
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const uint64_t i = (uint64_t)py * W + px;
            if (!vis[i]) continue;
            MsTriangle T;
            float q[3];
            const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
            ms_decode(k, &b, records, lists, NULL, (uint32_t)vis[i], &T);
            const float s = ms_weights(&T, cx, cy, q);
            ms_motion(k, &T, q, s, cx, cy, motion + 2 * i);
        }
}
