/* alpha_test_ref.c -- the definition of the alpha test: ALPHA_MASK_MODE's discard in the rasters ("basepass_MS_Main_depth
 * ALPHA_MASK_MODE=1", "basepass_MS_Main_visibility ALPHA_MASK_MODE=1", csrc/k_raster.hip) and the textured alpha test of the sun
 * rays ("shadowmask_CS_ShadowMask" with a texture table at t19, csrc/k_shadowmask.hip).  Compiled by the tests themselves with
 * gcc -O2 -ffp-contract=off (tests/alpha_test_ref.py): only the fmaf calls written here fuse.
 *
 * It includes the two references it extends, unedited: tests/material_textures_ref.c (the sampler, MaterialData, and through it the
 * mesh stage of tests/ref_mesh_stage.h) and tests/shadowmask_ref.c (the ray of a texel, the ray set-up, SmScene).
 *
 * ALPHA.  at_sample_alpha = component 3 of mt_sample: the footprint, tap count, lod, tap positions, trilinear and bilinear
 *   arithmetic, addressing and summation order of the colour channels, applied to byte 3 of the texel, (float)byte / 255.0f in
 *   both formats (alpha never goes through the sRGB table).  at_alpha_level0 = one bilinear fetch of mip 0.
 *
 * RASTER (at_raster).  The raster of tests/ref_mesh_stage.h (vr_raster) with its keep hook supplied: one step added.  A covered
 *   sample of a triangle (all three edge values e_i >= 0, den > 0, d > 0) passes, before it is merged into either target:
 *   1. q_i = e_i / w_i, s = (q0 + q1) + q2, from the sample's own edge values and the vertices' clip w;
 *   2. uv = fmaf(q2, a2, fmaf(q1, a1, q0 * a0)) / s of m_TexCoord (half -> float, exact);
 *   3. ddx(uv), ddy(uv) = the same interpolation of the same triangle with the edge functions re-evaluated at (cx + 1, cy) and
 *      at (cx, cy + 1), minus the centre value (the formulas of the TEXTURED resolve, tests/material_textures_ref.c);
 *   4. alpha = m_ConstAlbedo.w, times at_sample_alpha(albedo texture, m_IsWrapSampler, uv, ddx, ddy) if MaterialFlag_UseAlbedoTexture;
 *   5. the sample is discarded iff alpha < m_AlphaCutoff (a NaN alpha is kept);
 *   6. nothing of the triangle is drawn when m_MaterialDataIdx is past the buffer, or the albedo flag is set and no table is
 *      given, the descriptor index is past the table, the entry is empty or of another format.
 *   The surviving samples feed the same maxima, so the result does not depend on the draw order.  Parity with hardware unpinned.
 *
 * RAYS (at_trace).  occluded_brute of tests/shadowmask_ref.c restated with that file's fetch_tri and tri_candidate: every triangle of
 *   every instance, a loop of its own.  A candidate on a
 *   ForceNonOpaque instance whose material has MaterialFlag_UseAlbedoTexture counts iff
 *   m_ConstAlbedo.w * at_alpha_level0(albedo texture, m_IsWrapSampler, uv) >= m_AlphaCutoff, with InterpolateVertex's uv
 *   (raytracingcommon.hlsli:24-36, :189): b1 = V / det, b2 = W / det of the watertight test's edge values, b0 = (1.0f - b1) - b2,
 *   uv = ((0 + uv0 * b0) + uv1 * b1) + uv2 * b2, not fused.  A broken descriptor: the candidate does not count.  Texture-free
 *   materials keep m_ConstAlbedo.w >= m_AlphaCutoff.  numTextures < 0: no table, every material by the texture-free rule (today's
 *   kernel).  DEVIATION: the reference calls Sample in a compute shader, where the derivatives come from unrelated neighbouring
 *   rays; this build reads mip 0.
 */
#include "material_textures_ref.c"
#include "shadowmask_ref.c"

float at_sample_alpha(const MtTexture* t, int wrap, const float uv[2], const float dx[2], const float dy[2])
{
    float srgb[256], out[4];
    mt_srgb_table(srgb);                                                         /* never read by component 3 */
    mt_sample(t, srgb, wrap, uv, dx, dy, out, 0);
    return out[3];
}

float at_alpha_level0(const MtTexture* t, int wrap, float u, float v)
{
    float srgb[256], out[4];
    mt_srgb_table(srgb);
    bilinear(t, srgb, 0, wrap, u, v, out);
    return out[3];
}

static const MtTexture* table_entry(const MtTexture* textures, int64_t numTextures, uint32_t d)
{
    if (!textures || (int64_t)d >= numTextures || !textures[d].width) return 0;
    if (textures[d].format != MT_FORMAT_RGBA8 && textures[d].format != MT_FORMAT_SRGBA8) return 0;
    return &textures[d];
}

/* ---- the raster of one pass slot --------------------------------------------------------------------------------------------- */
typedef struct { MtMaterialData mat; const MtTexture* tex; uint64_t* counts; } AtKeep;

/* steps 1 to 5 for one covered sample: the raster's keep hook (tests/ref_mesh_stage.h) */
static int at_keep(void* ctx, const MsTriangle* T, float cx, float cy, uint64_t boxPixels)
{
    const AtKeep* a = (const AtKeep*)ctx;
    float alpha = a->mat.m_ConstAlbedo[3];
    if (a->tex) {
        float uv[3][2], tc[3][2], q[3];
        for (int j = 0; j < 3; ++j) { uv[j][0] = half_to_float(T->vtx[j]->m_TexCoord[0]); uv[j][1] = half_to_float(T->vtx[j]->m_TexCoord[1]); }
        for (int p = 0; p < 3; ++p) {                                                /* the centre, (cx + 1, cy), (cx, cy + 1) */
            const float s = ms_weights(T, p == 1 ? cx + 1.0f : cx, p == 2 ? cy + 1.0f : cy, q);
            for (int j = 0; j < 2; ++j) tc[p][j] = ms_interp(q, s, uv[0][j], uv[1][j], uv[2][j]);
        }
        const float dx[2] = { tc[1][0] - tc[0][0], tc[1][1] - tc[0][1] }, dy[2] = { tc[2][0] - tc[0][0], tc[2][1] - tc[0][1] };
        alpha = alpha * at_sample_alpha(a->tex, a->mat.m_Textures[0].m_IsWrapSampler != 0, tc[0], dx, dy);
    }
    const int discard = alpha < a->mat.m_AlphaCutoff;
    if (a->counts) ++a->counts[2 * (boxPixels > 1024u) + discard];
    return !discard;
}

/* alphaTest = 0: vr_raster.  order: NULL, or numVisible positions of `list` to draw (the payload carries the position, so disjoint
 * slices of a list drawn into images of their own and max-merged give the image of the whole list).  counts (optional, uint64[4]):
 * the covered samples (d > 0) of the slot's triangles that were kept and discarded, {kept, discarded} of the triangles whose
 * bounding box has at most 1024 pixels (drawn in place by the kernel's main launch) and {kept, discarded} of the larger ones
 * (queue, bin and tile launch). */
void at_raster(const OrcBasePassConstants* k, const OrcBasePassInstanceConstants* instances, const OrcMeshData* meshData,
               const OrcMeshletData* meshlets, const OrcRawVertexFormat* vertices, const uint32_t* vertexIds, const uint32_t* triangles,
               const OrcMeshletAmplificationData* records, const uint32_t* list, uint32_t numVisible, const uint32_t* order, uint32_t slot,
               const unsigned char* materials, uint32_t numMaterials, const MtTexture* textures, int64_t numTextures, int alphaTest,
               float* depth, uint64_t* vis, uint64_t* counts)
{
    const MsBuffers b = { instances, meshData, meshlets, vertices, vertexIds, triangles };
    for (uint32_t n = 0; n < numVisible; ++n) {
        const uint32_t v = order ? order[n] : n;
        AtKeep a = { .tex = 0, .counts = counts };
        if (alphaTest) {
            const OrcBasePassInstanceConstants* inst = &instances[records[list[v] >> 5].m_InstanceConstIdx];
            if (inst->m_MaterialDataIdx >= numMaterials) continue;
            memcpy(&a.mat, materials + (uint64_t)inst->m_MaterialDataIdx * sizeof a.mat, sizeof a.mat);
            if (a.mat.m_MaterialFlags & 1u) {
                a.tex = table_entry(textures, numTextures, a.mat.m_Textures[0].m_DescriptorIndex);
                if (!a.tex) continue;
            }
        }
        ms_raster_entry(k, &b, records, list, v, slot, alphaTest ? at_keep : NULL, &a, depth, vis);
    }
}

/* ---- the sun rays ------------------------------------------------------------------------------------------------------------ */
static int at_commits(const SmScene* s, const MtTexture* textures, int64_t numTextures, uint32_t inst, uint32_t flags, const uint16_t tc[3][2], float b1, float b2)
{
    if (flags != 2u) return 1;
    const uint32_t mi = s->instances[inst].material;
    if (mi >= s->numMaterials) return 0;
    MtMaterialData mat;
    memcpy(&mat, &s->materials[mi], sizeof mat);
    if (numTextures >= 0 && (mat.m_MaterialFlags & 1u)) {
        const MtTexture* tex = table_entry(textures, numTextures, mat.m_Textures[0].m_DescriptorIndex);
        if (!tex) return 0;
        const float b0 = (1.0f - b1) - b2;
        float uv[2];
        for (int j = 0; j < 2; ++j)
            uv[j] = ((0.0f + mt_half_to_float(tc[0][j]) * b0) + mt_half_to_float(tc[1][j]) * b1) + mt_half_to_float(tc[2][j]) * b2;
        return mat.m_ConstAlbedo[3] * at_alpha_level0(tex, mat.m_Textures[0].m_IsWrapSampler != 0, uv[0], uv[1]) >= mat.m_AlphaCutoff;
    }
    return mat.m_ConstAlbedo[3] >= mat.m_AlphaCutoff;
}

static int at_occluded(const SmScene* s, const MtTexture* textures, int64_t numTextures, F3 o, F3 d, float tmin, float tmax)
{
    for (uint32_t i = 0; i < s->numInstances; ++i) {
        const uint32_t flags = s->flags[i] & 3u, mesh = s->instances[i].mesh;
        if (!flags || mesh >= s->numMeshes) continue;
        float m[12];
        sm_object_from_world(s->instances[i].world, m);
        const SmRay r = make_ray(mul_point(o, m, 1), mul_point(d, m, 0));
        for (uint32_t t = 0; t < s->meshIndexCounts[mesh] / 3u; ++t) {
            SmTri T;
            SmTriHit h;
            uint16_t tc[3][2];
            if (!fetch_tri(s, mesh, t, 1, &T) || !tri_candidate(T.v[0], T.v[1], T.v[2], &r, &h) || !(h.t > tmin && h.t < tmax)) continue;
            for (int k = 0; k < 3; ++k) memcpy(tc[k], s->vertices + T.i[k] * 20u + 16u, 4);
            if (at_commits(s, textures, numTextures, i, flags, tc, h.b1, h.b2)) return 1;
        }
    }
    return 0;
}

/* sm_trace, brute force, with the table.  numTextures < 0: no table (equals sm_trace mode 0). */
void at_trace(const SmConsts* k, const SmScene* s, const MtTexture* textures, int64_t numTextures, const float* depth, const uint32_t* gbufferA,
              const uint32_t* noise, uint8_t* mask, uint16_t* lvd)
{
    for (uint32_t py = 0; py < k->H; ++py)
        for (uint32_t px = 0; px < k->W; ++px) {
            const uint64_t i = (uint64_t)py * k->W + px;
            float o[3], d[3], w[3];
            if (!sm_texel_ray(k, px, py, depth[i], gbufferA + 4 * i, noise, o, d, w)) { lvd[i] = 0x7BFFu; continue; }
            const F3 O = { o[0], o[1], o[2] }, D = { d[0], d[1], d[2] };
            mask[i] = at_occluded(s, textures, numTextures, O, D, k->rayStartOffset, 1e10f) ? 0u : 255u;
            const F3 v = { w[0] - k->camera[0], w[1] - k->camera[1], w[2] - k->camera[2] };
            lvd[i] = sm_half_bits(sqrtf(dot3f(v, v)));
        }
}
