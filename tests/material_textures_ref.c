/* material_textures_ref.c -- test reference of the TEXTURED G-buffer resolve (visibility_resolve.hip.h, "basepass_PS_Main_GBuffer"
 * with a texture table bound at t19): the software sampler, the analytic derivatives, GetCommonGBufferParams
 * (lightingcommon.hlsli:435-493) and tangent-free normal mapping (toyrenderer_common.hlsli:226-247) in scalar C.  Compiled by
 * the tests themselves with gcc -O2 -ffp-contract=off: only the fmaf calls written here and in the headers fuse.
 *
 * The resolve is the checked texel decode, the weights q_i, s and the motion of tests/ref_mesh_stage.h; the interpolated normal
 * and the debug byte are as in tests/gbuffer_ref.c, the packs and the vertex normal those of tests/ref_formats.h, log2Soft that
 * of tests/ref_soft_math.h.  Added per covered pixel:
 *   interp(a)  = fmaf(q2, a2, fmaf(q1, a1, q0 * a0)) / s, for the texture coordinate (m_TexCoord, half2 -> float, exact) and
 *                the world position mul(pos, World);
 *   ddx, ddy   = interp of the SAME triangle with the weights taken at (cx + 1, cy) and at (cx, cy + 1) (the triangle's
 *                plane extended), minus the centre value: three sample points of one weights function;
 *   sample(T)  : W, H = T's mip-0 size.  A = ddx(uv) * (W, H), B = ddy(uv) * (W, H); |A| = sqrtf(fmaf(A.y, A.y, A.x * A.x));
 *                A is the major axis iff |A| >= |B| (a NaN picks B); Pmax, Pmin the major and the other length;
 *                n = ceilf(Pmax / Pmin); N = n <= 16 ? n : 16 (Pmin = 0 and NaN give 16);
 *                x = Pmax / (float)N; lod = x > 0 ? log2Soft(x) : 0, clamped with fminf(fmaxf(., 0), mips - 1);
 *                l0 = floorf(lod), f = lod - l0, l1 = min(l0 + 1, mips - 1);
 *                tap i = 0 .. N - 1 at uv + major * (((float)i + 0.5f) / (float)N - 0.5f), major = ddx(uv) or ddy(uv);
 *                a tap = b0 + f * (b1 - b0), b0 and b1 the bilinear values of levels l0 and l1, both always evaluated;
 *                the result = (((0 + tap 0) + tap 1) + ...) / (float)N;
 *   bilinear   on a w x h level: tx = u * (float)w - 0.5f, x0 = floorf(tx), fx = tx - x0, columns x0 and x0 + 1;
 *                clamp: each as a float through fminf(fmaxf(., 0), w - 1) (a NaN gives column 0);
 *                wrap : i = (int)fminf(fmaxf(x0, -2^30), 2^30), the column is i mod w floored, the next one that + 1, or 0
 *                       behind the last; rows alike;
 *                value = lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy), lerp(x, y, s) = x + s * (y - x);
 *   texel      : 4 bytes R, G, B, A.  RGBA8_UNORM (10): (float)byte / 255.0f.  SRGBA8_UNORM (11): R, G, B through the 256-entry
 *                table (the sRGB transfer function in double precision, rounded once to float), A as UNORM;
 *   params     : albedo = m_ConstAlbedo * sample, roughness = mr.g, metallic = mr.b (defaults 1, 0), emissive = m_ConstEmissive
 *                * sample.rgb; with a normal map xy = 2.0f * n.xy - 1.0f, z = sqrtf(1.0f - fmaf(y, y, x * x)) (a NaN is kept),
 *                TBN of CalculateTBNWithoutTangent from ddx / ddy of the world position and of uv (cross3 of tests/ref_base.h,
 *                the float2 x float2x3 product fmaf(b, r1, a * r0), normalize = v / sqrtf(dot3)), normal =
 *                normalize(fmaf(u.z, n, fmaf(u.y, b, u.x * t))) with n the interpolated, not renormalised geometric normal;
 *   w          = RGBA8(roughness, metallic, 0, 0).
 * A pixel whose material names, in a flagged slot, a descriptor index at or past the table's count, an empty entry or an entry
 * of another format is left as it is in both outputs.
 * Parity with D3D hardware's fixed-point, vendor-specific anisotropic filtering stays unpinned.
 */
#include "ref_formats.h"
#include "ref_mesh_stage.h"
#include "ref_soft_math.h"

float mt_log2(float x) { return log2_soft(x); }
float mt_half_to_float(uint16_t h) { return half_to_float(h); }

/* ---- the sRGB table ---------------------------------------------------------------------------------------------------- */
void mt_srgb_table(float out[256])
{
    for (int i = 0; i < 256; ++i) {
        const double c = (double)i / 255.0;
        out[i] = (float)(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4));
    }
}

/* ---- textures ---------------------------------------------------------------------------------------------------------- */
#define MT_FORMAT_RGBA8 10u
#define MT_FORMAT_SRGBA8 11u
#define MT_MAX_MIPS 16

/* One entry of the texture table: width = 0 is an empty entry.  mips[k]: max(width >> k, 1) x max(height >> k, 1) x 4 bytes. */
typedef struct {
    uint32_t width, height, mipCount, format;
    const uint8_t* mips[MT_MAX_MIPS];
} MtTexture;

static uint32_t mip_dim(uint32_t d, uint32_t k) { return (d >> k) ? (d >> k) : 1u; }

static void texel(const MtTexture* t, const float* srgb, uint32_t level, uint32_t x, uint32_t y, float o[4])
{
    const uint8_t* p = t->mips[level] + ((uint64_t)y * mip_dim(t->width, level) + x) * 4u;
    for (int c = 0; c < 4; ++c)
        o[c] = (t->format == MT_FORMAT_SRGBA8 && c < 3) ? srgb[p[c]] : (float)p[c] / 255.0f;
}

static void axis(float u, uint32_t dim, int wrap, uint32_t* i0, uint32_t* i1, float* f)
{
    const float t = u * (float)dim - 0.5f, t0 = floorf(t);
    *f = t - t0;
    if (!wrap) {
        const float last = (float)(dim - 1u);
        *i0 = (uint32_t)fminf(fmaxf(t0, 0.0f), last);
        *i1 = (uint32_t)fminf(fmaxf(t0 + 1.0f, 0.0f), last);
        return;
    }
    const int i = (int)fminf(fmaxf(t0, -0x1p30f), 0x1p30f);
    int r = i % (int)dim;
    if (r < 0) r += (int)dim;
    *i0 = (uint32_t)r;
    *i1 = (uint32_t)r + 1u == dim ? 0u : (uint32_t)r + 1u;
}

static void bilinear(const MtTexture* t, const float* srgb, uint32_t level, int wrap, float u, float v, float o[4])
{
    uint32_t x0, x1, y0, y1;
    float fx, fy, t00[4], t10[4], t01[4], t11[4];
    axis(u, mip_dim(t->width, level), wrap, &x0, &x1, &fx);
    axis(v, mip_dim(t->height, level), wrap, &y0, &y1, &fy);
    texel(t, srgb, level, x0, y0, t00); texel(t, srgb, level, x1, y0, t10);
    texel(t, srgb, level, x0, y1, t01); texel(t, srgb, level, x1, y1, t11);
    for (int c = 0; c < 4; ++c) o[c] = lerp(lerp(t00[c], t10[c], fx), lerp(t01[c], t11[c], fx), fy);
}

/* The sampler.  uv, ddx(uv), ddy(uv) -> out[4]; info (optional): N, lod.  Returns N. */
uint32_t mt_sample(const MtTexture* t, const float* srgb, int wrap, const float uv[2], const float dx[2], const float dy[2], float out[4], float* lodOut)
{
    const float W = (float)t->width, H = (float)t->height;
    const float ax = dx[0] * W, ay = dx[1] * H, bx = dy[0] * W, by = dy[1] * H;
    const float lenA = sqrtf(fmaf(ay, ay, ax * ax)), lenB = sqrtf(fmaf(by, by, bx * bx));
    const int aMajor = lenA >= lenB;
    const float pmax = aMajor ? lenA : lenB, pmin = aMajor ? lenB : lenA;
    const float* major = aMajor ? dx : dy;
    const float n = ceilf(pmax / pmin);
    const uint32_t N = n <= 16.0f ? (uint32_t)n : 16u;
    const float fN = (float)N, x = pmax / fN, top = (float)(t->mipCount - 1u);
    const float lod = fminf(fmaxf(x > 0.0f ? mt_log2(x) : 0.0f, 0.0f), top);
    const float l0f = floorf(lod), f = lod - l0f;
    const uint32_t l0 = (uint32_t)l0f, l1 = l0 + 1u < t->mipCount ? l0 + 1u : t->mipCount - 1u;
    float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (uint32_t i = 0; i < N; ++i) {
        const float k = ((float)i + 0.5f) / fN - 0.5f;
        const float u = uv[0] + major[0] * k, v = uv[1] + major[1] * k;
        float b0[4], b1[4];
        bilinear(t, srgb, l0, wrap, u, v, b0);
        bilinear(t, srgb, l1, wrap, u, v, b1);
        for (int c = 0; c < 4; ++c) acc[c] = acc[c] + lerp(b0[c], b1[c], f);
    }
    for (int c = 0; c < 4; ++c) out[c] = acc[c] / fN;
    if (lodOut) *lodOut = lod;
    return N;
}

/* ---- MaterialData (ShaderInterop.h:150-172, 124 bytes) ------------------------------------------------------------------ */
typedef struct { uint32_t m_GlobalIndex, m_IsWrapSampler, m_DescriptorIndex, m_FeedbackTextureDescriptorIndex, m_MinMapTextureDescriptorIndex; } MtTextureData;
typedef struct {
    float m_ConstAlbedo[4];
    float m_ConstEmissive[3];
    float m_AlphaCutoff;
    MtTextureData m_Textures[4];              /* albedo, normal, metallic-roughness, emissive: flag bits 0..3 */
    uint32_t m_MaterialFlags;
    float m_ConstRoughness, m_ConstMetallic;
} MtMaterialData;

/* limits: ms_decode's (15 values) + numTextures.  gbuffer: uint32[H*W*4]; motion: float[H*W*2] (before the fp16 store);
 * aniso (optional): uint8[H*W*4], the N of the albedo, normal, metallic-roughness and emissive sample of each written pixel
 * (0: not sampled).  Pixels without a texel, or whose chain leaves a buffer or the table, are left as they are. */
void mt_gbuffer(const OrcBasePassConstants* k, const OrcBasePassInstanceConstants* instances, const OrcMeshData* meshData,
                const OrcMeshletData* meshlets, const OrcRawVertexFormat* vertices, const uint32_t* vertexIds, const uint32_t* triangles,
                const OrcMeshletAmplificationData* const* records, const uint32_t* const* lists, const uint64_t* vis,
                const unsigned char* materials, const MtTexture* textures, const uint64_t* limits, uint32_t* gbuffer, float* motion, uint8_t* aniso)
{
    float srgb[256];
    mt_srgb_table(srgb);
    const MsBuffers b = { instances, meshData, meshlets, vertices, vertexIds, triangles };
    const uint32_t W = k->m_OutputResolution[0], H = k->m_OutputResolution[1];
    const uint64_t numTextures = limits[15];
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const uint64_t i = (uint64_t)py * W + px;
            MsTriangle T;
            if (!vis[i] || !ms_decode(k, &b, records, lists, limits, (uint32_t)vis[i], &T)) continue;
            MtMaterialData mat;
            memcpy(&mat, materials + (uint64_t)T.inst->m_MaterialDataIdx * sizeof mat, sizeof mat);
            const MtTexture* tex[4] = { 0, 0, 0, 0 };
            int ok = 1;
            for (int c = 0; c < 4; ++c) {
                if (!(mat.m_MaterialFlags & (1u << c))) continue;
                const uint32_t d = mat.m_Textures[c].m_DescriptorIndex;
                if (d >= numTextures || !textures[d].width || (textures[d].format != MT_FORMAT_RGBA8 && textures[d].format != MT_FORMAT_SRGBA8)) { ok = 0; break; }
                tex[c] = &textures[d];
            }
            if (!ok) continue;
            float N[3][3], uv[3][2];
            for (int j = 0; j < 3; ++j) {
                vertex_normal(T.vtx[j]->m_PackedNormal, T.inst->m_WorldMatrix.m, N[j]);
                uv[j][0] = half_to_float(T.vtx[j]->m_TexCoord[0]);
                uv[j][1] = half_to_float(T.vtx[j]->m_TexCoord[1]);
            }
            const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
            /* point 0: the centre; 1: (cx + 1, cy); 2: (cx, cy + 1) */
            float q[3][3], s[3], tc[3][2], pw[3][3], n[3];
            for (int p = 0; p < 3; ++p) {
                s[p] = ms_weights(&T, p == 1 ? cx + 1.0f : cx, p == 2 ? cy + 1.0f : cy, q[p]);
                for (int c = 0; c < 2; ++c) tc[p][c] = ms_interp(q[p], s[p], uv[0][c], uv[1][c], uv[2][c]);
                for (int c = 0; c < 3; ++c) pw[p][c] = ms_interp(q[p], s[p], T.world[0][c], T.world[1][c], T.world[2][c]);
            }
            ms_motion(k, &T, q[0], s[0], cx, cy, motion + 2 * i);
            for (int c = 0; c < 3; ++c) n[c] = ms_interp(q[0], s[0], N[0][c], N[1][c], N[2][c]);
            float debugValue = 0.0f;
            uint32_t instanceSeed = T.rec->m_InstanceConstIdx, meshletSeed = T.rec->m_MeshletGroupOffset + T.lane;
            if (k->m_DebugMode == 2u) debugValue = quick_random_float(&instanceSeed);
            else if (k->m_DebugMode == 3u) debugValue = quick_random_float(&meshletSeed);
            else if (k->m_DebugMode == 12u) debugValue = (float)T.rec->m_MeshLOD / 255.0f;
            const float duvdx[2] = { tc[1][0] - tc[0][0], tc[1][1] - tc[0][1] }, duvdy[2] = { tc[2][0] - tc[0][0], tc[2][1] - tc[0][1] };
            /* GetCommonGBufferParams */
            float smp[4][4] = { { 1.0f, 1.0f, 1.0f, 1.0f }, { 0.5f, 0.5f, 1.0f, 0.0f }, { 0.0f, 1.0f, 0.0f, 0.0f }, { 1.0f, 1.0f, 1.0f, 0.0f } };
            for (int c = 0; c < 4; ++c) {
                uint32_t an = 0;
                if (tex[c]) an = mt_sample(tex[c], srgb, mat.m_Textures[c].m_IsWrapSampler != 0, tc[0], duvdx, duvdy, smp[c], 0);
                if (aniso) aniso[4 * i + c] = (uint8_t)an;
            }
            float normal[3] = { n[0], n[1], n[2] };
            if (tex[1]) {
                const float x = 2.0f * smp[1][0] - 1.0f, y = 2.0f * smp[1][1] - 1.0f;
                const float un[3] = { x, y, sqrtf(1.0f - fmaf(y, y, x * x)) };
                float dp1[3], dp2[3], m2[3], inv0[3], inv1[3], tv[3], bv[3], Tn[3], B[3], r[3];
                for (int c = 0; c < 3; ++c) { dp1[c] = pw[1][c] - pw[0][c]; dp2[c] = pw[2][c] - pw[0][c]; }
                cross3(dp1, dp2, m2);
                cross3(dp2, m2, inv0);
                cross3(m2, dp1, inv1);
                for (int c = 0; c < 3; ++c) {
                    tv[c] = fmaf(duvdy[0], inv1[c], duvdx[0] * inv0[c]);
                    bv[c] = fmaf(duvdy[1], inv1[c], duvdx[1] * inv0[c]);
                }
                normalize3(tv, Tn);
                normalize3(bv, B);
                for (int c = 0; c < 3; ++c) r[c] = fmaf(un[2], n[c], fmaf(un[1], B[c], un[0] * Tn[c]));
                normalize3(r, normal);
            }
            gbuffer[4 * i] = pack_rgba8(mat.m_ConstAlbedo[0] * smp[0][0], mat.m_ConstAlbedo[1] * smp[0][1], mat.m_ConstAlbedo[2] * smp[0][2], debugValue);
            gbuffer[4 * i + 1] = pack_oct(normal[0], normal[1], normal[2]);
            gbuffer[4 * i + 2] = pack_r9g9b9e5(mat.m_ConstEmissive[0] * smp[3][0], mat.m_ConstEmissive[1] * smp[3][1], mat.m_ConstEmissive[2] * smp[3][2]);
            gbuffer[4 * i + 3] = pack_rgba8(smp[2][1], smp[2][2], 0.0f, 0.0f);
        }
}
