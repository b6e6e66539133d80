/* texture_streaming_ref.c -- test reference of texture streaming: the STREAMED G-buffer resolve ("basepass_PS_Main_GBuffer" with a
 * min-mip or feedback map in the texture table at t19; material_textures.hip.h, visibility_resolve.hip.h), the decode of a feedback map,
 * and the residency rule of csrc/host/TextureResidency.cpp, in scalar C.  Everything of tests/material_textures_ref.c is used as it
 * is (included below): the resolve, the sampler's footprint, tap count, lod, taps, bilinear arithmetic and addressing.  Added:
 *
 * A streamable texture of W x H texels has a region of RW x RH texels of mip 0 (powers of two >= 4 that divide W and H); region
 * (rx, ry) is element ry * (W / RW) + rx of a map.
 *   point    : the mip-0 texel under u on an axis of dim texels: t0 = floorf(u * (float)dim); clamp: (uint)fminf(fmaxf(t0, 0), dim - 1);
 *              wrap: (int)fminf(fmaxf(t0, -2^30), 2^30) mod dim, floored.  The region under uv is (point(u) / RW, point(v) / RH).
 *   clamp    : lodWanted = mt_sample's clamped lod; minMip = the map's byte of the region under uv (0 without a map);
 *              lod = fminf(fmaxf(lodWanted, (float)minMip), mips - 1); l0, l1, f from lod; N and the tap positions unchanged.
 *   feedback : (only with m_bWriteSamplerFeedback != 0 and a feedback map) l0w = floorf(lodWanted), l1w = min(l0w + 1, mips - 1).  The
 *              region under uv is marked with l0w; for every tap each of the four texels (x, y) of the bilinear footprint at level
 *              l0w marks region ((x << l0w) / RW, (y << l0w) / RH) with l0w, and each of the four at level l1w marks its region with
 *              l1w.  A mark is word = min(word, level); a word starts as 0xFFFFFFFF.
 *   visualise: with m_bVisualizeMinMipTilesOnAlbedoOutput != 0 the albedo sample of a slot with a min-mip map is kMipColors[min(minMip, 15)].
 *   maps     : table entries: a min-mip map has format 8 (bytes), a feedback map format 9 (32-bit words), both W / RW x H / RH.  A
 *              flagged slot whose map index is not 0xFFFFFFFF and is past the table, empty, of another format or size, or whose
 *              texture has no region, leaves the pixel as it is.
 *   decode   : byte = word < 0xFF ? word : 0xFF.
 *
 * THE RESIDENCY RULE.  Level k is standard when every level j <= k has (W >> j) and (H >> j) a multiple >= 1 of RW and RH (a level of
 * a size that is no power of two stops being whole tiles early: 24 x 24 with 8 x 8 has one standard level, 48 x 32 two) and k < mips - 1
 * (the last level always belongs to the packed tail, which is resident); S = the number of standard levels.  Level k has
 * (W >> k) / RW x (H >> k) / RH tiles; the tile of level k that covers region (rx, ry) is (rx >> k, ry >> k).  One round = one processed (decoded) feedback of the texture:
 *   required : a region with byte q != 0xFF requires its covering tile at every standard level k >= q;
 *   map      : a required tile that is not resident is mapped (no budget); its idle count becomes 0;
 *   evict    : a resident tile that is not required adds one to its idle count and is unmapped when the count reaches evict_after:
 *              not required by any of the last evict_after rounds;
 *   minMip   : per region, the finest level m such that its covering tiles are resident at every standard level >= m; S if none.
 * A frame in which the texture's feedback is not processed changes nothing.
 *
 * NEGATIVE CONTROLS (tests/test_texture_streaming_rule_scenes.py; never defined by any other build).  -DTS_REF_MUTATE_<RULE> breaks one
 * rule of the sampler, so that the test can show that the rule scenes (tests/texture_streaming_rule_scenes.py) tell the broken rule
 * from the stated one.  Every mutant keeps its word and byte indices inside the maps (the two SWAP mutants by taking the index modulo
 * the region count).
 *   SWAP_REGION_FOOTPRINT  the footprint marks divide x by RH and y by RW          NO_ORIGIN_SHIFT   a texel marks (x / RW, y / RH): no << level
 *   SWAP_REGION_UNDER      the region under uv divides x by RH and y by RW         NO_L1W            no marks of the level-l1w footprint
 *   NO_L0W_FOOTPRINT       no marks of the level-l0w footprint                     NO_UNDER          no mark of the region under uv
 *   CLAMPED_LEVELS         the footprints of l0, l1 are marked (with l0, l1)       CENTRE_FOOTPRINT  every tap marks the footprints at uv itself
 *   ONE_TEXEL              texel (x0, y0) of a footprint marks alone               UNDER_CLAMP_MODE  the point under uv is always clamped
 *   CLAMP_REPLACES         lod = minMip != 0 ? minMip : lodWanted (no max)         UNDER_ROUNDS      point: t0 = floorf(u * dim + 0.5f)
 * -DTS_REF_LANE_DROP is no mutant: it marks through the kernel's per-lane drop (Marker in csrc/material_textures.hip.h) instead of
 * mark by mark, and must give the same words; with it, -DTS_REF_MUTATE_DROP_BY_INDEX drops on the word index alone, as the kernel's
 * negative control TR_STREAM_MUTATE_DROP_BY_INDEX does.
 */
#include "material_textures_ref.c"

#include <stdlib.h>

#define TS_FORMAT_MINMIP 8u
#define TS_FORMAT_FEEDBACK 9u
#define TS_NONE 0xFFFFFFFFu

static const float ts_mip_colours[16][3] = { { 1.0f, 1.0f, 1.0f }, { 1.0f, 0.25f, 0.25f }, { 0.25f, 1.0f, 0.25f }, { 0.25f, 0.25f, 1.0f }, { 1.0f, 0.25f, 1.0f },
    { 1.0f, 1.0f, 0.25f }, { 0.25f, 1.0f, 1.0f }, { 0.9f, 0.5f, 0.2f }, { 0.59f, 0.48f, 0.8f }, { 0.53f, 0.25f, 0.11f }, { 0.8f, 0.48f, 0.53f },
    { 0.64f, 0.8f, 0.48f }, { 0.48f, 0.75f, 0.8f }, { 0.5f, 0.25f, 0.75f }, { 0.99f, 0.68f, 0.42f }, { 0.4f, 0.5f, 0.6f } };

static uint32_t ts_point(float u, uint32_t dim, int wrap)
{
#ifdef TS_REF_MUTATE_UNDER_ROUNDS
    const float t0 = floorf(u * (float)dim + 0.5f);
#else
    const float t0 = floorf(u * (float)dim);
#endif
#ifdef TS_REF_MUTATE_UNDER_CLAMP_MODE
    wrap = 0;
#endif
    if (!wrap) return (uint32_t)fminf(fmaxf(t0, 0.0f), (float)(dim - 1u));
    const int i = (int)fminf(fmaxf(t0, -0x1p30f), 0x1p30f);
    int r = i % (int)dim;
    if (r < 0) r += (int)dim;
    return (uint32_t)r;
}

/* The marks of one sample.  lastIndex, lastLevel: the per-lane drop's state (TS_REF_LANE_DROP), one per sample as in the kernel. */
typedef struct { uint32_t* words; uint32_t lastIndex, lastLevel; } TsMarker;

static void ts_mark(TsMarker* m, uint32_t index, uint32_t level)
{
#ifdef TS_REF_LANE_DROP
#ifdef TS_REF_MUTATE_DROP_BY_INDEX
    if (index == m->lastIndex) return;
#else
    if (index == m->lastIndex && level >= m->lastLevel) return;
#endif
    m->lastIndex = index; m->lastLevel = level;
#endif
    if (level < m->words[index]) m->words[index] = level;
}

/* word of the region of mip-0 texel (x, y) */
static uint32_t ts_region(const MtTexture* t, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh, int footprint)
{
#if defined(TS_REF_MUTATE_SWAP_REGION_FOOTPRINT) || defined(TS_REF_MUTATE_SWAP_REGION_UNDER)
#ifdef TS_REF_MUTATE_SWAP_REGION_FOOTPRINT
    const int swap = footprint;
#else
    const int swap = !footprint;
#endif
    if (swap) return ((y / rw) * (t->width / rw) + x / rh) % ((t->width / rw) * (t->height / rh));
#endif
    (void)footprint;
    return (y / rh) * (t->width / rw) + x / rw;
}

static void ts_mark_footprint(const MtTexture* t, uint32_t level, int wrap, float u, float v, uint32_t rw, uint32_t rh, TsMarker* m)
{
    uint32_t x[2], y[2];
    float f;
    axis(u, mip_dim(t->width, level), wrap, &x[0], &x[1], &f);
    axis(v, mip_dim(t->height, level), wrap, &y[0], &y[1], &f);
#ifdef TS_REF_MUTATE_NO_ORIGIN_SHIFT
    const uint32_t shift = 0;
#else
    const uint32_t shift = level;
#endif
#ifdef TS_REF_MUTATE_ONE_TEXEL
    const int texels = 1;
#else
    const int texels = 2;
#endif
    for (int j = 0; j < texels; ++j)
        for (int i = 0; i < texels; ++i)
            ts_mark(m, ts_region(t, x[i] << shift, y[j] << shift, rw, rh, 1), level);
}

/* The streamed sampler.  minMip (bytes) and feedback (words) may each be NULL; rw, rh: the region.  Returns N; *minMipOut: the byte read. */
uint32_t ts_sample(const MtTexture* t, const float* srgb, int wrap, const float uv[2], const float dx[2], const float dy[2], uint32_t rw, uint32_t rh,
                   const uint8_t* minMipMap, uint32_t* feedback, float out[4], uint32_t* minMipOut)
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
    const float lodWanted = fminf(fmaxf(x > 0.0f ? mt_log2(x) : 0.0f, 0.0f), top);
    uint32_t under = 0, minMip = 0;
    if (minMipMap || feedback) under = ts_region(t, ts_point(uv[0], t->width, wrap), ts_point(uv[1], t->height, wrap), rw, rh, 0);
    if (minMipMap) minMip = minMipMap[under];
    if (minMipOut) *minMipOut = minMip;
#ifdef TS_REF_MUTATE_CLAMP_REPLACES
    const float lod = fminf(minMip != 0u ? (float)minMip : lodWanted, top);
#else
    const float lod = fminf(fmaxf(lodWanted, (float)minMip), top);
#endif
    const float l0f = floorf(lod), f = lod - l0f;
    const uint32_t l0 = (uint32_t)l0f, l1 = l0 + 1u < t->mipCount ? l0 + 1u : t->mipCount - 1u;
    const uint32_t l0w = (uint32_t)floorf(lodWanted), l1w = l0w + 1u < t->mipCount ? l0w + 1u : t->mipCount - 1u;
#ifdef TS_REF_MUTATE_CLAMPED_LEVELS
    const uint32_t m0 = l0, m1 = l1;
#else
    const uint32_t m0 = l0w, m1 = l1w;
#endif
    TsMarker marker = { feedback, 0xFFFFFFFFu, 0u };
#ifndef TS_REF_MUTATE_NO_UNDER
    if (feedback) ts_mark(&marker, under, l0w);
#endif
    float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (uint32_t i = 0; i < N; ++i) {
        const float k = ((float)i + 0.5f) / fN - 0.5f;
        const float u = uv[0] + major[0] * k, v = uv[1] + major[1] * k;
        float b0[4], b1[4];
        bilinear(t, srgb, l0, wrap, u, v, b0);
        bilinear(t, srgb, l1, wrap, u, v, b1);
        for (int c = 0; c < 4; ++c) acc[c] = acc[c] + lerp(b0[c], b1[c], f);
        if (feedback) {
#ifdef TS_REF_MUTATE_CENTRE_FOOTPRINT
            const float mu = uv[0], mv = uv[1];
#else
            const float mu = u, mv = v;
#endif
#ifndef TS_REF_MUTATE_NO_L0W_FOOTPRINT
            ts_mark_footprint(t, m0, wrap, mu, mv, rw, rh, &marker);
#endif
#ifndef TS_REF_MUTATE_NO_L1W
            ts_mark_footprint(t, m1, wrap, mu, mv, rw, rh, &marker);
#endif
        }
    }
    for (int c = 0; c < 4; ++c) out[c] = acc[c] / fN;
    return N;
}

/* The maps of slot `s`, which samples table entry d.  0: a named map that is no map of a texture like d's. */
static int ts_maps(const MtTextureData* s, const MtTexture* textures, const uint32_t* regions, uint64_t numTextures, uint32_t d, int writeFeedback,
                   const uint8_t** minMipMap, uint32_t** feedback)
{
    *minMipMap = 0; *feedback = 0;
    const uint32_t mm = s->m_MinMapTextureDescriptorIndex, fb = s->m_FeedbackTextureDescriptorIndex;
    if (mm == TS_NONE && fb == TS_NONE) return 1;
    const uint32_t rw = regions[2 * d], rh = regions[2 * d + 1];
    if (!rw || !rh) return 0;
    const uint32_t w = textures[d].width / rw, h = textures[d].height / rh;
    if (mm != TS_NONE) {
        if (mm >= numTextures || textures[mm].format != TS_FORMAT_MINMIP || textures[mm].width != w || textures[mm].height != h) return 0;
        *minMipMap = textures[mm].mips[0];
    }
    if (fb != TS_NONE) {
        if (fb >= numTextures || textures[fb].format != TS_FORMAT_FEEDBACK || textures[fb].width != w || textures[fb].height != h ||
            regions[2 * fb] != rw || regions[2 * fb + 1] != rh) return 0;
        if (writeFeedback) *feedback = (uint32_t*)textures[fb].mips[0];
    }
    return 1;
}

/* mt_gbuffer with the maps.  regions: uint32[2 * numTextures], (RW, RH) of each table entry (a feedback map carries its texture's), 0 = none.
 * The feedback maps among `textures` are written (their words must be initialised by the caller). */
void ts_gbuffer(const OrcBasePassConstants* k, const OrcBasePassInstanceConstants* instances, const OrcMeshData* meshData,
                const OrcMeshletData* meshlets, const OrcRawVertexFormat* vertices, const uint32_t* vertexIds, const uint32_t* triangles,
                const OrcMeshletAmplificationData* const* records, const uint32_t* const* lists, const uint64_t* vis,
                const unsigned char* materials, const MtTexture* textures, const uint64_t* limits, uint32_t* gbuffer, float* motion, uint8_t* aniso,
                const uint32_t* regions)
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
            const uint8_t* minMipMap[4];
            uint32_t* feedback[4];
            uint32_t region[4][2] = { { 0, 0 }, { 0, 0 }, { 0, 0 }, { 0, 0 } };
            int ok = 1;
            for (int c = 0; c < 4; ++c) {
                minMipMap[c] = 0; feedback[c] = 0;
                if (!(mat.m_MaterialFlags & (1u << c))) continue;
                const uint32_t d = mat.m_Textures[c].m_DescriptorIndex;
                if (d >= numTextures || !textures[d].width || (textures[d].format != MT_FORMAT_RGBA8 && textures[d].format != MT_FORMAT_SRGBA8)) { ok = 0; break; }
                if (!ts_maps(&mat.m_Textures[c], textures, regions, numTextures, d, k->m_bWriteSamplerFeedback != 0, &minMipMap[c], &feedback[c])) { ok = 0; break; }
                tex[c] = &textures[d];
                region[c][0] = regions[2 * d]; region[c][1] = regions[2 * d + 1];
            }
            if (!ok) continue;
            float N[3][3], uv[3][2];
            for (int j = 0; j < 3; ++j) {
                vertex_normal(T.vtx[j]->m_PackedNormal, T.inst->m_WorldMatrix.m, N[j]);
                uv[j][0] = half_to_float(T.vtx[j]->m_TexCoord[0]);
                uv[j][1] = half_to_float(T.vtx[j]->m_TexCoord[1]);
            }
            const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
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
            float smp[4][4] = { { 1.0f, 1.0f, 1.0f, 1.0f }, { 0.5f, 0.5f, 1.0f, 0.0f }, { 0.0f, 1.0f, 0.0f, 0.0f }, { 1.0f, 1.0f, 1.0f, 0.0f } };
            for (int c = 0; c < 4; ++c) {
                uint32_t an = 0, minMip = 0;
                if (tex[c]) an = ts_sample(tex[c], srgb, mat.m_Textures[c].m_IsWrapSampler != 0, tc[0], duvdx, duvdy, region[c][0], region[c][1], minMipMap[c], feedback[c], smp[c], &minMip);
                if (tex[c] && c == 0 && k->m_bVisualizeMinMipTilesOnAlbedoOutput && minMipMap[c])
                    for (int j = 0; j < 3; ++j) smp[0][j] = ts_mip_colours[minMip < 15u ? minMip : 15u][j];
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

void ts_decode(const uint32_t* words, uint32_t regions, uint8_t* out)
{
    for (uint32_t i = 0; i < regions; ++i) out[i] = (uint8_t)(words[i] < 0xFFu ? words[i] : 0xFFu);
}

/* ---- the residency rule -------------------------------------------------------------------------------------------------------- */
typedef struct { uint32_t width, height, mips, regionW, regionH, tileBytes; } TsTiled;          /* tileBytes: bytes uploaded per mapped tile */
typedef struct { uint32_t tilesTotal, tilesResident, tilesMapped, tilesUnmapped; uint64_t bytesUploaded; } TsStats;

uint32_t ts_standard_levels(const TsTiled* t)
{
    uint32_t s = 0;
    while (s + 1u < t->mips && (t->width >> s) >= t->regionW && (t->height >> s) >= t->regionH && (t->width >> s) % t->regionW == 0u && (t->height >> s) % t->regionH == 0u) ++s;
    return s;
}

static uint32_t tiles_x(const TsTiled* t, uint32_t k) { return (t->width >> k) / t->regionW; }
static uint32_t tiles_y(const TsTiled* t, uint32_t k) { return (t->height >> k) / t->regionH; }

/* first tile of level k in the residency arrays; level S: the total */
uint32_t ts_tile_offset(const TsTiled* t, uint32_t k)
{
    uint32_t off = 0;
    for (uint32_t j = 0; j < k; ++j) off += tiles_x(t, j) * tiles_y(t, j);
    return off;
}

/* One round.  feedback: the decoded bytes (one per region).  resident, idle: one entry per tile, updated in place.  mapped / unmapped
 * (optional): one byte per tile, set for the tiles this round maps / unmaps.  minMip: one byte per region, rewritten. */
void ts_residency_round(const TsTiled* t, const uint8_t* feedback, uint32_t evictAfter, uint8_t* resident, uint32_t* idle, uint8_t* mapped, uint8_t* unmapped,
                        uint8_t* minMip, TsStats* stats)
{
    const uint32_t S = ts_standard_levels(t), total = ts_tile_offset(t, S), rx = t->width / t->regionW, ry = t->height / t->regionH;
    uint8_t* required = (uint8_t*)calloc(total ? total : 1u, 1);
    for (uint32_t y = 0; y < ry; ++y)
        for (uint32_t x = 0; x < rx; ++x) {
            const uint32_t q = feedback[y * rx + x];
            if (q == 0xFFu) continue;
            for (uint32_t k = q; k < S; ++k) required[ts_tile_offset(t, k) + (y >> k) * tiles_x(t, k) + (x >> k)] = 1;
        }
    memset(stats, 0, sizeof *stats);
    stats->tilesTotal = total;
    for (uint32_t i = 0; i < total; ++i) {
        if (mapped) mapped[i] = 0;
        if (unmapped) unmapped[i] = 0;
        if (required[i]) {
            idle[i] = 0;
            if (!resident[i]) { resident[i] = 1; if (mapped) mapped[i] = 1; ++stats->tilesMapped; stats->bytesUploaded += t->tileBytes; }
        } else if (resident[i] && ++idle[i] >= evictAfter) {
            resident[i] = 0; if (unmapped) unmapped[i] = 1; ++stats->tilesUnmapped;
        }
        stats->tilesResident += resident[i];
    }
    free(required);
    for (uint32_t y = 0; y < ry; ++y)
        for (uint32_t x = 0; x < rx; ++x) {
            uint32_t m = S;
            while (m > 0 && resident[ts_tile_offset(t, m - 1u) + (y >> (m - 1u)) * tiles_x(t, m - 1u) + (x >> (m - 1u))]) --m;
            minMip[y * rx + x] = (uint8_t)m;
        }
}
