/* sigma_ref.c -- the definition of the sun shadow denoiser and of what feeds it: the penumbra output of "shadowmask_CS_ShadowMask"
 * with m_bDoDenoising != 0 and "shadowmask_CS_PackNormalAndRoughness" (csrc/k_shadowmask.hip), "SIGMA_Shadow_ClassifyTiles.cs",
 * "SIGMA_Shadow_Blur.cs" / "SIGMA_Shadow_PostBlur.cs" and "SIGMA_Shadow_TemporalStabilization.cs" (csrc/k_sigma.hip).  NRD is not in
 * the reference's tree, so these are the project's own statement of the published algorithm; csrc/k_sigma.hip's header states the
 * rules in words, this file states them in code.  Compiled by the tests with gcc -O2 -ffp-contract=off -I oracle (tests/sigma_ref.py).
 *
 * It includes tests/alpha_test_ref.c unedited, and through it tests/shadowmask_ref.c: the ray of a texel, the walk (sm_walk), the
 * triangle test and fetch, and the textured alpha test (at_commits).
 *
 * PENUMBRA.  t = the smallest t of a candidate with TMin < t < TMax that commits (the alpha test of ITS instance's material),
 *   by brute force over every triangle of every instance (mode 0, the definition) or by the walk (mode 1), whose visitor hands the
 *   best t so far to the triangle test as TMax and never stops.  Only t leaves, so there is no tie rule.  DEVIATION: the reference
 *   traces with ACCEPT_FIRST_HIT_AND_END_SEARCH and packs CommittedRayT() of whichever hit came first.  The word: no occluder 0x7BFF
 *   (65504); else binary16 of fminf(0.5f * (t * m_TanSunAngularRadius), 32768.0f).  A far texel (depth == 0) keeps u0; u1 as sm_trace.
 * PACK.  x, y: the octahedral encoding of UnpackGBuffer's normal (ref_formats.h: pack_oct's mapping) before its 16-bit store,
 *   z: roughness, w: 0; each channel (uint)rintf(saturate(v) * 1023.0f), x in bits 0-9.
 * SUMS, in the order written: the 5 x 5 window row by row (dy outer), sumW = sumW + w then sumR = sumR + w * y; the eight taps in
 *   table order, sum = sum + w * x then wsum = wsum + w; the 3 x 3 window row by row, m1 = m1 + v, m2 = m2 + v * v, n = n + 1.
 * PATH byte per texel (what the inputs of a test reached): 1 its tile is filtered (and it is not sky), 2 the blur radius was capped,
 *   4 the history was valid, 8 the clamp changed the fetched history.
 */
#include "alpha_test_ref.c"

typedef struct
{
    float clipToWorld[16];
    uint32_t W, H;
    float jitterX, jitterY, pixelUnproject, denoisingRange, planeDistanceSensitivity, stabilizationStrength, sigmaScale;
    uint32_t frameIndex, pass, resetHistory;
} SigmaConsts;                                                                                                    /* 112 bytes */

#define SG_TILE 16u
static const float kSgMaxBlurRadius = 16.0f, kSgPostBlurRadiusScale = 0.5f, kSgNoOccluder = 65504.0f;
static const float kSgPoisson[8][2] = { { -0.4706069f, -0.4427112f }, { -0.9057375f, 0.3003471f }, { -0.3487388f, 0.4037880f }, { 0.1023042f, 0.6439373f },
                                        { 0.5699277f, 0.3513750f }, { 0.2939128f, -0.1131226f }, { 0.7836658f, -0.4208784f }, { 0.1564120f, -0.8198990f } };
#define SG_C 0.92387953f
#define SG_S 0.38268343f
#define SG_Q 0.70710678f
static const float kSgRotation[16][2] = { { 1.0f, 0.0f }, { SG_C, SG_S }, { SG_Q, SG_Q }, { SG_S, SG_C }, { 0.0f, 1.0f }, { -SG_S, SG_C }, { -SG_Q, SG_Q }, { -SG_C, SG_S },
                                          { -1.0f, 0.0f }, { -SG_C, -SG_S }, { -SG_Q, -SG_Q }, { -SG_S, -SG_C }, { 0.0f, -1.0f }, { SG_S, -SG_C }, { SG_Q, -SG_Q }, { SG_C, -SG_S } };

uint32_t sg_consts_size(void) { return (uint32_t)sizeof(SigmaConsts); }

/* ---- the penumbra trace --------------------------------------------------------------------------------------------------------- */
static void texcoords(const SmScene* s, const SmTri* T, uint16_t tc[3][2])
{
    for (int k = 0; k < 3; ++k) memcpy(tc[k], s->vertices + T->i[k] * 20u + 16u, 4);
}

static float closest_commit_brute(const SmScene* s, const MtTexture* textures, int64_t numTextures, F3 o, F3 d, float tmin, float tmax)
{
    float best = tmax;
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
            texcoords(s, &T, tc);
            if (at_commits(s, textures, numTextures, i, flags, tc, h.b1, h.b2) && h.t < best) best = h.t;
        }
    }
    return best;
}

typedef struct { const MtTexture* textures; int64_t numTextures; float tmin, best; } SgClosest;

/* the closest-commit visitor of sm_walk (csrc/k_shadowmask.hip: closestCommit) */
static int closest_commit_walk(void* ctx, const SmScene* s, uint32_t inst, uint32_t flags, uint32_t mesh, uint32_t tri, const SmRay* r)
{
    SgClosest* c = (SgClosest*)ctx;
    SmTri T;
    SmTriHit h;
    uint16_t tc[3][2];
    if (!fetch_tri(s, mesh, tri, 0, &T) || !tri_candidate(T.v[0], T.v[1], T.v[2], r, &h) || !(h.t > c->tmin && h.t < c->best)) return 0;
    texcoords(s, &T, tc);
    if (at_commits(s, c->textures, c->numTextures, inst, flags, tc, h.b1, h.b2)) c->best = h.t;
    return 0;
}

uint16_t sg_pack_penumbra(int occluded, float t, float tanSunAngularRadius)
{
    return occluded ? float_to_half(fminf(0.5f * (t * tanSunAngularRadius), 32768.0f)) : 0x7BFFu;
}

/* numTextures < 0: no table, every material by the texture-free rule.  distance (optional): t per texel, TMax where nothing commits. */
void sg_trace_penumbra(const SmConsts* k, const SmScene* s, const MtTexture* textures, int64_t numTextures, const float* depth, const uint32_t* gbufferA,
                       const uint32_t* noise, int mode, uint16_t* penumbra, uint16_t* lvd, float* distance)
{
    const float tmax = 1e10f;
    for (uint32_t py = 0; py < k->H; ++py)
        for (uint32_t px = 0; px < k->W; ++px) {
            const uint64_t i = (uint64_t)py * k->W + px;
            float o[3], d[3], w[3];
            if (!sm_texel_ray(k, px, py, depth[i], gbufferA + 4 * i, noise, o, d, w)) { lvd[i] = 0x7BFFu; if (distance) distance[i] = tmax; continue; }
            const F3 O = { o[0], o[1], o[2] }, D = { d[0], d[1], d[2] };
            float t;
            if (mode) {
                SgClosest c = { textures, numTextures, k->rayStartOffset, tmax };
                sm_walk(s, O, D, closest_commit_walk, &c, 0);
                t = c.best;
            } else t = closest_commit_brute(s, textures, numTextures, O, D, k->rayStartOffset, tmax);
            penumbra[i] = sg_pack_penumbra(t < tmax, t, k->tanSunAngularRadius);
            if (distance) distance[i] = t;
            const F3 v = { w[0] - k->camera[0], w[1] - k->camera[1], w[2] - k->camera[2] };
            lvd[i] = sm_half_bits(sqrtf(dot3f(v, v)));
        }
}

/* ---- "shadowmask_CS_PackNormalAndRoughness" ---------------------------------------------------------------------------------- */
static uint32_t unorm10(float v) { return (uint32_t)rintf(saturate(v) * 1023.0f); }

void sg_pack_normal_roughness(uint32_t W, uint32_t H, const uint32_t* gbufferA, uint32_t* out)
{
    for (uint64_t i = 0; i < (uint64_t)W * H; ++i) {
        float n[3];
        unpack_oct(gbufferA[4 * i + 1], n);
        const float l1 = (fabsf(n[0]) + fabsf(n[1])) + fabsf(n[2]);
        float o[2] = { n[0] / l1, n[1] / l1 };
        if (!(n[2] / l1 >= 0.0f)) oct_fold(o[0], o[1], o);
        out[i] = unorm10(o[0] * 0.5f + 0.5f) | unorm10(o[1] * 0.5f + 0.5f) << 10 | unorm10(unpack_unorm8(gbufferA[4 * i + 3] & 0xFFu)) << 20;
    }
}

/* ---- the denoiser's terms ----------------------------------------------------------------------------------------------------- */
static float sg_half0(uint32_t w) { return half_to_float(w & 0xFFFFu); }
static float sg_half1(uint32_t w) { return half_to_float(w >> 16); }
static int sg_sky(uint32_t depthWord, float range) { return depthWord == 0x7BFFu || half_to_float(depthWord) >= range; }

static int sg_filtered(const uint8_t* tiles, uint32_t tw, uint32_t th, uint32_t tx, uint32_t ty)
{
    uint32_t bits = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const uint32_t x = dx < 0 ? (tx > 0u ? tx - 1u : 0u) : dx > 0 ? (tx + 1u < tw ? tx + 1u : tw - 1u) : tx;
            const uint32_t y = dy < 0 ? (ty > 0u ? ty - 1u : 0u) : dy > 0 ? (ty + 1u < th ? ty + 1u : th - 1u) : ty;
            bits |= tiles[(uint64_t)y * tw + x];
        }
    return (bits & 3u) == 3u;
}

static F3 sg_world(const SigmaConsts* k, uint32_t px, uint32_t py, float depth)                     /* worldPosition of tests/lighting_ref.c */
{
    const float* m = k->clipToWorld;
    const float u = ((float)px + 0.5f) / (float)k->W, v = ((float)py + 0.5f) / (float)k->H;
    const float cx = u * 2.0f + -1.0f, cy = v * -2.0f + 1.0f;
    float h[4];
    for (int j = 0; j < 4; ++j) h[j] = fmaf(depth, m[8 + j], fmaf(cy, m[4 + j], cx * m[j])) + m[12 + j];
    const F3 wp = { h[0] / h[3], h[1] / h[3], h[2] / h[3] };
    return wp;
}

static F3 sg_normal(uint32_t w)
{
    const float fx = (float)(w & 1023u) / 1023.0f * 2.0f - 1.0f, fy = (float)((w >> 10) & 1023u) / 1023.0f * 2.0f - 1.0f;
    float n[3] = { fx, fy, (1.0f - fabsf(fx)) - fabsf(fy) }, o[3];
    const float t = saturate(-n[2]);
    n[0] += n[0] >= 0.0f ? -t : t;
    n[1] += n[1] >= 0.0f ? -t : t;
    normalize3(n, o);
    const F3 r = { o[0], o[1], o[2] };
    return r;
}

void sg_decode_normal(uint32_t word, float* out) { const F3 n = sg_normal(word); out[0] = n.x; out[1] = n.y; out[2] = n.z; }

static float sg_plane(F3 Nc, F3 Xc, F3 Xq, float denom)
{
    const F3 d = { Xq.x - Xc.x, Xq.y - Xc.y, Xq.z - Xc.z };
    return fmaxf(0.0f, 1.0f - fabsf(dot3f(Nc, d)) / denom);
}

/* ---- "SIGMA_Shadow_ClassifyTiles.cs": tiles is ceil(W / 16) x ceil(H / 16) ------------------------------------------------------- */
void sg_classify(const SigmaConsts* k, const uint16_t* penumbra, const uint16_t* lvd, uint8_t* tiles, uint32_t* data)
{
    const uint32_t W = k->W, H = k->H, tw = (W + SG_TILE - 1u) / SG_TILE, th = (H + SG_TILE - 1u) / SG_TILE;
    memset(tiles, 0, (size_t)tw * th);
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const uint64_t i = (uint64_t)py * W + px;
            const float P = half_to_float(penumbra[i]);
            if (sg_sky(lvd[i], k->denoisingRange)) { data[i] = 0x3C00u | 0x7BFFu << 16; continue; }
            const int occ = P < kSgNoOccluder;
            tiles[(uint64_t)(py / SG_TILE) * tw + px / SG_TILE] |= occ ? 2u : 1u;
            data[i] = (occ ? 0u : 0x3C00u) | (uint32_t)float_to_half(P) << 16;
        }
}

/* ---- "SIGMA_Shadow_Blur.cs" (k->pass 0), "SIGMA_Shadow_PostBlur.cs" (k->pass 1).  path (optional): bits 1 and 2, OR-ed in ------- */
void sg_blur(const SigmaConsts* k, const uint32_t* in, const uint16_t* lvd, const float* depth, const uint32_t* normalRoughness, const uint8_t* tiles, uint32_t* out,
             uint8_t* path)
{
    const uint32_t W = k->W, H = k->H, tw = (W + SG_TILE - 1u) / SG_TILE, th = (H + SG_TILE - 1u) / SG_TILE;
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const uint64_t i = (uint64_t)py * W + px;
            const uint32_t own = in[i], zw = lvd[i];
            if (sg_sky(zw, k->denoisingRange) || !sg_filtered(tiles, tw, th, px / SG_TILE, py / SG_TILE)) { out[i] = own; continue; }
            if (path) path[i] |= 1u;
            const float x = sg_half0(own), y = sg_half1(own), zc = half_to_float(zw);
            const F3 Xc = sg_world(k, px, py, depth[i]), Nc = sg_normal(normalRoughness[i]);
            const float denom = k->planeDistanceSensitivity * zc;
            float r;
            if (k->pass == 0u) {
                float sumW = 0.0f, sumR = 0.0f;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int qx = (int)px + dx, qy = (int)py + dy;
                        if (qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)H) continue;
                        const uint64_t q = (uint64_t)qy * W + (uint32_t)qx;
                        const float yq = sg_half1(in[q]);
                        if (sg_sky(lvd[q], k->denoisingRange) || !(yq < kSgNoOccluder)) continue;
                        const float w = sg_plane(Nc, Xc, sg_world(k, (uint32_t)qx, (uint32_t)qy, depth[q]), denom);
                        sumW = sumW + w;
                        sumR = sumR + w * yq;
                    }
                if (!(sumW > 0.0f)) { out[i] = (own & 0xFFFFu) | 0x7BFFu << 16; continue; }
                r = sumR / sumW;
            } else {
                if (!(y < kSgNoOccluder)) { out[i] = own; continue; }
                r = y * kSgPostBlurRadiusScale;
            }
            const float unclamped = r / (zc * k->pixelUnproject), rpx = fminf(unclamped, kSgMaxBlurRadius);
            if (path && unclamped > kSgMaxBlurRadius) path[i] |= 2u;
            const uint32_t rot = (((px & 3u) | (py & 3u) << 2) + k->frameIndex + 5u * k->pass) & 15u;
            const float c = kSgRotation[rot][0], s = kSgRotation[rot][1];
            float sum = x, wsum = 1.0f;
            for (int t = 0; t < 8; ++t) {
                const float p0 = kSgPoisson[t][0], p1 = kSgPoisson[t][1];
                const float ox = (c * p0 - s * p1) * rpx, oy = (s * p0 + c * p1) * rpx;
                const float fx = floorf(((float)px + 0.5f) + ox), fy = floorf(((float)py + 0.5f) + oy);
                if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) continue;
                const uint32_t qx = (uint32_t)fx, qy = (uint32_t)fy;
                const uint64_t q = (uint64_t)qy * W + qx;
                if (sg_sky(lvd[q], k->denoisingRange)) continue;
                const float w = sg_plane(Nc, Xc, sg_world(k, qx, qy, depth[q]), denom);
                sum = sum + w * sg_half0(in[q]);
                wsum = wsum + w;
            }
            out[i] = (uint32_t)float_to_half(sum / wsum) | (k->pass == 0u ? (uint32_t)float_to_half(r) : own >> 16) << 16;
        }
}

/* ---- "SIGMA_Shadow_TemporalStabilization.cs".  path (optional): bits 1, 4 and 8, OR-ed in.  historyReads (optional): how many texels
 * of `history` were read ------------------------------------------------------------------------------------------------------------ */
typedef struct { uint32_t i0, i1; float f; } SgAxis;

static SgAxis sg_axis_of(float uv, uint32_t dim)                                  /* tests/bloom_ref.c's axis_of */
{
    const float t = uv * (float)dim - 0.5f, t0 = floorf(t), last = (float)(dim - 1u);
    SgAxis a;
    a.i0 = (uint32_t)fminf(fmaxf(t0, 0.0f), last);
    a.i1 = (uint32_t)fminf(fmaxf(t0 + 1.0f, 0.0f), last);
    a.f = t - t0;
    return a;
}

static uint32_t sg_clamped(uint32_t p, int d, uint32_t dim) { return d < 0 ? (p > 0u ? p - 1u : 0u) : d > 0 ? (p + 1u < dim ? p + 1u : dim - 1u) : p; }

void sg_stabilize(const SigmaConsts* k, const uint32_t* in, const uint16_t* lvd, const uint32_t* motion, const uint16_t* history, const uint8_t* tiles,
                  uint16_t* newHistory, uint8_t* mask, uint8_t* path, uint64_t* historyReads)
{
    const uint32_t W = k->W, H = k->H, tw = (W + SG_TILE - 1u) / SG_TILE, th = (H + SG_TILE - 1u) / SG_TILE;
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const uint64_t i = (uint64_t)py * W + px;
            if (sg_sky(lvd[i], k->denoisingRange)) { newHistory[i] = 0x3C00u; mask[i] = 255u; continue; }
            const uint32_t own = in[i];
            const float x = sg_half0(own), y = sg_half1(own);
            float out = x;
            const int filtered = sg_filtered(tiles, tw, th, px / SG_TILE, py / SG_TILE);
            if (path && filtered) path[i] |= 1u;
            if (y > 0.0f && y < kSgNoOccluder && filtered) {
                float m1 = 0.0f, m2 = 0.0f, n = 0.0f;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const uint64_t q = (uint64_t)sg_clamped(py, dy, H) * W + sg_clamped(px, dx, W);
                        if (sg_sky(lvd[q], k->denoisingRange)) continue;
                        const float v = sg_half0(in[q]);
                        m1 = m1 + v; m2 = m2 + v * v; n = n + 1.0f;
                    }
                const float mean = m1 / n, sd = sqrtf(fmaxf(m2 / n - mean * mean, 0.0f));
                const uint32_t mw = motion[i];
                const float hx = (((float)px + 0.5f) + sg_half0(mw)) - k->jitterX, hy = (((float)py + 0.5f) + sg_half1(mw)) - k->jitterY;
                if (k->resetHistory == 0u && hx >= 0.0f && hx < (float)W && hy >= 0.0f && hy < (float)H) {
                    const SgAxis ax = sg_axis_of(hx / (float)W, W), ay = sg_axis_of(hy / (float)H, H);
                    const float t00 = half_to_float(history[(uint64_t)ay.i0 * W + ax.i0]), t10 = half_to_float(history[(uint64_t)ay.i0 * W + ax.i1]);
                    const float t01 = half_to_float(history[(uint64_t)ay.i1 * W + ax.i0]), t11 = half_to_float(history[(uint64_t)ay.i1 * W + ax.i1]);
                    if (historyReads) *historyReads += 4;
                    const float f = lerp(lerp(t00, t10, ax.f), lerp(t01, t11, ax.f), ay.f);
                    if (fabsf(f) < float_of(0x7F800000u)) {
                        const float h = fminf(fmaxf(f, mean - k->sigmaScale * sd), mean + k->sigmaScale * sd);
                        if (path) path[i] |= (uint8_t)(4u | (h != f ? 8u : 0u));
                        out = lerp(x, h, k->stabilizationStrength);
                    }
                }
            }
            newHistory[i] = float_to_half(out);
            mask[i] = (uint8_t)(uint32_t)(saturate(out) * 255.0f + 0.5f);
        }
}
