/* ddgi_ref.c -- test reference of the DDGI ambient term of "deferredlighting_PS_Main" and of debug view 10 of
 * "deferredlighting_PS_Main_Debug" (csrc/ddgi_irradiance.hip.h, csrc/k_deferredlighting.hip).  Compiled by the tests themselves
 * with gcc -O2 -ffp-contract=off.  It includes lighting_ref.c for everything the pass had before (unpack, world position, the
 * directional light, the debug views, the R11G11B10_FLOAT store) and adds the irradiance query.
 *
 * The RTXGI SDK's Irradiance.hlsl is not part of this project: this file and the kernel's header are the project's own statement
 * of the published query (Majercik et al., JCGT 2019), and they are what the tests pin.
 *
 * TEXTURES here are dense arrays, slice after slice without padding: data uint16 [slices][cz][cx][4] (binary16 x, y, z, w),
 * irradiance uint32 [slices][cz * 8][cx * 8] (R bits 0-9, G 10-19, B 20-29), distance uint16 [slices][cz * 16][cx * 16][2].
 *
 * CONVENTION.  binary32 throughout, / and sqrtf correctly rounded, fmaf only in dot3 and the two polynomials.
 *   ext       = (spacing * (float)(counts - 1)) * 0.5f;  normalize(v) = v / sqrtf(dot3(v, v));
 *   viewDir   = normalize(world - cameraOrigin);  delta = |world - origin| - ext;
 *   blend     = 1 if all three delta < 0, else ((1 - saturate(delta.x / spacing.x)) * (1 - saturate(delta.y / spacing.y))) *
 *               (1 - saturate(delta.z / spacing.z));  !(blend > 0): (0, 0, 0);
 *   P         = world + (N * normalBias - viewDir * viewBias);
 *   base      = (int)fminf(fmaxf(((P - origin) + ext) / spacing, 0), (float)(counts - 1));
 *   probePos(c) = ((spacing * (float)c) - ext) + origin, + data(c).xyz * spacing with flags bit 0;
 *   alpha     = saturate((P - probePos(base)) / spacing);
 *   neighbour : off = (i & 1, (i >> 1) & 1, (i >> 2) & 1); c = min(base + off, counts - 1); skipped with flags bit 1 and
 *               data(c).w == 1.0f; dirW = normalize(pp - world); toB = pp - P; dist = sqrtf(dot3(toB, toB)); dirB = toB / dist;
 *               tri = fmaxf(0.001f, off ? alpha : 1 - alpha); wrap = (dot3(dirW, N) + 1) * 0.5f; w = wrap * wrap + 0.2f;
 *               d = 2 * bilinear(distance, probeUV(c, oct(-dirB), 14)); var = |d.x * d.x - d.y|; dist > d.x: v = dist - d.x,
 *               ch = var / (var + v * v), ch = fmaxf((ch * ch) * ch, 0); else ch = 1; w = w * fmaxf(0.05f, ch);
 *               w = fmaxf(0.000001f, w); w < 0.2f: w = w * ((w * w) * (1.0f / (0.2f * 0.2f))); w = w * ((tri.x * tri.y) * tri.z);
 *               e = pow(bilinear(irradiance, probeUV(c, oct(N), 6)), gamma * 0.5f); sum += w * e; wsum += w;
 *   result    = wsum == 0 ? 0 : ((((sum / wsum) * (sum / wsum)) * RN(2 pi)) * 1.0989f) * blend;
 *   oct(d)    : l = (|d.x| + |d.y|) + |d.z|; uv = d.xy / l; d.z < 0: uv = ((1 - |uv.y|) * s(uv.x), (1 - |uv.x|) * s(uv.y)), s(x) = x >= 0 ? 1 : -1;
 *   probeUV   : ((float)(c * N) + (float)N * 0.5f + o * ((float)interior * 0.5f)) / (float)textureDim, N = interior + 2;
 *   bilinear  : t = uv * (float)dim - 0.5f; t0 = floorf(t); f = t - t0; i = (int)fminf(fmaxf(t0, -1), (float)dim); texels
 *               (i + dim) % dim and (i + 1 + dim) % dim (wrap); lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy), lerp(x, y, s) = x + s * (y - x);
 *   texels    : UNORM10 (float)v / 1023.0f; binary16 exact;
 *   pow(x, e) : x > 0: dg_exp2(e * dg_log2(x)), the two software functions of tests/ref_soft_math.h; otherwise 0.
 *   PS_Main   : ambient = (albedo * (1 / pi)) * irr, times (float)ssao / 255.0f when m_SSAOEnabled (unbound: 255);
 *               rgb = lr_lit's rgb + ambient.  Debug view 10: irr.
 * A pixel exactly on a probe divides 0 by 0 and follows binary32 rules; the tests keep surfaces off probes.
 */
#include "lighting_ref.c"
#include "ref_soft_math.h"

typedef struct
{
    float origin[3];
    float probeNormalBias;
    float probeSpacing[3];
    float probeViewBias;
    int32_t probeCounts[3];
    float probeIrradianceEncodingGamma;
    uint32_t numIrradianceInteriorTexels;
    uint32_t numDistanceInteriorTexels;
    uint32_t flags;
    uint32_t pad;
} DgDesc;

/* what one query decided (the float64 check leaves out pixels that decide differently) and which branches it took */
typedef struct
{
    uint32_t inside;                           /* 1: blend == 1 by the inside test; 0: the product */
    int32_t base[3];
    uint32_t evaluated;                        /* 0: blend <= 0, nothing below is set */
    uint32_t skipMask, chebMask, crushMask, clampMask, relocMask, foldMask;   /* bit i: neighbour i (fold: bit 8 is oct(N)) */
    float blend;
} DgTrace;

/* branch counters, in pixels (dg_lighting adds to them) */
enum { DG_BLEND_ONE, DG_BLEND_PARTIAL, DG_BLEND_ZERO, DG_SKIPPED_SOME, DG_SKIPPED_ALL, DG_RELOCATED, DG_CHEB_TAKEN, DG_CHEB_NOT, DG_CRUSH_TAKEN, DG_CRUSH_NOT,
       DG_FOLD_TAKEN, DG_FOLD_NOT, DG_CLAMPED, DG_COUNTERS };

float dg_log2(float x) { return log2_soft(x); }
float dg_exp2(float x) { return exp2_signed(x); }
float dg_pow(float x, float e) { return pow_soft(x, e); }

/* returns 1 when the fold (d.z < 0) was taken */
static int dg_oct(const float d[3], float uv[2])
{
    const float l = (fabsf(d[0]) + fabsf(d[1])) + fabsf(d[2]);
    uv[0] = d[0] / l; uv[1] = d[1] / l;
    if (d[2] < 0.0f) oct_fold(uv[0], uv[1], uv);
    return d[2] < 0.0f;
}
void dg_oct_n(const float* d, uint64_t n, float* uv) { for (uint64_t i = 0; i < n; ++i) dg_oct(d + 3 * i, uv + 2 * i); }

typedef struct { uint32_t i0, i1; float f; } DgAxis;
static DgAxis axis_of(float uv, uint32_t dim)
{
    const float t = uv * (float)dim - 0.5f, t0 = floorf(t);
    const int i = (int)fminf(fmaxf(t0, -1.0f), (float)dim);
    const DgAxis a = { (uint32_t)(i + (int)dim) % dim, (uint32_t)(i + 1 + (int)dim) % dim, t - t0 };
    return a;
}

static float probe_coord(int c, uint32_t interior, float o, uint32_t dim)
{
    const uint32_t n = interior + 2u;
    return ((float)(c * (int)n) + (float)n * 0.5f + o * ((float)interior * 0.5f)) / (float)dim;
}

/* the bilinear fetch of probe c's irradiance tile at octahedral coordinate o, before the pow */
void dg_fetch_irradiance(const DgDesc* D, const uint32_t* irradiance, const int32_t c[3], const float o[2], float rgb[3])
{
    const uint32_t W = (uint32_t)D->probeCounts[0] * 8u, H = (uint32_t)D->probeCounts[2] * 8u;
    const DgAxis ax = axis_of(probe_coord(c[0], 6u, o[0], W), W), ay = axis_of(probe_coord(c[2], 6u, o[1], H), H);
    const uint32_t* s = irradiance + (uint64_t)c[1] * W * H;
    const uint32_t w00 = s[ay.i0 * W + ax.i0], w10 = s[ay.i0 * W + ax.i1], w01 = s[ay.i1 * W + ax.i0], w11 = s[ay.i1 * W + ax.i1];
    for (uint32_t ch = 0; ch < 3; ++ch) {
        const uint32_t sh = 10u * ch;
        const float t00 = (float)((w00 >> sh) & 1023u) / 1023.0f, t10 = (float)((w10 >> sh) & 1023u) / 1023.0f;
        const float t01 = (float)((w01 >> sh) & 1023u) / 1023.0f, t11 = (float)((w11 >> sh) & 1023u) / 1023.0f;
        rgb[ch] = lerp(lerp(t00, t10, ax.f), lerp(t01, t11, ax.f), ay.f);
    }
}

/* the same of the distance tile: (r, g) */
void dg_fetch_distance(const DgDesc* D, const uint16_t* distance, const int32_t c[3], const float o[2], float rg[2])
{
    const uint32_t W = (uint32_t)D->probeCounts[0] * 16u, H = (uint32_t)D->probeCounts[2] * 16u;
    const DgAxis ax = axis_of(probe_coord(c[0], 14u, o[0], W), W), ay = axis_of(probe_coord(c[2], 14u, o[1], H), H);
    const uint16_t* s = distance + (uint64_t)c[1] * W * H * 2u;
    for (uint32_t ch = 0; ch < 2; ++ch) {
        const float t00 = half_to_float(s[(ay.i0 * W + ax.i0) * 2u + ch]), t10 = half_to_float(s[(ay.i0 * W + ax.i1) * 2u + ch]);
        const float t01 = half_to_float(s[(ay.i1 * W + ax.i0) * 2u + ch]), t11 = half_to_float(s[(ay.i1 * W + ax.i1) * 2u + ch]);
        rg[ch] = lerp(lerp(t00, t10, ax.f), lerp(t01, t11, ax.f), ay.f);
    }
}

/* the volume's half extent, and probe number p's coordinates: p = (y * counts.z + z) * counts.x + x */
static void probe_extent(const DgDesc* D, float ext[3])
{
    for (int a = 0; a < 3; ++a) ext[a] = (D->probeSpacing[a] * (float)(D->probeCounts[a] - 1)) * 0.5f;
}

static inline void probe_coords(const DgDesc* D, uint32_t probe, int32_t c[3])
{
    const uint32_t cx = (uint32_t)D->probeCounts[0], cz = (uint32_t)D->probeCounts[2];
    c[0] = (int32_t)(probe % cx); c[1] = (int32_t)(probe / (cx * cz)); c[2] = (int32_t)((probe / cx) % cz);
}

static void probe_pos(const DgDesc* D, const float ext[3], const uint16_t* data, const int32_t c[3], float pp[3], float* state, int* relocated)
{
    const uint16_t* d = data + (((uint64_t)c[1] * (uint32_t)D->probeCounts[2] + (uint32_t)c[2]) * (uint32_t)D->probeCounts[0] + (uint32_t)c[0]) * 4u;
    for (int a = 0; a < 3; ++a) {
        pp[a] = (D->probeSpacing[a] * (float)c[a] - ext[a]) + D->origin[a];
        if (D->flags & 1u) pp[a] = pp[a] + half_to_float(d[a]) * D->probeSpacing[a];
    }
    *state = half_to_float(d[3]);
    if (relocated) *relocated = (D->flags & 1u) && ((d[0] | d[1] | d[2]) & 0x7FFFu) != 0;
}

/* coordinates, position and data.w of probe number `probe`, for the references that include this file */
static inline void probe_at(const DgDesc* D, const uint16_t* data, uint32_t probe, int32_t c[3], float pos[3], float* state)
{
    float ext[3];
    probe_extent(D, ext);
    probe_coords(D, probe, c);
    probe_pos(D, ext, data, c, pos, state, NULL);
}

void dg_irradiance(const DgDesc* D, const uint16_t* data, const uint32_t* irradiance, const uint16_t* distance, const float world[3], const float N[3],
                   const float cameraOrigin[3], float out[3], DgTrace* tr)
{
    DgTrace local;
    if (!tr) tr = &local;
    memset(tr, 0, sizeof *tr);
    out[0] = out[1] = out[2] = 0.0f;
    float ext[3], toPoint[3], viewDir[3], delta[3], P[3], basePos[3], alpha[3], state;
    int32_t last[3], base[3];
    probe_extent(D, ext);
    for (int a = 0; a < 3; ++a) {
        last[a] = D->probeCounts[a] - 1;
        toPoint[a] = world[a] - cameraOrigin[a];
    }
    normalize3(toPoint, viewDir);
    for (int a = 0; a < 3; ++a) delta[a] = fabsf(world[a] - D->origin[a]) - ext[a];
    float blend = 1.0f;
    tr->inside = delta[0] < 0.0f && delta[1] < 0.0f && delta[2] < 0.0f;
    if (!tr->inside)
        blend = ((1.0f - saturate(delta[0] / D->probeSpacing[0])) * (1.0f - saturate(delta[1] / D->probeSpacing[1]))) * (1.0f - saturate(delta[2] / D->probeSpacing[2]));
    tr->blend = blend;
    if (!(blend > 0.0f)) return;
    tr->evaluated = 1;
    for (int a = 0; a < 3; ++a) {
        P[a] = world[a] + (N[a] * D->probeNormalBias - viewDir[a] * D->probeViewBias);
        base[a] = (int32_t)fminf(fmaxf(((P[a] - D->origin[a]) + ext[a]) / D->probeSpacing[a], 0.0f), (float)last[a]);
        tr->base[a] = base[a];
    }
    probe_pos(D, ext, data, base, basePos, &state, NULL);
    for (int a = 0; a < 3; ++a) alpha[a] = saturate((P[a] - basePos[a]) / D->probeSpacing[a]);
    float nuv[2];
    if (dg_oct(N, nuv)) tr->foldMask |= 1u << 8;
    const float halfGamma = D->probeIrradianceEncodingGamma * 0.5f;

    float sum[3] = { 0.0f, 0.0f, 0.0f }, wsum = 0.0f;
    for (int i = 0; i < 8; ++i) {
        const int off[3] = { i & 1, (i >> 1) & 1, (i >> 2) & 1 };
        int32_t c[3];
        for (int a = 0; a < 3; ++a) {
            c[a] = base[a] + off[a] < last[a] ? base[a] + off[a] : last[a];
            if (c[a] != base[a] + off[a]) tr->clampMask |= 1u << i;
        }
        float pp[3], toW[3], dirW[3], toB[3], negDirB[3], tri[3], duv[2], rg[2], e[3];
        int relocated;
        probe_pos(D, ext, data, c, pp, &state, &relocated);
        if ((D->flags & 2u) && state == 1.0f) { tr->skipMask |= 1u << i; continue; }
        if (relocated) tr->relocMask |= 1u << i;
        for (int a = 0; a < 3; ++a) { toW[a] = pp[a] - world[a]; toB[a] = pp[a] - P[a]; }
        normalize3(toW, dirW);
        const float dist = sqrtf(dot3(toB, toB));
        for (int a = 0; a < 3; ++a) {
            negDirB[a] = -(toB[a] / dist);
            tri[a] = fmaxf(0.001f, off[a] ? alpha[a] : 1.0f - alpha[a]);
        }
        const float wrap = (dot3(dirW, N) + 1.0f) * 0.5f;
        float w = wrap * wrap + 0.2f;
        if (dg_oct(negDirB, duv)) tr->foldMask |= 1u << i;
        dg_fetch_distance(D, distance, c, duv, rg);
        const float mean = 2.0f * rg[0], mean2 = 2.0f * rg[1];
        const float var = fabsf(mean * mean - mean2);
        float ch = 1.0f;
        if (dist > mean) {
            const float v = dist - mean;
            ch = var / (var + v * v);
            ch = fmaxf((ch * ch) * ch, 0.0f);
            tr->chebMask |= 1u << i;
        }
        w = w * fmaxf(0.05f, ch);
        w = fmaxf(0.000001f, w);
        if (w < 0.2f) { w = w * ((w * w) * (1.0f / (0.2f * 0.2f))); tr->crushMask |= 1u << i; }
        w = w * ((tri[0] * tri[1]) * tri[2]);
        dg_fetch_irradiance(D, irradiance, c, nuv, e);
        for (int k = 0; k < 3; ++k) sum[k] = sum[k] + w * dg_pow(e[k], halfGamma);
        wsum = wsum + w;
    }
    if (wsum == 0.0f) return;
    for (int k = 0; k < 3; ++k) {
        const float r = sum[k] / wsum;
        out[k] = (((r * r) * 0x1.921fb6p+2f) * 1.0989f) * blend;
    }
}

/* One full-screen pass with the volume: lr_lighting's arguments plus the descriptor and the three textures.  PS_Main (debug 0)
 * adds the ambient term when k->m_bRTDDGIEnabled; _Debug (debug 1) writes the irradiance in mode 10; everything else is
 * lr_lighting's.  irr: float[H*W*3] or NULL, the query's result per written pixel; traces: DgTrace[H*W] or NULL;
 * counters: uint64[DG_COUNTERS] or NULL, added to. */
void dg_lighting(const LrConsts* k, int debug, const DgDesc* D, const uint16_t* data, const uint32_t* irradiance, const uint16_t* distance,
                 const uint32_t* gbuffer, const uint32_t* motion, const float* depth, const uint8_t* ssao, const uint8_t* shadow,
                 uint32_t* out, float* rgb, float* irr, DgTrace* traces, uint64_t* counters)
{
    const uint32_t W = k->m_LightingOutputResolution[0], H = k->m_LightingOutputResolution[1];
    const int query = debug ? k->m_DebugMode == 10u : k->m_bRTDDGIEnabled != 0u;
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const uint64_t i = (uint64_t)py * W + px;
            if (!(depth[i] > 0.0f)) continue;
            const float sh = shadow ? (float)shadow[i] / 255.0f : 1.0f;
            float c[3];
            if (debug) lr_debug(k, gbuffer + 4 * i, motion ? motion[i] : 0u, sh, ssao ? ssao[i] : 255u, c);
            else lr_lit(k, gbuffer + 4 * i, px, py, depth[i], sh, c);
            if (query) {
                LrGBuffer p;
                unpack_gbuffer(gbuffer + 4 * i, &p);
                float world[3], e[3];
                DgTrace t;
                world_position(k, px, py, depth[i], world);
                dg_irradiance(D, data, irradiance, distance, world, p.normal, k->m_CameraOrigin, e, &t);
                if (irr) memcpy(irr + 3 * i, e, sizeof e);
                if (traces) traces[i] = t;
                if (counters) {
                    const uint32_t live = ~t.skipMask & 0xFFu;
                    counters[t.inside ? DG_BLEND_ONE : t.evaluated ? DG_BLEND_PARTIAL : DG_BLEND_ZERO] += 1;
                    if (t.evaluated) {
                        counters[DG_SKIPPED_SOME] += t.skipMask != 0u;
                        counters[DG_SKIPPED_ALL] += t.skipMask == 0xFFu;
                        counters[DG_RELOCATED] += t.relocMask != 0u;
                        counters[DG_CHEB_TAKEN] += t.chebMask != 0u;
                        counters[DG_CHEB_NOT] += (live & ~t.chebMask) != 0u;
                        counters[DG_CRUSH_TAKEN] += t.crushMask != 0u;
                        counters[DG_CRUSH_NOT] += (live & ~t.crushMask) != 0u;
                        counters[DG_FOLD_TAKEN] += t.foldMask != 0u;
                        counters[DG_FOLD_NOT] += (((live | 0x100u) & ~t.foldMask)) != 0u;
                        counters[DG_CLAMPED] += t.clampMask != 0u;
                    }
                }
                if (debug) {
                    memcpy(c, e, sizeof e);
                } else {
                    const float ao = (float)(ssao ? ssao[i] : 255u) / 255.0f;
                    for (int ch = 0; ch < 3; ++ch) {
                        float ambient = (p.albedo[ch] * kInvPi) * e[ch];
                        if (k->m_SSAOEnabled) ambient = ambient * ao;
                        c[ch] = c[ch] + ambient;
                    }
                }
            }
            if (out) out[i] = lr_pack_r11g11b10(c[0], c[1], c[2]);
            if (rgb) memcpy(rgb + 3 * i, c, sizeof c);
        }
}

void dg_pow_n(const float* x, uint64_t n, float e, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = dg_pow(x[i], e); }

/* array forms for the tests: the query's inputs per pixel (world position, normal, albedo; untouched where depth is not > 0),
 * and the query at n given points */
void dg_inputs(const LrConsts* k, const uint32_t* gbuffer, const float* depth, float* world, float* normal, float* albedo)
{
    const uint32_t W = k->m_LightingOutputResolution[0], H = k->m_LightingOutputResolution[1];
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const uint64_t i = (uint64_t)py * W + px;
            if (!(depth[i] > 0.0f)) continue;
            LrGBuffer p;
            unpack_gbuffer(gbuffer + 4 * i, &p);
            world_position(k, px, py, depth[i], world + 3 * i);
            memcpy(normal + 3 * i, p.normal, sizeof p.normal);
            memcpy(albedo + 3 * i, p.albedo, sizeof p.albedo);
        }
}

void dg_irradiance_n(const DgDesc* D, const uint16_t* data, const uint32_t* irradiance, const uint16_t* distance, const float* world, const float* N,
                     const float cameraOrigin[3], uint64_t n, float* out, DgTrace* traces)
{
    for (uint64_t i = 0; i < n; ++i) dg_irradiance(D, data, irradiance, distance, world + 3 * i, N + 3 * i, cameraOrigin, out + 3 * i, traces ? traces + i : NULL);
}
