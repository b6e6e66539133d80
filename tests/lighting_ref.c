/* lighting_ref.c -- test reference of "deferredlighting_PS_Main" and "deferredlighting_PS_Main_Debug"
 * (csrc/k_deferredlighting.hip).  Compiled by the tests themselves with gcc -O2 -ffp-contract=off: only the fmaf calls
 * written here fuse.
 *
 * CONVENTION (parity unpinned; the kernel's header states it, DESIGN.md 3 repeats it).  IEEE binary32 throughout, / and sqrtf
 * correctly rounded.
 *   written   : a pixel is written iff its depth is > 0.0f (NaN, +-0 and negative depths leave u0 as it is);
 *   dot3      : fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x));  normalize(v) = v / sqrtf(dot3(v, v));  rcp(x) = 1.0f / x;
 *   saturate  : fminf(fmaxf(x, 0), 1) (a NaN gives 0);  lerp(x, y, s) = x + s * (y - x);  uint(x) truncates;
 *   unpack    : RGBA8 byte * (1.0f / 255.0f); unorm16 likewise by 1 / 65535 (one multiply by a constant each; tests/ref_formats.h); octahedral
 *               f = f * 2 - 1, z = (1 - |fx|) - |fy|, t = saturate(-z), x += (x >= 0 ? -t : t), same for y, normalize;
 *               R9G9B9E5 ldexpf(mantissa, E - 24) (exact);
 *   position  : uv = (px + 0.5f, py + 0.5f) / (float)resolution; clip = (u * 2 + -1, v * -2 + 1); the row vector
 *               (clip.x, clip.y, depth, 1) times m_ClipToWorld, each column fmaf(depth, m[2][j], fmaf(clip.y, m[1][j],
 *               clip.x * m[0][j])) + m[3][j]; world = xyz / w;
 *   PS_Main   : diffuse = albedo * (1 - metallic); f0 = lerp(0.04f, albedo, metallic); V = normalize(origin - world); L = the
 *               light vector as given; H = normalize(V + L); NdotV = saturate(|N.V| + 1e-5f), NdotL, NdotH, VdotH saturated;
 *               a = r * r, a2 = fminf(fmaxf(a * a, 0.0001f), 1); D = a2 / ((pi * d) * d), d = (NdotH * a2 - NdotH) * NdotH + 1;
 *               Vis = 0.5f * rcp(NdotL * (NdotV * (1 - a2) + a2) + NdotV * (NdotL * (1 - a2) + a2)); Fc = Pow5(1 - VdotH) =
 *               ((x * x) * (x * x)) * x, F = Fc + (1 - Fc) * f0; spec = (D * Vis) * F + EnvBRDFApprox(f0, r, NdotV);
 *               rgb = ((((albedoDiffuse * (1 / pi) + spec) * NdotL) * strength) * shadow) + emissive;
 *   EnvBRDF   : r4 = r * (-1, -0.0275f, -0.572f, 0.022f) + (1, 0.0425f, 1.04f, -0.04f); a004 = fminf(r4.x * r4.x,
 *               exp2(-9.28f * NdotV)) * r4.x + r4.y; AB = (-1.04f, 1.04f) * a004 + r4.zw; f0 * AB.x + AB.y;
 *   exp2(x)   : software, x <= 0: i = ceilf(x), f = x - i in (-1, 0] (exact: for |x| >= 1 both are multiples of ulp(x) and the
 *               difference is smaller than either; for |x| < 1 it is x itself -- floorf would make f = x + 1 inexact there),
 *               p = the degree-7 Horner polynomial below in fmaf, result ldexpf(p, i) (exact);
 *   shadow    : the R8_UNORM texel, (float)byte / 255.0f (unbound: 1.0f); SSAO: the R8_UINT texel (unbound: 255);
 *   _Debug    : shadowFactor = fmaxf(0.05f, shadow); 1 dot3(N, L) * shadowFactor; 2, 3 seed = uint(debug * 255.0f), three
 *               successive QuickRandomFloat; 4 albedo; 5 normal; 6 emissive; 7 metallic; 8 roughness; 9 (float)ssao / 255.0f;
 *               11 shadowFactor; 12 kLODColors[uint(debug * 255.0f)], an index >= 8 gives (0, 0, 0); 13 (motion.x / (float)W,
 *               motion.y / (float)H, 0); any other mode (0, 0, 0);
 *   store     : R11G11B10_FLOAT per channel: NaN -> exponent and mantissa all ones, negative and -0 -> 0, +inf -> infinity,
 *               finite above the largest finite -> the largest finite, else round to nearest even, subnormals included.
 */
#include "ref_formats.h"

/* ---- the formats of tests/ref_formats.h under this library's names ------------------------------------------------------ */
uint32_t lr_pack_ufloat(float v, uint32_t mbits) { return pack_ufloat(v, mbits); }
uint32_t lr_pack_r11g11b10(float r, float g, float b) { return pack_r11g11b10(r, g, b); }
float lr_unpack_unorm8(uint32_t byte) { return unpack_unorm8(byte); }
float lr_unpack_unorm16(uint32_t u) { return unpack_unorm16(u); }
void lr_unpack_oct(uint32_t word, float o[3]) { unpack_oct(word, o); }
void lr_unpack_r9g9b9e5(uint32_t v, float o[3]) { unpack_r9g9b9e5(v, o); }

/* ---- software exp2 for x <= 0 -----------------------------------------------------------------------------------------
 * 2^f on [-1, 0] as 1 + f * g(f), g the degree-6 interpolant of (2^f - 1) / f at the Chebyshev nodes of [-1, 0], coefficients
 * rounded to binary32.  ERROR, absolute, of p against 2^f in [0.5, 1] (the result scales both by 2^i exactly):
 *   truncation, coefficient rounding included (the polynomial below in exact arithmetic on 40001 points): 3.33e-9 = 0.112 * 2^-25,
 *               below half an ulp of the result (2^-25);
 *   Horner    : every fmaf rounds once, by at most half an ulp of its result, and the error of partial k reaches p times |f|^k <= 1.
 *               The partials lie in p1 [0.5, 0.694) p2 [0.193, 0.241) p3 [0.047, 0.056) p4 [0.0084, 0.0097) p5 [0.00119, 0.00133)
 *               p6 [0.000137, 0.000149), so their half ulps are 2^-25, 2^-27, 2^-29, 2^-31, 2^-34, 2^-37; the last fmaf gives p in
 *               [0.5, 1]: 2^-25.  Sum (1 + 1 + 2^-2 + 2^-4 + 2^-6 + 2^-9 + 2^-12) * 2^-25 = 2.3304 * 2^-25;
 *   bound     : LR_EXP2_BOUND = 2.46 * 2^-25 (7.33e-8) >= 2.3304 * 2^-25 + 0.112 * 2^-25, times 2^i; that is 1.23 ulp of a result
 *               in [0.5, 1).  f = 0 gives exactly 1, so integers give exact powers of two. */
static const float kExp2CeilC[8] = { 0x1.000000p+0f, 0x1.62e430p-1f, 0x1.ebfbdep-3f, 0x1.c6b024p-5f, 0x1.3b20d4p-7f, 0x1.5ca2c2p-10f, 0x1.383ffcp-13f, 0x1.7b4b46p-17f };
const double LR_EXP2_BOUND = 2.46 * 0x1p-25;

float lr_exp2(float x)
{
    const float i = ceilf(x), f = x - i;
    float p = kExp2CeilC[7];
    for (int k = 6; k >= 0; --k) p = fmaf(p, f, kExp2CeilC[k]);
    return ldexpf(p, (int)i);
}

/* ---- UnpackGBuffer ---------------------------------------------------------------------------------------------------- */
typedef struct
{
    float m_ClipToWorld[4][4];
    float m_CameraOrigin[3];
    uint32_t m_SSAOEnabled;
    uint32_t m_DebugMode;
    float m_DirectionalLightVector[3];
    float m_DirectionalLightStrength;
    uint32_t m_LightingOutputResolution[2];
    uint32_t m_bRTDDGIEnabled;
} LrConsts;

typedef struct { float albedo[3], debug, normal[3], emissive[3], roughness, metallic; } LrGBuffer;

static void unpack_gbuffer(const uint32_t g[4], LrGBuffer* o)
{
    for (int c = 0; c < 3; ++c) o->albedo[c] = lr_unpack_unorm8((g[0] >> (8 * c)) & 0xFFu);
    o->debug = lr_unpack_unorm8(g[0] >> 24);
    lr_unpack_oct(g[1], o->normal);
    lr_unpack_r9g9b9e5(g[2], o->emissive);
    o->roughness = lr_unpack_unorm8(g[3] & 0xFFu);
    o->metallic = lr_unpack_unorm8((g[3] >> 8) & 0xFFu);
}

static const float kPi = 3.14159265358979323846f, kInvPi = (float)(1.0 / 3.14159265358979323846);

static void world_position(const LrConsts* k, uint32_t px, uint32_t py, float depth, float o[3])
{
    const float u = ((float)px + 0.5f) / (float)k->m_LightingOutputResolution[0], v = ((float)py + 0.5f) / (float)k->m_LightingOutputResolution[1];
    const float cx = u * 2.0f + -1.0f, cy = v * -2.0f + 1.0f;
    float h[4];
    for (int j = 0; j < 4; ++j)
        h[j] = fmaf(depth, k->m_ClipToWorld[2][j], fmaf(cy, k->m_ClipToWorld[1][j], cx * k->m_ClipToWorld[0][j])) + k->m_ClipToWorld[3][j];
    o[0] = h[0] / h[3]; o[1] = h[1] / h[3]; o[2] = h[2] / h[3];
}

static void env_brdf_approx(const float f0[3], float roughness, float ndotv, float o[3])
{
    const float rx = roughness * -1.0f + 1.0f, ry = roughness * -0.0275f + 0.0425f, rz = roughness * -0.572f + 1.04f, rw = roughness * 0.022f + -0.04f;
    const float a004 = fminf(rx * rx, lr_exp2(-9.28f * ndotv)) * rx + ry;
    const float A = -1.04f * a004 + rz, B = 1.04f * a004 + rw;
    for (int c = 0; c < 3; ++c) o[c] = f0[c] * A + B;
}

/* PS_Main of one pixel: the float3 before the store */
void lr_lit(const LrConsts* k, const uint32_t g[4], uint32_t px, uint32_t py, float depth, float shadow, float rgb[3])
{
    LrGBuffer p;
    unpack_gbuffer(g, &p);
    float world[3], toEye[3], V[3], VL[3], H[3], diffuse[3], f0[3], env[3];
    world_position(k, px, py, depth, world);
    const float oneMinusMetal = 1.0f - p.metallic, dielectric = 0.08f * 0.5f;
    for (int c = 0; c < 3; ++c) {
        diffuse[c] = p.albedo[c] * oneMinusMetal;
        f0[c] = dielectric + p.metallic * (p.albedo[c] - dielectric);
        toEye[c] = k->m_CameraOrigin[c] - world[c];
    }
    normalize3(toEye, V);
    const float* L = k->m_DirectionalLightVector;
    for (int c = 0; c < 3; ++c) VL[c] = V[c] + L[c];
    normalize3(VL, H);
    const float NdotV = saturate(fabsf(dot3(p.normal, V)) + 1e-5f), NdotL = saturate(dot3(p.normal, L));
    const float NdotH = saturate(dot3(p.normal, H)), VdotH = saturate(dot3(V, H));
    const float a = p.roughness * p.roughness, a2 = fminf(fmaxf(a * a, 0.0001f), 1.0f);
    const float d = (NdotH * a2 - NdotH) * NdotH + 1.0f;
    const float D = a2 / ((kPi * d) * d);
    const float smithV = NdotL * (NdotV * (1.0f - a2) + a2), smithL = NdotV * (NdotL * (1.0f - a2) + a2);
    const float Vis = 0.5f * (1.0f / (smithV + smithL));
    const float x = 1.0f - VdotH, xx = x * x, Fc = (xx * xx) * x;
    const float DVis = D * Vis;
    env_brdf_approx(f0, p.roughness, NdotV, env);
    for (int c = 0; c < 3; ++c) {
        const float F = Fc + (1.0f - Fc) * f0[c];
        const float spec = DVis * F + env[c];
        rgb[c] = (((diffuse[c] * kInvPi + spec) * NdotL) * k->m_DirectionalLightStrength) * shadow + p.emissive[c];
    }
}

static const float kLODColors[8][3] = { { 1.0f, 0.0f, 0.0f }, { 1.0f, 0.5f, 0.0f }, { 1.0f, 1.0f, 0.0f }, { 0.5f, 1.0f, 0.0f },
                                        { 0.0f, 1.0f, 0.0f }, { 0.0f, 0.5f, 1.0f }, { 0.0f, 0.0f, 1.0f }, { 0.5f, 0.0f, 1.0f } };

/* PS_Main_Debug of one pixel; motion: the RG16_FLOAT texel (x in the low half) */
void lr_debug(const LrConsts* k, const uint32_t g[4], uint32_t motion, float shadow, uint32_t ssao, float rgb[3])
{
    LrGBuffer p;
    unpack_gbuffer(g, &p);
    const float shadowFactor = fmaxf(0.05f, shadow);
    rgb[0] = rgb[1] = rgb[2] = 0.0f;
    switch (k->m_DebugMode) {
    case 1: rgb[0] = rgb[1] = rgb[2] = dot3(p.normal, k->m_DirectionalLightVector) * shadowFactor; break;
    case 2: case 3: {
        uint32_t seed = (uint32_t)(p.debug * 255.0f);
        rgb[0] = quick_random_float(&seed); rgb[1] = quick_random_float(&seed); rgb[2] = quick_random_float(&seed);
        break; }
    case 4: memcpy(rgb, p.albedo, sizeof p.albedo); break;
    case 5: memcpy(rgb, p.normal, sizeof p.normal); break;
    case 6: memcpy(rgb, p.emissive, sizeof p.emissive); break;
    case 7: rgb[0] = rgb[1] = rgb[2] = p.metallic; break;
    case 8: rgb[0] = rgb[1] = rgb[2] = p.roughness; break;
    case 9: rgb[0] = rgb[1] = rgb[2] = (float)ssao / 255.0f; break;
    case 11: rgb[0] = rgb[1] = rgb[2] = shadowFactor; break;
    case 12: {
        const uint32_t lod = (uint32_t)(p.debug * 255.0f);
        if (lod < 8u) memcpy(rgb, kLODColors[lod], sizeof kLODColors[lod]);
        break; }
    case 13:
        rgb[0] = half_to_float(motion & 0xFFFFu) / (float)k->m_LightingOutputResolution[0];
        rgb[1] = half_to_float(motion >> 16) / (float)k->m_LightingOutputResolution[1];
        break;
    default: break;
    }
}

/* One full-screen pass.  gbuffer: uint32[H*W*4]; motion: uint32[H*W] (debug only, may be NULL otherwise); depth: float[H*W];
 * ssao / shadow: uint8[H*W] or NULL (unbound).  out: uint32[H*W] packed words and / or rgb: float[H*W*3], either may be NULL;
 * texels whose depth is not > 0 keep what they hold. */
void lr_lighting(const LrConsts* k, int debug, const uint32_t* gbuffer, const uint32_t* motion, const float* depth, const uint8_t* ssao,
                 const uint8_t* shadow, uint32_t* out, float* rgb)
{
    const uint32_t W = k->m_LightingOutputResolution[0], H = k->m_LightingOutputResolution[1];
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const uint64_t i = (uint64_t)py * W + px;
            if (!(depth[i] > 0.0f)) continue;
            const float sh = shadow ? (float)shadow[i] / 255.0f : 1.0f;
            float c[3];
            if (debug) lr_debug(k, gbuffer + 4 * i, motion ? motion[i] : 0u, sh, ssao ? ssao[i] : 255u, c);
            else lr_lit(k, gbuffer + 4 * i, px, py, depth[i], sh, c);
            if (out) out[i] = lr_pack_r11g11b10(c[0], c[1], c[2]);
            if (rgb) memcpy(rgb + 3 * i, c, sizeof c);
        }
}

/* array forms for the tests */
void lr_pack_ufloat_n(const float* v, uint64_t n, uint32_t mbits, uint32_t* out) { for (uint64_t i = 0; i < n; ++i) out[i] = lr_pack_ufloat(v[i], mbits); }
void lr_exp2_n(const float* x, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = lr_exp2(x[i]); }
void lr_unpack_unorm8_n(const uint32_t* v, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = lr_unpack_unorm8(v[i]); }
void lr_unpack_unorm16_n(const uint32_t* v, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = lr_unpack_unorm16(v[i]); }
void lr_unpack_oct_n(const uint32_t* v, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) lr_unpack_oct(v[i], out + 3 * i); }
void lr_unpack_r9g9b9e5_n(const uint32_t* v, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) lr_unpack_r9g9b9e5(v[i], out + 3 * i); }
