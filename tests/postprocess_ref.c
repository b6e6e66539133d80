/* postprocess_ref.c -- test reference of "adaptluminance_CS_GenerateLuminanceHistogram", "adaptluminance_CS_AdaptExposure" and
 * "postprocess_PS_PostProcess" (csrc/k_postprocess.hip, csrc/soft_math.hip.h, csrc/r11g11b10.hip.h).  Compiled by the tests
 * themselves with gcc -O2 -ffp-contract=off: only the fmaf calls written here fuse.
 *
 * CONVENTION (parity unpinned; the kernel's header states it, DESIGN.md 3 repeats it).  It extends the lighting convention
 * (lighting_ref.c): IEEE binary32, / correctly rounded, dot3 = fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)), min / max = fminf /
 * fmaxf (a NaN operand is dropped), saturate = fminf(fmaxf(x, 0), 1) (a NaN gives 0), lerp(x, y, s) = x + s * (y - x) always
 * evaluated, uint(x) truncates.
 *   load      : R11G11B10_FLOAT, exact: exponent 0 -> mantissa * 2^(-14 - mbits); exponent 31 -> +inf (mantissa 0) or a NaN
 *               carrying the mantissa; else (1 + mantissa / 2^mbits) * 2^(exponent - 15);
 *   luminance : dot3(rgb, (float)0.212671, (float)0.715160, (float)0.072169);
 *   bin       : lum >= 0.005f ? uint(saturate((log2(lum) - minLog) * invRange) * 254.0f + 1.0f) : 0 (NaN -> 0, +inf -> 255);
 *   adapt     : sum = wrapping uint32 sum of count[i] * i; avg = (float)sum / fmaxf((float)nbPixels - (float)count[0], 1.0f)
 *               - 1.0f; lum = exp2(((avg / 254.0f) * range) + minLog); adapted = last + (lum - last) * speed; exposure =
 *               middleGray / (adapted * (1.0f - middleGray));
 *   post      : rgb = lerp(colour, bloom, strength); sceneLuminance = manual, or the luminance buffer's float when manual ==
 *               0.0f; rgb *= middleGray / sceneLuminance; PBRNeutralToneMapping; pow(rgb, 1.0f / 2.2f); store;
 *   tone curve: startCompression = (float)(0.8 - 0.04), d = (float)(1. - (0.8 - 0.04)) (literal-only subexpressions folded in
 *               float64, rounded once), d * d a binary32 product, desaturation (float)0.15; x = min(r, min(g, b)); offset =
 *               x < 0.08f ? x - (6.25f * x) * x : 0.04f; rgb -= offset; peak = max(r, max(g, b)); peak < startCompression
 *               returns; newPeak = 1.0f - (d * d) / ((peak + d) - startCompression); rgb *= newPeak / peak; g = 1.0f - 1.0f /
 *               (desaturation * (peak - newPeak) + 1.0f); lerp(rgb, newPeak, g);
 *   pow       : x > 0 ? exp2((1.0f / 2.2f) * log2(x)) : 0 (zero, negative, NaN -> 0; +inf -> NaN, stored as 0);
 *   store     : each channel uint(saturate(c) * 255.0f + 0.5f), R in the low byte, alpha 255.
 *   A zero scene luminance makes the scale +inf: a nonzero colour becomes +inf, which the curve turns into NaN (inf * (1 / inf));
 *   a zero colour is 0 * inf = NaN at once.  Both are stored as bytes 0, 0, 0, 255.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static float saturate(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

/* ---- the R11G11B10_FLOAT load ------------------------------------------------------------------------------------------ */
float pr_unpack_ufloat(uint32_t c, uint32_t mbits)
{
    const uint32_t e = c >> mbits, m = c & ((1u << mbits) - 1u);
    if (e == 0u) return (float)m * (1.0f / (float)(1u << (14u + mbits)));
    return float_of((e == 31u ? 0x7F800000u : (e + 112u) << 23) | m << (23u - mbits));
}

static void unpack_r11g11b10(uint32_t w, float rgb[3])
{
    rgb[0] = pr_unpack_ufloat(w & 0x7FFu, 6); rgb[1] = pr_unpack_ufloat((w >> 11) & 0x7FFu, 6); rgb[2] = pr_unpack_ufloat(w >> 22, 5);
}

/* ---- software log2 for x > 0 ---------------------------------------------------------------------------------------------
 * x = 2^k * m with m in [sqrt(1/2), sqrt(2)): the bits are split at 0x3F3504F3 (a subnormal x is scaled by 2^24 first, exact).
 * f = m - 1 in [-0.29290, 0.41422) is exact (Sterbenz).  log2(1 + f) = f * P(f), P the degree-9 interpolant of log2(1 + f) / f
 * at the Chebyshev nodes of that interval, coefficients rounded to binary32; the result is fmaf(f, P, (float)k).
 * ERROR, absolute, of f * P(f) against log2(1 + f):
 *   truncation, coefficient rounding included (the polynomial in exact arithmetic on 4001 points): 9.35e-9 = 0.314 * 2^-25;
 *   Horner    : every fmaf rounds once, by at most half an ulp of its result; the error of partial j reaches the value times
 *               |f|^(j+1), |f| <= 0.41422.  The partials lie in p0 [1.207, 1.708) p1 [0.568, 0.903) p2 [0.368, 0.620)
 *               p3 [0.271, 0.473) p4 [0.214, 0.383) p5 [0.177, 0.322) p6 [0.149, 0.280) p7 [0.133, 0.255) p8 [0.140, 0.217),
 *               half ulps 2^-24, 2^-25, 2^-25, 2^-26 (p3 .. p7), 2^-27: sum (0.8284 + 0.1716 + 0.0711 + 0.0147 + 0.0061 +
 *               0.0025 + 0.0010 + 0.0004 + 0.0001) * 2^-25 = 1.096 * 2^-25;
 *   last fmaf : rounds the result r once: half an ulp of r, at most 2^-24 * |r|;
 *   bound     : |pr_log2(x) - log2(x)| <= PR_LOG2_BOUND + 2^-24 * |pr_log2(x)| with PR_LOG2_BOUND = 1.45 * 2^-25 (4.32e-8)
 *               >= (0.314 + 1.096) * 2^-25.  f = 0 gives exactly k: powers of two are exact. */
static const float kLog2C[10] = { 0x1.715476p+0f, -0x1.715470p-1f, 0x1.ec70aap-2f, -0x1.715a70p-2f, 0x1.277a52p-2f,
                                  -0x1.eab7a8p-3f, 0x1.a38c64p-3f, -0x1.87f6aap-3f, 0x1.7a63c4p-3f, -0x1.b84fe0p-4f };
const double PR_LOG2_BOUND = 1.45 * 0x1p-25;

float pr_log2(float x)
{
    uint32_t u = bits_of(x);
    if (u == 0x7F800000u) return x;
    int bias = -127;
    if (u < 0x00800000u) { u = bits_of(x * 0x1p24f); bias = -151; }
    u += 0x3F800000u - 0x3F3504F3u;
    const int k = (int)(u >> 23) + bias;
    const float f = float_of((u & 0x007FFFFFu) + 0x3F3504F3u) - 1.0f;
    float p = kLog2C[9];
    for (int j = 8; j >= 0; --j) p = fmaf(p, f, kLog2C[j]);
    return fmaf(f, p, (float)k);
}

/* ---- software exp2, either sign ------------------------------------------------------------------------------------------
 * i = rintf(x), f = x - i in [-0.5, 0.5].  EXACT on both sides of zero: for |x| < 0.5, i = 0 and f = x; otherwise i != 0,
 * x and i are both multiples of ulp(x), and |f| <= 0.5 <= |x|, so f is a multiple of ulp(x) no larger than x: representable.
 * (The lighting pass's x - ceilf(x) is exact for x <= 0 only: for 0 < x < 0.5 it is x - 1, which needs more bits than x has.)
 * 2^f = 1 + f * g(f), g the degree-5 interpolant of (2^f - 1) / f at the Chebyshev nodes of [-0.5, 0.5], coefficients rounded
 * to binary32; the result is ldexpf(p, i), exact unless subnormal.  i is clamped to [-300, 300] before the conversion so that
 * NaN and huge arguments are defined (a NaN p stays NaN; 2^300 p overflows to +inf; 2^-300 p is 0).
 * ERROR, absolute, of p against 2^f in [0.7071, 1.4143] (the result scales both by 2^i):
 *   truncation, coefficient rounding included: 6.96e-9 = 0.234 * 2^-25;
 *   Horner    : partials p0 [0.707, 1.415) p1 [0.585, 0.829) p2 [0.214, 0.271) p3 [0.0510, 0.0607) p4 [0.00898, 0.01033)
 *               p5 [0.00126, 0.00142), half ulps 2^-24, 2^-25, 2^-26 (p2 reaches 0.27 > 0.25), 2^-29, 2^-31, 2^-34, each
 *               reaching p times |f|^j <= 2^-j: (2 + 0.5 + 0.125 + 0.0078 + 0.0010 + 0.0001) * 2^-25 = 2.634 * 2^-25;
 *   bound     : PR_EXP2_BOUND = 2.9 * 2^-25 (8.64e-8) >= (0.234 + 2.634) * 2^-25, times 2^i.  f = 0 gives exactly 1. */
static const float kExp2C[7] = { 0x1.000000p+0f, 0x1.62e430p-1f, 0x1.ebfbe0p-3f, 0x1.c6af6cp-5f, 0x1.3b2a54p-7f, 0x1.5f0890p-10f, 0x1.44138ap-13f };
const double PR_EXP2_BOUND = 2.9 * 0x1p-25;

float pr_exp2_reduced(float x) { return x - rintf(x); }

float pr_exp2(float x)
{
    const float i = rintf(x), f = x - i;
    float p = kExp2C[6];
    for (int j = 5; j >= 0; --j) p = fmaf(p, f, kExp2C[j]);
    return ldexpf(p, (int)fminf(fmaxf(i, -300.0f), 300.0f));
}

/* ---- pow(x, 1 / 2.2f) ----------------------------------------------------------------------------------------------------
 * y = kInvGamma * l, l = pr_log2(x) <= 0 on (0, 1].  ERROR of the result on (0, 1], relative: the exponent y is off by at most
 * dy = kInvGamma * (PR_LOG2_BOUND + 2^-24 |l|) + 2^-24 |y| (log2's error scaled, the product's rounding), which moves 2^y by the
 * factor 2^dy, that is by at most 0.6932 * dy * (1 + dy) relatively; pr_exp2 adds PR_EXP2_BOUND / 0.7071 relative to its result.
 * PR_POW_BOUND_A + PR_POW_BOUND_B * |log2 x| bounds the relative error against x^kInvGamma with the rounded kInvGamma:
 * A = 0.6932 * 0.45455 * 4.32e-8 + 8.64e-8 / 0.7071 = 1.36e-8 + 1.222e-7 -> 1.37e-7; B = 0.6932 * 2 * 0.45455 * 2^-24 = 3.76e-8
 * -> 3.8e-8.  Absolute, the result being at most 1: at most 1.37e-7 + 3.8e-8 * |log2 x| * x^0.4545 <= 1.37e-7 + 4.4e-8. */
static const float kInvGamma = 1.0f / 2.2f;                                  /* 0x1.d1745cp-2f */
const double PR_POW_BOUND_A = 1.37e-7, PR_POW_BOUND_B = 3.8e-8;

float pr_pow_gamma(float x) { return x > 0.0f ? pr_exp2(kInvGamma * pr_log2(x)) : 0.0f; }

/* ---- the histogram ------------------------------------------------------------------------------------------------------- */
static const float kLumR = 0.212671f, kLumG = 0.715160f, kLumB = 0.072169f;

float pr_luminance(uint32_t word)
{
    float c[3];
    unpack_r11g11b10(word, c);
    return fmaf(c[2], kLumB, fmaf(c[1], kLumG, c[0] * kLumR));
}

uint32_t pr_bin(uint32_t word, float minLog, float invRange)
{
    const float lum = pr_luminance(word);
    if (!(lum >= 0.005f)) return 0u;
    const float logLum = saturate((pr_log2(lum) - minLog) * invRange);
    return (uint32_t)(logLum * 254.0f + 1.0f);
}

/* adds to histogram[256] */
void pr_histogram(const uint32_t* words, uint64_t n, float minLog, float invRange, uint32_t* histogram)
{
    for (uint64_t i = 0; i < n; ++i) histogram[pr_bin(words[i], minLog, invRange)] += 1u;
}

/* ---- CS_AdaptExposure ---------------------------------------------------------------------------------------------------- */
typedef struct { float minLog, range, speed; uint32_t nbPixels; float middleGray; } PrAdaptParams;

void pr_adapt_exposure(const PrAdaptParams* k, const uint32_t* histogram, float* luminance, float* exposure)
{
    uint32_t sum = 0;
    for (uint32_t i = 0; i < 256u; ++i) sum += histogram[i] * i;
    const float avg = (float)sum / fmaxf((float)k->nbPixels - (float)histogram[0], 1.0f) - 1.0f;
    const float lum = pr_exp2(((avg / 254.0f) * k->range) + k->minLog);
    const float last = *luminance, adapted = last + (lum - last) * k->speed;
    *luminance = adapted;
    *exposure = k->middleGray / (adapted * (1.0f - k->middleGray));
}

/* ---- PS_PostProcess ------------------------------------------------------------------------------------------------------ */
typedef struct { uint32_t dims[2]; float manualExposure, middleGray, whitePoint, bloomStrength; } PrPostParams;

static const float kStartCompression = (float)(0.8 - 0.04), kD = (float)(1. - (0.8 - 0.04)), kDesaturation = 0.15f;

static void tone_map(float c[3])
{
    const float x = fminf(c[0], fminf(c[1], c[2]));
    const float offset = x < 0.08f ? x - (6.25f * x) * x : 0.04f;
    for (int j = 0; j < 3; ++j) c[j] = c[j] - offset;
    const float peak = fmaxf(c[0], fmaxf(c[1], c[2]));
    if (peak < kStartCompression) return;
    const float newPeak = 1.0f - (kD * kD) / ((peak + kD) - kStartCompression);
    const float ratio = newPeak / peak;
    for (int j = 0; j < 3; ++j) c[j] = c[j] * ratio;
    const float g = 1.0f - 1.0f / (kDesaturation * (peak - newPeak) + 1.0f);
    for (int j = 0; j < 3; ++j) c[j] = c[j] + g * (newPeak - c[j]);
}

static uint32_t unorm8(float c) { return (uint32_t)(saturate(c) * 255.0f + 0.5f); }

/* one texel; srgb (may be NULL): the three floats before the store */
uint32_t pr_post_texel(const PrPostParams* k, uint32_t colour, uint32_t bloom, float bufferLuminance, float* srgb)
{
    float c[3], b[3];
    unpack_r11g11b10(colour, c);
    unpack_r11g11b10(bloom, b);
    for (int j = 0; j < 3; ++j) c[j] = c[j] + k->bloomStrength * (b[j] - c[j]);
    float sceneLuminance = k->manualExposure;
    if (sceneLuminance == 0.0f) sceneLuminance = bufferLuminance;
    const float lumScale = k->middleGray / sceneLuminance;
    for (int j = 0; j < 3; ++j) c[j] = c[j] * lumScale;
    tone_map(c);
    for (int j = 0; j < 3; ++j) c[j] = pr_pow_gamma(c[j]);
    if (srgb) memcpy(srgb, c, sizeof c);
    return unorm8(c[0]) | unorm8(c[1]) << 8 | unorm8(c[2]) << 16 | 0xFF000000u;
}

/* n texels; bloom may be NULL (unbound: 0, 0, 0); srgb may be NULL */
void pr_post(const PrPostParams* k, const uint32_t* colour, const uint32_t* bloom, uint64_t n, float bufferLuminance, uint32_t* out, float* srgb)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = pr_post_texel(k, colour[i], bloom ? bloom[i] : 0u, bufferLuminance, srgb ? srgb + 3 * i : 0);
}

/* the tone curve alone, for the constants' test: in place on n float3 */
void pr_tone_map_n(float* rgb, uint64_t n) { for (uint64_t i = 0; i < n; ++i) tone_map(rgb + 3 * i); }
void pr_constants(float out[8])
{
    out[0] = kLumR; out[1] = kLumG; out[2] = kLumB; out[3] = kStartCompression; out[4] = kD; out[5] = kD * kD; out[6] = kDesaturation; out[7] = kInvGamma;
}

/* array forms for the tests */
void pr_unpack_ufloat_n(const uint32_t* c, uint64_t n, uint32_t mbits, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = pr_unpack_ufloat(c[i], mbits); }
void pr_log2_n(const float* x, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = pr_log2(x[i]); }
void pr_exp2_n(const float* x, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = pr_exp2(x[i]); }
void pr_exp2_reduced_n(const float* x, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = pr_exp2_reduced(x[i]); }
void pr_pow_gamma_n(const float* x, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = pr_pow_gamma(x[i]); }
void pr_luminance_n(const uint32_t* w, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = pr_luminance(w[i]); }
void pr_bin_n(const uint32_t* w, uint64_t n, float minLog, float invRange, uint32_t* out) { for (uint64_t i = 0; i < n; ++i) out[i] = pr_bin(w[i], minLog, invRange); }
