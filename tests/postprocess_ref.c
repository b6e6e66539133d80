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
#include "ref_formats.h"
#include "ref_soft_math.h"

/* ---- the load of tests/ref_formats.h and the software log2 and exp2 of tests/ref_soft_math.h (which derives the two bounds)
 * under this library's names ------------------------------------------------------------------------------------------------ */
float pr_unpack_ufloat(uint32_t c, uint32_t mbits) { return unpack_ufloat(c, mbits); }
const double PR_LOG2_BOUND = LOG2_SOFT_BOUND, PR_EXP2_BOUND = EXP2_SIGNED_BOUND;
float pr_log2(float x) { return log2_soft(x); }
float pr_exp2(float x) { return exp2_signed(x); }
float pr_exp2_reduced(float x) { return x - rintf(x); }

/* ---- pow(x, 1 / 2.2f) ----------------------------------------------------------------------------------------------------
 * y = kInvGamma * l, l = pr_log2(x) <= 0 on (0, 1].  ERROR of the result on (0, 1], relative: the exponent y is off by at most
 * dy = kInvGamma * (PR_LOG2_BOUND + 2^-24 |l|) + 2^-24 |y| (log2's error scaled, the product's rounding), which moves 2^y by the
 * factor 2^dy, that is by at most 0.6932 * dy * (1 + dy) relatively; pr_exp2 adds PR_EXP2_BOUND / 0.7071 relative to its result.
 * PR_POW_BOUND_A + PR_POW_BOUND_B * |log2 x| bounds the relative error against x^kInvGamma with the rounded kInvGamma:
 * A = 0.6932 * 0.45455 * 4.32e-8 + 8.64e-8 / 0.7071 = 1.36e-8 + 1.222e-7 -> 1.37e-7; B = 0.6932 * 2 * 0.45455 * 2^-24 = 3.76e-8
 * -> 3.8e-8.  Absolute, the result being at most 1: at most 1.37e-7 + 3.8e-8 * |log2 x| * x^0.4545 <= 1.37e-7 + 4.4e-8. */
static const float kInvGamma = 1.0f / 2.2f;                                  /* 0x1.d1745cp-2f */
const double PR_POW_BOUND_A = 1.37e-7, PR_POW_BOUND_B = 3.8e-8;

float pr_pow_gamma(float x) { return pow_soft(x, kInvGamma); }

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
