/* ref_soft_math.h -- the software log2, two-sided exp2 and arc cosine of the passes, stated ONCE for every C reference of tests/
 * with their derivations and error bounds: the CPU counterpart of csrc/soft_math.hip.h, which repeats these functions word for
 * word, and independent of it.  Compiled with the references by gcc -O2 -ffp-contract=off: only the fmaf calls written here fuse.
 * The lighting pass's one-sided exp2 (ceil, degree 7, x <= 0) is another function and stays in tests/lighting_ref.c.  The software
 * sine and cosine stay in tests/gtao_ref.c, where tests/test_gtao_ref.py reads their coefficients, and in tests/shadowmask_ref.c.
 */
#ifndef TESTS_REF_SOFT_MATH_H
#define TESTS_REF_SOFT_MATH_H

#include "ref_base.h"

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
 *   bound     : |log2_soft(x) - log2(x)| <= LOG2_SOFT_BOUND + 2^-24 * |log2_soft(x)| with LOG2_SOFT_BOUND = 1.45 * 2^-25 (4.32e-8)
 *               >= (0.314 + 1.096) * 2^-25.  f = 0 gives exactly k: powers of two are exact. */
#define LOG2_SOFT_BOUND (1.45 * 0x1p-25)
static const float kLog2C[10] = { 0x1.715476p+0f, -0x1.715470p-1f, 0x1.ec70aap-2f, -0x1.715a70p-2f, 0x1.277a52p-2f,
                                  -0x1.eab7a8p-3f, 0x1.a38c64p-3f, -0x1.87f6aap-3f, 0x1.7a63c4p-3f, -0x1.b84fe0p-4f };

static inline float log2_soft(float x)
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
 *   bound     : EXP2_SIGNED_BOUND = 2.9 * 2^-25 (8.64e-8) >= (0.234 + 2.634) * 2^-25, times 2^i.  f = 0 gives exactly 1. */
#define EXP2_SIGNED_BOUND (2.9 * 0x1p-25)
static const float kExp2C[7] = { 0x1.000000p+0f, 0x1.62e430p-1f, 0x1.ebfbe0p-3f, 0x1.c6af6cp-5f, 0x1.3b2a54p-7f, 0x1.5f0890p-10f, 0x1.44138ap-13f };

static inline float exp2_signed(float x)
{
    const float i = rintf(x), f = x - i;
    float p = kExp2C[6];
    for (int j = 5; j >= 0; --j) p = fmaf(p, f, kExp2C[j]);
    return ldexpf(p, (int)fminf(fmaxf(i, -300.0f), 300.0f));
}

/* pow(x, e) of the passes: zero, negative and NaN bases give 0 */
static inline float pow_soft(float x, float e) { return x > 0.0f ? exp2_signed(e * log2_soft(x)) : 0.0f; }

/* ---- software arc cosine -------------------------------------------------------------------------------------------------
 * asin(s) = s + s * z * P(z), z = s * s in [0, 0.25]; P is the degree-4 weighted least-squares fit of (asin(sqrt z) / sqrt z
 * - 1) / z at 400 Chebyshev nodes of [0, 0.25] (weight s z, so that the error of the sum is what is minimised), coefficients
 * rounded to binary32.  |s + s z P(z) - asin s| <= 0.038 * 2^-24 on 400 001 points, coefficients as rounded.
 *   |x| <= 0.5: z = x * x, t = fmaf(x * z, P, x), result RN(pi / 2) - t;
 *   |x| >  0.5: z = (1 - |x|) * 0.5 (exact: Sterbenz, then a power of two), s = sqrtf(z) <= 0.5, t = fmaf(s * z, P, s), r = 2 t
 *               (exact); x > 0: r, else RN(pi) - r.  acos(1) = 0 and acos(-1) = RN(pi) exactly; !(|x| <= 1) gives NaN.
 * ERROR, absolute, in units of 2^-24.  t: its fmaf rounds once, t <= 0.5236: 0.5; the product s * z carries two roundings and
 * multiplies P <= 0.1875, the term is <= 0.0236: 0.047; P's four fmaf round by <= 2^-26 together, times |s z| <= 0.125: 0.03;
 * truncation 0.038: t within 0.62.  For |x| > 0.5 add sqrtf's half ulp 2^-26 times asin' <= 1.1547: 0.289, and P read at z
 * rather than RN(s)^2, 2^-23 relative: 0.054; t within 0.963, r within 1.93.  The last subtraction rounds by <= 2^-23 (results
 * in [2, pi]): 2; RN(pi / 2) is off by 0.733 and RN(pi) by 1.467.  So |x| <= 0.5: 3.36; x > 0.5: 1.93; x < -0.5: 5.4.
 * ACOS_SOFT_BOUND = 5.5 * 2^-24 (3.28e-7). */
#define ACOS_SOFT_BOUND (5.5 * 0x1p-24)
static const float kAcosC[5] = { 0x1.555626p-3f, 0x1.32ea80p-4f, 0x1.766edcp-5f, 0x1.7b4b14p-6f, 0x1.665bcap-5f };

static inline float acos_poly(float z)
{
    float p = kAcosC[4];
    for (int j = 3; j >= 0; --j) p = fmaf(p, z, kAcosC[j]);
    return p;
}

static inline float acos_soft(float x)
{
    const float a = fabsf(x);
    if (!(a <= 1.0f)) return nanf("");
    if (a <= 0.5f) {
        const float z = x * x;
        return 0x1.921fb6p+0f - fmaf(x * z, acos_poly(z), x);
    }
    const float z = (1.0f - a) * 0.5f, s = sqrtf(z);
    const float r = 2.0f * fmaf(s * z, acos_poly(z), s);
    return x > 0.0f ? r : 0x1.921fb6p+1f - r;
}

#endif
