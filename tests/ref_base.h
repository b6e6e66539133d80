/* ref_base.h -- what every C reference of tests/ shares below the level of a format: bit casts, the scalar and float[3] helpers of the
 * lighting convention, and binary16 <-> binary32.  Each rule is stated here ONCE; the references include this file, never a copy.
 * Compiled with them by gcc -O2 -ffp-contract=off: only the fmaf calls written here fuse.
 *   saturate  : fminf(fmaxf(x, 0), 1) (a NaN gives 0);  lerp(x, y, s) = x + s * (y - x), always evaluated;
 *   dot3      : fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x));  normalize3(v) = v / sqrtf(dot3(v, v)), one division per component;
 *   cross3    : each component fmaf(a, b, -(c * d));
 *   edge      : the edge function of the rasters, fmaf(b.x - a.x, p.y - a.y, -((b.y - a.y) * (p.x - a.x))).
 */
#ifndef TESTS_REF_BASE_H
#define TESTS_REF_BASE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

static inline uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline float saturate(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
static inline float lerp(float x, float y, float s) { return x + s * (y - x); }

static inline float dot3(const float a[3], const float b[3]) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }

static inline void cross3(const float a[3], const float b[3], float o[3])
{
    o[0] = fmaf(a[1], b[2], -(a[2] * b[1]));
    o[1] = fmaf(a[2], b[0], -(a[0] * b[2]));
    o[2] = fmaf(a[0], b[1], -(a[1] * b[0]));
}

static inline void normalize3(const float v[3], float o[3])
{
    const float len = sqrtf(dot3(v, v));
    for (int j = 0; j < 3; ++j) o[j] = v[j] / len;
}

static inline float edge(float ax, float ay, float bx, float by, float px, float py)
{
    return fmaf(bx - ax, py - ay, -((by - ay) * (px - ax)));
}

/* ---- binary16 -> binary32, exact ------------------------------------------------------------------------------------------ */
static inline float half_to_float(uint32_t h)
{
    const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 31u) return float_of(s | 0x7F800000u | m << 13);                /* infinity, or a NaN carrying the mantissa */
    if (e == 0u) return float_of(s | bits_of((float)m * 0x1p-24f));          /* subnormal or zero */
    return float_of(s | (e + 112u) << 23 | m << 13);
}

/* ---- binary32 -> binary16: round to nearest even, overflow to infinity, every NaN to 0x7E00 (its sign never shows) ---------- */
static inline uint16_t float_to_half(float f)
{
    const uint32_t u = bits_of(f), s = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return 0x7E00u;
    if (a >= 0x477FF000u) return (uint16_t)(s | 0x7C00u);                     /* >= 65520: infinity (65520 is the tie, to even) */
    if (a < 0x38800000u) return (uint16_t)(s | (uint32_t)rintf(float_of(a) * 0x1p24f));   /* below 2^-14: a multiple of 2^-24, rintf ties to even; 0x0400 is 2^-14 */
    return (uint16_t)(s | (((a - 0x38000000u) + 0x0FFFu + ((a >> 13) & 1u)) >> 13));      /* a carry moves into the exponent */
}

#endif
