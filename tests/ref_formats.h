/* ref_formats.h -- the number formats of the G-buffer, the HDR targets and the vertex stream as the C references of tests/ state them,
 * each ONCE: the CPU counterpart of csrc/r11g11b10.hip.h, csrc/gbuffer_unpack.hip.h and the pack half of
 * csrc/visibility_resolve.hip.h, and independent of all three.  uint(x) truncates, round = rintf (half to even).
 *   ufloat    : the unsigned 5-bit-exponent float of R11G11B10_FLOAT, mbits = 6 (R, G) or 5 (B).
 *               load, exact: exponent 0 -> mantissa * 2^(-14 - mbits); exponent 31 -> +inf (mantissa 0) or a NaN carrying the
 *               mantissa; else (1 + mantissa / 2^mbits) * 2^(exponent - 15).
 *               store: NaN -> exponent and mantissa all ones, negative and -0 -> 0, +inf -> infinity, finite above the largest
 *               finite -> the largest finite, else round to nearest even, subnormals included;
 *   RGBA8     : pack uint(saturate(c) * 255.0f), R in the low byte; unpack byte * (1.0f / 255.0f), unorm16 u * (1 / 65535) as a
 *               binary32 constant: one multiply by a constant each;
 *   octahedral: pack  p = n / ((|x| + |y|) + |z|); !(p.z >= 0): the fold; p.xy * 0.5f + 0.5f; unorm 2 x 16, rounded;
 *               fold  (x, y) -> ((1 - |y|) * s(x), (1 - |x|) * s(y)), s(x) = x >= 0 ? 1 : -1;
 *               unpack f = f * 2 - 1, z = (1 - |fx|) - |fy|, t = saturate(-z), x += (x >= 0 ? -t : t), same for y, normalize
 *               (the fold in its branch-free form: another sequence of roundings than the fold above);
 *   R9G9B9E5  : pack by the shared-exponent bias trick; unpack ldexpf(mantissa, E - 24) (exact);
 *   normal    : the vertex stream's R10G10B10A2, x in bits 20-29, y 10-19, z 0-9: (float)q / 1023.0f, * 2.0f, - 1.0f;
 *               the world normal normalize(mul(unpack, adjugate(World3x3))), adjugate rows cross(r1, r2), cross(r2, r0),
 *               cross(r0, r1), the row-vector product as an fmaf chain;
 *   random    : QuickRandomFloat, the LCG seed = 1664525 * seed + 1013904223, (float)(seed & 0xFFFFFF) / 2^24.
 */
#ifndef TESTS_REF_FORMATS_H
#define TESTS_REF_FORMATS_H

#include "ref_base.h"

/* ---- R11G11B10_FLOAT ---------------------------------------------------------------------------------------------------- */
static inline float unpack_ufloat(uint32_t c, uint32_t mbits)
{
    const uint32_t e = c >> mbits, m = c & ((1u << mbits) - 1u);
    if (e == 0u) return (float)m * (1.0f / (float)(1u << (14u + mbits)));
    return float_of((e == 31u ? 0x7F800000u : (e + 112u) << 23) | m << (23u - mbits));
}

static inline uint32_t pack_ufloat(float v, uint32_t mbits)
{
    const uint32_t shift = 23u - mbits, inf = 31u << mbits, maxFinite = inf - 1u, u = bits_of(v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return inf | ((1u << mbits) - 1u);
    if (u >> 31) return 0u;
    if (u == 0x7F800000u) return inf;
    if (u >= 0x38800000u) {
        const uint32_t r = u - (112u << 23);
        const uint32_t q = (r + ((1u << (shift - 1)) - 1u) + ((r >> shift) & 1u)) >> shift;
        return q < maxFinite ? q : maxFinite;
    }
    return (uint32_t)rintf(v * (float)(1u << (14u + mbits)));
}

static inline void unpack_r11g11b10(uint32_t w, float rgb[3])
{
    rgb[0] = unpack_ufloat(w & 0x7FFu, 6); rgb[1] = unpack_ufloat((w >> 11) & 0x7FFu, 6); rgb[2] = unpack_ufloat(w >> 22, 5);
}

static inline uint32_t pack_r11g11b10(float r, float g, float b) { return pack_ufloat(r, 6) | pack_ufloat(g, 6) << 11 | pack_ufloat(b, 5) << 22; }

/* ---- RGBA8, unorm16 ----------------------------------------------------------------------------------------------------- */
static inline uint32_t pack_rgba8(float r, float g, float b, float a)
{
    return (uint32_t)(saturate(r) * 255.0f) | (uint32_t)(saturate(g) * 255.0f) << 8 | (uint32_t)(saturate(b) * 255.0f) << 16 |
           (uint32_t)(saturate(a) * 255.0f) << 24;
}

static inline float unpack_unorm8(uint32_t byte) { return (float)byte * (1.0f / 255.0f); }
static inline float unpack_unorm16(uint32_t u) { return (float)u * (1.0f / 65535.0f); }

/* ---- the octahedral normal ---------------------------------------------------------------------------------------------- */
static inline void oct_fold(float x, float y, float o[2])
{
    o[0] = (1.0f - fabsf(y)) * (x >= 0.0f ? 1.0f : -1.0f);
    o[1] = (1.0f - fabsf(x)) * (y >= 0.0f ? 1.0f : -1.0f);
}

static inline uint32_t pack_oct(float nx, float ny, float nz)
{
    const float l1 = (fabsf(nx) + fabsf(ny)) + fabsf(nz);
    float o[2] = { nx / l1, ny / l1 };
    if (!(nz / l1 >= 0.0f)) oct_fold(o[0], o[1], o);
    const uint32_t ux = (uint32_t)rintf(saturate(o[0] * 0.5f + 0.5f) * 65535.0f), uy = (uint32_t)rintf(saturate(o[1] * 0.5f + 0.5f) * 65535.0f);
    return ux | uy << 16;
}

static inline void unpack_oct(uint32_t word, float o[3])
{
    const float fx = unpack_unorm16(word & 0xFFFFu) * 2.0f - 1.0f, fy = unpack_unorm16(word >> 16) * 2.0f - 1.0f;
    float n[3] = { fx, fy, (1.0f - fabsf(fx)) - fabsf(fy) };
    const float t = saturate(-n[2]);
    n[0] += n[0] >= 0.0f ? -t : t;
    n[1] += n[1] >= 0.0f ? -t : t;
    normalize3(n, o);
}

/* ---- R9G9B9E5 ----------------------------------------------------------------------------------------------------------- */
static inline uint32_t pack_r9g9b9e5(float r, float g, float b)
{
    const float kMaxVal = float_of(0x477F8000u), kMinVal = float_of(0x37800000u);
    r = fminf(fmaxf(r, 0.0f), kMaxVal);
    g = fminf(fmaxf(g, 0.0f), kMaxVal);
    b = fminf(fmaxf(b, 0.0f), kMaxVal);
    const float maxChannel = fmaxf(fmaxf(kMinVal, r), fmaxf(g, b));
    const float bias = float_of((bits_of(maxChannel) + 0x07804000u) & 0x7F800000u);
    const uint32_t R = bits_of(r + bias), G = bits_of(g + bias), B = bits_of(b + bias);
    const uint32_t E = (bits_of(bias) << 4) + 0x10000000u;
    return E | B << 18 | G << 9 | (R & 0x1FFu);
}

static inline void unpack_r9g9b9e5(uint32_t v, float o[3])
{
    const int e = (int)(v >> 27) - 24;
    o[0] = ldexpf((float)(v & 0x1FFu), e); o[1] = ldexpf((float)((v >> 9) & 0x1FFu), e); o[2] = ldexpf((float)((v >> 18) & 0x1FFu), e);
}

/* ---- the vertex normal -------------------------------------------------------------------------------------------------- */
static inline void unpack_normal10(uint32_t packed, float o[3])
{
    const float x = (float)((packed >> 20) & 0x3FFu) / 1023.0f, y = (float)((packed >> 10) & 0x3FFu) / 1023.0f, z = (float)(packed & 0x3FFu) / 1023.0f;
    o[0] = x * 2.0f - 1.0f; o[1] = y * 2.0f - 1.0f; o[2] = z * 2.0f - 1.0f;
}

/* normalize(mul(unpack(word), adjugate(World3x3))); world: the 4 x 4 world matrix, row vectors */
static inline void vertex_normal(uint32_t word, const float world[4][4], float o[3])
{
    float u[3], r0[3], r1[3], r2[3], n[3];
    unpack_normal10(word, u);
    cross3(world[1], world[2], r0);
    cross3(world[2], world[0], r1);
    cross3(world[0], world[1], r2);
    for (int j = 0; j < 3; ++j) n[j] = fmaf(u[2], r2[j], fmaf(u[1], r1[j], u[0] * r0[j]));
    normalize3(n, o);
}

/* ---- QuickRandomFloat: steps the seed ----------------------------------------------------------------------------------- */
static inline float quick_random_float(uint32_t* seed)
{
    *seed = 1664525u * *seed + 1013904223u;
    return (float)(*seed & 0x00FFFFFFu) / 16777216.0f;
}

#endif
