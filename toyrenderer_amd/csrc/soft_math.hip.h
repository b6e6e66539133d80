// soft_math.hip.h -- log2, a two-sided exp2 and an arc cosine in software, for the passes behind LightingOutput
// (k_postprocess.hip) and the sky pass (k_sky.hip).  v_log_f32 and v_exp_f32 are good to 1 ulp only and cannot be restated
// on a CPU; these can, and tests/ref_soft_math.h restates the three word for word (log2_soft, exp2_signed, acos_soft) next
// to the derivation of the coefficients and of the error bounds, once for every C reference under tests/.  The
// lighting pass keeps its own exp2Soft (direct_light.hip.h): that one is proven for x <= 0 only and its words must not move.
//
//   log2Soft(x), x > 0 (the callers test; +inf gives +inf): a subnormal x is first scaled by 2^24 (exact).  The bits are split
//             at sqrt(1/2): k = exponent, m in [0x1.6a09e6p-1, 0x1.6a09e6p+0), f = m - 1 (exact, Sterbenz), P the degree-9 Horner
//             polynomial below in fma, result fma(f, P, (float)k).  |error| <= 1.45 * 2^-25 + 2^-24 * |result|.
//   exp2Signed(x), any sign: i = rint(x), f = x - i in [-0.5, 0.5], exact on both sides of 0 (|x| < 0.5: i = 0 and f = x;
//             otherwise i != 0, x and i are multiples of ulp(x) and |f| <= 0.5 <= |x|, so f is a multiple of ulp(x) no larger
//             than x: representable).  p = the degree-6 Horner polynomial in fma, in [0x1.6a09e6p-1, 0x1.6a09e8p+0]; result
//             ldexp(p, clamp(i, -300, 300)) (exact unless subnormal; the clamp makes NaN and huge arguments defined: NaN gives
//             NaN, +inf gives NaN (inf - inf), -inf likewise).  |error| <= 2.9 * 2^-25 * 2^i.
//   acosSoft(x): a = |x|; !(a <= 1) (outside [-1, 1], NaN) gives NaN.  asin(s) = s + s * z * P(z), z = s * s in [0, 0.25], P the
//             degree-4 polynomial below: the weighted least-squares fit of (asin(sqrt z) / sqrt z - 1) / z at 400 Chebyshev nodes,
//             coefficients rounded to binary32; |s + s z P(z) - asin s| <= 0.038 * 2^-24 on 400 001 points, coefficients as rounded.
//               a <= 0.5: z = x * x, t = fma(x * z, P, x), result RN(pi / 2) - t;
//               a >  0.5: z = (1 - a) * 0.5 (exact: Sterbenz, then a power of two), s = sqrt(z) <= 0.5, t = fma(s * z, P, s),
//                         r = 2 * t (exact); x > 0: r, else RN(pi) - r.  acos(1) = 0 and acos(-1) = RN(pi) exactly.
//             ERROR, absolute, in units of 2^-24.  t: its fma rounds once, t <= 0.5236: 0.5; the product s * z carries two
//             roundings and multiplies P <= 0.1875, the term is <= 0.0236: 0.047; P's four fma round by <= 2^-26 together, times
//             |s z| <= 0.125: 0.03; truncation 0.038: t within 0.62.  For a > 0.5 add sqrt's half ulp 2^-26 times asin' <= 1.1547:
//             0.289, and P read at z rather than RN(s)^2, 2^-23 relative: 0.054; t within 0.963, r within 1.93.  The last
//             subtraction rounds by <= 2^-23 (results in [2, pi]): 2; RN(pi / 2) is off by 0.733 and RN(pi) by 1.467.  So
//             |x| <= 0.5: 3.36; x > 0.5: 1.93; x < -0.5: 5.4.  BOUND 5.5 * 2^-24 (3.28e-7); measured maximum in DESIGN.md 9.
//   sinSoft(x), cosSoft(x), |x| <= 10 (the ambient occlusion pass, k_ambientocclusion.hip, forms |x| <= 3 pi; tests/gtao_ref.c restates
//             them word for word as gt_sin / gt_cos next to the derivation of the coefficients): !(|x| <= 10) (larger, infinite,
//             NaN) gives NaN.  k = rint(x * RN(2 / pi)); r = x - k * pi / 2 by three fma against 0x1.921p+0 + 0x1.f6ap-13 +
//             0x1.110b46p-26 (the first two with 11 low zero bits: their products with k are exact); z = r * r; on |r| < 0.8
//               sin r = fma(r * z, S(z), r), cos r = fma(z * z, C(z), fma(-0.5, z, 1)), S and C degree 2 in fma;
//             the quadrant (k, + 1 for the cosine) & 3 picks S, C, -S, -C.  BOUND 3 * 2^-24 absolute.
#pragma once

#include "cull_math.hip.h"

namespace softmath
{

__device__ __forceinline__ float log2Soft(float x)
{
#ifdef TR_POST_EXPERIMENT_HW_LOGEXP            // negative control only (profiles/postprocess/): the hardware's v_log_f32
    return __builtin_amdgcn_logf(x);
#else
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if (u == 0x7F800000u) return x;
    int bias = -127;
    if (u < 0x00800000u) { u = __builtin_bit_cast(uint32_t, x * 0x1p24f); bias = -151; }
    u += 0x3F800000u - 0x3F3504F3u;
    const int k = (int)(u >> 23) + bias;
    const float f = __builtin_bit_cast(float, (u & 0x007FFFFFu) + 0x3F3504F3u) - 1.0f;
    float p = -0x1.b84fe0p-4f;
    p = cm::fma_(p, f, 0x1.7a63c4p-3f);
    p = cm::fma_(p, f, -0x1.87f6aap-3f);
    p = cm::fma_(p, f, 0x1.a38c64p-3f);
    p = cm::fma_(p, f, -0x1.eab7a8p-3f);
    p = cm::fma_(p, f, 0x1.277a52p-2f);
    p = cm::fma_(p, f, -0x1.715a70p-2f);
    p = cm::fma_(p, f, 0x1.ec70aap-2f);
    p = cm::fma_(p, f, -0x1.715470p-1f);
    p = cm::fma_(p, f, 0x1.715476p+0f);
    return cm::fma_(f, p, (float)k);
#endif
}

__device__ __forceinline__ float exp2Signed(float x)
{
#ifdef TR_POST_EXPERIMENT_HW_LOGEXP            // negative control only (profiles/postprocess/): the hardware's v_exp_f32
    return __builtin_amdgcn_exp2f(x);
#else
    const float i = __builtin_rintf(x), f = x - i;
    float p = 0x1.44138ap-13f;
    p = cm::fma_(p, f, 0x1.5f0890p-10f);
    p = cm::fma_(p, f, 0x1.3b2a54p-7f);
    p = cm::fma_(p, f, 0x1.c6af6cp-5f);
    p = cm::fma_(p, f, 0x1.ebfbe0p-3f);
    p = cm::fma_(p, f, 0x1.62e430p-1f);
    p = cm::fma_(p, f, 1.0f);
    return __builtin_ldexpf(p, (int)cm::min_(cm::max_(i, -300.0f), 300.0f));
#endif
}

__device__ __forceinline__ float acosPoly(float z)
{
    float p = 0x1.665bcap-5f;
    p = cm::fma_(p, z, 0x1.7b4b14p-6f);
    p = cm::fma_(p, z, 0x1.766edcp-5f);
    p = cm::fma_(p, z, 0x1.32ea80p-4f);
    return cm::fma_(p, z, 0x1.555626p-3f);
}

__device__ __forceinline__ float acosSoft(float x)
{
    const float a = __builtin_fabsf(x);
    if (!(a <= 1.0f)) return __builtin_nanf("");
    if (a <= 0.5f) {
        const float z = x * x;
        return 0x1.921fb6p+0f - cm::fma_(x * z, acosPoly(z), x);
    }
    const float z = (1.0f - a) * 0.5f, s = cm::sqrt_(z);
    const float r = 2.0f * cm::fma_(s * z, acosPoly(z), s);
    return x > 0.0f ? r : 0x1.921fb6p+1f - r;
}

// quarter 0: sine, 1: cosine = sin(x + pi / 2)
__device__ __forceinline__ float sinCosSoft(float x, int quarter)
{
    if (!(__builtin_fabsf(x) <= 10.0f)) return __builtin_nanf("");
    const float k = __builtin_rintf(x * 0x1.45f306p-1f);
    float r = cm::fma_(-k, 0x1.921p+0f, x);
    r = cm::fma_(-k, 0x1.f6ap-13f, r);
    r = cm::fma_(-k, 0x1.110b46p-26f, r);
    const float z = r * r;
    const int q = ((int)k + quarter) & 3;
    float v;
    if (q & 1) {
        float p = 0x1.99bcaap-16f;
        p = cm::fma_(p, z, -0x1.6c0b94p-10f);
        p = cm::fma_(p, z, 0x1.55554ap-5f);
        v = cm::fma_(z * z, p, cm::fma_(-0.5f, z, 1.0f));
    } else {
        float p = -0x1.98896ep-13f;
        p = cm::fma_(p, z, 0x1.1104a6p-7f);
        p = cm::fma_(p, z, -0x1.55553cp-3f);
        v = cm::fma_(r * z, p, r);
    }
    return (q & 2) ? -v : v;
}
__device__ __forceinline__ float sinSoft(float x) { return sinCosSoft(x, 0); }
__device__ __forceinline__ float cosSoft(float x) { return sinCosSoft(x, 1); }

} // namespace softmath
