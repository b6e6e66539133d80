// soft_math.hip.h -- log2 and a two-sided exp2 in software, for the passes behind LightingOutput (k_postprocess.hip).
// v_log_f32 and v_exp_f32 are good to 1 ulp only and cannot be restated on a CPU; these can, and tests/postprocess_ref.c
// restates them word for word (pr_log2, pr_exp2) next to the derivation of the coefficients and of the error bounds.  The
// lighting pass keeps its own exp2Soft (k_deferredlighting.hip): that one is proven for x <= 0 only and its words must not move.
//
//   log2Soft(x), x > 0 (the callers test; +inf gives +inf): a subnormal x is first scaled by 2^24 (exact).  The bits are split
//             at sqrt(1/2): k = exponent, m in [0x1.6a09e6p-1, 0x1.6a09e6p+0), f = m - 1 (exact, Sterbenz), P the degree-9 Horner
//             polynomial below in fma, result fma(f, P, (float)k).  |error| <= 1.45 * 2^-25 + 2^-24 * |result|.
//   exp2Signed(x), any sign: i = rint(x), f = x - i in [-0.5, 0.5], exact on both sides of 0 (|x| < 0.5: i = 0 and f = x;
//             otherwise i != 0, x and i are multiples of ulp(x) and |f| <= 0.5 <= |x|, so f is a multiple of ulp(x) no larger
//             than x: representable).  p = the degree-6 Horner polynomial in fma, in [0x1.6a09e6p-1, 0x1.6a09e8p+0]; result
//             ldexp(p, clamp(i, -300, 300)) (exact unless subnormal; the clamp makes NaN and huge arguments defined: NaN gives
//             NaN, +inf gives NaN (inf - inf), -inf likewise).  |error| <= 2.9 * 2^-25 * 2^i.
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

} // namespace softmath
