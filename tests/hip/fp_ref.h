// fp_ref.h -- correctly rounded binary32 references for the arithmetic probes (tests/hip/cull_arith_probe.hip).
//
// Host and device: the probe library compiles it for gfx950 (the checks) and for the host (the CPU tests compare it
// with exact rational arithmetic).  Nothing here uses an fp32 division or square root.
//
// Method.  A candidate is taken from fp64 -- RN32(RN64(a / b)) or RN32(RN64(sqrt a)) -- and the rounding is then SETTLED
// exactly at the midpoints next to it, so the result does not depend on how the fp64 operation was lowered either:
//   * double rounding through binary64 is harmless for + - * / sqrt when 53 >= 2 * 24 + 2 (Figueroa, "When is double
//     rounding innocuous?", SIGNUM 1995), subnormal binary32 results included (they carry fewer than 24 bits); the
//     candidate is therefore already correct, and the settling step is a second, independent proof of it;
//   * a midpoint m between two adjacent binary32 values has at most 25 significant bits, so each sign below is exact:
//       sqrt(x):  sign(m * m - x)         m * m has <= 50 bits (exact in binary64), the fma rounds once
//       n / d:    sign(m * d - n)         m * d has <= 49 bits
//       1 / x:    sign(x * m - 1)         x * m has <= 49 bits
//       rsqrt(x): sign(x * (m * m) - 1)   m * m has <= 50 bits and is exact, the fma rounds once
//     A once-rounded value is zero only when the exact one is (no product here leaves binary64's normal range), so the
//     sign of the fma is the sign of the exact difference.  A tie (exactly on a midpoint) goes to the even neighbour.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FR_HD __host__ __device__ inline
#else
#include <math.h>
#define FR_HD inline
#endif

namespace fr
{

constexpr uint32_t kNaN = 0x7FC00000u;
constexpr uint32_t kInf = 0x7F800000u;
constexpr uint32_t kSign = 0x80000000u;

FR_HD uint32_t bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
FR_HD float flt(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
FR_HD bool isNaN(uint32_t u) { return (u & 0x7FFFFFFFu) > kInf; }

// value of a non-negative pattern; the pattern of +inf stands for 2^128, the first value past FLT_MAX at its spacing
FR_HD double val(uint32_t u) { return u == kInf ? 0x1p128 : (double)flt(u); }

// sgn(m) = sign(m - t) for the exact positive real t; c = a candidate pattern within a few ulp of RN(t)
template <class S>
FR_HD uint32_t settle(uint32_t c, S sgn)
{
    for (int it = 0; it < 4; ++it) {
        if (c < kInf) {
            const int s = sgn(0.5 * (val(c) + val(c + 1u)));
            if (s < 0 || (s == 0 && ((c + 1u) & 1u) == 0u)) { ++c; continue; }
        }
        if (c > 0u) {
            const int s = sgn(0.5 * (val(c - 1u) + val(c)));
            if (s > 0 || (s == 0 && ((c - 1u) & 1u) == 0u)) { --c; continue; }
        }
        break;
    }
    return c;
}

FR_HD int sign(double e) { return (e > 0.0) - (e < 0.0); }

// RN(sqrt(x)); NaN for x < 0 and NaN, sqrt(-0) = -0
FR_HD uint32_t sqrtRN(uint32_t x)
{
    if (isNaN(x)) return kNaN;
    if ((x & 0x7FFFFFFFu) == 0u) return x;
    if (x & kSign) return kNaN;
    if (x == kInf) return kInf;
    const double X = (double)flt(x);
    return settle(bits((float)sqrt(X)), [X](double m) { return sign(fma(m, m, -X)); });
}

// RN(n / d) with IEEE special cases
FR_HD uint32_t divRN(uint32_t n, uint32_t d)
{
    if (isNaN(n) || isNaN(d)) return kNaN;
    const uint32_t s = (n ^ d) & kSign, an = n & 0x7FFFFFFFu, ad = d & 0x7FFFFFFFu;
    if ((an == 0u && ad == 0u) || (an == kInf && ad == kInf)) return kNaN;
    if (an == kInf || ad == 0u) return s | kInf;
    if (an == 0u || ad == kInf) return s;
    const double N = (double)flt(an), D = (double)flt(ad);
    return s | settle(bits((float)(N / D)), [N, D](double m) { return sign(fma(m, D, -N)); });
}

// RN(1 / x)
FR_HD uint32_t rcpRN(uint32_t x)
{
    if (isNaN(x)) return kNaN;
    const uint32_t s = x & kSign, a = x & 0x7FFFFFFFu;
    if (a == 0u) return s | kInf;
    if (a == kInf) return s;
    const double X = (double)flt(a);
    return s | settle(bits((float)(1.0 / X)), [X](double m) { return sign(fma(X, m, -1.0)); });
}

// RN(1 / sqrt(x)); NaN for x < 0 and NaN, rsqrt(+-0) = +-inf
FR_HD uint32_t rsqRN(uint32_t x)
{
    if (isNaN(x)) return kNaN;
    if ((x & 0x7FFFFFFFu) == 0u) return (x & kSign) | kInf;
    if (x & kSign) return kNaN;
    if (x == kInf) return 0u;
    const double X = (double)flt(x);
    return settle(bits((float)(1.0 / sqrt(X))), [X](double m) { return sign(fma(X, m * m, -1.0)); });
}

// distance in representable values (ulps) of two non-NaN patterns; +0 and -0 are one apart
FR_HD uint64_t ulpDist(uint32_t a, uint32_t b)
{
    const int64_t oa = (a & kSign) ? -(int64_t)(a & 0x7FFFFFFFu) - 1 : (int64_t)a;
    const int64_t ob = (b & kSign) ? -(int64_t)(b & 0x7FFFFFFFu) - 1 : (int64_t)b;
    return (uint64_t)(oa > ob ? oa - ob : ob - oa);
}

// a result equals the reference: NaN as NaN (any payload), everything else bit for bit (signs of zero and infinity included)
FR_HD bool same(uint32_t got, uint32_t ref) { return isNaN(ref) ? isNaN(got) : got == ref; }

// floor(log2(x)) of a finite x >= 1, settled with exact powers of two
FR_HD int floorLog2(uint32_t x)
{
    const double X = (double)flt(x);
    int e = (int)floor(log2(X));
    if (ldexp(1.0, e) > X) --e;
    if (ldexp(1.0, e + 1) <= X) ++e;
    return e;
}

} // namespace fr
