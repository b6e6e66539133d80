// r11g11b10.hip.h -- the store into TRHIP_FORMAT_R11G11B10_FLOAT (LightingOutput) and the load from it: R in bits 0-10, G in
// bits 11-21, B in bits 22-31; each channel an unsigned float with 5 exponent bits (bias 15) and 6, 6, 5 mantissa bits.  Host
// and device: the clear command (trhip_core.cpp) and the lighting kernels (k_deferredlighting.hip) store the same words; the
// passes behind LightingOutput (k_postprocess.hip) load them.
//
// CONVENTION (restated in tests/ref_formats.h), per channel: a NaN gives exponent and mantissa all ones;
// negative values and -0 give 0; +inf gives the infinity pattern; a finite value above the largest finite (65024 with 6
// mantissa bits, 64512 with 5) gives that largest finite; everything else rounds to nearest, ties to even, subnormals
// (below 2^-14) included.
// The load is exact (every value of the format is a binary32 number): exponent 0 gives mantissa * 2^(-14 - MBITS), subnormals
// included; exponent 31 gives +inf for mantissa 0 and otherwise a NaN that carries the mantissa in its top bits; everything
// else (1 + mantissa / 2^MBITS) * 2^(exponent - 15).  pack(unpack(c)) == c for every code (restated in tests/ref_formats.h).
#pragma once

#include <cstdint>

namespace trhip
{

template <uint32_t MBITS>
__host__ __device__ inline uint32_t packUFloat(float v)
{
    constexpr uint32_t kShift = 23u - MBITS, kInf = 31u << MBITS, kMaxFinite = kInf - 1u;
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return kInf | ((1u << MBITS) - 1u);       // NaN
    if (u >> 31) return 0u;                                                         // negative, -0
    if (u == 0x7F800000u) return kInf;
    if (u >= 0x38800000u) {                                                         // >= 2^-14: a normal number of the format
        const uint32_t r = u - (112u << 23);                                        // exponent rebiased 127 -> 15
        const uint32_t q = (r + ((1u << (kShift - 1)) - 1u) + ((r >> kShift) & 1u)) >> kShift;   // round to nearest even; a carry moves into the exponent
        return q < kMaxFinite ? q : kMaxFinite;
    }
    return (uint32_t)__builtin_rintf(v * (float)(1u << (14u + MBITS)));             // subnormal: units of 2^(-14 - MBITS), exact product; 2^MBITS is the smallest normal
}

__host__ __device__ inline uint32_t packR11G11B10(float r, float g, float b)
{
    return packUFloat<6>(r) | packUFloat<6>(g) << 11 | packUFloat<5>(b) << 22;
}

template <uint32_t MBITS>
__host__ __device__ inline float unpackUFloat(uint32_t c)
{
    const uint32_t e = c >> MBITS, m = c & ((1u << MBITS) - 1u);
    if (e == 0u) return (float)m * (1.0f / (float)(1u << (14u + MBITS)));           // a power of two: the product is exact
    return __builtin_bit_cast(float, (e == 31u ? 0x7F800000u : (e + 112u) << 23) | m << (23u - MBITS));
}

struct Rgb { float r, g, b; };
__host__ __device__ inline Rgb unpackR11G11B10(uint32_t w)
{
    return { unpackUFloat<6>(w & 0x7FFu), unpackUFloat<6>((w >> 11) & 0x7FFu), unpackUFloat<5>(w >> 22) };
}

} // namespace trhip
