// material_textures.hip.h -- the texture table (the stand-in of ResourceDescriptorHeap[...]) and the software sampler of
// SampleMaterialValue (lightingcommon.hlsli:340-406), for the TEXTURED instantiation of the resolve (visibility_resolve.hip.h).
// Only the `Sample` branch with minMip = 0 is reachable from the base pass: no min-mip texture, no sampler feedback, no
// SampleLevel / SampleGrad overrides (they stay out with texture streaming).  The samplers are the reference's 16x
// anisotropic wrap and clamp samplers (CommonResources.cpp:292-293), selected by m_IsWrapSampler.
//
// CONVENTION (restated in tests/material_textures_ref.c).  For a texture of W x H texels at mip 0 and `mips` levels,
// level k of max(W >> k, 1) x max(H >> k, 1), sampled at uv with the derivatives ddx(uv), ddy(uv) (visibility_resolve.hip.h):
//   footprint : A = ddx(uv) * (W, H), B = ddy(uv) * (W, H) in mip-0 texels; |A| = sqrt(fma(A.y, A.y, A.x * A.x)); A is the major
//               axis iff |A| >= |B| (a NaN picks B); Pmax, Pmin = the major and the other length;
//   taps      : n = ceil(Pmax / Pmin), N = n <= 16 ? n : 16 (Pmin = 0 and NaN give 16): EXT_texture_filter_anisotropic's classic form;
//   lod       : x = Pmax / (float)N, lod = x > 0 ? log2Soft(x) : 0 (soft_math.hip.h), then fmin(fmax(lod, 0), mips - 1);
//               l0 = floor(lod), f = lod - l0, l1 = min(l0 + 1, mips - 1);
//   tap i     : at uv + major * (((float)i + 0.5f) / (float)N - 0.5f), major = the longer of ddx(uv), ddy(uv), not fused;
//               trilinear: b0 + f * (b1 - b0) of the bilinear values of levels l0 and l1, both always evaluated;
//   result    : (((0 + tap 0) + tap 1) + ...) / (float)N, summed in order;
//   bilinear  : k_bloom.hip's: tx = u * (float)w - 0.5f, x0 = floor(tx), fx = tx - x0, columns x0 and x0 + 1, rows alike,
//               lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy) with lerp(x, y, s) = x + s * (y - x);
//   addressing: clamp: each column as a float through fmin(fmax(., 0), w - 1) (a NaN gives column 0);
//               wrap : i = (int)fmin(fmax(x0, -2^30), 2^30), the column is i mod w floored, the next one that + 1, or 0 behind the last;
//   texel     : one 4-byte load, R in the low byte.  RGBA8_UNORM: (float)byte / 255.0f.  SRGBA8_UNORM: R, G, B through the device's
//               256-entry table (the sRGB transfer function evaluated in double precision on the host, rounded once to float),
//               before filtering, as D3D does; alpha stays linear (and is never read: GBufferA stores no alpha).
// Both tables (sRGB, and byte / 255.0f) are staged in LDS by the workgroup: a texel costs one global load and three LDS reads.
// Parity with D3D hardware's fixed-point, vendor-specific anisotropic filtering stays unpinned.
//
// ALPHA (sampleAlpha, alphaLevel0; restated in tests/alpha_test_ref.c): SampleMaterialValue(...).a for ALPHA_MASK_MODE's discard in
// the rasters (k_raster.hip) and the alpha test of the sun rays (k_shadowmask.hip).  sampleAlpha is `sample` on bits 24-31 of the
// texel: the same footprint, tap count, lod, tap positions, trilinear and bilinear arithmetic, addressing and summation order.  A
// texel is (float)byte / 255.0f, one correctly rounded division, in both formats: alpha is linear in SRGBA8_UNORM too and never goes
// through the sRGB table, so neither function needs the LDS tables.  alphaLevel0 is one bilinear fetch of mip 0.
#pragma once

#include "../../include/trhip.h"
#include "screen_pass.hip.h"
#include "soft_math.hip.h"

namespace mtex
{

// One entry of the device-side table (trhip_texture_table_t::entries, 96 bytes).  base == nullptr: an empty entry.
struct TableEntry
{
    const uint32_t* base;
    uint32_t width, height, mips, format;
    uint32_t mipOffset[16];                    // first texel of level k, in texels
    uint32_t pad[2];
};
static_assert(sizeof(TableEntry) == 96, "the host fills 96-byte entries");

constexpr uint32_t kLdsFloats = 512;           // [0, 256) sRGB -> linear, [256, 512) byte / 255.0f

// Every thread of a 256-thread workgroup, before any of them leaves.
__device__ __forceinline__ void stageTables(float* lds, const float* srgb, uint32_t tid)
{
    lds[tid] = srgb[tid];
    lds[256u + tid] = (float)tid / 255.0f;
    __syncthreads();
}

__device__ __forceinline__ bool sampled(const TableEntry& e) { return e.base && (e.format == TRHIP_FORMAT_RGBA8_UNORM || e.format == TRHIP_FORMAT_SRGBA8_UNORM); }

struct Axis { uint32_t i0, i1; float f; };

__device__ __forceinline__ Axis axisOf(float u, uint32_t dim, bool wrap)
{
    const float t = u * (float)dim - 0.5f, t0 = __builtin_floorf(t), f = t - t0;
    if (!wrap) {
        const float last = (float)(dim - 1u);
        return { (uint32_t)cm::min_(cm::max_(t0, 0.0f), last), (uint32_t)cm::min_(cm::max_(t0 + 1.0f, 0.0f), last), f };
    }
    const int i = (int)cm::min_(cm::max_(t0, -0x1p30f), 0x1p30f);
    int r;
    if ((dim & (dim - 1u)) == 0u) r = i & (int)(dim - 1u);                       // the floored modulo of a power of two
    else { r = i % (int)dim; if (r < 0) r += (int)dim; }
    return { (uint32_t)r, (uint32_t)r + 1u == dim ? 0u : (uint32_t)r + 1u, f };
}

using sp::lerp_;

// rgbTable: the LDS table the colour bytes go through (sRGB or UNORM)
__device__ __forceinline__ cm::F3 bilinear(const TableEntry& e, const float* rgbTable, uint32_t level, bool wrap, float u, float v)
{
    const uint32_t w = (e.width >> level) ? (e.width >> level) : 1u, h = (e.height >> level) ? (e.height >> level) : 1u;
    const Axis x = axisOf(u, w, wrap), y = axisOf(v, h, wrap);
    const uint32_t* p = e.base + e.mipOffset[level];
    const uint32_t w00 = p[y.i0 * w + x.i0], w10 = p[y.i0 * w + x.i1], w01 = p[y.i1 * w + x.i0], w11 = p[y.i1 * w + x.i1];
    cm::F3 o;
    o.x = lerp_(lerp_(rgbTable[w00 & 0xFFu], rgbTable[w10 & 0xFFu], x.f), lerp_(rgbTable[w01 & 0xFFu], rgbTable[w11 & 0xFFu], x.f), y.f);
    o.y = lerp_(lerp_(rgbTable[(w00 >> 8) & 0xFFu], rgbTable[(w10 >> 8) & 0xFFu], x.f), lerp_(rgbTable[(w01 >> 8) & 0xFFu], rgbTable[(w11 >> 8) & 0xFFu], x.f), y.f);
    o.z = lerp_(lerp_(rgbTable[(w00 >> 16) & 0xFFu], rgbTable[(w10 >> 16) & 0xFFu], x.f), lerp_(rgbTable[(w01 >> 16) & 0xFFu], rgbTable[(w11 >> 16) & 0xFFu], x.f), y.f);
    return o;
}

// SampleMaterialValue(...).rgb.  e: sampled(e); lds: stageTables' array.
__device__ __forceinline__ cm::F3 sample(const TableEntry& e, const float* lds, bool wrap, float u, float v, float dudx, float dvdx, float dudy, float dvdy)
{
    const float W = (float)e.width, H = (float)e.height;
    const float ax = dudx * W, ay = dvdx * H, bx = dudy * W, by = dvdy * H;
    const float lenA = cm::sqrt_(cm::fma_(ay, ay, ax * ax)), lenB = cm::sqrt_(cm::fma_(by, by, bx * bx));
    const bool aMajor = lenA >= lenB;
    const float pmax = aMajor ? lenA : lenB, pmin = aMajor ? lenB : lenA;
    const float mu = aMajor ? dudx : dudy, mv = aMajor ? dvdx : dvdy;
    const float n = __builtin_ceilf(pmax / pmin);
    const uint32_t N = n <= 16.0f ? (uint32_t)n : 16u;
    const float fN = (float)N, x = pmax / fN, top = (float)(e.mips - 1u);
    const float lod = cm::min_(cm::max_(x > 0.0f ? softmath::log2Soft(x) : 0.0f, 0.0f), top);
    const float l0f = __builtin_floorf(lod), f = lod - l0f;
    const uint32_t l0 = (uint32_t)l0f, l1 = l0 + 1u < e.mips ? l0 + 1u : e.mips - 1u;
    const float* rgbTable = lds + (e.format == TRHIP_FORMAT_SRGBA8_UNORM ? 0u : 256u);
    cm::F3 acc = { 0.0f, 0.0f, 0.0f };
#pragma unroll 1
    for (uint32_t i = 0; i < N; ++i) {
        const float k = ((float)i + 0.5f) / fN - 0.5f;
        const float tu = u + mu * k, tv = v + mv * k;
        const cm::F3 b0 = bilinear(e, rgbTable, l0, wrap, tu, tv), b1 = bilinear(e, rgbTable, l1, wrap, tu, tv);
        acc.x = acc.x + lerp_(b0.x, b1.x, f);
        acc.y = acc.y + lerp_(b0.y, b1.y, f);
        acc.z = acc.z + lerp_(b0.z, b1.z, f);
    }
    return { acc.x / fN, acc.y / fN, acc.z / fN };
}

// ---- the alpha channel (see ALPHA above) --------------------------------------------------------------------------------------
__device__ __forceinline__ float alphaOf(uint32_t texel) { return cm::div_((float)(texel >> 24), 255.0f); }

__device__ __forceinline__ float bilinearAlpha(const TableEntry& e, uint32_t level, bool wrap, float u, float v)
{
    const uint32_t w = (e.width >> level) ? (e.width >> level) : 1u, h = (e.height >> level) ? (e.height >> level) : 1u;
    const Axis x = axisOf(u, w, wrap), y = axisOf(v, h, wrap);
    const uint32_t* p = e.base + e.mipOffset[level];
    const uint32_t w00 = p[y.i0 * w + x.i0], w10 = p[y.i0 * w + x.i1], w01 = p[y.i1 * w + x.i0], w11 = p[y.i1 * w + x.i1];
    return lerp_(lerp_(alphaOf(w00), alphaOf(w10), x.f), lerp_(alphaOf(w01), alphaOf(w11), x.f), y.f);
}

// SampleMaterialValue(...).a.  e: sampled(e).  The lines of `sample` up to the loop, repeated: `sample` itself stays as it is.
__device__ __forceinline__ float sampleAlpha(const TableEntry& e, bool wrap, float u, float v, float dudx, float dvdx, float dudy, float dvdy)
{
    const float W = (float)e.width, H = (float)e.height;
    const float ax = dudx * W, ay = dvdx * H, bx = dudy * W, by = dvdy * H;
    const float lenA = cm::sqrt_(cm::fma_(ay, ay, ax * ax)), lenB = cm::sqrt_(cm::fma_(by, by, bx * bx));
    const bool aMajor = lenA >= lenB;
    const float pmax = aMajor ? lenA : lenB, pmin = aMajor ? lenB : lenA;
    const float mu = aMajor ? dudx : dudy, mv = aMajor ? dvdx : dvdy;
    const float n = __builtin_ceilf(pmax / pmin);
    const uint32_t N = n <= 16.0f ? (uint32_t)n : 16u;
    const float fN = (float)N, x = pmax / fN, top = (float)(e.mips - 1u);
    const float lod = cm::min_(cm::max_(x > 0.0f ? softmath::log2Soft(x) : 0.0f, 0.0f), top);
    const float l0f = __builtin_floorf(lod), f = lod - l0f;
    const uint32_t l0 = (uint32_t)l0f, l1 = l0 + 1u < e.mips ? l0 + 1u : e.mips - 1u;
    float acc = 0.0f;
#pragma unroll 1
    for (uint32_t i = 0; i < N; ++i) {
        const float k = ((float)i + 0.5f) / fN - 0.5f;
        const float tu = u + mu * k, tv = v + mv * k;
        acc = acc + lerp_(bilinearAlpha(e, l0, wrap, tu, tv), bilinearAlpha(e, l1, wrap, tu, tv), f);
    }
    return acc / fN;
}

// One bilinear fetch of mip 0: what a ray reads, which has no pixel quad to differentiate over (k_shadowmask.hip).
__device__ __forceinline__ float alphaLevel0(const TableEntry& e, bool wrap, float u, float v) { return bilinearAlpha(e, 0u, wrap, u, v); }

} // namespace mtex
