// material_textures.hip.h -- the texture table (the stand-in of ResourceDescriptorHeap[...]) and the software sampler of
// SampleMaterialValue (lightingcommon.hlsli:340-406), for the TEXTURED instantiation of the resolve (visibility_resolve.hip.h).
// `sample` is the `Sample` branch with minMip = 0; `sampleStreamed` (below, "texture streaming") adds the min-mip clamp and the feedback
// marks for the STREAMED instantiation.  No SampleLevel / SampleGrad overrides.  The samplers are the reference's 16x
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
//   texel     : one 4-byte word, R in the low byte (the fetch: one load per texel of RGBA8_UNORM / SRGBA8_UNORM, the decode below for
//               the block-compressed formats).  UNORM: (float)byte / 255.0f.  SRGBA8_UNORM and the _SRGB block formats: R, G, B
//               through the device's 256-entry table (the sRGB transfer function evaluated in double precision on the host, rounded
//               once to float), before filtering, as D3D does; alpha stays linear (and is never read: GBufferA stores no alpha).
// Both tables (sRGB, and byte / 255.0f) are staged in LDS by the workgroup: a texel costs one global load and three LDS reads.
//
// BLOCK-COMPRESSED FORMATS (BC1, BC2, BC3, their _SRGB variants, BC4, BC5; restated in tests/bc_ref.c).  A BC texture
// samples exactly as the RGBA8_UNORM (or SRGBA8_UNORM) texture of its decoded words would: nothing above changes.  Level k is
// ceil(w_k / 4) x ceil(h_k / 4) blocks, row-major, from mipOffset[k]; texel (x, y) is texel i = 4 * (y & 3) + (x & 3) of block
// (x >> 2, y >> 2).  A texel costs one aligned 8- or 16-byte load of its block (shared by the texels of the footprint that lie in
// the same block) and the decode of that one texel; texels of an edge block beyond the level are never addressed.  The decode is
// integer, every division truncates, all fields are little-endian:
//   colour block (8 bytes): c0, c1 RGB565 at bytes 0-1 and 2-3, texel i's index at bits 2i of bytes 4-7; endpoints to 8 bits by bit
//               replication (r5 << 3 | r5 >> 2, g6 << 2 | g6 >> 4); four-colour mode: p2 = (2 p0 + p1) / 3, p3 = (p0 + 2 p1) / 3,
//               alpha 255; three-colour mode: p2 = (p0 + p1) / 2, p3 = (0, 0, 0, 0).  BC1: four-colour iff c0 > c1; BC2, BC3: always.
//   alpha block (8 bytes; BC3's alpha, BC4, each half of BC5): a0, a1, texel i's index at bits 3i of the 48 bits that follow;
//               a0 > a1: p[k] = ((8 - k) a0 + (k - 1) a1) / 7, k = 2..7; else p[k] = ((6 - k) a0 + (k - 1) a1) / 5, k = 2..5, p6 = 0, p7 = 255.
//   BC2: bytes 0-7 sixteen 4-bit alphas (texel i at bits 4i, times 17), then the colour block.  BC3: alpha block, colour block.
//   BC4: (R, 0, 0, 255).  BC5: the R block, the G block: (R, G, 0, 255).
// The format branch sits inside the fetch (fetchQuad, fetchQuads): lanes of one wave hold entries of different formats.
// Parity with D3D hardware's fixed-point, vendor-specific anisotropic filtering stays unpinned.
//
// ALPHA (sampleAlpha, alphaLevel0; restated in tests/alpha_test_ref.c): SampleMaterialValue(...).a for ALPHA_MASK_MODE's discard in
// the rasters (k_raster.hip) and the alpha test of the sun rays (k_shadowmask.hip).  sampleAlpha is `sample` on bits 24-31 of the
// texel: the same footprint, tap count, lod, tap positions, trilinear and bilinear arithmetic, addressing and summation order.  A
// texel is (float)byte / 255.0f, one correctly rounded division, in every format: alpha is linear in SRGBA8_UNORM and the _SRGB block
// formats too and never goes through the sRGB table, so neither function needs the LDS tables.  The texels come from the same fetchQuad.  alphaLevel0 is one bilinear fetch of mip 0.
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
    uint32_t mipOffset[16];                    // first texel (or block) of level k, in 4-byte words from base
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

__device__ __forceinline__ bool blockCompressed(uint32_t format) { return format >= TRHIP_FORMAT_BC1_UNORM && format <= TRHIP_FORMAT_BC5_UNORM; }
__device__ __forceinline__ bool srgbDecoded(uint32_t format)
{
    return format == TRHIP_FORMAT_SRGBA8_UNORM || format == TRHIP_FORMAT_BC1_UNORM_SRGB || format == TRHIP_FORMAT_BC2_UNORM_SRGB || format == TRHIP_FORMAT_BC3_UNORM_SRGB;
}
__device__ __forceinline__ bool sampled(const TableEntry& e)
{
    return e.base && (e.format == TRHIP_FORMAT_RGBA8_UNORM || e.format == TRHIP_FORMAT_SRGBA8_UNORM || blockCompressed(e.format));
}

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

// ---- the texel fetch (see BLOCK-COMPRESSED FORMATS above) --------------------------------------------------------------------
// One block in four words.  An 8-byte block is held twice, so that a colour block is always w[2], w[3] and the first (or only)
// alpha block always w[0], w[1].
struct Block { uint32_t w[4]; };

__device__ __forceinline__ Block loadBlock(const uint32_t* level, uint32_t index, bool wide)
{
    if (wide) {
        const uint4 v = *(const uint4*)(level + 4u * index);
        return { { v.x, v.y, v.z, v.w } };
    }
    const uint2 v = *(const uint2*)(level + 2u * index);
    return { { v.x, v.y, v.x, v.y } };
}

// texel i of a colour block: R, G, B in bits 0-23, alpha 255 or (three-colour mode, index 3) 0 in bits 24-31
__device__ __forceinline__ uint32_t colourTexel(uint32_t ends, uint32_t indices, uint32_t i, bool bc1)
{
    const uint32_t c0 = ends & 0xFFFFu, c1 = ends >> 16, k = (indices >> (2u * i)) & 3u;
    const bool four = !bc1 || c0 > c1;
    const uint32_t r0 = c0 >> 11, g0 = (c0 >> 5) & 63u, b0 = c0 & 31u, r1 = c1 >> 11, g1 = (c1 >> 5) & 63u, b1 = c1 & 31u;
    auto mix = [&](uint32_t p0, uint32_t p1) {
        return k == 0u ? p0 : k == 1u ? p1 : four ? (k == 2u ? (2u * p0 + p1) / 3u : (p0 + 2u * p1) / 3u) : (k == 2u ? (p0 + p1) / 2u : 0u);
    };
    const uint32_t r = mix(r0 << 3 | r0 >> 2, r1 << 3 | r1 >> 2), g = mix(g0 << 2 | g0 >> 4, g1 << 2 | g1 >> 4), b = mix(b0 << 3 | b0 >> 2, b1 << 3 | b1 >> 2);
    return r | g << 8 | b << 16 | (!four && k == 3u ? 0u : 0xFF000000u);
}

// texel i of an alpha block (lo: bytes 0-3, hi: bytes 4-7)
__device__ __forceinline__ uint32_t alphaTexel(uint32_t lo, uint32_t hi, uint32_t i)
{
    const uint32_t a0 = lo & 0xFFu, a1 = (lo >> 8) & 0xFFu;
    const uint32_t k = (uint32_t)((((uint64_t)hi << 32 | lo) >> 16) >> (3u * i)) & 7u;
    const uint32_t eight = ((8u - k) * a0 + (k - 1u) * a1) / 7u, six = k == 6u ? 0u : k == 7u ? 255u : ((6u - k) * a0 + (k - 1u) * a1) / 5u;
    return k == 0u ? a0 : k == 1u ? a1 : a0 > a1 ? eight : six;
}

// the RGBA8 word of texel i of a block of `format`
__device__ __forceinline__ uint32_t decodeTexel(uint32_t format, const Block& b, uint32_t i)
{
    if (format <= TRHIP_FORMAT_BC3_UNORM_SRGB) {
        const uint32_t c = colourTexel(b.w[2], b.w[3], i, format <= TRHIP_FORMAT_BC1_UNORM_SRGB);
        if (format <= TRHIP_FORMAT_BC1_UNORM_SRGB) return c;
        const uint32_t a = format <= TRHIP_FORMAT_BC2_UNORM_SRGB ? ((uint32_t)(((uint64_t)b.w[1] << 32 | b.w[0]) >> (4u * i)) & 15u) * 17u : alphaTexel(b.w[0], b.w[1], i);
        return (c & 0xFFFFFFu) | a << 24;
    }
    const uint32_t g = format == TRHIP_FORMAT_BC5_UNORM ? alphaTexel(b.w[2], b.w[3], i) : 0u;
    return alphaTexel(b.w[0], b.w[1], i) | g << 8 | 0xFF000000u;
}

// The four RGBA8 words of a bilinear footprint, and where it lies: columns and rows of a level w texels wide.
struct Quad { uint32_t w00, w10, w01, w11; };
struct Footprint { uint32_t level, w; Axis x, y; };

__device__ __forceinline__ Footprint footprintOf(const TableEntry& e, uint32_t level, bool wrap, float u, float v)
{
    const uint32_t w = (e.width >> level) ? (e.width >> level) : 1u, h = (e.height >> level) ? (e.height >> level) : 1u;
    return { level, w, axisOf(u, w, wrap), axisOf(v, h, wrap) };
}

__device__ __forceinline__ Quad plainQuad(const TableEntry& e, const Footprint& f)
{
    const uint32_t* p = e.base + e.mipOffset[f.level];
    return { p[f.y.i0 * f.w + f.x.i0], p[f.y.i0 * f.w + f.x.i1], p[f.y.i1 * f.w + f.x.i0], p[f.y.i1 * f.w + f.x.i1] };
}

__device__ __forceinline__ Quad blockQuad(const TableEntry& e, const Footprint& f)
{
    const uint32_t* p = e.base + e.mipOffset[f.level];
    const uint32_t format = e.format, w = f.w;
    const Axis &x = f.x, &y = f.y;
    const bool wide = format != TRHIP_FORMAT_BC1_UNORM && format != TRHIP_FORMAT_BC1_UNORM_SRGB && format != TRHIP_FORMAT_BC4_UNORM;
    const uint32_t bw = (w + 3u) >> 2;
    const uint32_t bx0 = x.i0 >> 2, bx1 = x.i1 >> 2, row0 = (y.i0 >> 2) * bw, row1 = (y.i1 >> 2) * bw;
    const uint32_t tx0 = x.i0 & 3u, tx1 = x.i1 & 3u, ty0 = 4u * (y.i0 & 3u), ty1 = 4u * (y.i1 & 3u);
    Quad q;
    Block left = loadBlock(p, row0 + bx0, wide), right = left;
    if (bx1 != bx0) right = loadBlock(p, row0 + bx1, wide);
    q.w00 = decodeTexel(format, left, ty0 + tx0);
    q.w10 = decodeTexel(format, right, ty0 + tx1);
    if (row1 != row0) {
        left = loadBlock(p, row1 + bx0, wide);
        right = left;
        if (bx1 != bx0) right = loadBlock(p, row1 + bx1, wide);
    }
    q.w01 = decodeTexel(format, left, ty1 + tx0);
    q.w11 = decodeTexel(format, right, ty1 + tx1);
    return q;
}

// THE TEXEL FETCH, for every sampled format, which bilinear and bilinearAlpha share: the words of one footprint, or of the two
// footprints of a trilinear tap under one format branch, so that the eight loads of an RGBA8 tap are issued together as before.
// `blocks`: blockCompressed(e.format), which a caller with a tap loop evaluates once.  The block path is laid out of line.
__device__ __forceinline__ Quad fetchQuad(const TableEntry& e, bool blocks, const Footprint& f)
{
    if (__builtin_expect(blocks, 0)) return blockQuad(e, f);
    return plainQuad(e, f);
}

__device__ __forceinline__ void fetchQuads(const TableEntry& e, bool blocks, const Footprint& f0, const Footprint& f1, Quad& q0, Quad& q1)
{
    if (__builtin_expect(blocks, 0)) { q0 = blockQuad(e, f0); q1 = blockQuad(e, f1); }
    else { q0 = plainQuad(e, f0); q1 = plainQuad(e, f1); }
}

// rgbTable: the LDS table the colour bytes go through (sRGB or UNORM)
__device__ __forceinline__ cm::F3 bilinear(const Quad& q, const Footprint& fp, const float* rgbTable)
{
    const Axis &x = fp.x, &y = fp.y;
    const uint32_t w00 = q.w00, w10 = q.w10, w01 = q.w01, w11 = q.w11;
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
    const float* rgbTable = lds + (srgbDecoded(e.format) ? 0u : 256u);
    const bool blocks = blockCompressed(e.format);
    cm::F3 acc = { 0.0f, 0.0f, 0.0f };
#pragma unroll 1
    for (uint32_t i = 0; i < N; ++i) {
        const float k = ((float)i + 0.5f) / fN - 0.5f;
        const float tu = u + mu * k, tv = v + mv * k;
        const Footprint f0 = footprintOf(e, l0, wrap, tu, tv), f1 = footprintOf(e, l1, wrap, tu, tv);
        Quad q0, q1;
        fetchQuads(e, blocks, f0, f1, q0, q1);
        const cm::F3 b0 = bilinear(q0, f0, rgbTable), b1 = bilinear(q1, f1, rgbTable);
        acc.x = acc.x + lerp_(b0.x, b1.x, f);
        acc.y = acc.y + lerp_(b0.y, b1.y, f);
        acc.z = acc.z + lerp_(b0.z, b1.z, f);
    }
    return { acc.x / fN, acc.y / fN, acc.z / fN };
}

// ---- texture streaming: the min-mip clamp and the feedback marks (the STREAMED instantiation of the resolve) -----------------------
// CONVENTION (restated in tests/texture_streaming_ref.c).  A streamable texture has a region of 2^sx x 2^sy texels of
// mip 0 (TableEntry::pad); region (rx, ry) is word or byte ry * (W >> sx) + rx of a map.
//   point     : the mip-0 texel under u on an axis of `dim` texels: t0 = floor(u * (float)dim); clamp: (uint)fmin(fmax(t0, 0), dim - 1)
//               (a NaN gives 0); wrap: (int)fmin(fmax(t0, -2^30), 2^30) mod dim, floored.  The region under uv is (point(u) >> sx,
//               point(v) >> sy): PointWrap / PointClampMaxReductionSampler on a map of one texel per region.
//   clamp     : with lodWanted = `sample`'s clamped lod and minMip the byte of the region under uv, lod = fmin(fmax(lodWanted,
//               (float)minMip), mips - 1); l0, l1 and f come from this lod; N and the tap positions are `sample`'s (they come from the
//               footprint).  Without a map lod = lodWanted: `sample` itself.
//   feedback  : (WriteSamplerFeedback; the project's own statement, D3D's is implementation-defined.)  l0w = floor(lodWanted), l1w =
//               min(l0w + 1, mips - 1).  The region under uv is marked with l0w.  For every tap, each of the four texels (columns i0,
//               i1 x rows i0, i1) of the level-l0w footprint marks the region of its mip-0 origin, ((x << l0w) >> sx, (y << l0w) >> sy),
//               with l0w, and each of the four of the level-l1w footprint marks its region with l1w.  A mark is word = min(word, level).
//               The footprints are those of the UNCLAMPED levels: feedback does not depend on residency.  No texel is fetched for it.
// THE WRITE.  Marking as stated is up to 1 + 16 x 8 atomics per sample, nearly all of them to one or two words, from 64 lanes that
// mostly look at the same regions.  min is idempotent and order-independent, so marks may be dropped and merged freely: a lane drops
// a mark that repeats a region of the same footprint or that its last mark already covers (same word, level not lower); what is left
// is merged across the wave before the atomic goes out: the first lane still to be served issues the one atomic for all the lanes that
// hold its (word, level), until no lane is left: one atomic per wave and distinct (word, level).  -DTRHIP_FEEDBACK_NAIVE builds the per-mark atomic, for tools/texture_streaming_cost.py.
// Negative controls (profiles/gbuffer/streaming_mutations.txt): eleven -D builds that each break one rule of the clamp, of the marks or
// of the write (TR_STREAM_MUTATE_*) fail tests/test_gpu_texture_streaming_rules.py.  Each changes a value or a choice between in-range
// indices only: a mark that is left out, a level between 0 and mips - 1, a texel of the level's own footprint, an origin that is NOT
// shifted up (so never beyond the shifted one).  None touches a loop bound, a barrier, an early return or an index beyond a map, and
// the merge loop of emitMark still ends under MERGE_BY_WORD, because the leader always matches itself.
struct Stream
{
    const uint8_t* minMip;                     // the slot's min-mip map, or nullptr
    uint32_t* feedback;                        // the slot's feedback map when feedback is written, or nullptr
    uint32_t shiftX, shiftY, regionsX;
};

__device__ __forceinline__ uint32_t pointOf(float u, uint32_t dim, bool wrap)
{
#ifdef TR_STREAM_MUTATE_UNDER_ROUNDS            // negative control only: the nearest texel boundary, not the texel under u (clamped or wrapped below as before)
    const float t0 = __builtin_floorf(u * (float)dim + 0.5f);
#else
    const float t0 = __builtin_floorf(u * (float)dim);
#endif
    if (!wrap) return (uint32_t)cm::min_(cm::max_(t0, 0.0f), (float)(dim - 1u));
    const int i = (int)cm::min_(cm::max_(t0, -0x1p30f), 0x1p30f);
    int r;
    if ((dim & (dim - 1u)) == 0u) r = i & (int)(dim - 1u);
    else { r = i % (int)dim; if (r < 0) r += (int)dim; }
    return (uint32_t)r;
}

__device__ __forceinline__ uint32_t regionUnder(const TableEntry& e, const Stream& st, bool wrap, float u, float v)
{
    return (pointOf(v, e.height, wrap) >> st.shiftY) * st.regionsX + (pointOf(u, e.width, wrap) >> st.shiftX);
}

// one atomic per distinct (word, level) among the lanes that call it together
__device__ __forceinline__ void emitMark(uint32_t* words, uint32_t index, uint32_t level)
{
#ifdef TRHIP_FEEDBACK_NAIVE
    atomicMin(words + index, level);
#else
    // A loop over a wave-uniform mask of the lanes still to be served, which every calling lane runs to its end: the loop that each
    // lane leaves as soon as it matches the first active lane is folded by the compiler into "the first lane alone" (seen in the
    // assembly), which loses marks.
    uint32_t* p = words + index;
    const uint32_t lo = (uint32_t)(uintptr_t)p, hi = (uint32_t)((uintptr_t)p >> 32), lane = __lane_id();
    uint64_t todo = __builtin_amdgcn_ballot_w64(true);
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
#ifdef TR_STREAM_MUTATE_MERGE_BY_WORD           // negative control only: the leader's level goes out for every lane on its word
        const bool same = (lo == (uint32_t)__builtin_amdgcn_readlane((int)lo, (int)leader)) & (hi == (uint32_t)__builtin_amdgcn_readlane((int)hi, (int)leader));
#else
        const bool same = (lo == (uint32_t)__builtin_amdgcn_readlane((int)lo, (int)leader)) & (hi == (uint32_t)__builtin_amdgcn_readlane((int)hi, (int)leader)) &
                          (level == (uint32_t)__builtin_amdgcn_readlane((int)level, (int)leader));
#endif
        if (lane == leader) atomicMin(p, level);
        todo &= ~__builtin_amdgcn_ballot_w64(same);
    }
#endif
}

struct Marker
{
    uint32_t* words; uint32_t lastIndex, lastLevel;
    __device__ __forceinline__ void mark(uint32_t index, uint32_t level)
    {
#if defined(TR_STREAM_MUTATE_DROP_BY_INDEX)     // negative control only: a lower level that follows a higher one to the same word is dropped
        if (index == lastIndex) return;
#elif !defined(TRHIP_FEEDBACK_NAIVE)
        if (index == lastIndex && level >= lastLevel) return;                           // the last mark covers it
#endif
        emitMark(words, index, level);
        lastIndex = index; lastLevel = level;
    }
    // the four texels of a footprint of level f.level
    __device__ __forceinline__ void markFootprint(const Stream& st, const Footprint& f)
    {
#ifdef TR_STREAM_MUTATE_NO_ORIGIN_SHIFT         // negative control only: the level texel's own index, never beyond its mip-0 origin
        const uint32_t up = 0u;
#else
        const uint32_t up = f.level;
#endif
        const uint32_t rx0 = (f.x.i0 << up) >> st.shiftX, rx1 = (f.x.i1 << up) >> st.shiftX;
        const uint32_t r0 = ((f.y.i0 << up) >> st.shiftY) * st.regionsX, r1 = ((f.y.i1 << up) >> st.shiftY) * st.regionsX;
#if defined(TR_STREAM_MUTATE_ONE_TEXEL)         // negative control only: texel (i0, i0) marks alone
        mark(r0 + rx0, f.level);
#elif defined(TRHIP_FEEDBACK_NAIVE)
        mark(r0 + rx0, f.level); mark(r0 + rx1, f.level); mark(r1 + rx0, f.level); mark(r1 + rx1, f.level);
#else
        mark(r0 + rx0, f.level);
        if (rx1 != rx0) mark(r0 + rx1, f.level);
        if (r1 != r0) {
            mark(r1 + rx0, f.level);
            if (rx1 != rx0) mark(r1 + rx1, f.level);
        }
#endif
    }
};

// SampleMaterialValue(...).rgb with a min-mip map and / or a feedback map.  minMipOut: the byte read (0 without a map).
__device__ __forceinline__ cm::F3 sampleStreamed(const TableEntry& e, const Stream& st, const float* lds, bool wrap, float u, float v, float dudx, float dvdx, float dudy, float dvdy,
                                                 uint32_t& minMipOut)
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
    const float lodWanted = cm::min_(cm::max_(x > 0.0f ? softmath::log2Soft(x) : 0.0f, 0.0f), top);
    const bool mapped = st.minMip || st.feedback;
    const uint32_t under = mapped ? regionUnder(e, st, wrap, u, v) : 0u;
    const uint32_t minMip = st.minMip ? st.minMip[under] : 0u;
    minMipOut = minMip;
#ifdef TR_STREAM_MUTATE_CLAMP_REPLACES          // negative control only: a min-mip byte that is not 0 replaces the lod instead of bounding it
    const float lod = cm::min_(minMip != 0u ? (float)minMip : lodWanted, top);
#else
    const float lod = cm::min_(cm::max_(lodWanted, (float)minMip), top);
#endif
    const float l0f = __builtin_floorf(lod), f = lod - l0f;
    const uint32_t l0 = (uint32_t)l0f, l1 = l0 + 1u < e.mips ? l0 + 1u : e.mips - 1u;
#ifdef TR_STREAM_MUTATE_CLAMPED_LEVELS          // negative control only: the footprints of the clamped levels are marked
    const uint32_t l0w = (uint32_t)__builtin_floorf(lodWanted), m0 = l0, m1 = l1;
#else
    const uint32_t l0w = (uint32_t)__builtin_floorf(lodWanted), l1w = l0w + 1u < e.mips ? l0w + 1u : e.mips - 1u, m0 = l0w, m1 = l1w;
#endif
    Marker marker = { st.feedback, 0xFFFFFFFFu, 0u };
#ifndef TR_STREAM_MUTATE_NO_UNDER               // negative control only: no mark of the region under uv
    if (st.feedback) marker.mark(under, l0w);
#endif
    const float* rgbTable = lds + (srgbDecoded(e.format) ? 0u : 256u);
    const bool blocks = blockCompressed(e.format);
    cm::F3 acc = { 0.0f, 0.0f, 0.0f };
#pragma unroll 1
    for (uint32_t i = 0; i < N; ++i) {
        const float k = ((float)i + 0.5f) / fN - 0.5f;
        const float tu = u + mu * k, tv = v + mv * k;
        const Footprint f0 = footprintOf(e, l0, wrap, tu, tv), f1 = footprintOf(e, l1, wrap, tu, tv);
        Quad q0, q1;
        fetchQuads(e, blocks, f0, f1, q0, q1);
        if (st.feedback) {                                                              // address arithmetic only, while the texels are in flight
#ifdef TR_STREAM_MUTATE_CENTRE_FOOTPRINT        // negative control only: every tap marks the footprints at uv itself
            marker.markFootprint(st, footprintOf(e, m0, wrap, u, v));
            marker.markFootprint(st, footprintOf(e, m1, wrap, u, v));
#else
#ifndef TR_STREAM_MUTATE_NO_L0W_FOOTPRINT       // negative control only: no marks of the level-l0w footprint
            marker.markFootprint(st, m0 == l0 ? f0 : footprintOf(e, m0, wrap, tu, tv));
#endif
#ifndef TR_STREAM_MUTATE_NO_L1W                 // negative control only: no marks of the level-l1w footprint
            marker.markFootprint(st, m1 == l1 ? f1 : m1 == l0 ? f0 : footprintOf(e, m1, wrap, tu, tv));
#endif
#endif
        }
        const cm::F3 b0 = bilinear(q0, f0, rgbTable), b1 = bilinear(q1, f1, rgbTable);
        acc.x = acc.x + lerp_(b0.x, b1.x, f);
        acc.y = acc.y + lerp_(b0.y, b1.y, f);
        acc.z = acc.z + lerp_(b0.z, b1.z, f);
    }
    return { acc.x / fN, acc.y / fN, acc.z / fN };
}

// kMipColors (toyrenderer_common.hlsli:9-28): albedo of m_bVisualizeMinMipTilesOnAlbedoOutput, by min(minMip, 15)
__device__ __forceinline__ cm::F3 mipColour(uint32_t minMip)
{
    static constexpr float c[16][3] = { { 1.0f, 1.0f, 1.0f }, { 1.0f, 0.25f, 0.25f }, { 0.25f, 1.0f, 0.25f }, { 0.25f, 0.25f, 1.0f }, { 1.0f, 0.25f, 1.0f }, { 1.0f, 1.0f, 0.25f },
                                        { 0.25f, 1.0f, 1.0f }, { 0.9f, 0.5f, 0.2f }, { 0.59f, 0.48f, 0.8f }, { 0.53f, 0.25f, 0.11f }, { 0.8f, 0.48f, 0.53f }, { 0.64f, 0.8f, 0.48f },
                                        { 0.48f, 0.75f, 0.8f }, { 0.5f, 0.25f, 0.75f }, { 0.99f, 0.68f, 0.42f }, { 0.4f, 0.5f, 0.6f } };
    const uint32_t i = minMip < 15u ? minMip : 15u;
    return { c[i][0], c[i][1], c[i][2] };
}

// ---- the alpha channel (see ALPHA above) --------------------------------------------------------------------------------------
__device__ __forceinline__ float alphaOf(uint32_t texel) { return cm::div_((float)(texel >> 24), 255.0f); }

__device__ __forceinline__ float bilinearAlpha(const Quad& q, const Footprint& fp)
{
    const Axis &x = fp.x, &y = fp.y;
    const uint32_t w00 = q.w00, w10 = q.w10, w01 = q.w01, w11 = q.w11;
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
    const bool blocks = blockCompressed(e.format);
    float acc = 0.0f;
#pragma unroll 1
    for (uint32_t i = 0; i < N; ++i) {
        const float k = ((float)i + 0.5f) / fN - 0.5f;
        const float tu = u + mu * k, tv = v + mv * k;
        const Footprint f0 = footprintOf(e, l0, wrap, tu, tv), f1 = footprintOf(e, l1, wrap, tu, tv);
        Quad q0, q1;
        fetchQuads(e, blocks, f0, f1, q0, q1);
        acc = acc + lerp_(bilinearAlpha(q0, f0), bilinearAlpha(q1, f1), f);
    }
    return acc / fN;
}

// One bilinear fetch of mip 0: what a ray reads, which has no pixel quad to differentiate over (k_shadowmask.hip).
__device__ __forceinline__ float alphaLevel0(const TableEntry& e, bool wrap, float u, float v)
{
    const Footprint f = footprintOf(e, 0u, wrap, u, v);
    return bilinearAlpha(fetchQuad(e, blockCompressed(e.format), f), f);
}

} // namespace mtex
