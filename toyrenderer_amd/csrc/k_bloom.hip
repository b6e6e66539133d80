// k_bloom.hip -- BloomRenderer's mip chain (source/BloomRenderer.cpp, source/shaders/bloom.hlsl, the full-screen pass of
// Graphic.cpp:832-860): "bloom_PS_Downsample" (13 bilinear taps; the first pass Karis-weighted) and "bloom_PS_Upsample" (9
// bilinear taps at +- m_FilterRadius in UV, 3 x 3 tent; BlendOpaque, so the destination mip is OVERWRITTEN, not added to).
// The texture it builds is what "postprocess_PS_PostProcess" reads at t2 (k_postprocess.hip).
//
// CONVENTION (parity unpinned; restated in tests/bloom_ref.c and DESIGN.md 3).  The shared part (binary32 rules, lerp, dot3) is
// stated in screen_pass.hip.h; min / max = fmin / fmax (a NaN operand is dropped), loads and stores through r11g11b10.hip.h.  Here:
//   uv:       per axis ((float)p + 0.5f) / (float)destDim, p the destination texel, destDim the bound u0 mip's size;
//   taps:     as the HLSL writes them: inUV.x - 2 * x, inUV.x - x, inUV.x, inUV.x + x, inUV.x + 2 * x and the same in y, with
//             x, y = m_InvSourceResolution (downsample) or m_FilterRadius (upsample); 2 * x is an exact product;
//   bilinear: SampleLevel(LinearClamp, uv, 0) on a W x H mip: tx = uv.x * (float)W - 0.5f; x0 = floor(tx); fx = tx - x0; the
//             texel columns x0 and x0 + 1.0f, each clamped to [0, W - 1] as floats (fmin(fmax(., 0), W - 1): a NaN gives column 0)
//             and then converted; the same in y; per channel lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy).  This is the
//             project's definition: D3D hardware filters with fixed-point weights, and parity with it stays unpinned, as for the
//             other passes;
//   sums:     left to right as the HLSL writes them.  First downsample: groups (a + b + d + e), (b + c + e + f), (d + e + g + h),
//             (e + f + h + i) each * 0.03125f (the folded literal 0.125f / 4.0f), (j + k + l + m) * 0.125f; each group times
//             KarisAverage(group) = 1.0f / (1.0f + RGBToLuminance(group) * 0.25f) (the post pass's luminance dot3); the five
//             added in order; max(., 0.0001f) per channel.  Later downsamples: e * 0.125f, += (a + c + g + i) * 0.03125f,
//             += (b + d + f + h) * 0.0625f, += (j + k + l + m) * 0.125f.  Upsample: e * 4.0f, += (b + d + f + h) * 2.0f,
//             += (a + c + g + i), *= 0.0625f;
//   special:  inf - inf in a lerp gives NaN; max(NaN, 0.0001f) gives 0.0001f; a NaN is stored as the format's NaN code.
// Every texel of the destination mip is written.
//
// KERNELS.  One thread per destination texel in screen_pass.hip.h's tile.  The 13 (9) taps share 5 (3) columns and
// 5 (3) rows, so the column / row indices and weights are computed once per axis: the same expressions, so the same words.
// Texels are read straight from global memory through L1 / L2 with 4-byte loads and decoded per tap; no LDS.  Neighbouring
// destination texels share most of their 52 (36) source texels, so the other design for the downsample stages a workgroup's
// source footprint in LDS once (bloomDownsampleLdsKernel, built with -DTR_BLOOM_LDS_DOWNSAMPLE=1); every variant evaluates the
// same per-texel expression, so all give the same words.  The upsample is not tiled: its source is a quarter of its
// destination, its footprint grows with m_FilterRadius * sourceWidth without bound, and a 64 x 4 destination tile at the
// default radius touches about (32 + 2 r) x (2 + 2 r) source texels, which L1 holds.
//
// CODE OBJECT (-Rpass-analysis=kernel-resource-usage, gfx950): bloomDownsampleKernel 181 VGPRs (the compiler issues the 52
// loads ahead of the arithmetic), no LDS, 2 waves per SIMD; bloomDownsampleLdsKernel 189 VGPRs, 8192 B LDS, 2 waves per SIMD;
// bloomUpsampleKernel 125 VGPRs, no LDS, 4 waves per SIMD; no scratch in any.
//
// MEASURED: see profiles/bloom/README.md.
#include "cull_math.hip.h"
#include "r11g11b10.hip.h"
#include "screen_pass.hip.h"

namespace
{

using namespace interop;

constexpr uint32_t kBloomTileW = 64, kBloomTileH = 4;   // tests/test_gpu_bloom.py takes its sizes from these names: pinned to the shared tile
static_assert(kBloomTileW == sp::kTileW && kBloomTileH == sp::kTileH, "the bloom kernels run in the shared tile");

// The downsample's other design, for the cost comparison (profiles/bloom/): a workgroup stages the source footprint of its
// kBloomLdsTileW x kBloomLdsTileH destination tile once in LDS, as raw words, and takes its taps from there.  The footprint is
// derived from the tile's first and last destination texel through the same coordinate expression (every step of it is
// monotone in the texel index), so it holds for any size ratio and any m_InvSourceResolution; a workgroup whose footprint
// exceeds kBloomLdsWords reads global memory instead.
#ifndef TR_BLOOM_LDS_DOWNSAMPLE
#define TR_BLOOM_LDS_DOWNSAMPLE 0
#endif
constexpr uint32_t kBloomLdsTileW = 32, kBloomLdsTileH = 8, kBloomLdsWords = 2048;   // a 2:1 tile needs (2 * 32 + 6) * (2 * 8 + 6) = 1540 words

struct BloomArgs
{
    const uint32_t* src;                       // R11G11B10_FLOAT, the bound t0 mip, srcW x srcH
    uint32_t* dst;                             // R11G11B10_FLOAT, the bound u0 mip, dstW x dstH
    uint32_t srcW, srcH, dstW, dstH;
    BloomConsts k;
};

using sp::Axis;                                 // one axis of SampleLevel(LinearClamp): screen_pass.hip.h, shared with k_taa.hip
using sp::axisOf;
using sp::lerp_;
__device__ __forceinline__ cm::F3 add(cm::F3 a, cm::F3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
__device__ __forceinline__ cm::F3 mul(cm::F3 a, float s) { return { a.x * s, a.y * s, a.z * s }; }

// Where a tap's four texels come from: the source mip in global memory, or a workgroup's staged footprint in LDS.
struct GlobalSource
{
    const uint32_t* src; uint32_t pitch;
    __device__ __forceinline__ uint32_t word(uint32_t x, uint32_t y) const { return src[(uint64_t)y * pitch + x]; }
};
struct LdsSource
{
    const uint32_t* tile; uint32_t x0, y0, pitch;                          // the footprint's first column and row and its width
    __device__ __forceinline__ uint32_t word(uint32_t x, uint32_t y) const { return tile[(y - y0) * pitch + (x - x0)]; }
};

template <typename Source>
__device__ __forceinline__ cm::F3 tap(const Source& s, const Axis& x, const Axis& y)
{
    const uint32_t w00 = s.word(x.i0, y.i0), w10 = s.word(x.i1, y.i0), w01 = s.word(x.i0, y.i1), w11 = s.word(x.i1, y.i1);
#ifdef TR_BLOOM_EXPERIMENT_STORE_ONLY          // attribution only (profiles/bloom/): the pass's loads without its arithmetic
    return { __builtin_bit_cast(float, w00 ^ w10), __builtin_bit_cast(float, w01), __builtin_bit_cast(float, w11) };
#else
    const trhip::Rgb t00 = trhip::unpackR11G11B10(w00), t10 = trhip::unpackR11G11B10(w10);
    const trhip::Rgb t01 = trhip::unpackR11G11B10(w01), t11 = trhip::unpackR11G11B10(w11);
    return { lerp_(lerp_(t00.r, t10.r, x.f), lerp_(t01.r, t11.r, x.f), y.f),
             lerp_(lerp_(t00.g, t10.g, x.f), lerp_(t01.g, t11.g, x.f), y.f),
             lerp_(lerp_(t00.b, t10.b, x.f), lerp_(t01.b, t11.b, x.f), y.f) };
#endif
}

__device__ __forceinline__ cm::F3 karis(cm::F3 g)                         // bloom.hlsl:9-14, 72-76: group *= KarisAverage(group)
{
    const float luma = cm::dot3(g, { 0x1.b38cdap-3f, 0x1.6e2974p-1f, 0x1.279aaep-4f }) * 0.25f;
    return mul(g, cm::div_(1.0f, 1.0f + luma));
}

__device__ __forceinline__ void store(const BloomArgs& a, uint32_t px, uint32_t py, cm::F3 c)
{
#ifdef TR_BLOOM_EXPERIMENT_STORE_ONLY
    a.dst[(uint64_t)py * a.dstW + px] = __builtin_bit_cast(uint32_t, c.x) ^ __builtin_bit_cast(uint32_t, c.y) ^ __builtin_bit_cast(uint32_t, c.z);
#else
    a.dst[(uint64_t)py * a.dstW + px] = trhip::packR11G11B10(c.x, c.y, c.z);
#endif
}

// The five columns (rows) of the downsample's taps for destination texel p: uv - 2 x, uv - x, uv, uv + x, uv + 2 x.
struct Axes5 { Axis m2, m1, c, p1, p2; };
__device__ __forceinline__ Axes5 downsampleAxes(uint32_t p, uint32_t dstDim, uint32_t srcDim, float step)
{
    const float uv = cm::div_((float)p + 0.5f, (float)dstDim);
    return { axisOf(uv - 2.0f * step, srcDim), axisOf(uv - step, srcDim), axisOf(uv, srcDim), axisOf(uv + step, srcDim), axisOf(uv + 2.0f * step, srcDim) };
}

template <typename Source>
__device__ __forceinline__ void downsampleTexel(const BloomArgs& a, const Source& s, uint32_t px, uint32_t py)   // bloom.hlsl:16-89
{
    const Axes5 X = downsampleAxes(px, a.dstW, a.srcW, a.k.m_InvSourceResolution.x), Y = downsampleAxes(py, a.dstH, a.srcH, a.k.m_InvSourceResolution.y);
    const cm::F3 A = tap(s, X.m2, Y.p2), B = tap(s, X.c, Y.p2), C = tap(s, X.p2, Y.p2);
    const cm::F3 D = tap(s, X.m2, Y.c), E = tap(s, X.c, Y.c), F = tap(s, X.p2, Y.c);
    const cm::F3 G = tap(s, X.m2, Y.m2), H = tap(s, X.c, Y.m2), I = tap(s, X.p2, Y.m2);
    const cm::F3 J = tap(s, X.m1, Y.p1), K = tap(s, X.p1, Y.p1), L = tap(s, X.m1, Y.m1), M = tap(s, X.p1, Y.m1);
    cm::F3 d;
    if (a.k.m_bIsFirstDownsample) {
        const cm::F3 g0 = karis(mul(add(add(add(A, B), D), E), 0.03125f));
        const cm::F3 g1 = karis(mul(add(add(add(B, C), E), F), 0.03125f));
        const cm::F3 g2 = karis(mul(add(add(add(D, E), G), H), 0.03125f));
        const cm::F3 g3 = karis(mul(add(add(add(E, F), H), I), 0.03125f));
        const cm::F3 g4 = karis(mul(add(add(add(J, K), L), M), 0.125f));
        d = add(add(add(add(g0, g1), g2), g3), g4);
        d = { cm::max_(d.x, 0.0001f), cm::max_(d.y, 0.0001f), cm::max_(d.z, 0.0001f) };
    } else {
        d = mul(E, 0.125f);
        d = add(d, mul(add(add(add(A, C), G), I), 0.03125f));
        d = add(d, mul(add(add(add(B, D), F), H), 0.0625f));
        d = add(d, mul(add(add(add(J, K), L), M), 0.125f));
    }
    store(a, px, py, d);
}

__global__ __launch_bounds__(sp::kBlock) void bloomDownsampleKernel(BloomArgs a)
{
    const sp::Pixel at = sp::pixel();
    if (!at.inside(a.dstW, a.dstH)) return;
    downsampleTexel(a, GlobalSource{ a.src, a.srcW }, at.x, at.y);
}

// Cost comparison only unless TR_BLOOM_LDS_DOWNSAMPLE is set (profiles/bloom/).  The first and the last texel of the tile give
// the footprint: the smallest first index and the largest second index over the five taps (the step may have either sign).
__device__ __forceinline__ void footprint(uint32_t first, uint32_t last, uint32_t dstDim, uint32_t srcDim, float step, uint32_t* lo, uint32_t* hi)
{
    const Axes5 f = downsampleAxes(first, dstDim, srcDim, step), l = downsampleAxes(last, dstDim, srcDim, step);
    *lo = min(min(min(f.m2.i0, f.m1.i0), min(f.c.i0, f.p1.i0)), f.p2.i0);
    *hi = max(max(max(l.m2.i1, l.m1.i1), max(l.c.i1, l.p1.i1)), l.p2.i1);
}

__global__ __launch_bounds__(sp::kBlock) void bloomDownsampleLdsKernel(BloomArgs a)
{
    __shared__ uint32_t tile[kBloomLdsWords];
    const uint32_t tx = threadIdx.x % kBloomLdsTileW, ty = threadIdx.x / kBloomLdsTileW;
    const uint32_t bx = blockIdx.x * kBloomLdsTileW, by = blockIdx.y * kBloomLdsTileH, px = bx + tx, py = by + ty;
    uint32_t x0, x1, y0, y1;                                                // uniform over the workgroup
    footprint(bx, min(bx + kBloomLdsTileW, a.dstW) - 1u, a.dstW, a.srcW, a.k.m_InvSourceResolution.x, &x0, &x1);
    footprint(by, min(by + kBloomLdsTileH, a.dstH) - 1u, a.dstH, a.srcH, a.k.m_InvSourceResolution.y, &y0, &y1);
    const bool inside = px < a.dstW && py < a.dstH;
    const uint32_t fw = x1 - x0 + 1u, fh = y1 - y0 + 1u;                   // x1 >= x0: both are clamped, monotone indices
    if (x1 < x0 || y1 < y0 || (uint64_t)fw * fh > kBloomLdsWords) {         // a NaN step can order them the other way: no staging
        if (inside) downsampleTexel(a, GlobalSource{ a.src, a.srcW }, px, py);
        return;
    }
    for (uint32_t i = threadIdx.x; i < fw * fh; i += sp::kBlock) {
        const uint32_t r = i / fw, c = i - r * fw;
        tile[i] = a.src[(uint64_t)(y0 + r) * a.srcW + x0 + c];
    }
    __syncthreads();
    if (inside) downsampleTexel(a, LdsSource{ tile, x0, y0, fw }, px, py);
}

__global__ __launch_bounds__(sp::kBlock) void bloomUpsampleKernel(BloomArgs a)               // bloom.hlsl:93-129
{
    const sp::Pixel at = sp::pixel();
    if (!at.inside(a.dstW, a.dstH)) return;
    const uint32_t px = at.x, py = at.y;
    const float u = cm::div_((float)px + 0.5f, (float)a.dstW), v = cm::div_((float)py + 0.5f, (float)a.dstH);
    const float r = a.k.m_FilterRadius;
    const GlobalSource s{ a.src, a.srcW };
    const Axis xm = axisOf(u - r, a.srcW), x0 = axisOf(u, a.srcW), xp = axisOf(u + r, a.srcW);
    const Axis ym = axisOf(v - r, a.srcH), y0 = axisOf(v, a.srcH), yp = axisOf(v + r, a.srcH);
    const cm::F3 A = tap(s, xm, yp), B = tap(s, x0, yp), C = tap(s, xp, yp);
    const cm::F3 D = tap(s, xm, y0), E = tap(s, x0, y0), F = tap(s, xp, y0);
    const cm::F3 G = tap(s, xm, ym), H = tap(s, x0, ym), I = tap(s, xp, ym);
    cm::F3 up = mul(E, 4.0f);
    up = add(up, mul(add(add(add(B, D), F), H), 2.0f));
    up = add(up, add(add(add(A, C), G), I));
    store(a, px, py, mul(up, 0.0625f));
}

int recordBloom(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const bool up = ctx.variant != 0;
    const BloomConsts* k = (const BloomConsts*)ctx.constants(0, sizeof(BloomConsts));
    TRHIP_REQUIRE(k, "%s: b0 or push constants (BloomConsts, 16 bytes) missing", name);
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_R11G11B10_FLOAT, "Texture_SRV t0 = the R11G11B10_FLOAT source texture", true, sp::kAnyMip },
                                 { TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_R11G11B10_FLOAT, "Texture_UAV u0 = the R11G11B10_FLOAT destination texture", true, sp::kAnyMip } };
    trhip_texture_t* tex[2];
    uint32_t mip[2];
    if (const int rc = sp::bindTextures(ctx, want, tex, 0, 0, nullptr, mip)) return rc;             // source and destination each have their mip's own size
    const trhip_texture_t *src = tex[0], *dst = tex[1];
    TRHIP_REQUIRE(src->mipPtr(mip[0]) != dst->mipPtr(mip[1]), "%s: t0 and u0 are the same mip %u of one texture", name, mip[0]);
    BloomArgs a = sp::zeroed<BloomArgs>();
    a.src = (const uint32_t*)src->mipPtr(mip[0]);
    a.dst = (uint32_t*)dst->mipPtr(mip[1]);
    a.srcW = src->mipW(mip[0]); a.srcH = src->mipH(mip[0]);
    a.dstW = dst->mipW(mip[1]); a.dstH = dst->mipH(mip[1]);
    a.k = *k;
    if (const int rc = sp::requireCover(ctx, sp::kGroupSide, sp::kGroupSide, a.dstW, a.dstH, " destination mip")) return rc;
    const dim3 grid = sp::tiles(a.dstW, a.dstH), block(sp::kTileW, sp::kTileH);
    if (up)
        sp::launch(ctx, bloomUpsampleKernel, "bloomUpsampleKernel", grid, block, a);
    else if (TR_BLOOM_LDS_DOWNSAMPLE)
        sp::launch(ctx, bloomDownsampleLdsKernel, "bloomDownsampleLdsKernel", sp::tiles(a.dstW, a.dstH, kBloomLdsTileW, kBloomLdsTileH), dim3(sp::kBlock), a);
    else
        sp::launch(ctx, bloomDownsampleKernel, "bloomDownsampleKernel", grid, block, a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("bloom_PS_Downsample", recordBloom, 0);
trhip::ShaderRegistrar r1("bloom_PS_Upsample", recordBloom, 1);

} // namespace
