// k_taa.hip -- "taa_CS_TemporalResolve": the temporal anti-aliasing resolve between LightingOutput and the post pass, the place
// of the reference's TAARenderer (source/TAARenderer.cpp).  That renderer only calls DLSS or FSR, and neither SDK is in the
// reference's tree, so the entry name and the resolve are this project's own statement of the published algorithm: Karis, "High
// Quality Temporal Supersampling" (SIGGRAPH 2014), with the closest-depth velocity dilation and the neighbourhood clamp of Pedersen,
// "Temporal Reprojection Anti-Aliasing in INSIDE" (GDC 2016).  tests/taa_ref.c is the definition; the host side (Halton jitter,
// the jittered m_ViewToClip, g_AntiAliasedLightingOutput, the post pass's input) is the reference's.
//
// BINDINGS, all W x H = m_OutputDims, one mip: t0 LightingOutput (R11G11B10_FLOAT), t1 the frame's depth (R32_FLOAT, reverse Z),
// t2 the motion target (RG16_FLOAT, previous minus current position in pixels), t3 the previous history (RGBA16_FLOAT: xyz the
// colour, w the accumulated sample count), u0 the new history (RGBA16_FLOAT, another texture than t3), u1
// AntiAliasedLightingOutput (R11G11B10_FLOAT); b0 or push constants: the 32 bytes of TAAConsts.
//
// CONVENTION (parity unpinned; restated in tests/taa_ref.c and DESIGN.md 3).  The shared part (binary32 rules, lerp, dot3, the
// binary16 load and store, the sampler axis) is stated in screen_pass.hip.h; min / max = fmin / fmax (a NaN operand is dropped),
// R11G11B10_FLOAT through r11g11b10.hip.h.  For the pixel p = (px, py):
//   window:   columns max(px - 1, 0), px, min(px + 1, W - 1) and the same rows, as integers; nine texels, visited row by row;
//   YCoCg:    Y = (0.25f * R + 0.5f * G) + 0.25f * B; Co = 0.5f * R - 0.5f * B; Cg = (0.5f * G - 0.25f * R) - 0.25f * B;
//   box:      lo = hi = the first texel's YCoCg, then per channel lo = min(lo, .), hi = max(hi, .) over the other eight in
//             order (a NaN channel of a texel is dropped; none of these values is -0); c = the centre texel's RGB;
//   dilation: best = the centre's depth at the centre's position; over the nine in order, a texel whose depth is > best (a NaN
//             never is) replaces it; mv = the two binary16 of the motion texel at that position;
//   history:  hp.x = (((float)px + 0.5f) + mv.x) - m_JitterDelta.x, the same in y.  Valid when m_bResetHistory == 0, hp.x >= 0.0f,
//             hp.x < (float)W, hp.y >= 0.0f, hp.y < (float)H (a NaN fails) and the four channels of the fetch are finite.  The
//             fetch is SampleLevel(LinearClamp, (hp.x / (float)W, hp.y / (float)H), 0) of t3 exactly as k_bloom.hip states it
//             (sp::axisOf per axis; per channel lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy)), over all four channels; t3 is
//             not read for a pixel that m_bResetHistory or the position test already decides;
//   clamp:    k = YCoCg(history.xyz); per channel q = min(max(k, lo), hi) + 0.0f (the sum makes a zero +0, whichever zero min or
//             max returns).  If q == k in all three channels (a NaN compares unequal) h = history.xyz as fetched, else
//             h = ((q.Y + q.Co) - q.Cg, q.Y + q.Cg, (q.Y - q.Co) - q.Cg);
//   blend:    n = min(max(history.w, 0.0f), m_MaxSampleCount); alpha = max(1.0f / (n + 1.0f), m_MinBlend); L = the post pass's
//             luminance dot3(rgb, (0x1.b38cdap-3f, 0x1.6e2974p-1f, 0x1.279aaep-4f)); wc = alpha / (1.0f + L(c));
//             wh = (1.0f - alpha) / (1.0f + L(h)); out = (c * wc + h * wh) / (wc + wh) per channel, one division each.  With
//             invalid history out = c and n = 0.0f.  Nothing treats a NaN or an infinite c specially: with valid history an
//             infinite channel of c makes wc 0 and out NaN, which both stores keep as their NaN codes, and the next frame finds
//             that history not finite and starts the pixel again;
//   store:    u0 = (out, min(n + 1.0f, m_MaxSampleCount)) as four binary16 (round to nearest even, a NaN as 0x7E00), u1 = out
//             packed to R11G11B10_FLOAT.  Every texel of both is written.
// OUT OF SCOPE: Catmull-Rom history filtering; variance clipping; depth- or velocity-based disocclusion tests
// beyond the clamp; sharpening (the reference's m_FSRSharpening defaults to 0); upscaling (render size = display size, as the
// reference passes to FSR); a reactive mask (the reference's own TODO).  Sky texels carry the cleared motion (0, 0), as they do
// into the reference's FSR call, so under camera rotation only the clamp bounds them.
//
// KERNELS.  One thread per pixel.  A pixel touches about 32 bytes of its own (4 colour, 4 depth, 4 motion, 8 history read; 8
// history and 4 colour written); the 3 x 3 colour and depth windows are shared ninefold between neighbours.  taaLdsKernel, the
// product, stages the colour words and depths of a kTaaLdsTileW x kTaaLdsTileH tile with its one-texel halo in LDS once per
// workgroup, at the clamped coordinates, so a thread indexes it without clamping; motion and history go straight through L1 with
// 4- and 8-byte loads.  taaKernel (-DTR_TAA_LDS=0) is the plain design: everything straight through L1 in screen_pass.hip.h's
// 64 x 4 tile.  Both evaluate the same per-pixel expression, so both give the same words (the whole of tests/test_gpu_taa.py
// passes on either build, and the city frame's checksums agree).
//
// CODE OBJECT (-Rpass-analysis=kernel-resource-usage, gfx950): taaLdsKernel 49 VGPRs, 2720 B LDS; taaKernel 50 VGPRs, no LDS; each
// 8 waves per SIMD, no scratch.  The load-and-store builds: 12 and 10 VGPRs.
//
// MEASURED (tools/taa_cost.py, generated city of 2251 instances at 3840 x 2160, the jitter advancing every frame; builds alternated
// three times on one MI355X, median and spread; profiles/taa/).  The resolve inside the frame: plain 162.9 us (1.0), LDS 141.4
// (0.2); alone on the textures the frames left behind: plain 152.7 (3.7), LDS 146.1 (3.9).  The LDS design wins by 21.5 us in the
// frame and 6.6 us alone, more than either spread, so it is the product.  Its 265 MB alone would stream in 41.0 us at the box's
// 6.48 TB/s, and a build that only loads and stores the pass's own bytes (-DTR_TAA_EXPERIMENT_STORE_ONLY) takes 42.4 us (0.4) in
// the plain shape and 60.1 (0.5) with the staging: the pass is 3.3 times the plain floor, and the rest is arithmetic: nine
// R11G11B10_FLOAT decodes and YCoCg transforms, sixteen binary16 decodes and eight correctly rounded divisions per pixel.
// Negative controls (profiles/taa/mutations.txt): seven -D builds that each drop one rule (TR_TAA_MUTATE_*) fail 8 to 10 of the 16
// GPU tests each.
#include "cull_math.hip.h"
#include "r11g11b10.hip.h"
#include "screen_pass.hip.h"

namespace
{

using namespace interop;

#ifndef TR_TAA_LDS
#define TR_TAA_LDS 1                           // 1: the LDS-staged design, the product (MEASURED above); 0: the plain one, for the cost comparison
#endif
constexpr uint32_t kTaaTileW = 64, kTaaTileH = 4;            // the plain kernel's tile; tests/test_gpu_taa.py takes its sizes from these names
static_assert(kTaaTileW == sp::kTileW && kTaaTileH == sp::kTileH, "the plain kernel runs in the shared tile");
constexpr uint32_t kTaaLdsTileW = 32, kTaaLdsTileH = 8;      // (32 + 2) x (8 + 2) = 340 staged texels, 2720 bytes
constexpr uint32_t kTaaLdsPitch = kTaaLdsTileW + 2u, kTaaLdsRows = kTaaLdsTileH + 2u;
static_assert(kTaaLdsTileW * kTaaLdsTileH == sp::kBlock, "one thread per pixel of the staged tile");

struct TaaArgs
{
    const uint32_t* colour;                    // t0 R11G11B10_FLOAT
    const float* depth;                        // t1 R32_FLOAT
    const uint32_t* motion;                    // t2 RG16_FLOAT: x in the low half
    const uint2* history;                      // t3 RGBA16_FLOAT
    uint2* newHistory;                         // u0 RGBA16_FLOAT
    uint32_t* out;                             // u1 R11G11B10_FLOAT
    TAAConsts k;
};

// A window coordinate: px + d (d = -1, 0, 1) clamped to [0, dim - 1].
__device__ __forceinline__ uint32_t windowAt(uint32_t p, int d, uint32_t dim)
{
#ifdef TR_TAA_MUTATE_BORDER                    // negative control only (profiles/taa/mutations.txt): the window wraps around the image
    return d < 0 ? (p > 0u ? p - 1u : dim - 1u) : d > 0 ? (p + 1u < dim ? p + 1u : 0u) : p;
#else
    return d < 0 ? (p > 0u ? p - 1u : 0u) : d > 0 ? (p + 1u < dim ? p + 1u : dim - 1u) : p;
#endif
}

// Where the window's colour words and depths come from: global memory, or the workgroup's staged tile.
struct GlobalWindow
{
    const uint32_t* colour; const float* depth; uint32_t px, py, W, H;
    __device__ __forceinline__ uint64_t at(int dx, int dy) const { return (uint64_t)windowAt(py, dy, H) * W + windowAt(px, dx, W); }
    __device__ __forceinline__ uint32_t word(int dx, int dy) const { return colour[at(dx, dy)]; }
    __device__ __forceinline__ float z(int dx, int dy) const { return depth[at(dx, dy)]; }
};
struct LdsWindow
{
    const uint32_t* colour; const float* depth; uint32_t tx, ty;          // the thread's place in the tile; the halo adds one
    __device__ __forceinline__ uint32_t at(int dx, int dy) const { return (uint32_t)((int)ty + 1 + dy) * kTaaLdsPitch + (uint32_t)((int)tx + 1 + dx); }
    __device__ __forceinline__ uint32_t word(int dx, int dy) const { return colour[at(dx, dy)]; }
    __device__ __forceinline__ float z(int dx, int dy) const { return depth[at(dx, dy)]; }
};

__device__ __forceinline__ cm::F3 toYCoCg(cm::F3 c)
{
    return { (0.25f * c.x + 0.5f * c.y) + 0.25f * c.z, 0.5f * c.x - 0.5f * c.z, (0.5f * c.y - 0.25f * c.x) - 0.25f * c.z };
}
__device__ __forceinline__ cm::F3 fromYCoCg(cm::F3 k) { return { (k.x + k.y) - k.z, k.x + k.z, (k.x - k.y) - k.z }; }
__device__ __forceinline__ float luminance(cm::F3 c) { return cm::dot3(c, { 0x1.b38cdap-3f, 0x1.6e2974p-1f, 0x1.279aaep-4f }); }
__device__ __forceinline__ bool finite_(float x) { return __builtin_fabsf(x) < __builtin_inff(); }
__device__ __forceinline__ float half0(uint32_t w) { return (float)sp::halfOf(w); }
__device__ __forceinline__ float half1(uint32_t w) { return (float)sp::halfOf(w >> 16); }

struct History { float r, g, b, n; };

// SampleLevel(LinearClamp, (u, v), 0) of the W x H history, all four channels.
__device__ __forceinline__ History fetchHistory(const uint2* t, uint32_t W, uint32_t H, float u, float v)
{
    const sp::Axis x = sp::axisOf(u, W), y = sp::axisOf(v, H);
    const uint2 t00 = t[(uint64_t)y.i0 * W + x.i0], t10 = t[(uint64_t)y.i0 * W + x.i1], t01 = t[(uint64_t)y.i1 * W + x.i0], t11 = t[(uint64_t)y.i1 * W + x.i1];
    using sp::lerp_;
    return { lerp_(lerp_(half0(t00.x), half0(t10.x), x.f), lerp_(half0(t01.x), half0(t11.x), x.f), y.f),
             lerp_(lerp_(half1(t00.x), half1(t10.x), x.f), lerp_(half1(t01.x), half1(t11.x), x.f), y.f),
             lerp_(lerp_(half0(t00.y), half0(t10.y), x.f), lerp_(half0(t01.y), half0(t11.y), x.f), y.f),
             lerp_(lerp_(half1(t00.y), half1(t10.y), x.f), lerp_(half1(t01.y), half1(t11.y), x.f), y.f) };
}

template <typename Window>
__device__ __forceinline__ void resolvePixel(const TaaArgs& a, const Window& w, uint32_t px, uint32_t py)
{
    const uint32_t W = a.k.m_OutputDims.x, H = a.k.m_OutputDims.y;
    const uint64_t i = (uint64_t)py * W + px;
#ifdef TR_TAA_EXPERIMENT_STORE_ONLY            // attribution only (profiles/taa/): the pass's own bytes without its window or its arithmetic
    const uint32_t word = w.word(0, 0), zw = __builtin_bit_cast(uint32_t, w.z(0, 0)), mw = a.motion[i];
    const uint2 hw = a.history[i];
    a.newHistory[i] = { hw.x ^ word, hw.y ^ zw };
    a.out[i] = word ^ mw;
#else
    // the neighbourhood box and the nearest surface, one pass over the nine
    cm::F3 lo = {}, hi = {}, c = {};
    float best = w.z(0, 0);
    int bx = 0, by = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const trhip::Rgb t = trhip::unpackR11G11B10(w.word(dx, dy));
            const cm::F3 k = toYCoCg({ t.r, t.g, t.b });
            if (dy == -1 && dx == -1) {
                lo = hi = k;
            } else {
                lo = { cm::min_(lo.x, k.x), cm::min_(lo.y, k.y), cm::min_(lo.z, k.z) };
                hi = { cm::max_(hi.x, k.x), cm::max_(hi.y, k.y), cm::max_(hi.z, k.z) };
            }
            if (dy == 0 && dx == 0) c = { t.r, t.g, t.b };
#ifndef TR_TAA_MUTATE_DILATION                 // negative control only: the centre's own motion
            const float z = w.z(dx, dy);
            if (z > best) { best = z; bx = dx; by = dy; }
#endif
        }
    const uint32_t mw = a.motion[(uint64_t)windowAt(py, by, H) * W + windowAt(px, bx, W)];
#ifdef TR_TAA_MUTATE_JITTER                    // negative control only: the jitter delta is not taken out
    const float hx = ((float)px + 0.5f) + half0(mw), hy = ((float)py + 0.5f) + half1(mw);
#else
    const float hx = (((float)px + 0.5f) + half0(mw)) - a.k.m_JitterDelta.x, hy = (((float)py + 0.5f) + half1(mw)) - a.k.m_JitterDelta.y;
#endif
    bool valid = a.k.m_bResetHistory == 0u && hx >= 0.0f && hx < (float)W && hy >= 0.0f && hy < (float)H;
    cm::F3 out = c;
    float n = 0.0f;
    if (valid) {
        const History f = fetchHistory(a.history, W, H, cm::div_(hx, (float)W), cm::div_(hy, (float)H));
#ifndef TR_TAA_MUTATE_FINITE                   // negative control only: a history that is not finite is blended
        valid = finite_(f.r) && finite_(f.g) && finite_(f.b) && finite_(f.n);
#endif
        if (valid) {
            cm::F3 h = { f.r, f.g, f.b };
#ifndef TR_TAA_MUTATE_CLAMP                    // negative control only: the history is taken as fetched
            const cm::F3 k = toYCoCg(h);
            const cm::F3 q = { cm::min_(cm::max_(k.x, lo.x), hi.x) + 0.0f, cm::min_(cm::max_(k.y, lo.y), hi.y) + 0.0f, cm::min_(cm::max_(k.z, lo.z), hi.z) + 0.0f };
            if (!(q.x == k.x && q.y == k.y && q.z == k.z)) h = fromYCoCg(q);
#endif
            n = cm::min_(cm::max_(f.n, 0.0f), a.k.m_MaxSampleCount);
#ifdef TR_TAA_MUTATE_ALPHA                     // negative control only: a constant blend factor
            const float alpha = a.k.m_MinBlend;
#else
            const float alpha = cm::max_(cm::div_(1.0f, n + 1.0f), a.k.m_MinBlend);
#endif
#ifdef TR_TAA_MUTATE_LUMA                      // negative control only: unweighted blend
            const float wc = alpha, wh = 1.0f - alpha;
#else
            const float wc = cm::div_(alpha, 1.0f + luminance(c)), wh = cm::div_(1.0f - alpha, 1.0f + luminance(h));
#endif
            const float sum = wc + wh;
            out = { cm::div_(c.x * wc + h.x * wh, sum), cm::div_(c.y * wc + h.y * wh, sum), cm::div_(c.z * wc + h.z * wh, sum) };
        }
    }
    const float count = cm::min_(n + 1.0f, a.k.m_MaxSampleCount);
    a.newHistory[i] = { sp::halfBits(out.x) | sp::halfBits(out.y) << 16, sp::halfBits(out.z) | sp::halfBits(count) << 16 };
    a.out[i] = trhip::packR11G11B10(out.x, out.y, out.z);
#endif
}

__global__ __launch_bounds__(sp::kBlock) void taaKernel(TaaArgs a)
{
    const uint32_t W = a.k.m_OutputDims.x, H = a.k.m_OutputDims.y;
    const sp::Pixel at = sp::pixel();
    if (!at.inside(W, H)) return;
    resolvePixel(a, GlobalWindow{ a.colour, a.depth, at.x, at.y, W, H }, at.x, at.y);
}

// The product unless built with -DTR_TAA_LDS=0.  Staged texel (r, c) is the image texel at row by - 1 + r and
// column bx - 1 + c, each clamped into the image: what the plain kernel's window reads there.
__global__ __launch_bounds__(sp::kBlock) void taaLdsKernel(TaaArgs a)
{
    __shared__ uint32_t colour[kTaaLdsPitch * kTaaLdsRows];
    __shared__ float depth[kTaaLdsPitch * kTaaLdsRows];
    const uint32_t W = a.k.m_OutputDims.x, H = a.k.m_OutputDims.y;
    const uint32_t tx = threadIdx.x % kTaaLdsTileW, ty = threadIdx.x / kTaaLdsTileW;
    const uint32_t bx = blockIdx.x * kTaaLdsTileW, by = blockIdx.y * kTaaLdsTileH;       // inside the image: the grid is ceil(W / tile) x ceil(H / tile)
    for (uint32_t s = threadIdx.x; s < kTaaLdsPitch * kTaaLdsRows; s += sp::kBlock) {
        const uint32_t r = s / kTaaLdsPitch, c = s - r * kTaaLdsPitch;
        // row by - 1 + r and column bx - 1 + c, clamped to [0, H - 1] and [0, W - 1] without going below zero on the way
        const uint32_t y = by + r > 0u ? (by + r - 1u < H ? by + r - 1u : H - 1u) : 0u;
        const uint32_t x = bx + c > 0u ? (bx + c - 1u < W ? bx + c - 1u : W - 1u) : 0u;
        colour[s] = a.colour[(uint64_t)y * W + x];
        depth[s] = a.depth[(uint64_t)y * W + x];
    }
    __syncthreads();
    const uint32_t px = bx + tx, py = by + ty;
    if (px < W && py < H) resolvePixel(a, LdsWindow{ colour, depth, tx, ty }, px, py);
}

int recordTaa(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const TAAConsts* k = (const TAAConsts*)ctx.constants(0, sizeof(TAAConsts));
    TRHIP_REQUIRE(k, "%s: b0 or push constants (TAAConsts, 32 bytes) missing", name);
    const uint32_t W = k->m_OutputDims.x, H = k->m_OutputDims.y;
    TRHIP_REQUIRE(W && H, "%s: m_OutputDims %ux%u is empty", name, W, H);
    if (const int rc = sp::requireCover(ctx, sp::kGroupSide, sp::kGroupSide, W, H)) return rc;
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_R11G11B10_FLOAT, "Texture_SRV t0 = the R11G11B10_FLOAT LightingOutput", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 1, TRHIP_FORMAT_R32_FLOAT, "Texture_SRV t1 = the R32_FLOAT depth texture", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 2, TRHIP_FORMAT_RG16_FLOAT, "Texture_SRV t2 = the RG16_FLOAT motion target", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 3, TRHIP_FORMAT_RGBA16_FLOAT, "Texture_SRV t3 = the RGBA16_FLOAT previous history", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_RGBA16_FLOAT, "Texture_UAV u0 = the RGBA16_FLOAT new history, mip 0", true, sp::kOneMipAt0 },
                                 { TRHIP_BIND_TEXTURE_UAV, 1, TRHIP_FORMAT_R11G11B10_FLOAT, "Texture_UAV u1 = the R11G11B10_FLOAT AntiAliasedLightingOutput, mip 0", true, sp::kOneMipAt0 } };
    trhip_texture_t* tex[6];
    if (const int rc = sp::bindTextures(ctx, want, tex, W, H, "m_OutputDims")) return rc;
    TRHIP_REQUIRE(tex[3] != tex[4], "%s: t3 and u0 are the same texture '%s': the history is read at other texels than the one written", name, tex[3]->name.c_str());
    TRHIP_REQUIRE(tex[0] != tex[5], "%s: t0 and u1 are the same texture '%s': the window reads the neighbours' colours", name, tex[0]->name.c_str());
    TaaArgs a = sp::zeroed<TaaArgs>();
    a.colour = (const uint32_t*)tex[0]->ptr;
    a.depth = (const float*)tex[1]->ptr;
    a.motion = (const uint32_t*)tex[2]->ptr;
    a.history = (const uint2*)tex[3]->ptr;
    a.newHistory = (uint2*)tex[4]->ptr;
    a.out = (uint32_t*)tex[5]->ptr;
    a.k = *k;
    if (TR_TAA_LDS)
        sp::launch(ctx, taaLdsKernel, "taaLdsKernel", sp::tiles(W, H, kTaaLdsTileW, kTaaLdsTileH), dim3(sp::kBlock), a);
    else
        sp::launch(ctx, taaKernel, "taaKernel", sp::tiles(W, H), dim3(sp::kTileW, sp::kTileH), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("taa_CS_TemporalResolve", recordTaa, 0);

} // namespace
