// k_sigma.hip -- the sun shadow denoiser behind "shadowmask_CS_ShadowMask" with m_bDoDenoising != 0 (k_shadowmask.hip), the place of
// ShadowMaskRenderer::DenoiseShadows (source/ShadowMaskRenderer.cpp:337-500).  That function only calls NRD's SIGMA, and NRD is not
// in the reference's tree, so the denoiser is this project's own statement of the published algorithm (NVIDIA Real-Time Denoisers,
// SIGMA shadow: tile classification, a penumbra-sized Poisson blur in two passes, a temporal stabilisation with a variance clamp).
// tests/sigma_ref.c is the definition.  The entry names are the ones the reference's loop forms from NRD's file names
// (ShadowMaskRenderer.cpp:473-495): "SIGMA_Shadow_ClassifyTiles.cs", "SIGMA_Shadow_Blur.cs", "SIGMA_Shadow_PostBlur.cs" (one kernel
// with SIGMA_Shadow_Blur.cs; m_Pass is 0 and 1) and "SIGMA_Shadow_TemporalStabilization.cs".
//
// BINDINGS.  b0 or push constants: the 112 bytes of SigmaConsts.  W x H = m_OutputDims, one mip; tiles: ceil(W / 16) x ceil(H / 16).
//   ClassifyTiles: t0 the penumbra (R16_FLOAT), t1 the linear view depth (R16_FLOAT); u0 the tile texture (R8_UINT), u1 shadow data
//             (RG16_FLOAT); groups of 16 x 16 pixels covering the image;
//   Blur, PostBlur: t0 shadow data in (RG16_FLOAT), t1 the linear view depth, t2 the depth (R32_FLOAT), t3 the normal roughness texture
//             (R10G10B10A2_UNORM, "shadowmask_CS_PackNormalAndRoughness"), t4 the tile texture; u0 shadow data out (another texture than
//             t0); groups of 8 x 8 pixels covering the image;
//   TemporalStabilization: t0 shadow data, t1 the linear view depth, t2 the motion target (RG16_FLOAT, previous minus current position in
//             pixels), t3 the previous history (R16_FLOAT), t4 the tile texture; u0 the new history (R16_FLOAT, another texture than
//             t3), u1 the shadow mask (R8_UNORM); groups of 8 x 8.
//
// CONVENTION (parity unpinned; restated in tests/sigma_ref.c).  screen_pass.hip.h's shared part: binary32, no contraction, cm::div_ and
// cm::sqrt_, min / max = fmin / fmax, worldPosition, lerp, the binary16 load and store, sp::axisOf.  No libm: the eight Poisson taps
// and the sixteen rotations by multiples of pi / 8 are binary32 literals, the same in tests/sigma_ref.c.
//   terms:    P, the penumbra, and every other binary16 is read exactly.  occluded: P < 65504 (a NaN is not).  sky: the linear view
//             depth's word is 0x7BFF or its value is >= m_DenoisingRange (a NaN is not).  A sky texel contributes to no sum.
//   classify: shadow data = sky ? (1, 65504) : (occluded ? 0 : 1, P) (a NaN P is stored as 0x7E00); the tile's byte: bit 0 some non-sky
//             texel of the tile is lit, bit 1 some is occluded; texels outside the image count for nothing.
//   filtered: a texel's tile is filtered iff the OR of the bytes of the 3 x 3 tiles around it, tile coordinates clamped, is 3.  A sky
//             texel and a texel of a tile that is not filtered pass through every pass: Blur and PostBlur copy its word, the
//             stabilisation takes out = x; neither reads a neighbour or the history.  The blur radius is capped at kSigmaTile = 16
//             pixels, the tile's side, so one tile of dilation is enough: nothing a filtered texel's tap can reach lies beyond the
//             tiles that made it filtered.
//   blur:     (x, y) the texel's shadow data, zc its linear view depth, Xc = worldPosition of its R32 depth, Nc the normal roughness
//             texel's normal (xy = code / 1023.0f * 2 - 1 through gbuffer_unpack.hip.h's octahedral mapping);
//             plane(Xq) = max(0, 1 - |dot3(Nc, Xq - Xc)| / (m_PlaneDistanceSensitivity * zc)).
//             Pass 0: over the 5 x 5 window row by row, texels outside the image skipped, the centre included, each non-sky texel q
//             with y_q < 65504: sumW = sumW + plane(Xq), sumR = sumR + plane(Xq) * y_q.  Not sumW > 0: the word out is (x's word,
//             0x7BFF).  Else r = sumR / sumW.  Pass 1: not y < 65504: the word passes through; else r = y * kPostBlurRadiusScale.
//             r_px = min(r / (zc * m_PixelUnproject), 16).  Rotation index ((px & 3) | (py & 3) << 2) + m_FrameIndex + 5 * m_Pass) & 15,
//             (c, s) its pair; tap i = 0..7 in order: offset ((c * p.x - s * p.y) * r_px, (s * p.x + c * p.y) * r_px), texel
//             floor(((float)px + 0.5f) + offset.x) and the same in y, skipped when outside the image (a NaN is) or sky;
//             sum = sum + plane(Xq) * x_q, wsum = wsum + plane(Xq), starting from sum = x, wsum = 1.  Out: x = sum / wsum, y = r in
//             pass 0 and the texel's own y in pass 1, both through the binary16 store.
//   stabilisation: a sky texel: history 1.0, mask 255.  Else out = x, and for a texel of a filtered tile with 0 < y < 65504 (65504:
//             no occluder near; 0: a hard edge, which is why hard shadows come out as the raw mask): over the 3 x 3 window at clamped
//             coordinates (k_taa.hip's window) row by row, sky texels left out, m1 = m1 + v, m2 = m2 + v * v, n of them;
//             mean = m1 / n, sd = sqrt(max(m2 / n - mean * mean, 0)); the history position is k_taa.hip's,
//             (((float)px + 0.5f) + mv.x) - m_JitterDelta.x, with the texel's OWN motion (no closest-depth dilation: the mask has no
//             depth edge of its own to follow); valid when m_bResetHistory == 0, the position is inside the image and the
//             LinearClamp fetch (sp::axisOf, lerp of lerps) is finite; h = min(max(fetch, mean - m_SigmaScale * sd), mean +
//             m_SigmaScale * sd); out = lerp(x, h, m_StabilizationStrength).  History = binary16 of out, mask = uint(saturate(out) *
//             255.0f + 0.5f), the back buffer's UNORM store.  Every texel of both is written.
// SETTINGS.  m_PlaneDistanceSensitivity 0.02 and m_StabilizationStrength 5 / 6 are NRD's published defaults.  m_SigmaScale (the
// driver's default 2.0: NRD's antilag-free clamp of two standard deviations, wide enough to keep a converged penumbra, narrow enough to
// drop a shadow that moved away) and kPostBlurRadiusScale = 0.5 (the second pass cleans what the first left, over half its
// footprint, as NRD's post-blur shrinks its radius) have no published default.  NOBODY HAS JUDGED ANY OF THESE ON A PICTURE FROM
// THIS BUILD.
// OUT OF SCOPE: SmoothTiles beyond the 3 x 3 OR, translucency, SplitScreen and validation, disocclusion tests beyond the clamp,
// AccumulationMode other than continue or reset.
//
// KERNELS.  One thread per pixel, every index checked before use; classify is one 256-thread workgroup per tile, its two bits reduced
// by wave ballots and four LDS words, the byte stored once by thread 0: no atomics.  Windows and taps go straight through L1:
// untuned, nothing is staged in LDS.
// MEASURED (tools/sigma_cost.py, generated city of 2251 instances at 3840 x 2160, soft shadows, the frame counter advancing; three
// rounds on one MI355X, median and spread in us; profiles/sigma/): pack 31.3 (0.1), ClassifyTiles 26.6 (0.7), Blur 30.6 (0.1), PostBlur
// 25.7 (0.0), TemporalStabilization 30.9 (0.3), 145 us together, beside 25.6, 10.2, 23.0, 23.0 and 19.2 us that each pass's own bytes
// would take at the box's 6.48 TB/s.  This is the PASS-THROUGH path: on that scene nearly every texel is in shadow and 16 of 32400
// tiles are filtered.  A frame with penumbrae across the screen has not been measured.  Negative controls (profiles/sigma/
// mutations.txt): seven -D builds that each drop one rule (TR_SIGMA_MUTATE_*, one of them in k_shadowmask.hip) fail 11 to 21 of the
// 65 GPU tests each.
// CODE OBJECT (-Rpass-analysis=kernel-resource-usage, gfx950): sigmaClassifyKernel 8 VGPRs, 16 B LDS; sigmaBlurKernel 45 VGPRs;
// sigmaStabilizeKernel 35 VGPRs; each 8 waves per SIMD, no scratch.
#include "cull_math.hip.h"
#include "gbuffer_unpack.hip.h"
#include "screen_pass.hip.h"

namespace
{

using namespace interop;
using cm::F3;

constexpr uint32_t kSigmaTile = 16;            // the classified tile's side AND the blur radius cap in pixels: one tile of dilation covers every tap
constexpr float kMaxBlurRadius = (float)kSigmaTile;
constexpr float kPostBlurRadiusScale = 0.5f;
constexpr float kNoOccluder = 65504.0f;
constexpr uint32_t kNoOccluderWord = 0x7BFFu, kOneWord = 0x3C00u;

__device__ const float kPoisson[8][2] = { { -0.4706069f, -0.4427112f }, { -0.9057375f, 0.3003471f }, { -0.3487388f, 0.4037880f }, { 0.1023042f, 0.6439373f },
                                          { 0.5699277f, 0.3513750f }, { 0.2939128f, -0.1131226f }, { 0.7836658f, -0.4208784f }, { 0.1564120f, -0.8198990f } };
#define SIGMA_C 0.92387953f
#define SIGMA_S 0.38268343f
#define SIGMA_Q 0.70710678f
__device__ const float kRotation[16][2] = { { 1.0f, 0.0f }, { SIGMA_C, SIGMA_S }, { SIGMA_Q, SIGMA_Q }, { SIGMA_S, SIGMA_C }, { 0.0f, 1.0f }, { -SIGMA_S, SIGMA_C },
                                            { -SIGMA_Q, SIGMA_Q }, { -SIGMA_C, SIGMA_S }, { -1.0f, 0.0f }, { -SIGMA_C, -SIGMA_S }, { -SIGMA_Q, -SIGMA_Q }, { -SIGMA_S, -SIGMA_C },
                                            { 0.0f, -1.0f }, { SIGMA_S, -SIGMA_C }, { SIGMA_Q, -SIGMA_Q }, { SIGMA_C, -SIGMA_S } };

__device__ __forceinline__ float half0(uint32_t w) { return (float)sp::halfOf(w); }
__device__ __forceinline__ float half1(uint32_t w) { return (float)sp::halfOf(w >> 16); }
__device__ __forceinline__ bool finite_(float x) { return __builtin_fabsf(x) < __builtin_inff(); }

__device__ __forceinline__ bool isSky(uint32_t depthWord, float range)
{
#ifdef TR_SIGMA_MUTATE_SKY                     // negative control only (profiles/sigma/mutations.txt): the range does not make a texel sky
    return depthWord == kNoOccluderWord;
#else
    return depthWord == kNoOccluderWord || half0(depthWord) >= range;
#endif
}

// The OR of the 3 x 3 tiles around (tx, ty), coordinates clamped; tx < tw and ty < th.
__device__ __forceinline__ bool filteredTile(const uint8_t* tiles, uint32_t tw, uint32_t th, uint32_t tx, uint32_t ty)
{
#ifdef TR_SIGMA_MUTATE_DILATION                // negative control only: the texel's own tile decides
    return (tiles[(uint64_t)ty * tw + tx] & 3u) == 3u;
#else
    uint32_t bits = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const uint32_t x = dx < 0 ? (tx > 0u ? tx - 1u : 0u) : dx > 0 ? (tx + 1u < tw ? tx + 1u : tw - 1u) : tx;
            const uint32_t y = dy < 0 ? (ty > 0u ? ty - 1u : 0u) : dy > 0 ? (ty + 1u < th ? ty + 1u : th - 1u) : ty;
            bits |= tiles[(uint64_t)y * tw + x];
        }
    return (bits & 3u) == 3u;
#endif
}

// ---- "SIGMA_Shadow_ClassifyTiles.cs" ------------------------------------------------------------------------------------------------
struct ClassifyArgs { const uint16_t* penumbra; const uint16_t* lvd; uint8_t* tiles; uint32_t* data; uint32_t tw; SigmaConsts k; };

__global__ __launch_bounds__(kSigmaTile * kSigmaTile) void sigmaClassifyKernel(ClassifyArgs a)
{
    __shared__ uint32_t waveBits[kSigmaTile * kSigmaTile / 64u];
    const uint32_t W = a.k.m_OutputDims.x, H = a.k.m_OutputDims.y;
    const sp::Pixel at = sp::pixel<kSigmaTile, kSigmaTile>();
    bool lit = false, occ = false;
    if (at.inside(W, H)) {
        const uint64_t i = at.index(W);
        const uint32_t pw = a.penumbra[i];
        const float P = half0(pw);
        uint32_t word = kOneWord | kNoOccluderWord << 16;
        if (!isSky(a.lvd[i], a.k.m_DenoisingRange)) {
            occ = P < kNoOccluder;
            lit = !occ;
            word = (occ ? 0u : kOneWord) | sp::halfBits(P) << 16;
        }
        a.data[i] = word;
    }
    const uint32_t t = threadIdx.y * kSigmaTile + threadIdx.x;
    const unsigned long long anyLit = __ballot(lit), anyOcc = __ballot(occ);
    if ((t & 63u) == 0u) waveBits[t >> 6] = (anyLit ? 1u : 0u) | (anyOcc ? 2u : 0u);
    __syncthreads();
    if (t == 0u) {                                 // one plain store per tile by one lane
        uint32_t bits = 0;
#pragma unroll
        for (uint32_t w = 0; w < kSigmaTile * kSigmaTile / 64u; ++w) bits |= waveBits[w];
        a.tiles[(uint64_t)blockIdx.y * a.tw + blockIdx.x] = (uint8_t)bits;
    }
}

// ---- "SIGMA_Shadow_Blur.cs", "SIGMA_Shadow_PostBlur.cs" -------------------------------------------------------------------------------
struct BlurArgs
{
    const uint32_t* in;                        // t0 RG16_FLOAT: x in the low half
    const uint16_t* lvd;                       // t1 R16_FLOAT
    const float* depth;                        // t2 R32_FLOAT
    const uint32_t* normalRoughness;           // t3 R10G10B10A2_UNORM
    const uint8_t* tiles;                      // t4 R8_UINT
    uint32_t* out;                             // u0 RG16_FLOAT
    uint32_t tw, th;
    SigmaConsts k;
};

__device__ __forceinline__ F3 decodeNormal(uint32_t w)
{
    const float fx = cm::div_((float)(w & 1023u), 1023.0f) * 2.0f - 1.0f, fy = cm::div_((float)((w >> 10) & 1023u), 1023.0f) * 2.0f - 1.0f;
    F3 n = { fx, fy, (1.0f - __builtin_fabsf(fx)) - __builtin_fabsf(fy) };
    const float t = sp::saturate_(-n.z);
    n.x += n.x >= 0.0f ? -t : t;
    n.y += n.y >= 0.0f ? -t : t;
    return gbuf::normalize_(n);
}

__device__ __forceinline__ float planeWeight(F3 Nc, F3 Xc, F3 Xq, float denom)
{
#ifdef TR_SIGMA_MUTATE_PLANE                   // negative control only: every tap counts fully
    return 1.0f;
#else
    const F3 d = { Xq.x - Xc.x, Xq.y - Xc.y, Xq.z - Xc.z };
    return cm::max_(0.0f, 1.0f - cm::div_(__builtin_fabsf(cm::dot3(Nc, d)), denom));
#endif
}

__global__ __launch_bounds__(sp::kBlock) void sigmaBlurKernel(BlurArgs a)
{
    const SigmaConsts& k = a.k;
    const uint32_t W = k.m_OutputDims.x, H = k.m_OutputDims.y;
    const sp::Pixel at = sp::pixel();
    if (!at.inside(W, H)) return;
    const uint32_t px = at.x, py = at.y;
    const uint64_t i = at.index(W);
    const uint32_t own = a.in[i], zw = a.lvd[i];
    if (isSky(zw, k.m_DenoisingRange) || !filteredTile(a.tiles, a.tw, a.th, px / kSigmaTile, py / kSigmaTile)) { a.out[i] = own; return; }
    const float x = half0(own), y = half1(own), zc = half0(zw);
    const F3 Xc = sp::worldPosition(k.m_ClipToWorld, px, py, W, H, a.depth[i]), Nc = decodeNormal(a.normalRoughness[i]);
    const float denom = k.m_PlaneDistanceSensitivity * zc;
    float r;
    if (k.m_Pass == 0u) {
        float sumW = 0.0f, sumR = 0.0f;
        for (int dy = -2; dy <= 2; ++dy)
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = (int)px + dx, qy = (int)py + dy;
                if (qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)H) continue;
                const uint64_t q = (uint64_t)qy * W + (uint32_t)qx;
                const float yq = half1(a.in[q]);
                if (isSky(a.lvd[q], k.m_DenoisingRange) || !(yq < kNoOccluder)) continue;
                const float w = planeWeight(Nc, Xc, sp::worldPosition(k.m_ClipToWorld, (uint32_t)qx, (uint32_t)qy, W, H, a.depth[q]), denom);
                sumW = sumW + w;
                sumR = sumR + w * yq;
            }
        if (!(sumW > 0.0f)) { a.out[i] = (own & 0xFFFFu) | kNoOccluderWord << 16; return; }
        r = cm::div_(sumR, sumW);
    } else {
        if (!(y < kNoOccluder)) { a.out[i] = own; return; }
        r = y * kPostBlurRadiusScale;
    }
#ifdef TR_SIGMA_MUTATE_RADIUS_CAP              // negative control only: the radius is not capped at the tile's side (a tap outside the image is still skipped)
    const float rpx = cm::div_(r, zc * k.m_PixelUnproject);
#else
    const float rpx = cm::min_(cm::div_(r, zc * k.m_PixelUnproject), kMaxBlurRadius);
#endif
    const uint32_t rot = (((px & 3u) | (py & 3u) << 2) + k.m_FrameIndex + 5u * k.m_Pass) & 15u;
    const float c = kRotation[rot][0], s = kRotation[rot][1];
    float sum = x, wsum = 1.0f;
    for (int t = 0; t < 8; ++t) {
        const float p0 = kPoisson[t][0], p1 = kPoisson[t][1];
        const float ox = (c * p0 - s * p1) * rpx, oy = (s * p0 + c * p1) * rpx;
        const float fx = __builtin_floorf(((float)px + 0.5f) + ox), fy = __builtin_floorf(((float)py + 0.5f) + oy);
        if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) continue;
        const uint32_t qx = (uint32_t)fx, qy = (uint32_t)fy;
        const uint64_t q = (uint64_t)qy * W + qx;
        if (isSky(a.lvd[q], k.m_DenoisingRange)) continue;
        const float w = planeWeight(Nc, Xc, sp::worldPosition(k.m_ClipToWorld, qx, qy, W, H, a.depth[q]), denom);
        sum = sum + w * half0(a.in[q]);
        wsum = wsum + w;
    }
    a.out[i] = sp::halfBits(cm::div_(sum, wsum)) | (k.m_Pass == 0u ? sp::halfBits(r) : (own >> 16)) << 16;
}

// ---- "SIGMA_Shadow_TemporalStabilization.cs" --------------------------------------------------------------------------------------------
struct StabilizeArgs
{
    const uint32_t* in;                        // t0 RG16_FLOAT
    const uint16_t* lvd;                       // t1 R16_FLOAT
    const uint32_t* motion;                    // t2 RG16_FLOAT
    const uint16_t* history;                   // t3 R16_FLOAT
    const uint8_t* tiles;                      // t4 R8_UINT
    uint16_t* newHistory;                      // u0 R16_FLOAT
    uint8_t* mask;                             // u1 R8_UNORM
    uint32_t tw, th;
    SigmaConsts k;
};

__device__ __forceinline__ uint32_t clampedAt(uint32_t p, int d, uint32_t dim) { return d < 0 ? (p > 0u ? p - 1u : 0u) : d > 0 ? (p + 1u < dim ? p + 1u : dim - 1u) : p; }

__global__ __launch_bounds__(sp::kBlock) void sigmaStabilizeKernel(StabilizeArgs a)
{
    const SigmaConsts& k = a.k;
    const uint32_t W = k.m_OutputDims.x, H = k.m_OutputDims.y;
    const sp::Pixel at = sp::pixel();
    if (!at.inside(W, H)) return;
    const uint32_t px = at.x, py = at.y;
    const uint64_t i = at.index(W);
    if (isSky(a.lvd[i], k.m_DenoisingRange)) { a.newHistory[i] = (uint16_t)kOneWord; a.mask[i] = 255u; return; }
    const uint32_t own = a.in[i];
    const float x = half0(own), y = half1(own);
    float out = x;
    if (y > 0.0f && y < kNoOccluder && filteredTile(a.tiles, a.tw, a.th, px / kSigmaTile, py / kSigmaTile)) {
        float m1 = 0.0f, m2 = 0.0f, n = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const uint64_t q = (uint64_t)clampedAt(py, dy, H) * W + clampedAt(px, dx, W);
                if (isSky(a.lvd[q], k.m_DenoisingRange)) continue;
                const float v = half0(a.in[q]);
                m1 = m1 + v; m2 = m2 + v * v; n = n + 1.0f;
            }
        const float mean = cm::div_(m1, n), sd = cm::sqrt_(cm::max_(cm::div_(m2, n) - mean * mean, 0.0f));
        const uint32_t mw = a.motion[i];
#ifdef TR_SIGMA_MUTATE_JITTER                  // negative control only: the jitter delta is not taken out
        const float hx = ((float)px + 0.5f) + half0(mw), hy = ((float)py + 0.5f) + half1(mw);
#else
        const float hx = (((float)px + 0.5f) + half0(mw)) - k.m_JitterDelta.x, hy = (((float)py + 0.5f) + half1(mw)) - k.m_JitterDelta.y;
#endif
        if (k.m_bResetHistory == 0u && hx >= 0.0f && hx < (float)W && hy >= 0.0f && hy < (float)H) {
            const sp::Axis ax = sp::axisOf(cm::div_(hx, (float)W), W), ay = sp::axisOf(cm::div_(hy, (float)H), H);
            const float t00 = half0(a.history[(uint64_t)ay.i0 * W + ax.i0]), t10 = half0(a.history[(uint64_t)ay.i0 * W + ax.i1]);
            const float t01 = half0(a.history[(uint64_t)ay.i1 * W + ax.i0]), t11 = half0(a.history[(uint64_t)ay.i1 * W + ax.i1]);
            const float f = sp::lerp_(sp::lerp_(t00, t10, ax.f), sp::lerp_(t01, t11, ax.f), ay.f);
            if (finite_(f)) {
#ifdef TR_SIGMA_MUTATE_CLAMP                   // negative control only: the history is taken as fetched
                const float h = f;
#else
                const float h = cm::min_(cm::max_(f, mean - k.m_SigmaScale * sd), mean + k.m_SigmaScale * sd);
#endif
                out = sp::lerp_(x, h, k.m_StabilizationStrength);
            }
        }
    }
    a.newHistory[i] = (uint16_t)sp::halfBits(out);
    a.mask[i] = (uint8_t)(uint32_t)(sp::saturate_(out) * 255.0f + 0.5f);
}

// ---- record side -----------------------------------------------------------------------------------------------------------------
const SigmaConsts* sigmaConsts(trhip::DispatchCtx& ctx, uint32_t groupSide, uint32_t& W, uint32_t& H, int& rc)
{
    const char* name = ctx.shaderName;
    rc = TRHIP_ERR_INVALID;
    const SigmaConsts* k = (const SigmaConsts*)ctx.constants(0, sizeof(SigmaConsts));
    if (!k) { trhip::fail(TRHIP_ERR_INVALID, "%s: b0 or push constants (SigmaConsts, 112 bytes) missing", name); return nullptr; }
    W = k->m_OutputDims.x; H = k->m_OutputDims.y;
    if (!W || !H) { trhip::fail(TRHIP_ERR_INVALID, "%s: m_OutputDims %ux%u is empty", name, W, H); return nullptr; }
    rc = sp::requireCover(ctx, groupSide, groupSide, W, H);
    return rc == TRHIP_OK ? k : nullptr;
}

int bindTiles(trhip::DispatchCtx& ctx, uint32_t type, uint32_t slot, uint32_t W, uint32_t H, trhip_texture_t*& tiles)
{
    const sp::Binding want[] = { { type, slot, TRHIP_FORMAT_R8_UINT, type == TRHIP_BIND_TEXTURE_UAV ? "Texture_UAV u0 = the R8_UINT tile texture (one mip)" : "Texture_SRV t4 = the R8_UINT tile texture (one mip)", true, sp::kOneMipAt0 } };
    trhip_texture_t* tex[1];
    if (const int rc = sp::bindTextures(ctx, want, tex, (W + kSigmaTile - 1u) / kSigmaTile, (H + kSigmaTile - 1u) / kSigmaTile, "ceil(m_OutputDims / 16)")) return rc;
    tiles = tex[0];
    return TRHIP_OK;
}

int recordClassify(trhip::DispatchCtx& ctx)
{
    uint32_t W, H; int rc;
    const SigmaConsts* k = sigmaConsts(ctx, kSigmaTile, W, H, rc);
    if (!k) return rc;
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_R16_FLOAT, "Texture_SRV t0 = the R16_FLOAT shadow penumbra texture", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 1, TRHIP_FORMAT_R16_FLOAT, "Texture_SRV t1 = the R16_FLOAT linear view depth", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_UAV, 1, TRHIP_FORMAT_RG16_FLOAT, "Texture_UAV u1 = the RG16_FLOAT shadow data (one mip)", true, sp::kOneMipAt0 } };
    trhip_texture_t *tex[3], *tiles;
    if (const int e = sp::bindTextures(ctx, want, tex, W, H, "m_OutputDims")) return e;
    if (const int e = bindTiles(ctx, TRHIP_BIND_TEXTURE_UAV, 0, W, H, tiles)) return e;
    ClassifyArgs a = sp::zeroed<ClassifyArgs>();
    a.penumbra = (const uint16_t*)tex[0]->ptr; a.lvd = (const uint16_t*)tex[1]->ptr; a.tiles = (uint8_t*)tiles->ptr; a.data = (uint32_t*)tex[2]->ptr;
    a.tw = tiles->width; a.k = *k;
    sp::launch(ctx, sigmaClassifyKernel, "sigmaClassifyKernel", sp::tiles(W, H, kSigmaTile, kSigmaTile), dim3(kSigmaTile, kSigmaTile), a);
    return TRHIP_OK;
}

int recordBlur(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    uint32_t W, H; int rc;
    const SigmaConsts* k = sigmaConsts(ctx, sp::kGroupSide, W, H, rc);
    if (!k) return rc;
    TRHIP_REQUIRE(k->m_Pass == (uint32_t)ctx.variant, "%s: m_Pass is %u: this entry is pass %d (SIGMA_Shadow_Blur.cs: 0, SIGMA_Shadow_PostBlur.cs: 1)", name, k->m_Pass, ctx.variant);
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_RG16_FLOAT, "Texture_SRV t0 = the RG16_FLOAT shadow data to read", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 1, TRHIP_FORMAT_R16_FLOAT, "Texture_SRV t1 = the R16_FLOAT linear view depth", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 2, TRHIP_FORMAT_R32_FLOAT, "Texture_SRV t2 = the R32_FLOAT depth texture", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 3, TRHIP_FORMAT_R10G10B10A2_UNORM, "Texture_SRV t3 = the R10G10B10A2_UNORM normal roughness texture", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_RG16_FLOAT, "Texture_UAV u0 = the RG16_FLOAT shadow data to write (one mip)", true, sp::kOneMipAt0 } };
    trhip_texture_t *tex[5], *tiles;
    if (const int e = sp::bindTextures(ctx, want, tex, W, H, "m_OutputDims")) return e;
    if (const int e = bindTiles(ctx, TRHIP_BIND_TEXTURE_SRV, 4, W, H, tiles)) return e;
    TRHIP_REQUIRE(tex[0] != tex[4], "%s: t0 and u0 are the same texture '%s': the taps read the neighbours' shadow data", name, tex[0]->name.c_str());
    BlurArgs a = sp::zeroed<BlurArgs>();
    a.in = (const uint32_t*)tex[0]->ptr; a.lvd = (const uint16_t*)tex[1]->ptr; a.depth = (const float*)tex[2]->ptr; a.normalRoughness = (const uint32_t*)tex[3]->ptr;
    a.tiles = (const uint8_t*)tiles->ptr; a.out = (uint32_t*)tex[4]->ptr; a.tw = tiles->width; a.th = tiles->height; a.k = *k;
    sp::launch(ctx, sigmaBlurKernel, "sigmaBlurKernel", sp::tiles(W, H), dim3(sp::kTileW, sp::kTileH), a);
    return TRHIP_OK;
}

int recordStabilize(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    uint32_t W, H; int rc;
    const SigmaConsts* k = sigmaConsts(ctx, sp::kGroupSide, W, H, rc);
    if (!k) return rc;
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_RG16_FLOAT, "Texture_SRV t0 = the RG16_FLOAT shadow data", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 1, TRHIP_FORMAT_R16_FLOAT, "Texture_SRV t1 = the R16_FLOAT linear view depth", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 2, TRHIP_FORMAT_RG16_FLOAT, "Texture_SRV t2 = the RG16_FLOAT motion target", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 3, TRHIP_FORMAT_R16_FLOAT, "Texture_SRV t3 = the R16_FLOAT previous shadow history", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_R16_FLOAT, "Texture_UAV u0 = the R16_FLOAT new shadow history (one mip)", true, sp::kOneMipAt0 },
                                 { TRHIP_BIND_TEXTURE_UAV, 1, TRHIP_FORMAT_R8_UNORM, "Texture_UAV u1 = the R8_UNORM shadow mask (one mip)", true, sp::kOneMipAt0 } };
    trhip_texture_t *tex[6], *tiles;
    if (const int e = sp::bindTextures(ctx, want, tex, W, H, "m_OutputDims")) return e;
    if (const int e = bindTiles(ctx, TRHIP_BIND_TEXTURE_SRV, 4, W, H, tiles)) return e;
    TRHIP_REQUIRE(tex[3] != tex[4], "%s: t3 and u0 are the same texture '%s': the history is read at other texels than the one written", name, tex[3]->name.c_str());
    TRHIP_REQUIRE(tex[1] != tex[3] && tex[1] != tex[4], "%s: the linear view depth '%s' is bound as a history too", name, tex[1]->name.c_str());
    StabilizeArgs a = sp::zeroed<StabilizeArgs>();
    a.in = (const uint32_t*)tex[0]->ptr; a.lvd = (const uint16_t*)tex[1]->ptr; a.motion = (const uint32_t*)tex[2]->ptr; a.history = (const uint16_t*)tex[3]->ptr;
    a.tiles = (const uint8_t*)tiles->ptr; a.newHistory = (uint16_t*)tex[4]->ptr; a.mask = (uint8_t*)tex[5]->ptr; a.tw = tiles->width; a.th = tiles->height; a.k = *k;
    sp::launch(ctx, sigmaStabilizeKernel, "sigmaStabilizeKernel", sp::tiles(W, H), dim3(sp::kTileW, sp::kTileH), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("SIGMA_Shadow_ClassifyTiles.cs", recordClassify, 0);
trhip::ShaderRegistrar r1("SIGMA_Shadow_Blur.cs", recordBlur, 0);
trhip::ShaderRegistrar r2("SIGMA_Shadow_PostBlur.cs", recordBlur, 1);
trhip::ShaderRegistrar r3("SIGMA_Shadow_TemporalStabilization.cs", recordStabilize, 0);

} // namespace
