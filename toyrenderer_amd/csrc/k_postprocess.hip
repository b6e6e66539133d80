// k_postprocess.hip -- the two renderers between LightingOutput and the back buffer: "adaptluminance_CS_GenerateLuminanceHistogram"
// and "adaptluminance_CS_AdaptExposure" (source/AdaptLuminanceRenderer.cpp, source/shaders/adaptluminance.hlsl) and
// "postprocess_PS_PostProcess" (source/PostProcessRenderer.cpp, source/shaders/postprocess.hlsl: exposure, PBRNeutralToneMapping,
// LinearToSRGB).  Sky, TAA, AO, the shadow mask and DDGI stay out of scope; bloom enters as an optional input
// texture: the caller's, or the one k_bloom.hip generates (a mip chain, read at mip 0).
//
// CONVENTION (parity unpinned; restated in tests/postprocess_ref.c and DESIGN.md 3).  The shared part (binary32 rules, saturate,
// lerp, dot3) is stated in screen_pass.hip.h; min / max = fmin / fmax (a NaN operand is dropped).
//   load:     R11G11B10_FLOAT decoded exactly (r11g11b10.hip.h), subnormal, inf and NaN codes included;
//   RGBToLuminance: dot3(rgb, (0x1.b38cdap-3f, 0x1.6e2974p-1f, 0x1.279aaep-4f)): 0.212671, 0.715160, 0.072169 rounded once;
//   log2, exp2: software (soft_math.hip.h): log2Soft for x > 0, exp2Signed for either sign;
//   pow(x, 1 / 2.2f): x > 0 ? exp2Signed(0x1.d1745cp-2f * log2Soft(x)) : 0 (zero, negative and NaN give 0); the constant is
//             1.0f / 2.2f, one correctly rounded binary32 division of 1 by the rounded 2.2f.  An infinite x gives NaN (stored
//             as 0); the tone curve never produces one;
//   histogram bin: lum >= 0.005f ? uint(saturate((log2Soft(lum) - m_MinLogLuminance) * m_InverseLogLuminanceRange) * 254.0f + 1.0f)
//             : 0; a NaN luminance fails the test (bin 0), +inf gives bin 255;
//   CS_AdaptExposure: sum = the wrapping uint32 sum of count[i] * i; avg = (float)sum / fmax((float)m_NbPixels - (float)count[0],
//             1.0f) - 1.0f; lum = exp2Signed(((avg / 254.0f) * m_LogLuminanceRange) + m_MinLogLuminance); adapted = last +
//             (lum - last) * m_AdaptationSpeed, stored to u0[0]; u1 = m_MiddleGray / (adapted * (1.0f - m_MiddleGray));
//   PS_PostProcess: rgb = lerp(colour, bloom, m_BloomStrength) (unbound bloom: 0, 0, 0); sceneLuminance = m_ManualExposure, or
//             t1[0] when that is == 0.0f; rgb *= m_MiddleGray / sceneLuminance (a zero luminance gives +inf: a nonzero colour
//             becomes +inf, the curve turns it into NaN, a zero colour is NaN at once; either is stored as byte 0);
//   PBRNeutralToneMapping: literal-only subexpressions are folded in float64 and rounded once (DXC's literal-float rule):
//             startCompression = 0.8 - 0.04 = 0x1.851eb8p-1f, d = 1. - startCompression = 0x1.eb851ep-3f; d * d is the
//             binary32 product 0x1.d7dbf4p-5f; desaturation 0x1.333334p-3f.  x = min(r, min(g, b)); offset = x < 0.08f ?
//             x - (6.25f * x) * x : 0.04f; rgb -= offset; peak = max(r, max(g, b)); peak < startCompression returns; newPeak =
//             1.0f - (d * d) / ((peak + d) - startCompression); rgb *= newPeak / peak (one division, three products);
//             g = 1.0f - 1.0f / (desaturation * (peak - newPeak) + 1.0f); lerp(rgb, newPeak, g);
//   store:    RGBA8_UNORM, each channel uint(saturate(c) * 255.0f + 0.5f) (D3D's float -> UNORM: a NaN gives 0), R in the low
//             byte, alpha 255.  Every texel is written.
//
// KERNELS.  Histogram: the reference's shape (one 16 x 16 group per tile, 256 global adds each) makes 8.3 M same-address
// global atomics for a 3840 x 2160 image.  Here a fixed grid of kHistGroupsPerCU workgroups per CU walks the image as a linear
// array of 16-byte vectors (4 texels per lane and trip; rows need no alignment; the last W * H mod 4 texels are taken by the
// first lanes of workgroup 0); bins accumulate in one LDS histogram per workgroup with no-return adds, a run of neighbouring
// lanes with the same bin adding once (its length, from its first lane: one shuffle and one ballot), and each workgroup ends
// with one no-return global add per nonzero bin.  Counts are integers: every design gives the same words.
// AdaptExposure: one 256-thread workgroup, the reference's LDS tree; thread 0 does the float arithmetic.  PostProcess: one
// thread per pixel in screen_pass.hip.h's tile, 4-byte loads of colour and bloom, one 4-byte store, no LDS.
//
// CODE OBJECT (-Rpass-analysis=kernel-resource-usage): histogramKernel 23 VGPRs, 1024 B LDS; adaptExposureKernel 8 VGPRs, 1024 B
// LDS; postProcessKernel 12 VGPRs, no LDS; each 8 waves per SIMD, no scratch.
//
// MEASURED (tools/postprocess_cost.py, generated city of 2251 instances at 3840 x 2160, 206 bins used, the largest holding 3.13 M of
// the 8.29 M pixels; builds alternated three times on one MI355X, median and spread; profiles/postprocess/).  Histogram: the
// reference's shape 609.7 us (0.4); the fixed grid with a sub-histogram per wave 36.5 (0.7), with one histogram per workgroup 36.4
// (0.8), per wave with merged lanes 34.4 (0.4), one histogram with merged lanes 34.4 (0.2).  On an image of one value: 609.5, 34.2,
// 34.1, 26.2, 26.0.  So the fixed grid stays (17 times faster); merging lanes wins by 2 us on the city and 8 us on one value, more
// than any spread; private sub-histograms change nothing within the spread on either image, so the simpler single histogram stays.
// Its 33 MB alone would stream in 5.1 us at the box's 6.48 TB/s: the pass is the arithmetic of 8.3 M software log2.
// AdaptExposure 6.4 us (0.1), a launch.  PostProcess 39.1 us (0.3) against 10.2 us for its 66 MB and 15.6 us (0.7) for a build that
// only loads and stores; with bloom bound 44.9 (0.3) against 15.4 us for 100 MB and 23.9 (0.5) store-only: three pow and four
// correctly rounded divisions per pixel are 21-23 us.  Negative controls: the hardware's v_log_f32 / v_exp_f32 change 71 of the
// city frame's 8 294 400 back-buffer words and no histogram bin, and 4 of the 19 GPU tests fail; truncation in the store changes
// 4 255 129 words and 9 tests fail.
#include "cull_math.hip.h"
#include "r11g11b10.hip.h"
#include "screen_pass.hip.h"
#include "soft_math.hip.h"

namespace
{

using namespace interop;

constexpr uint32_t kBlock = 256;                                          // the histogram's and the adapt pass's workgroup
constexpr uint32_t kHistGroupSide = 16;                                   // the histogram entry's [numthreads(16, 16, 1)]: group counts cover the image
constexpr uint32_t kHistGroupsPerCU = 4;                                  // a 3840 x 2160 image: 8100 vector trips over 1024 workgroups
constexpr uint32_t kHistTexelsPerLane = 4, kHistWaves = kBlock / 64, kBins = 256;
// The two answers to same-address LDS adds within a wave.  The defaults are the product: merged lanes measured faster, private
// sub-histograms did not (MEASURED above); the other combinations are cost comparisons only (profiles/postprocess/).
#ifndef TR_HISTOGRAM_PER_WAVE
#define TR_HISTOGRAM_PER_WAVE 0                 // 1: a private sub-histogram per wave; 0: one histogram per workgroup
#endif
#ifndef TR_HISTOGRAM_MERGE_LANES
#define TR_HISTOGRAM_MERGE_LANES 1              // 1: equal bins of neighbouring lanes are merged into one add
#endif
constexpr bool kHistPerWave = TR_HISTOGRAM_PER_WAVE != 0, kHistMergeLanes = TR_HISTOGRAM_MERGE_LANES != 0;

__device__ __forceinline__ float luminance(uint32_t word)
{
    const trhip::Rgb c = trhip::unpackR11G11B10(word);
    return cm::dot3({ c.r, c.g, c.b }, { 0x1.b38cdap-3f, 0x1.6e2974p-1f, 0x1.279aaep-4f });
}

__device__ __forceinline__ uint32_t histogramBin(uint32_t word, float minLog, float invRange)   // adaptluminance.hlsl:23-37
{
    const float lum = luminance(word);
    if (!(lum >= 0.005f)) return 0u;
    const float logLum = sp::saturate_((softmath::log2Soft(lum) - minLog) * invRange);
    return (uint32_t)(logLum * 254.0f + 1.0f);
}

struct HistogramArgs
{
    const uint32_t* color;                     // R11G11B10_FLOAT, W * H words
    uint32_t* histogram;                       // 256 words, added to
    uint64_t texels;
    float minLog, invRange;
    uint32_t width, height;
};

#ifdef TR_HISTOGRAM_EXPERIMENT_REFERENCE_SHAPE  // cost comparison only (profiles/postprocess/): one 16 x 16 group per tile, 256 global adds each
__global__ __launch_bounds__(kBlock) void histogramKernel(HistogramArgs a)
{
    __shared__ uint32_t bins[kBins];
    const uint32_t t = threadIdx.y * kHistGroupSide + threadIdx.x;
    bins[t] = 0u;
    __syncthreads();
    const sp::Pixel at = sp::pixel<kHistGroupSide, kHistGroupSide>();
    if (at.inside(a.width, a.height)) atomicAdd(&bins[histogramBin(a.color[at.index(a.width)], a.minLog, a.invRange)], 1u);
    __syncthreads();
    atomicAdd(&a.histogram[t], bins[t]);
}
#else
// One count into the LDS histogram `mine`, from every lane of a full wave (lanes without a texel pass valid = false).  With
// kHistMergeLanes a run of neighbouring lanes with the same bin adds once, its length, from its first lane.
__device__ __forceinline__ void addBin(uint32_t* mine, uint32_t bin, bool valid)
{
    if constexpr (kHistMergeLanes) {
        const uint32_t lane = threadIdx.x & 63u, key = valid ? bin : 0xFFFFFFFFu;
        const uint32_t before = __shfl_up(key, 1);
        const bool head = lane == 0u || before != key;
        const uint64_t heads = __ballot(head), after = lane == 63u ? 0ull : heads >> (lane + 1u);
        const uint32_t length = after ? (uint32_t)__builtin_ctzll(after) + 1u : 64u - lane;
        if (head && valid) atomicAdd(&mine[bin], length);
    } else if (valid) {
        atomicAdd(&mine[bin], 1u);
    }
}

__global__ __launch_bounds__(kBlock) void histogramKernel(HistogramArgs a)
{
    constexpr uint32_t kCopies = kHistPerWave ? kHistWaves : 1u;
    __shared__ uint32_t bins[kCopies * kBins];
    uint32_t* mine = bins + (kHistPerWave ? threadIdx.x / 64u : 0u) * kBins;
    for (uint32_t w = 0; w < kCopies; ++w) bins[w * kBins + threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t vectors = a.texels / kHistTexelsPerLane, stride = (uint64_t)gridDim.x * kBlock;
    const uint4* color4 = (const uint4*)a.color;                           // the texture's memory is 256-byte aligned
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < vectors; base += stride) {   // uniform over the workgroup: addBin needs whole waves
        const uint64_t v = base + threadIdx.x;
        const bool valid = v < vectors;
        const uint4 w = valid ? color4[v] : uint4{ 0u, 0u, 0u, 0u };
        addBin(mine, histogramBin(w.x, a.minLog, a.invRange), valid);
        addBin(mine, histogramBin(w.y, a.minLog, a.invRange), valid);
        addBin(mine, histogramBin(w.z, a.minLog, a.invRange), valid);
        addBin(mine, histogramBin(w.w, a.minLog, a.invRange), valid);
    }
    const uint64_t tail = vectors * kHistTexelsPerLane + threadIdx.x;     // the last W * H mod 4 texels, by the first lanes of workgroup 0
    if (blockIdx.x == 0) {
        const bool valid = tail < a.texels;
        addBin(mine, valid ? histogramBin(a.color[tail], a.minLog, a.invRange) : 0u, valid);
    }
    __syncthreads();
    uint32_t n = 0;
    for (uint32_t w = 0; w < kCopies; ++w) n += bins[w * kBins + threadIdx.x];
    if (n) atomicAdd(&a.histogram[threadIdx.x], n);
}
#endif

int recordHistogram(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const GenerateLuminanceHistogramParameters* k = (const GenerateLuminanceHistogramParameters*)ctx.constants(0, sizeof(GenerateLuminanceHistogramParameters));
    TRHIP_REQUIRE(k, "%s: push constants (GenerateLuminanceHistogramParameters, 16 bytes) missing", name);
    const uint32_t W = k->m_SrcColorDims.x, H = k->m_SrcColorDims.y;
    TRHIP_REQUIRE(W && H, "%s: m_SrcColorDims %ux%u is empty", name, W, H);
    if (const int rc = sp::requireCover(ctx, kHistGroupSide, kHistGroupSide, W, H)) return rc;
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_R11G11B10_FLOAT, "Texture_SRV t0 = the R11G11B10_FLOAT colour", true, sp::kOneMip } };
    trhip_texture_t* color[1];
    if (const int rc = sp::bindTextures(ctx, want, color, W, H, "m_SrcColorDims")) return rc;
    trhip_buffer_t* hist = ctx.buffer(TRHIP_BIND_STRUCTURED_UAV, 0);
    TRHIP_REQUIRE(hist && hist->byteSize >= kBins * 4, "%s: needs StructuredBuffer_UAV u0 = the histogram of at least 256 uint32", name);
    HistogramArgs a = sp::zeroed<HistogramArgs>();
    a.color = (const uint32_t*)color[0]->ptr;
    a.histogram = (uint32_t*)hist->ptr;
    a.texels = (uint64_t)W * H;
    a.minLog = k->m_MinLogLuminance; a.invRange = k->m_InverseLogLuminanceRange;
    a.width = W; a.height = H;
#ifdef TR_HISTOGRAM_EXPERIMENT_REFERENCE_SHAPE
    const dim3 grid = sp::tiles(W, H, kHistGroupSide, kHistGroupSide), block(kHistGroupSide, kHistGroupSide);
#else
    const uint64_t trips = (a.texels / kHistTexelsPerLane + kBlock - 1) / kBlock, most = (uint64_t)ctx.computeUnits() * kHistGroupsPerCU;
    const dim3 grid((uint32_t)(trips < 1 ? 1 : trips < most ? trips : most)), block(kBlock);
#endif
    sp::launch(ctx, histogramKernel, "histogramKernel", grid, block, a);
    return TRHIP_OK;
}

struct AdaptArgs
{
    AdaptExposureParameters k;
    const uint32_t* histogram;
    float* luminance;                          // one float, read and written
    float* exposure;                           // the 1 x 1 R32_FLOAT texel
};

__global__ __launch_bounds__(kBlock) void adaptExposureKernel(AdaptArgs a)                    // adaptluminance.hlsl:58-96
{
    __shared__ uint32_t weighted[kBins];
    const uint32_t t = threadIdx.x, count = a.histogram[t];
    weighted[t] = count * t;
    __syncthreads();
    for (uint32_t half = kBins >> 1; half > 0; half >>= 1) {
        if (t < half) weighted[t] += weighted[t + half];
        __syncthreads();
    }
    if (t != 0) return;
    const float avg = cm::div_((float)weighted[0], cm::max_((float)a.k.m_NbPixels - (float)count, 1.0f)) - 1.0f;
    const float lum = softmath::exp2Signed((cm::div_(avg, 254.0f) * a.k.m_LogLuminanceRange) + a.k.m_MinLogLuminance);
    const float last = a.luminance[0], adapted = last + (lum - last) * a.k.m_AdaptationSpeed;
    a.luminance[0] = adapted;
    a.exposure[0] = cm::div_(a.k.m_MiddleGray, adapted * (1.0f - a.k.m_MiddleGray));
}

int recordAdaptExposure(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const AdaptExposureParameters* k = (const AdaptExposureParameters*)ctx.constants(0, sizeof(AdaptExposureParameters));
    TRHIP_REQUIRE(k, "%s: push constants (AdaptExposureParameters, 20 bytes) missing", name);
    TRHIP_REQUIRE(!ctx.indirect && ctx.gx == 1 && ctx.gy == 1 && ctx.gz == 1, "%s: needs a direct dispatch of (1, 1, 1)", name);
    trhip_buffer_t* hist = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 0);
    TRHIP_REQUIRE(hist && hist->byteSize >= kBins * 4, "%s: needs StructuredBuffer_SRV t0 = the histogram of at least 256 uint32", name);
    trhip_buffer_t* lum = ctx.buffer(TRHIP_BIND_STRUCTURED_UAV, 0);
    TRHIP_REQUIRE(lum && lum->byteSize >= 4, "%s: needs StructuredBuffer_UAV u0 = the luminance buffer of one float", name);
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_UAV, 1, TRHIP_FORMAT_R32_FLOAT, "Texture_UAV u1 = the R32_FLOAT exposure texture, mip 0", true, sp::kAt0 } };
    trhip_texture_t* exposure[1];
    if (const int rc = sp::bindTextures(ctx, want, exposure, 1, 1, "the exposure texture")) return rc;
    AdaptArgs a = sp::zeroed<AdaptArgs>();
    a.k = *k;
    a.histogram = (const uint32_t*)hist->ptr;
    a.luminance = (float*)lum->ptr;
    a.exposure = (float*)exposure[0]->ptr;
    sp::launch(ctx, adaptExposureKernel, "adaptExposureKernel", dim3(1), dim3(kBlock), a);
    return TRHIP_OK;
}

struct PostArgs
{
    PostProcessParameters k;
    const uint32_t* color;                     // R11G11B10_FLOAT
    const float* luminance;                    // one float, or nullptr with a manual exposure
    const uint32_t* bloom;                     // R11G11B10_FLOAT or nullptr (0, 0, 0)
    uint32_t* out;                             // RGBA8_UNORM
};

__device__ __forceinline__ float powGamma(float x) { return x > 0.0f ? softmath::exp2Signed(0x1.d1745cp-2f * softmath::log2Soft(x)) : 0.0f; }

__device__ __forceinline__ uint32_t unorm8(float c)
{
#ifdef TR_POST_EXPERIMENT_TRUNC_STORE          // negative control only (profiles/postprocess/): truncation instead of + 0.5f
    return (uint32_t)(sp::saturate_(c) * 255.0f);
#else
    return (uint32_t)(sp::saturate_(c) * 255.0f + 0.5f);
#endif
}

__device__ __forceinline__ cm::F3 pbrNeutralToneMapping(cm::F3 c)                              // postprocess.hlsl:23-42
{
    const float startCompression = 0x1.851eb8p-1f, d = 0x1.eb851ep-3f, desaturation = 0x1.333334p-3f;
    const float x = cm::min_(c.x, cm::min_(c.y, c.z));
    const float offset = x < 0.08f ? x - (6.25f * x) * x : 0.04f;
    c = { c.x - offset, c.y - offset, c.z - offset };
    const float peak = cm::max_(c.x, cm::max_(c.y, c.z));
    if (peak < startCompression) return c;
    const float newPeak = 1.0f - cm::div_(d * d, (peak + d) - startCompression);
    const float ratio = cm::div_(newPeak, peak);
    c = { c.x * ratio, c.y * ratio, c.z * ratio };
    const float g = 1.0f - cm::div_(1.0f, desaturation * (peak - newPeak) + 1.0f);
    return { c.x + g * (newPeak - c.x), c.y + g * (newPeak - c.y), c.z + g * (newPeak - c.z) };
}

__global__ __launch_bounds__(sp::kBlock) void postProcessKernel(PostArgs a)                       // postprocess.hlsl:44-69
{
    const uint32_t W = a.k.m_OutputDims.x, H = a.k.m_OutputDims.y;
    const sp::Pixel at = sp::pixel();
    if (!at.inside(W, H)) return;
    const uint64_t i = at.index(W);
    const uint32_t word = a.color[i], bloomWord = a.bloom ? a.bloom[i] : 0u;
#ifdef TR_POST_EXPERIMENT_STORE_ONLY            // attribution only (profiles/postprocess/): the pass's bytes without its arithmetic
    a.out[i] = word ^ bloomWord;
#else
    const trhip::Rgb c = trhip::unpackR11G11B10(word), b = trhip::unpackR11G11B10(bloomWord);
    const float s = a.k.m_BloomStrength;
    cm::F3 rgb = { c.r + s * (b.r - c.r), c.g + s * (b.g - c.g), c.b + s * (b.b - c.b) };
    float sceneLuminance = a.k.m_ManualExposure;
    if (sceneLuminance == 0.0f) sceneLuminance = a.luminance[0];
    const float lumScale = cm::div_(a.k.m_MiddleGray, sceneLuminance);
    rgb = pbrNeutralToneMapping({ rgb.x * lumScale, rgb.y * lumScale, rgb.z * lumScale });
    a.out[i] = unorm8(powGamma(rgb.x)) | unorm8(powGamma(rgb.y)) << 8 | unorm8(powGamma(rgb.z)) << 16 | 0xFF000000u;
#endif
}

int recordPostProcess(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const PostProcessParameters* k = (const PostProcessParameters*)ctx.constants(0, sizeof(PostProcessParameters));
    TRHIP_REQUIRE(k, "%s: b0 or push constants (PostProcessParameters, 24 bytes) missing", name);
    const uint32_t W = k->m_OutputDims.x, H = k->m_OutputDims.y;
    TRHIP_REQUIRE(W && H, "%s: m_OutputDims %ux%u is empty", name, W, H);
    if (const int rc = sp::requireCover(ctx, sp::kGroupSide, sp::kGroupSide, W, H)) return rc;
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_R11G11B10_FLOAT, "Texture_SRV t0 = the R11G11B10_FLOAT colour input", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_SRV, 2, TRHIP_FORMAT_R11G11B10_FLOAT, "Texture_SRV t2 = the R11G11B10_FLOAT bloom texture", false, sp::kOneMipOrAt0 },   // may be the bloom chain: mip 0 is read
                                 { TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_RGBA8_UNORM, "Texture_UAV u0 = the RGBA8_UNORM back buffer, mip 0", true, sp::kOneMipAt0 } };
    trhip_texture_t* tex[3];
    if (const int rc = sp::bindTextures(ctx, want, tex, W, H, "m_OutputDims")) return rc;
    trhip_buffer_t* lum = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 1);
    TRHIP_REQUIRE(!lum || lum->byteSize >= 4, "%s: StructuredBuffer_SRV t1 = the luminance buffer holds one float", name);
    TRHIP_REQUIRE(lum || k->m_ManualExposure != 0.0f, "%s: m_ManualExposure is 0: needs StructuredBuffer_SRV t1 = the luminance buffer", name);
    PostArgs a = sp::zeroed<PostArgs>();
    a.k = *k;
    a.color = (const uint32_t*)tex[0]->ptr;
    a.luminance = lum ? (const float*)lum->ptr : nullptr;
    a.bloom = tex[1] ? (const uint32_t*)tex[1]->ptr : nullptr;
    a.out = (uint32_t*)tex[2]->ptr;
    sp::launch(ctx, postProcessKernel, "postProcessKernel", sp::tiles(W, H), dim3(sp::kTileW, sp::kTileH), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("adaptluminance_CS_GenerateLuminanceHistogram", recordHistogram, 0);
trhip::ShaderRegistrar r1("adaptluminance_CS_AdaptExposure", recordAdaptExposure, 0);
trhip::ShaderRegistrar r2("postprocess_PS_PostProcess", recordPostProcess, 0);

} // namespace
