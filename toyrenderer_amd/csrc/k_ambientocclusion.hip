// k_ambientocclusion.hip -- AmbientOcclusionRenderer's three compute passes (source/AmbientOcclusionRenderer.cpp,
// source/shaders/ambientocclusion.hlsl, extern/xegtao/XeGTAO.hlsli): "ambientocclusion_CS_XeGTAO_PrefilterDepths",
// "ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0" and "ambientocclusion_CS_XeGTAO_Denoise".  The texture they build is
// what "deferredlighting_PS_Main*" reads at t3 (k_deferredlighting.hip).  The configuration is the one the reference compiles:
// binary16 arithmetic (lpfloat = float16_t), 16-bit working depths, no bent normals, no debug output, the default constants
// compiled in (radius multiplier 1.457, falloff range 0.615, distribution power 2, thin-occluder compensation 0).
//
// BINDINGS, direct dispatches only; samplers are accepted and ignored.
//   prefilter: b0 = GTAOConstants (96 bytes), t0 = the R32_FLOAT depth, u0..u4 = mips 0..4 of ONE R16_FLOAT texture of 5 mips at
//              the depth's size; ceil(W / 16) x ceil(H / 16) groups of 8 x 8 threads, one 2 x 2 quad per thread.
//   main:      b0; b1 = push XeGTAOMainPassConstantBuffer (68 bytes); t0 = that chain, t2 = GBufferA (RGBA32_UINT), u0 = the working AO
//              term (R8_UINT), u1 = the edges (R8_UNORM); ceil(W / 8) x ceil(H / 8) groups, one pixel per thread.  The reference's t1,
//              a 64 x 64 R16_UINT table of Hilbert indices, is NOT bound: the index is computed (hilbertIndex below; same values,
//              checked for all 4096 entries in tests/test_gtao_ref.py).
//   denoise:   b0; b1 = push XeGTAODenoiseConstants (4 bytes); t0 = the AO term (R8_UINT), t1 = the edges, u0 = the output
//              (R8_UINT, not t0); ceil(W / 16) x ceil(H / 8) groups, two horizontal pixels per thread.
// A pass writes exactly the texels inside its targets' extents; a store outside a mip's extent is dropped.
//
// CONVENTION: tests/gtao_ref.c is the definition and this file follows it function by function.  In short: every
// lpfloat + - * is the IEEE binary16 operation, which here is the native instruction; / and sqrt are the binary32 operation on
// the exact values rounded once to binary16 (equal to the IEEE binary16 result as 24 >= 2 * 11 + 2; hipcc's own fp16 division is
// an approximation with a fix-up and is not used); nothing is contracted; composite operations are spelled out in source order;
// expression types follow HLSL; sin, cos, log2 and pow are softmath:: functions in binary32 rounded once; FastSqrt and FastACos are
// the reference's bit trick and polynomial.  A NaN never decides a word by its sign or payload: every NaN ends in a comparison,
// an fmin / fmax or toUint, which give the same on both sides.
//
// KERNELS.  One wave per group in all three, as the reference's [numthreads(8, 8, 1)].  The prefilter's mips 2..4 go through 128
// bytes of LDS like the reference's groupshared array.  The main pass is arithmetic: at Ultra 9 slices x 2 steps x 2 sides = 36
// depth fetches against about 60 software sines and cosines, 27 FastACos, and some 150 binary32 divisions and square roots per
// pixel; its fetches are 2-byte loads that neighbouring pixels share through L1 / L2.  Quality is wave-uniform, so the loops do not
// diverge.  -DTR_AO_EXPERIMENT_HW_TRIG (tools/ao_cost.py only, never the product, not bit-exact) replaces the software sine, cosine,
// log2 and exp2 by the hardware's approximations to show what exactness costs.  Code object and measurements: profiles/ao/README.md.
#include "cull_math.hip.h"
#include "screen_pass.hip.h"
#include "soft_math.hip.h"

namespace
{

using namespace interop;

typedef _Float16 hf;
struct H3 { hf x, y, z; };
struct H4 { hf x, y, z, w; };

constexpr uint32_t kAoGroup = 8;                                           // threads per side of a group, all three passes

__device__ __forceinline__ hf r16(float x) { return (hf)x; }
__device__ __forceinline__ hf hadd(hf a, hf b) { return a + b; }
__device__ __forceinline__ hf hsub(hf a, hf b) { return a - b; }
__device__ __forceinline__ hf hmul(hf a, hf b) { return a * b; }
// The compiler may not see that a binary32 operand came from a binary16 value: it would narrow the operation to binary16 again
// (fptrunc(fdiv(fpext, fpext)) is an fdiv of halves), whose lowering on this target goes through approximate reciprocals.
__device__ __forceinline__ float opaque(float x) { asm("" : "+v"(x)); return x; }
__device__ __forceinline__ hf hdiv(hf a, hf b) { return (hf)cm::div_(opaque((float)a), opaque((float)b)); }
__device__ __forceinline__ hf hsqrt(hf a) { return (hf)cm::sqrt_(opaque((float)a)); }
__device__ __forceinline__ hf hmin(hf a, hf b) { return (hf)cm::min_((float)a, (float)b); }
__device__ __forceinline__ hf hmax(hf a, hf b) { return (hf)cm::max_((float)a, (float)b); }
__device__ __forceinline__ hf hsat(hf a) { return (hf)cm::min_(cm::max_((float)a, 0.0f), 1.0f); }
__device__ __forceinline__ hf habs(hf a) { return (hf)__builtin_fabsf((float)a); }
__device__ __forceinline__ hf hrint(hf a) { return (hf)__builtin_rintf((float)a); }
__device__ __forceinline__ hf hfloor(hf a) { return (hf)__builtin_floorf((float)a); }
__device__ __forceinline__ hf hlerp(hf x, hf y, hf s) { return hadd(x, hmul(s, hsub(y, x))); }
__device__ __forceinline__ hf hdot2(hf ax, hf ay, hf bx, hf by) { return hadd(hmul(ax, bx), hmul(ay, by)); }
__device__ __forceinline__ hf hdot3(H3 a, H3 b) { return hadd(hadd(hmul(a.x, b.x), hmul(a.y, b.y)), hmul(a.z, b.z)); }
__device__ __forceinline__ hf hdot4(H4 a, H4 b) { return hadd(hadd(hadd(hmul(a.x, b.x), hmul(a.y, b.y)), hmul(a.z, b.z)), hmul(a.w, b.w)); }
__device__ __forceinline__ hf hlength3(H3 a) { return hsqrt(hdot3(a, a)); }
__device__ __forceinline__ H3 hnormalize3(H3 a) { const hf l = hlength3(a); return { hdiv(a.x, l), hdiv(a.y, l), hdiv(a.z, l) }; }
__device__ __forceinline__ H3 hcross(H3 a, H3 b)
{
    return { hsub(hmul(a.y, b.z), hmul(a.z, b.y)), hsub(hmul(a.z, b.x), hmul(a.x, b.z)), hsub(hmul(a.x, b.y), hmul(a.y, b.x)) };
}
__device__ __forceinline__ hf hsign(hf x) { return x > (hf)0.0f ? (hf)1.0f : x < (hf)0.0f ? (hf)-1.0f : (hf)0.0f; }
__device__ __forceinline__ uint32_t toUint(float x) { return !(x >= 0.0f) ? 0u : x >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)x; }
using sp::halfOf;

// the literals of XeGTAO.hlsli as binary16 (tests/gtao_ref.c has the same table)
constexpr hf H_PI = (hf)0x1.92p+1f, H_PI_HALF = (hf)0x1.92p+0f, H_GOLDEN = (hf)0x1.3c8p-1f, H_0_9992 = (hf)0x1.ff8p-1f, H_1_3 = (hf)0x1.4ccp+0f;
constexpr hf H_0_011 = (hf)0x1.688p-7f, H_2_9 = (hf)0x1.734p+1f, H_64_255 = (hf)0x1.01p-2f, H_16_255 = (hf)0x1.01p-4f, H_4_255 = (hf)0x1.01p-6f;
constexpr hf H_1_255 = (hf)0x1.01p-8f, H_ACOS_C = (hf)-0x1.40cp-3f, H_DIAG = (hf)0x1.b34p-2f, H_0_615 = (hf)0x1.3bp-1f, H_1_457 = (hf)0x1.75p+0f;
constexpr hf H_0_03 = (hf)0x1.eb8p-6f, H_0_05 = (hf)0x1.998p-5f;
constexpr hf H0 = (hf)0.0f, H1 = (hf)1.0f;

#ifdef TR_AO_EXPERIMENT_HW_TRIG                // negative control only (profiles/ao/): v_sin_f32, v_cos_f32, v_log_f32, v_exp_f32
__device__ __forceinline__ hf hsin(hf x) { return r16(__builtin_amdgcn_sinf((float)x * 0x1.45f306p-3f)); }
__device__ __forceinline__ hf hcos(hf x) { return r16(__builtin_amdgcn_cosf((float)x * 0x1.45f306p-3f)); }
__device__ __forceinline__ float log2_(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float exp2_(float x) { return __builtin_amdgcn_exp2f(x); }
#else
__device__ __forceinline__ hf hsin(hf x) { return r16(softmath::sinSoft((float)x)); }
__device__ __forceinline__ hf hcos(hf x) { return r16(softmath::cosSoft((float)x)); }
__device__ __forceinline__ float log2_(float x) { return softmath::log2Soft(x); }
__device__ __forceinline__ float exp2_(float x) { return softmath::exp2Signed(x); }
#endif
__device__ __forceinline__ hf hlog2(hf x) { return x > H0 ? r16(log2_((float)x)) : (hf)-__builtin_inff(); }
__device__ __forceinline__ hf hpow(hf v, hf p) { return v > H0 ? r16(exp2_((float)p * log2_((float)v))) : H0; }

__device__ __forceinline__ hf fastSqrt(float x)                            // XeGTAO_FastSqrt
{
    return r16(__builtin_bit_cast(float, 0x1FBD1DF5u + (uint32_t)(__builtin_bit_cast(int32_t, x) >> 1)));
}
__device__ __forceinline__ hf fastACos(hf inX)                             // XeGTAO_FastACos
{
    const hf x = habs(inX);
    hf res = hadd(hmul(H_ACOS_C, x), H_PI_HALF);
    res = hmul(res, fastSqrt((float)hsub(H1, x)));
    return inX >= H0 ? res : hsub(H_PI, res);
}

__device__ __forceinline__ uint32_t hilbertIndex(uint32_t x, uint32_t y)  // XeGTAO::HilbertIndex of (x, y) mod 64, branch-free
{
    uint32_t index = 0u;
    x &= 63u; y &= 63u;
#pragma unroll
    for (uint32_t level = 32u; level > 0u; level >>= 1) {
        const uint32_t rx = (x & level) != 0u, ry = (y & level) != 0u;
        index += level * level * ((3u * rx) ^ ry);
        const uint32_t flip = 63u * (rx & (ry ^ 1u));
        const uint32_t fx = x ^ flip, fy = y ^ flip;
        const uint32_t swap = (fx ^ fy) & (0u - (ry ^ 1u));
        x = fx ^ swap; y = fy ^ swap;
    }
    return index;
}

__device__ __forceinline__ uint32_t clampi(int32_t v, uint32_t dim) { return v < 0 ? 0u : (uint32_t)v >= dim ? dim - 1u : (uint32_t)v; }

struct DepthChain { const uint16_t* mip[5]; uint32_t w[5], h[5]; };

// ---- pass 1 ------------------------------------------------------------------------------------------------------------------
struct PrefilterArgs
{
    GTAOConstants k;
    const float* depth;                        // R32_FLOAT, W x H
    uint16_t* mip[5];                          // R16_FLOAT
    uint32_t w[5], h[5];
};

__device__ __forceinline__ hf viewDepth(float d, const GTAOConstants& k)
{
    return r16(cm::clamp_(cm::div_(k.DepthUnpackConsts.x, k.DepthUnpackConsts.y - d), 0.0f, 65504.0f));
}

__device__ __forceinline__ void falloffTerms(const GTAOConstants& k, hf effectRadius, hf& mul, hf& add)
{
    const hf falloffRange = hmul(H_0_615, effectRadius);
    const hf falloffFrom = hmul(effectRadius, hsub(H1, r16(k.EffectFalloffRange)));
    mul = hdiv((hf)-1.0f, falloffRange);
    add = hadd(hdiv(falloffFrom, falloffRange), H1);
}

__device__ __forceinline__ hf mipFilter(hf d0, hf d1, hf d2, hf d3, hf mul, hf add)
{
    const hf maxDepth = hmax(hmax(d0, d1), hmax(d2, d3));
    const hf w0 = hsat(hadd(hmul(hsub(maxDepth, d0), mul), add));
    const hf w1 = hsat(hadd(hmul(hsub(maxDepth, d1), mul), add));
    const hf w2 = hsat(hadd(hmul(hsub(maxDepth, d2), mul), add));
    const hf w3 = hsat(hadd(hmul(hsub(maxDepth, d3), mul), add));
    const hf weightSum = hadd(hadd(hadd(w0, w1), w2), w3);
    return hdiv(hadd(hadd(hadd(hmul(w0, d0), hmul(w1, d1)), hmul(w2, d2)), hmul(w3, d3)), weightSum);
}

__global__ __launch_bounds__(kAoGroup * kAoGroup) void aoPrefilterKernel(PrefilterArgs a)
{
    __shared__ hf scratch[8][8];
    const uint32_t tx = threadIdx.x, ty = threadIdx.y, bx = blockIdx.x * kAoGroup + tx, by = blockIdx.y * kAoGroup + ty, px = bx * 2u, py = by * 2u;   // one 2 x 2 quad per thread
    const uint32_t W = a.w[0], H = a.h[0];
    const uint32_t x0 = clampi((int32_t)px, W), x1 = clampi((int32_t)px + 1, W), y0 = clampi((int32_t)py, H), y1 = clampi((int32_t)py + 1, H);
    const hf d0 = viewDepth(a.depth[(uint64_t)y0 * W + x0], a.k), d1 = viewDepth(a.depth[(uint64_t)y0 * W + x1], a.k);
    const hf d2 = viewDepth(a.depth[(uint64_t)y1 * W + x0], a.k), d3 = viewDepth(a.depth[(uint64_t)y1 * W + x1], a.k);
    if (px < W && py < H) a.mip[0][(uint64_t)py * W + px] = sp::halfBits((float)d0);
    if (px + 1u < W && py < H) a.mip[0][(uint64_t)py * W + px + 1u] = sp::halfBits((float)d1);
    if (px < W && py + 1u < H) a.mip[0][(uint64_t)(py + 1u) * W + px] = sp::halfBits((float)d2);
    if (px + 1u < W && py + 1u < H) a.mip[0][(uint64_t)(py + 1u) * W + px + 1u] = sp::halfBits((float)d3);
    hf mul, add;                                                           // XeGTAO_DepthMIPFilter's uniform terms
    falloffTerms(a.k, hmul(hmul((hf)0.75f, r16(a.k.EffectRadius)), H_1_457), mul, add);
    const hf dm1 = mipFilter(d0, d1, d2, d3, mul, add);
    if (bx < a.w[1] && by < a.h[1]) a.mip[1][(uint64_t)by * a.w[1] + bx] = sp::halfBits((float)dm1);
    scratch[tx][ty] = dm1;
    __syncthreads();
#pragma unroll
    for (uint32_t level = 2; level <= 4; ++level) {
        const uint32_t step = 1u << (level - 1u), half = step >> 1;
        if ((tx & (step - 1u)) == 0u && (ty & (step - 1u)) == 0u) {
            const hf v = mipFilter(scratch[tx][ty], scratch[tx + half][ty], scratch[tx][ty + half], scratch[tx + half][ty + half], mul, add);
            const uint32_t ox = bx >> (level - 1u), oy = by >> (level - 1u);
            if (ox < a.w[level] && oy < a.h[level]) a.mip[level][(uint64_t)oy * a.w[level] + ox] = sp::halfBits((float)v);
            scratch[tx][ty] = v;
        }
        __syncthreads();
    }
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------------------
struct MainArgs
{
    GTAOConstants k;
    XeGTAOMainPassConstantBuffer push;
    DepthChain chain;
    const uint4* gbufferA;                     // RGBA32_UINT
    uint8_t* outAO;                            // R8_UINT
    uint8_t* outEdges;                         // R8_UNORM
};

__device__ __forceinline__ H4 calculateEdges(hf c, hf l, hf r, hf t, hf b)
{
    H4 e = { hsub(l, c), hsub(r, c), hsub(t, c), hsub(b, c) };
    const hf slopeLR = hmul(hsub(e.y, e.x), (hf)0.5f), slopeTB = hmul(hsub(e.w, e.z), (hf)0.5f);
    const H4 adj = { hadd(e.x, slopeLR), hadd(e.y, -slopeLR), hadd(e.z, slopeTB), hadd(e.w, -slopeTB) };
    e.x = hmin(habs(e.x), habs(adj.x)); e.y = hmin(habs(e.y), habs(adj.y)); e.z = hmin(habs(e.z), habs(adj.z)); e.w = hmin(habs(e.w), habs(adj.w));
    const hf den = hmul(c, H_0_011);
    return { hsat(hsub((hf)1.25f, hdiv(e.x, den))), hsat(hsub((hf)1.25f, hdiv(e.y, den))), hsat(hsub((hf)1.25f, hdiv(e.z, den))), hsat(hsub((hf)1.25f, hdiv(e.w, den))) };
}
__device__ __forceinline__ hf packEdges(H4 e)
{
    const H4 q = { hrint(hmul(hsat(e.x), H_2_9)), hrint(hmul(hsat(e.y), H_2_9)), hrint(hmul(hsat(e.z), H_2_9)), hrint(hmul(hsat(e.w), H_2_9)) };
    return hdot4(q, { H_64_255, H_16_255, H_4_255, H_1_255 });
}
__device__ __forceinline__ uint8_t unorm8Store(hf v) { return (uint8_t)toUint(cm::min_(cm::max_((float)v, 0.0f), 1.0f) * 255.0f + 0.5f); }
__device__ __forceinline__ hf unorm8Load(uint8_t b) { return r16(cm::div_(opaque((float)b), 255.0f)); }
__device__ __forceinline__ uint8_t uint8Store(uint32_t w) { return (uint8_t)(w < 255u ? w : 255u); }

__device__ __forceinline__ cm::F3 viewPosition(float sx, float sy, float depth, const GTAOConstants& k)
{
    return { (k.NDCToViewMul.x * sx + k.NDCToViewAdd.x) * depth, (k.NDCToViewMul.y * sy + k.NDCToViewAdd.y) * depth, depth };
}
__device__ __forceinline__ float sampleLevel(const DepthChain& c, float u, float v, hf mip)
{
    const int level = (int)cm::clamp_(__builtin_floorf((float)mip + 0.5f), 0.0f, 4.0f);
    const uint32_t w = c.w[level], h = c.h[level];
    const uint32_t x = (uint32_t)cm::clamp_(__builtin_floorf(u * (float)w), 0.0f, (float)(w - 1u)), y = (uint32_t)cm::clamp_(__builtin_floorf(v * (float)h), 0.0f, (float)(h - 1u));
    return (float)halfOf(c.mip[level][(uint64_t)y * w + x]);
}

// UnpackOctadehron of GBufferA.y as k_deferredlighting.hip states it, the row vector (n, 1) times the matrix, z negated
__device__ __forceinline__ cm::F3 viewNormal(uint4 g, const XeGTAOMainPassConstantBuffer& p)
{
    const float fx = (float)(g.y & 0xFFFFu) * (1.0f / 65535.0f) * 2.0f - 1.0f, fy = (float)(g.y >> 16) * (1.0f / 65535.0f) * 2.0f - 1.0f;
    cm::F3 n = { fx, fy, (1.0f - __builtin_fabsf(fx)) - __builtin_fabsf(fy) };
    const float t = cm::min_(cm::max_(-n.z, 0.0f), 1.0f);
    n.x += n.x >= 0.0f ? -t : t;
    n.y += n.y >= 0.0f ? -t : t;
    const float len = cm::sqrt_(cm::dot3(n, n));
    n = { cm::div_(n.x, len), cm::div_(n.y, len), cm::div_(n.z, len) };
    float o[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
        o[j] = cm::fma_(n.z, p.m_WorldToViewNoTranslate.m[2][j], cm::fma_(n.y, p.m_WorldToViewNoTranslate.m[1][j], n.x * p.m_WorldToViewNoTranslate.m[0][j])) + p.m_WorldToViewNoTranslate.m[3][j];
    return { o[0], o[1], o[2] * -1.0f };
}

__global__ __launch_bounds__(kAoGroup * kAoGroup) void aoMainKernel(MainArgs a)
{
    const sp::Pixel at = sp::pixel<kAoGroup, kAoGroup>();
    const uint32_t px = at.x, py = at.y, W = a.chain.w[0], H = a.chain.h[0];
    if (!at.inside(W, H)) return;
    const GTAOConstants& k = a.k;
    const uint32_t quality = a.push.m_Quality < 4u ? a.push.m_Quality : 0u;
    const hf sliceCount = quality == 0u ? (hf)1.0f : quality == 1u ? (hf)2.0f : quality == 2u ? (hf)3.0f : (hf)9.0f;
    const hf stepsPerSlice = quality == 2u ? (hf)3.0f : (hf)2.0f;
    uint32_t noiseIndex = hilbertIndex(px % 64u, py % 64u);
    noiseIndex += (uint32_t)(288 * (k.NoiseIndex % 64));
    const float n0 = 0.5f + (float)noiseIndex * 0.75487766624669276005f, n1 = 0.5f + (float)noiseIndex * 0.5698402909980532659114f;
    const hf noiseSlice = r16(n0 - __builtin_floorf(n0)), noiseSample = r16(n1 - __builtin_floorf(n1));
    const cm::F3 nf = viewNormal(a.gbufferA[(uint64_t)py * W + px], a.push);
    const H3 viewspaceNormal = { r16(nf.x), r16(nf.y), r16(nf.z) };

    const float nspx = ((float)px + 0.5f) * k.ViewportPixelSize.x, nspy = ((float)py + 0.5f) * k.ViewportPixelSize.y;
    const uint32_t xl = clampi((int32_t)px - 1, W), xr = clampi((int32_t)px + 1, W), yt = clampi((int32_t)py - 1, H), yb = clampi((int32_t)py + 1, H);
    const uint16_t* mip0 = a.chain.mip[0];
    hf viewspaceZ = halfOf(mip0[(uint64_t)py * W + px]);
    const hf pixLZ = halfOf(mip0[(uint64_t)py * W + xl]), pixRZ = halfOf(mip0[(uint64_t)py * W + xr]);
    const hf pixTZ = halfOf(mip0[(uint64_t)yt * W + px]), pixBZ = halfOf(mip0[(uint64_t)yb * W + px]);
    a.outEdges[(uint64_t)py * W + px] = unorm8Store(packEdges(calculateEdges(viewspaceZ, pixLZ, pixRZ, pixTZ, pixBZ)));

    viewspaceZ = hmul(viewspaceZ, H_0_9992);
    const cm::F3 pixCenterPos = viewPosition(nspx, nspy, (float)viewspaceZ, k);
    const cm::F3 neg = { -pixCenterPos.x, -pixCenterPos.y, -pixCenterPos.z };
    const float negLen = cm::sqrt_(cm::dot3(neg, neg));
    const H3 viewVec = { r16(cm::div_(neg.x, negLen)), r16(cm::div_(neg.y, negLen)), r16(cm::div_(neg.z, negLen)) };

    const hf effectRadius = hmul(r16(k.EffectRadius), H_1_457);
    hf falloffMul, falloffAdd;
    falloffTerms(k, effectRadius, falloffMul, falloffAdd);

    hf visibility = H0;
    const float pixelDirX = (float)viewspaceZ * k.NDCToViewMul_x_PixelSize.x;
    const hf screenspaceRadius = hdiv(effectRadius, r16(pixelDirX));
    visibility = hadd(visibility, hmul(hsat(hdiv(hsub((hf)10.0f, screenspaceRadius), (hf)100.0f)), (hf)0.5f));
    const hf minS = hdiv(H_1_3, screenspaceRadius);
    const hf pixelSizeX = r16(k.ViewportPixelSize.x), pixelSizeY = r16(k.ViewportPixelSize.y);

    for (hf slice = H0; slice < sliceCount; slice += H1) {
        const hf sliceK = hdiv(hadd(slice, noiseSlice), sliceCount);
        const hf phi = hmul(sliceK, H_PI);
        const hf cosPhi = hcos(phi), sinPhi = hsin(phi);
        const hf omegaX = hmul(cosPhi, screenspaceRadius), omegaY = hmul(-sinPhi, screenspaceRadius);
        const H3 directionVec = { cosPhi, sinPhi, H0 };
        const hf dv = hdot3(directionVec, viewVec);
        const H3 orthoDirectionVec = { hsub(directionVec.x, hmul(dv, viewVec.x)), hsub(directionVec.y, hmul(dv, viewVec.y)), hsub(directionVec.z, hmul(dv, viewVec.z)) };
        const H3 axisVec = hnormalize3(hcross(orthoDirectionVec, viewVec));
        const hf na = hdot3(viewspaceNormal, axisVec);
        const H3 projectedNormalVec = { hsub(viewspaceNormal.x, hmul(axisVec.x, na)), hsub(viewspaceNormal.y, hmul(axisVec.y, na)), hsub(viewspaceNormal.z, hmul(axisVec.z, na)) };
        const hf signNorm = hsign(hdot3(orthoDirectionVec, projectedNormalVec));
        hf projectedNormalVecLength = hlength3(projectedNormalVec);
        const hf cosNorm = hsat(hdiv(hdot3(projectedNormalVec, viewVec), projectedNormalVecLength));
        const hf n = hmul(signNorm, fastACos(cosNorm));
        const hf lowHorizonCos0 = hcos(hadd(n, H_PI_HALF)), lowHorizonCos1 = hcos(hsub(n, H_PI_HALF));
        hf horizonCos0 = lowHorizonCos0, horizonCos1 = lowHorizonCos1;

        for (hf step = H0; step < stepsPerSlice; step += H1) {
            const hf stepBaseNoise = hmul(hadd(slice, hmul(step, stepsPerSlice)), H_GOLDEN);
            const hf sn = hadd(noiseSample, stepBaseNoise);
            const hf stepNoise = hsub(sn, hfloor(sn));
            hf s = hdiv(hadd(step, stepNoise), stepsPerSlice);
            s = hmul(s, s);
            s = hadd(s, minS);
            hf offX = hmul(s, omegaX), offY = hmul(s, omegaY);
            const hf sampleOffsetLength = hsqrt(hdot2(offX, offY, offX, offY));
            const hf mipLevel = r16(cm::clamp_((float)hlog2(sampleOffsetLength) - k.DepthMIPSamplingOffset, 0.0f, 5.0f));
            offX = hmul(hrint(offX), pixelSizeX); offY = hmul(hrint(offY), pixelSizeY);

            const float u0 = nspx + (float)offX, v0 = nspy + (float)offY, u1 = nspx - (float)offX, v1 = nspy - (float)offY;
            const float SZ0 = sampleLevel(a.chain, u0, v0, mipLevel), SZ1 = sampleLevel(a.chain, u1, v1, mipLevel);
            const cm::F3 p0 = viewPosition(u0, v0, SZ0, k), p1 = viewPosition(u1, v1, SZ1, k);
            const cm::F3 d0 = { p0.x - pixCenterPos.x, p0.y - pixCenterPos.y, p0.z - pixCenterPos.z };
            const cm::F3 d1 = { p1.x - pixCenterPos.x, p1.y - pixCenterPos.y, p1.z - pixCenterPos.z };
            const hf sampleDist0 = r16(cm::sqrt_(cm::dot3(d0, d0))), sampleDist1 = r16(cm::sqrt_(cm::dot3(d1, d1)));
            const float sd0 = (float)sampleDist0, sd1 = (float)sampleDist1;
            const H3 hv0 = { r16(cm::div_(d0.x, sd0)), r16(cm::div_(d0.y, sd0)), r16(cm::div_(d0.z, sd0)) };
            const H3 hv1 = { r16(cm::div_(d1.x, sd1)), r16(cm::div_(d1.y, sd1)), r16(cm::div_(d1.z, sd1)) };
            const hf weight0 = hsat(hadd(hmul(sampleDist0, falloffMul), falloffAdd)), weight1 = hsat(hadd(hmul(sampleDist1, falloffMul), falloffAdd));
            hf shc0 = hdot3(hv0, viewVec), shc1 = hdot3(hv1, viewVec);
            shc0 = hlerp(lowHorizonCos0, shc0, weight0);
            shc1 = hlerp(lowHorizonCos1, shc1, weight1);
            horizonCos0 = hmax(horizonCos0, shc0);
            horizonCos1 = hmax(horizonCos1, shc1);
        }
        projectedNormalVecLength = hlerp(projectedNormalVecLength, H1, H_0_05);
        const hf h0 = -fastACos(horizonCos1), h1 = fastACos(horizonCos0);
        const hf sinN = hsin(n);
        const hf th0 = hmul((hf)2.0f, h0), th1 = hmul((hf)2.0f, h1);
        const hf iarc0 = hdiv(hsub(hadd(cosNorm, hmul(th0, sinN)), hcos(hsub(th0, n))), (hf)4.0f);
        const hf iarc1 = hdiv(hsub(hadd(cosNorm, hmul(th1, sinN)), hcos(hsub(th1, n))), (hf)4.0f);
        visibility = hadd(visibility, hmul(projectedNormalVecLength, hadd(iarc0, iarc1)));
    }
    visibility = hdiv(visibility, sliceCount);
    visibility = hpow(visibility, r16(k.FinalValuePower));
    visibility = hmax(H_0_03, visibility);
    visibility = hsat(hdiv(visibility, (hf)1.5f));
    a.outAO[(uint64_t)py * W + px] = uint8Store(toUint((float)hadd(hmul(visibility, (hf)255.0f), (hf)0.5f)));
}

// ---- pass 3 ------------------------------------------------------------------------------------------------------------------
struct DenoiseArgs
{
    GTAOConstants k;
    uint32_t finalApply;
    const uint8_t* ao;                         // R8_UINT
    const uint8_t* edges;                      // R8_UNORM
    uint8_t* out;                              // R8_UINT
    uint32_t W, H;
};

__device__ __forceinline__ H4 unpackEdges(hf packed)
{
    const uint32_t p = toUint((float)hmul(packed, (hf)255.5f));
    return { hsat(hdiv((hf)(float)((p >> 6) & 3u), (hf)3.0f)), hsat(hdiv((hf)(float)((p >> 4) & 3u), (hf)3.0f)), hsat(hdiv((hf)(float)((p >> 2) & 3u), (hf)3.0f)),
             hsat(hdiv((hf)(float)(p & 3u), (hf)3.0f)) };
}

__device__ __forceinline__ void denoisePixel(const DenoiseArgs& a, uint32_t px, uint32_t py)
{
    const uint32_t W = a.W, H = a.H;
    const hf blurAmount = a.finalApply ? r16(a.k.DenoiseBlurBeta) : hdiv(r16(a.k.DenoiseBlurBeta), (hf)5.0f);
    const uint32_t xs[3] = { clampi((int32_t)px - 1, W), px, clampi((int32_t)px + 1, W) }, ys[3] = { clampi((int32_t)py - 1, H), py, clampi((int32_t)py + 1, H) };
    auto EDGE = [&](int ix, int iy) { return unpackEdges(unorm8Load(a.edges[(uint64_t)ys[iy] * W + xs[ix]])); };
    auto VIS = [&](int ix, int iy) { return hdiv((hf)(float)a.ao[(uint64_t)ys[iy] * W + xs[ix]], (hf)255.0f); };
    const H4 eL = EDGE(0, 1), eT = EDGE(1, 0), eR = EDGE(2, 1), eB = EDGE(1, 2);
    H4 eC = EDGE(1, 1);
    eC.x = hmul(eC.x, eL.y); eC.y = hmul(eC.y, eR.x); eC.z = hmul(eC.z, eT.w); eC.w = hmul(eC.w, eB.z);
    const hf edginess = hmul(hdiv(hsat(hsub(hsub((hf)4.0f, (hf)2.5f), hdot4(eC, { H1, H1, H1, H1 }))), hsub((hf)4.0f, (hf)2.5f)), (hf)0.5f);
    eC.x = hsat(hadd(eC.x, edginess)); eC.y = hsat(hadd(eC.y, edginess)); eC.z = hsat(hadd(eC.z, edginess)); eC.w = hsat(hadd(eC.w, edginess));
    const hf weightTL = hmul(H_DIAG, hadd(hmul(eC.x, eL.z), hmul(eC.z, eT.x)));
    const hf weightTR = hmul(H_DIAG, hadd(hmul(eC.z, eT.y), hmul(eC.y, eR.z)));
    const hf weightBL = hmul(H_DIAG, hadd(hmul(eC.w, eB.x), hmul(eC.x, eL.w)));
    const hf weightBR = hmul(H_DIAG, hadd(hmul(eC.y, eR.w), hmul(eC.w, eB.y)));
    hf sumWeight = blurAmount;
    hf sum = hmul(VIS(1, 1), sumWeight);
    auto addSample = [&](hf v, hf w) { sum = hadd(sum, hmul(w, v)); sumWeight = hadd(sumWeight, w); };
    addSample(VIS(0, 1), eC.x);
    addSample(VIS(2, 1), eC.y);
    addSample(VIS(1, 0), eC.z);
    addSample(VIS(1, 2), eC.w);
    addSample(VIS(0, 0), weightTL);
    addSample(VIS(2, 0), weightTR);
    addSample(VIS(0, 2), weightBL);
    addSample(VIS(2, 2), weightBR);
    hf aoTerm = hdiv(sum, sumWeight);
    aoTerm = hmul(aoTerm, a.finalApply ? (hf)1.5f : H1);
    a.out[(uint64_t)py * W + px] = uint8Store(toUint((float)hadd(hmul(aoTerm, (hf)255.0f), (hf)0.5f)));
}

__global__ __launch_bounds__(kAoGroup * kAoGroup) void aoDenoiseKernel(DenoiseArgs a)
{
    const uint32_t px = (blockIdx.x * kAoGroup + threadIdx.x) * 2u, py = blockIdx.y * kAoGroup + threadIdx.y;
    if (py >= a.H) return;
    if (px < a.W) denoisePixel(a, px, py);
    if (px + 1u < a.W) denoisePixel(a, px + 1u, py);
}

// ---- recording -----------------------------------------------------------------------------------------------------------------
const GTAOConstants* gtaoConstants(trhip::DispatchCtx& ctx)
{
    trhip_buffer_t* cb = ctx.buffer(TRHIP_BIND_CONSTANT_BUFFER, 0);
    if (!cb || cb->byteSize != sizeof(GTAOConstants)) return nullptr;
    return (const GTAOConstants*)ctx.constants(0, sizeof(GTAOConstants));
}

// t0 of the main pass, u0..u4 of the prefilter: one R16_FLOAT texture of exactly 5 mips
bool isDepthChain(const trhip_texture_t* t) { return t && t->format == TRHIP_FORMAT_R16_FLOAT && t->mips == 5; }

int recordPrefilter(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const GTAOConstants* k = gtaoConstants(ctx);
    TRHIP_REQUIRE(k, "%s: constant buffer b0 (GTAOConstants, 96 bytes) missing or of another size", name);
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_R32_FLOAT, "Texture_SRV t0 = the R32_FLOAT depth buffer (one mip)", true, sp::kOneMipAt0 } };
    trhip_texture_t* depthAt[1];
    if (const int rc = sp::bindTextures(ctx, want, depthAt)) return rc;
    const trhip_texture_t* depth = depthAt[0];
    uint32_t mip = 0;
    PrefilterArgs a = sp::zeroed<PrefilterArgs>();
    trhip_texture_t* chain = ctx.texture(TRHIP_BIND_TEXTURE_UAV, 0, &mip);
    TRHIP_REQUIRE(isDepthChain(chain), "%s: needs Texture_UAV u0..u4 = mips 0..4 of one R16_FLOAT texture with 5 mips", name);
    TRHIP_REQUIRE(chain->width == depth->width && chain->height == depth->height, "%s: t0 is %ux%u, the working depth chain %ux%u", name, depth->width,
                  depth->height, chain->width, chain->height);
    for (uint32_t j = 0; j < 5; ++j) {
        trhip_texture_t* t = ctx.texture(TRHIP_BIND_TEXTURE_UAV, j, &mip);
        TRHIP_REQUIRE(t == chain && mip == j, "%s: needs Texture_UAV u%u = mip %u of the texture at u0", name, j, j);
        a.mip[j] = (uint16_t*)chain->mipPtr(j);
        a.w[j] = chain->mipW(j); a.h[j] = chain->mipH(j);
    }
    a.k = *k;
    a.depth = (const float*)depth->ptr;
    if (const int rc = sp::requireCover(ctx, 2u * kAoGroup, 2u * kAoGroup, a.w[0], a.h[0])) return rc;   // one 2 x 2 quad per thread
    sp::launch(ctx, aoPrefilterKernel, "aoPrefilterKernel", sp::tiles(a.w[0], a.h[0], 2u * kAoGroup, 2u * kAoGroup), dim3(kAoGroup, kAoGroup), a);
    return TRHIP_OK;
}

int recordMain(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const GTAOConstants* k = gtaoConstants(ctx);
    TRHIP_REQUIRE(k, "%s: constant buffer b0 (GTAOConstants, 96 bytes) missing or of another size", name);
    const XeGTAOMainPassConstantBuffer* push = (const XeGTAOMainPassConstantBuffer*)ctx.constants(1, sizeof(XeGTAOMainPassConstantBuffer));
    TRHIP_REQUIRE(push && ctx.pushBytes == sizeof(XeGTAOMainPassConstantBuffer), "%s: push constants b1 (XeGTAOMainPassConstantBuffer, 68 bytes) missing or of another size", name);
    uint32_t mip = 0;
    trhip_texture_t* chain = ctx.texture(TRHIP_BIND_TEXTURE_SRV, 0, &mip);
    TRHIP_REQUIRE(isDepthChain(chain) && mip == 0, "%s: needs Texture_SRV t0 = the R16_FLOAT working depth chain with 5 mips", name);
    const uint32_t W = chain->width, H = chain->height;
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 2, TRHIP_FORMAT_RGBA32_UINT, "Texture_SRV t2 = GBufferA (RGBA32_UINT)", true, sp::kOneMipAt0 },
                                 { TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_R8_UINT, "Texture_UAV u0 = the working AO term (R8_UINT)", true, sp::kOneMipAt0 },
                                 { TRHIP_BIND_TEXTURE_UAV, 1, TRHIP_FORMAT_R8_UNORM, "Texture_UAV u1 = the edges (R8_UNORM)", true, sp::kOneMipAt0 } };
    trhip_texture_t* tex[3];
    if (const int rc = sp::bindTextures(ctx, want, tex, W, H, "the working depth chain")) return rc;
    MainArgs a = sp::zeroed<MainArgs>();
    a.k = *k;
    a.push = *push;
    for (uint32_t j = 0; j < 5; ++j) { a.chain.mip[j] = (const uint16_t*)chain->mipPtr(j); a.chain.w[j] = chain->mipW(j); a.chain.h[j] = chain->mipH(j); }
    a.gbufferA = (const uint4*)tex[0]->ptr;
    a.outAO = (uint8_t*)tex[1]->ptr;
    a.outEdges = (uint8_t*)tex[2]->ptr;
    if (const int rc = sp::requireCover(ctx, kAoGroup, kAoGroup, W, H)) return rc;
    sp::launch(ctx, aoMainKernel, "aoMainKernel", sp::tiles(W, H, kAoGroup, kAoGroup), dim3(kAoGroup, kAoGroup), a);
    return TRHIP_OK;
}

int recordDenoise(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const GTAOConstants* k = gtaoConstants(ctx);
    TRHIP_REQUIRE(k, "%s: constant buffer b0 (GTAOConstants, 96 bytes) missing or of another size", name);
    const XeGTAODenoiseConstants* push = (const XeGTAODenoiseConstants*)ctx.constants(1, sizeof(XeGTAODenoiseConstants));
    TRHIP_REQUIRE(push && ctx.pushBytes == sizeof(XeGTAODenoiseConstants), "%s: push constants b1 (XeGTAODenoiseConstants, 4 bytes) missing or of another size", name);
    const sp::Binding wantSrc[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_R8_UINT, "Texture_SRV t0 = the AO term (R8_UINT)", true, sp::kOneMipAt0 } };
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_SRV, 1, TRHIP_FORMAT_R8_UNORM, "Texture_SRV t1 = the edges (R8_UNORM)", true, sp::kOneMipAt0 },
                                 { TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_R8_UINT, "Texture_UAV u0 = the output (R8_UINT)", true, sp::kOneMipAt0 } };
    trhip_texture_t *bound[1], *tex[2];
    if (const int rc = sp::bindTextures(ctx, wantSrc, bound)) return rc;                             // the size is the AO term's
    const trhip_texture_t *src = bound[0];
    const uint32_t W = src->width, H = src->height;
    if (const int rc = sp::bindTextures(ctx, want, tex, W, H, "t0")) return rc;
    const trhip_texture_t *edges = tex[0], *dst = tex[1];
    TRHIP_REQUIRE(dst->ptr != src->ptr, "%s: t0 and u0 are the same texture", name);
    DenoiseArgs a = sp::zeroed<DenoiseArgs>();
    a.k = *k;
    a.finalApply = push->m_FinalApply;
    a.ao = (const uint8_t*)src->ptr;
    a.edges = (const uint8_t*)edges->ptr;
    a.out = (uint8_t*)dst->ptr;
    a.W = W; a.H = H;
    if (const int rc = sp::requireCover(ctx, 2u * kAoGroup, kAoGroup, W, H)) return rc;             // two horizontal pixels per thread
    sp::launch(ctx, aoDenoiseKernel, "aoDenoiseKernel", sp::tiles(W, H, 2u * kAoGroup, kAoGroup), dim3(kAoGroup, kAoGroup), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("ambientocclusion_CS_XeGTAO_PrefilterDepths", recordPrefilter, 0);
trhip::ShaderRegistrar r1("ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0", recordMain, 0);
trhip::ShaderRegistrar r2("ambientocclusion_CS_XeGTAO_Denoise", recordDenoise, 0);

} // namespace
