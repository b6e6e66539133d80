// k_sky.hip -- "sky_PS_HosekWilkieSky": the reference's full-screen pass between DeferredLightingRenderer and BloomRenderer
// (source/SkyRenderer.cpp, source/shaders/sky.hlsl): the Hosek-Wilkie sky radiance into every texel of LightingOutput that the
// base pass did not draw.  The ten parameter rows come from the host (csrc/host/SkyRenderer.cpp, toyrenderer_amd/sky.py).
//
// BINDINGS: b0 = SkyPassParameters (256 bytes, a constant buffer: too large for push constants), t0 = the R32_FLOAT depth (the
// stand-in of the read-only depth attachment), u0 = the R11G11B10_FLOAT target at mip 0; samplers are accepted and ignored.  A
// direct dispatch of 8x8-pixel groups covering the target; the resolution is the bound target's (the block carries none).
//
// WHICH PIXELS: the reference draws a triangle at kFarDepth = 0 with depth test GreaterOrEqual and no depth write.  The
// stand-in: a pixel is written iff its depth word satisfies depth <= 0.0f (+0, -0 and negative; NaN is skipped): the exact
// complement of the lighting pass apart from NaN, which neither writes.  Every other texel of u0 keeps what it held.
//
// CONVENTION (parity unpinned; restated in tests/sky_ref.c and DESIGN.md 3).  The shared part is stated in screen_pass.hip.h:
//   worldPosition is its function at depth 0.9f over the bound target's size; V = normalize(worldPosition - m_CameraPosition),
//             v / sqrt(dot3(v, v));
//   cosTheta = fmin(fmax(V.y, 0), 1) (a NaN gives 0); cosGamma = dot3(V, m_SunLightDir); gamma = softmath::acosSoft(cosGamma):
//             outside [-1, 1] or NaN gives NaN, which a view ray that meets the sun direction to the last bit can produce
//             (dot3 of two unit vectors may round above 1); kept, as the reference's acos does the same;
//   exp(x) =  softmath::exp2Signed(x * 0x1.715476p+0f) (RN(log2 e)); pow(b, 1.5) = b * sqrt(b) (a negative base gives NaN);
//             pow(c, 256), c > 0 = eight successive squarings;
//   per channel: chi = (1 + cg * cg) / pow((1 + H * H) - ((2 * cg) * H), 1.5);
//             hw = (1 + A * exp(B / (cosTheta + 0.01f))) * ((((C + D * exp(E * gamma)) + F * (cg * cg)) + G * chi) + I * sqrt(cosTheta));
//             R = (-Z) * hw; if (cg > 0) R = R + pow(cg, 256) * 0.5f;
//   1 + H * H, -Z and the other uniform subexpressions are the same operations in the same order: they cost scalar registers;
//   store:    R11G11B10_FLOAT as in r11g11b10.hip.h (negative to 0, above the largest finite clamps); alpha is dropped.
//
// KERNEL: one thread per pixel, no LDS.  The depth word is read first and a drawn pixel ends there (4 B); a sky pixel stores
// 4 B more.  Per sky pixel six exponentials, three 3/2 powers, an arc cosine, eight squarings and about ten correctly rounded
// divisions and square roots: the arithmetic is the cost.  The tile is screen_pass.hip.h's.  Code object and measurements:
// profiles/sky/README.md.
#include "cull_math.hip.h"
#include "r11g11b10.hip.h"
#include "screen_pass.hip.h"
#include "soft_math.hip.h"

namespace
{

using namespace interop;

constexpr uint32_t kSkyBlock = 256, kSkyTileW = 64;   // tests/test_gpu_sky.py takes its sizes from these names: pinned to the shared tile
static_assert(kSkyBlock == sp::kBlock && kSkyTileW == sp::kTileW, "the sky pass runs in the shared tile");

struct SkyArgs
{
    SkyPassParameters k;
    const float* depth;                        // R32_FLOAT
    uint32_t* out;                             // R11G11B10_FLOAT
    uint32_t W, H;
};

#ifdef TR_SKY_EXPERIMENT_HW_EXP                // negative control only (profiles/sky/): v_exp_f32 and approximate division in the radiance (the world position is the shared one)
__device__ __forceinline__ float sdiv(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float exp_(float x) { return __builtin_amdgcn_exp2f(x * 0x1.715476p+0f); }
#else
__device__ __forceinline__ float sdiv(float a, float b) { return cm::div_(a, b); }
__device__ __forceinline__ float exp_(float x) { return softmath::exp2Signed(x * 0x1.715476p+0f); }
#endif
__device__ __forceinline__ float pow15(float b) { return b * cm::sqrt_(b); }

__device__ __forceinline__ cm::F3 skyPixel(const SkyArgs& a, uint32_t px, uint32_t py)
{
    const SkyPassParameters& k = a.k;
    const cm::F3 w = sp::worldPosition(k.m_ClipToWorld, px, py, a.W, a.H, 0.9f);
    const cm::F3 d = { w.x - k.m_CameraPosition[0], w.y - k.m_CameraPosition[1], w.z - k.m_CameraPosition[2] };
    const float len = cm::sqrt_(cm::dot3(d, d));
    const cm::F3 V = { sdiv(d.x, len), sdiv(d.y, len), sdiv(d.z, len) };
    const float ct = cm::min_(cm::max_(V.y, 0.0f), 1.0f);
    const float cg = cm::dot3(V, { k.m_SunLightDir[0], k.m_SunLightDir[1], k.m_SunLightDir[2] });
    const float gamma = softmath::acosSoft(cg);
    const float cg2 = cg * cg, onePlusCg2 = 1.0f + cg2, twoCg = 2.0f * cg, invCt = ct + 0.01f, sqrtCt = cm::sqrt_(ct);
    float sun = 0.0f;
    if (cg > 0.0f) {
        float p = cg;
        for (int i = 0; i < 8; ++i) p = p * p;
        sun = p * 0.5f;
    }
    const Vector4* P = k.m_HosekParams.m_Params;
    auto channel = [&](float A, float B, float C, float D, float E, float F, float G, float H, float I, float Z) {
        const float chi = sdiv(onePlusCg2, pow15((1.0f + H * H) - twoCg * H));
        const float first = 1.0f + A * exp_(sdiv(B, invCt));
        const float hw = first * ((((C + D * exp_(E * gamma)) + F * cg2) + G * chi) + I * sqrtCt);
        const float R = -Z * hw;
        return cg > 0.0f ? R + sun : R;
    };
    return { channel(P[0].x, P[1].x, P[2].x, P[3].x, P[4].x, P[5].x, P[6].x, P[7].x, P[8].x, P[9].x),
             channel(P[0].y, P[1].y, P[2].y, P[3].y, P[4].y, P[5].y, P[6].y, P[7].y, P[8].y, P[9].y),
             channel(P[0].z, P[1].z, P[2].z, P[3].z, P[4].z, P[5].z, P[6].z, P[7].z, P[8].z, P[9].z) };
}

__global__ __launch_bounds__(sp::kBlock) void skyKernel(SkyArgs a)
{
    const sp::Pixel at = sp::pixel();
    if (!at.inside(a.W, a.H)) return;
    const uint64_t i = at.index(a.W);
    const float depth = a.depth[i];
    if (!(depth <= 0.0f)) return;                                                                  // drawn (or NaN): costs 4 B
#ifdef TR_SKY_EXPERIMENT_STORE_ONLY             // attribution only (profiles/sky/): the pass's bytes without its arithmetic
    a.out[i] = __builtin_bit_cast(uint32_t, depth) ^ at.x;
#else
    const cm::F3 rgb = skyPixel(a, at.x, at.y);
    a.out[i] = trhip::packR11G11B10(rgb.x, rgb.y, rgb.z);
#endif
}

int recordSky(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    const SkyPassParameters* k = (const SkyPassParameters*)ctx.constants(0, sizeof(SkyPassParameters));
    TRHIP_REQUIRE(k, "%s: constant buffer b0 (SkyPassParameters, 256 bytes) missing or short", name);
    const sp::Binding wantTarget[] = { { TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_R11G11B10_FLOAT, "Texture_UAV u0 = the R11G11B10_FLOAT LightingOutput, mip 0", true, sp::kAt0 } };
    const sp::Binding wantDepth[] = { { TRHIP_BIND_TEXTURE_SRV, 0, TRHIP_FORMAT_R32_FLOAT, "the R32_FLOAT depth buffer (one mip, read at mip 0) at Texture_SRV t0", true, sp::kOneMipAt0 } };
    trhip_texture_t *dst[1], *depth[1];
    if (const int rc = sp::bindTextures(ctx, wantTarget, dst)) return rc;                            // the resolution is the bound target's
    if (const int rc = sp::bindTextures(ctx, wantDepth, depth, dst[0]->width, dst[0]->height, "u0")) return rc;
    SkyArgs a = sp::zeroed<SkyArgs>();
    a.k = *k;
    a.depth = (const float*)depth[0]->ptr;
    a.out = (uint32_t*)dst[0]->mipPtr(0);
    a.W = dst[0]->width; a.H = dst[0]->height;
    TRHIP_REQUIRE(a.W && a.H, "%s: u0 is empty", name);
    if (const int rc = sp::requireCover(ctx, sp::kGroupSide, sp::kGroupSide, a.W, a.H)) return rc;
    sp::launch(ctx, skyKernel, "skyKernel", sp::tiles(a.W, a.H), dim3(sp::kTileW, sp::kTileH), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("sky_PS_HosekWilkieSky", recordSky, 0);

} // namespace
