// screen_pass.hip.h -- what the image passes share: the full-screen tile, a pixel's world position, the small arithmetic
// helpers, and, on the record side, the binding table, the dispatch check and the launch.  For the passes behind the G-buffer
// and the resolve (visibility_resolve.hip.h); the cull's translation units do not include it.
//
// CONVENTION, the part these passes have in common (parity unpinned; restated in each pass's tests/*_ref.c and in DESIGN.md 3).
// IEEE binary32, no contraction, fma only where written, / and sqrt correctly rounded (cm::div_, cm::sqrt_):
//   saturate(x) = fmin(fmax(x, 0), 1) (a NaN gives 0); lerp(x, y, s) = x + s * (y - x), always evaluated (s = 0 included: an
//             infinite x gives NaN); dot3 = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)) (cm::dot3); uint(x) truncates;
//   inUV = (px + 0.5f, py + 0.5f) / float2(resolution), one division per axis; UVToClipXY uv * (2, -2) + (-1, 1), multiply then add;
//   worldPosition = xyz / w of the row vector (clipXY, depth, 1) times m_ClipToWorld, each column
//             fma(depth, m[2][j], fma(clip.y, m[1][j], clip.x * m[0][j])) + m[3][j] (the motion resolve's 4-column product); the
//             lighting pass and the sky call the function, the shadow mask's trace keeps the sequence written out (see there);
//   binary16: a load is exact; a store rounds to nearest even and every NaN is stored as the one word 0x7E00.
// TILE.  A full-screen pass runs one thread per pixel in workgroups of kBlock threads covering kTileW x kTileH pixels: a wave is
// one kTileW-wide row segment (against 16 x 4: equal within the spread, profiles/lighting/).  The reference draws these passes as
// [numthreads(8, 8, 1)] groups, whose counts must cover the image.  Kernels of another shape keep their constants and use pixel<W, H>().
#pragma once

#include "cull_math.hip.h"
#include "trhip_internal.h"

namespace sp
{

// ---- device side -------------------------------------------------------------------------------------------------------------
constexpr uint32_t kBlock = 256, kTileW = 64, kTileH = 4;
constexpr uint32_t kGroupSide = 8;             // the reference entries' [numthreads(8, 8, 1)]
static_assert(kTileW * kTileH == kBlock, "tile shape");

struct Pixel
{
    uint32_t x, y;
    __device__ __forceinline__ bool inside(uint32_t W, uint32_t H) const { return x < W && y < H; }
    __device__ __forceinline__ uint64_t index(uint32_t W) const { return (uint64_t)y * W + x; }
};

// The pixel of this thread in a launch of dim3(TILE_W, TILE_H) blocks.
template <uint32_t TILE_W = kTileW, uint32_t TILE_H = kTileH>
__device__ __forceinline__ Pixel pixel() { return { blockIdx.x * TILE_W + threadIdx.x, blockIdx.y * TILE_H + threadIdx.y }; }

__device__ __forceinline__ cm::F3 worldPosition(const interop::Matrix& clipToWorld, uint32_t px, uint32_t py, uint32_t W, uint32_t H, float depth)
{
    const float u = cm::div_((float)px + 0.5f, (float)W), v = cm::div_((float)py + 0.5f, (float)H);
    const float cx = u * 2.0f + -1.0f, cy = v * -2.0f + 1.0f;                                      // UVToClipXY
    float h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        h[j] = cm::fma_(depth, clipToWorld.m[2][j], cm::fma_(cy, clipToWorld.m[1][j], cx * clipToWorld.m[0][j])) + clipToWorld.m[3][j];
    return { cm::div_(h[0], h[3]), cm::div_(h[1], h[3]), cm::div_(h[2], h[3]) };
}

__device__ __forceinline__ float saturate_(float x) { return cm::min_(cm::max_(x, 0.0f), 1.0f); }
__device__ __forceinline__ float lerp_(float x, float y, float s) { return x + s * (y - x); }

// One axis of SampleLevel(LinearClamp, uv, 0) on a mip `dim` texels wide (k_bloom.hip's CONVENTION states it; the temporal resolve
// reads its history through the same words): the two texel indices and the weight of the second.
struct Axis { uint32_t i0, i1; float f; };

__device__ __forceinline__ Axis axisOf(float uv, uint32_t dim)
{
    const float t = uv * (float)dim - 0.5f, t0 = __builtin_floorf(t), last = (float)(dim - 1u);
#ifdef TR_BLOOM_EXPERIMENT_FIXED_POINT         // negative control only (profiles/bloom/): a fixed-point sampler weight
    const float f = (float)(uint32_t)((t - t0) * 256.0f) / 256.0f;
#else
    const float f = t - t0;
#endif
    return { (uint32_t)cm::min_(cm::max_(t0, 0.0f), last), (uint32_t)cm::min_(cm::max_(t0 + 1.0f, 0.0f), last), f };
}

__device__ __forceinline__ _Float16 halfOf(uint32_t low16) { return __builtin_bit_cast(_Float16, (uint16_t)low16); }
__device__ __forceinline__ uint32_t halfBits(float f) { return f != f ? 0x7E00u : (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f); }

// ---- record side -------------------------------------------------------------------------------------------------------------
// What a pass asks of the mips of a texture it binds.  The rules differ per pass, and the tables say which holds where.
enum Mips : uint32_t
{
    kOneMip,                                   // a single-mip texture (a UAV's mip is then 0: the dispatch checks its range; an SRV's is not looked at)
    kOneMipAt0,                                // a single-mip texture bound at mip 0
    kOneMipOrAt0,                              // a single-mip texture, or mip 0 of a chain
    kAt0,                                      // mip 0 of any texture
    kAnyMip,                                   // any mip in range; the size is that mip's
};

struct Binding { uint32_t type, slot, format; const char* what; bool required; Mips mips; };

// Looks up every entry of a pass's table: tex[j] (and mip[j]) is what is bound for want[j], nullptr where an optional entry is
// unbound.  With a sizeName every bound entry must be W x H, the size that the name stands for in the refusal.
template <size_t N>
int bindTextures(const trhip::DispatchCtx& ctx, const Binding (&want)[N], trhip_texture_t* (&tex)[N], uint32_t W = 0, uint32_t H = 0, const char* sizeName = nullptr,
                 uint32_t* mip = nullptr)
{
    const char* name = ctx.shaderName;
    for (size_t j = 0; j < N; ++j) {
        const Binding& w = want[j];
        uint32_t m = 0;
        trhip_texture_t* t = tex[j] = ctx.texture(w.type, w.slot, &m);
        if (mip) mip[j] = m;
        if (!t && !w.required) continue;
        TRHIP_REQUIRE(t && t->format == w.format, "%s: needs %s", name, w.what);
        if (w.mips == kAnyMip) {
            TRHIP_REQUIRE(m < t->mips, "%s: %c%u mip %u out of range (the texture has %u)", name, w.type == TRHIP_BIND_TEXTURE_UAV ? 'u' : 't', w.slot, m, t->mips);
        } else {
            const bool one = t->mips == 1, at0 = m == 0;
            TRHIP_REQUIRE(w.mips == kOneMip ? one : w.mips == kOneMipAt0 ? one && at0 : w.mips == kOneMipOrAt0 ? one || at0 : at0, "%s: needs %s", name, w.what);
        }
        const uint32_t tw = w.mips == kAnyMip ? t->mipW(m) : t->width, th = w.mips == kAnyMip ? t->mipH(m) : t->height;
        TRHIP_REQUIRE(!sizeName || (tw == W && th == H), "%s: %s is %ux%u, %s is %ux%u", name, w.what, tw, th, sizeName, W, H);
    }
    return TRHIP_OK;
}

// The dispatch a pass needs: direct, with groups of A x B pixels (the reference entry's) covering W x H (`the` ... `noun` around
// the size where a pass names what it covers).
inline int requireCover(const trhip::DispatchCtx& ctx, uint32_t A, uint32_t B, uint32_t W, uint32_t H, const char* noun = nullptr)
{
    TRHIP_REQUIRE(!ctx.indirect, "%s: needs a direct dispatch of %ux%u-pixel groups", ctx.shaderName, A, B);
    TRHIP_REQUIRE((uint64_t)ctx.gx * A >= W && (uint64_t)ctx.gy * B >= H, "%s: a direct dispatch of %ux%u-pixel groups covering %s%ux%u%s", ctx.shaderName, A, B,
                  noun ? "the " : "", W, H, noun ? noun : "");
    return TRHIP_OK;
}

inline dim3 tiles(uint32_t W, uint32_t H, uint32_t tileW = kTileW, uint32_t tileH = kTileH) { return dim3((W + tileW - 1) / tileW, (H + tileH - 1) / tileH); }

template <typename Args> Args zeroed() { Args a; memset(&a, 0, sizeof a); return a; }             // kernel arguments, padding included

// Emits the pass's one launch.
template <typename Args>
void launch(const trhip::DispatchCtx& ctx, void (*kernel)(Args), const char* kernelName, dim3 grid, dim3 block, const Args& a, const char* op = "main")
{
    ctx.emit(op, [=](hipStream_t s) {
        TRHIP_LAUNCH(kernel, grid, block, 0, s, a);
        return trhip::launchStatus(kernelName); });
}

} // namespace sp
