// k_giprobeblend.hip -- "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=1" and "... =0": the two passes of
// GIRenderer::RenderDDGI (source/GIRenderer.cpp) that fold a probe's 256 traced rays (k_giprobetrace.hip's records, or any buffer of
// that layout) into its octahedral irradiance and distance tiles.  The RTXGI SDK's ProbeBlendingCS.hlsl is not part of this project:
// this is the project's own statement of the published blend (Majercik et al., JCGT 2019) with the settings GIRenderer.cpp:74-121
// configures; tests/ddgi_update_ref.c is the definition and the functions below repeat it word for word.
//
// BINDINGS.  b0 ddgiu::Block (DDGIUpdateConsts, then the DDGIVolumeDesc's host copy; 160 bytes); StructuredBuffer_SRV t1 the ray
// records, float4[numProbes * 256] (rgb radiance, w distance: < 0 marks a back face); Texture_SRV t3 the RGBA16_FLOAT array of probe
// data; radiance: Texture_UAV u1 the R10G10B10A2_UNORM irradiance array; distance: Texture_UAV u2 the RG16_FLOAT distance array.  A
// direct dispatch of (counts.x, counts.z, counts.y) groups, one per probe.  With DDGIVolumeDesc::flags bit 2 (kDDGIFlag_Variability) the
// radiance pass also needs StructuredBuffer_UAV u4 = the probe variability, float[counts.y][6 * counts.z][6 * counts.x]: the interior
// texels of the irradiance array in that array's order, without borders; with the bit clear u4 is not looked at.
//
// CONVENTION (ddgi_update.hip.h states the ray direction, the octahedral decode and a probe's index).
//   left alone: with flags bit 1 (classification) a probe whose data.w == 1.0f, and any probe with kDDGIBackfaceRayLimit = 25 or more
//             records of w < 0: not a texel of its tile is written, border included;
//   texelDir  = octDecode of interior texel (ix, iy)'s centre; sums run over the rays 0..255 in that order;
//   radiance  : records with w < 0 are skipped; w = fmax(0, dot3(texelDir, rayDir)); sum += rgb * w (product, then sum); sumW += w;
//             res = powSoft(sum / (2.0f * fmax(sumW, 1e-9f * 256.0f)), 1.0f / gamma) per channel; prev = (float)code / 1023.0f;
//             prev == (0, 0, 0): the store is res (a cleared texel takes the first estimate whole).  Otherwise h = probeHysteresis;
//             delta = res - prev; fmax of the three |delta| > probeIrradianceThreshold: h = fmax(0, h - 0.75f);
//             sqrt(dot3(delta, delta)) > probeBrightnessThreshold: delta = delta * 0.25f; step = (1.0f - h) * delta;
//             when fmax of (prev + delta) < fmax of prev (darker): step = fmin(fmax(1.0f / 1024.0f, |step|), |delta|) * sign(step) per
//             channel, sign(0) = 0: without it ten bits never reach black; the store is prev + step;
//             code = (uint)rint(saturate(store) * 1023.0f) (round to nearest even; a NaN gives 0), alpha 3;
//   variability (flags bit 2; tests/ddgi_variability_ref.c: dv_texel): per channel s2 = (res - prev) * (res - out), out the eased value
//             before saturate and the 10-bit store; L = (0.2126f, 0.7152f, 0.0722f); lumS2 = dot3(s2, L); lumMean = dot3(out, L);
//             the value is (lumMean <= 1.0f / 1024.0f || !(lumS2 > 0.0f)) ? 0.0f : sqrt(lumS2) / lumMean, the coefficient of variation.
//             The floor of one 10-bit code and the > 0 guard are the project's own: a channel product can be negative, and no NaN
//             is born here.  A probe that is left alone writes none of its 36 values;
//   distance  : w = powSoft(fmax(0, dot3(texelDir, rayDir)), probeDistanceExponent); d = fmin(|record.w|, 1.5f * sqrt(dot3(spacing,
//             spacing))); sum.x += d * w; sum.y += (d * d) * w; sumW += w; res = sum / (2.0f * fmax(sumW, 1e-9f * 256.0f));
//             prev = the binary16 texel; h = prev == (0, 0) ? 0 : probeHysteresis; the store is lerp(res, prev, h) = res + h * (prev -
//             res), rounded to binary16 (nearest even, a NaN as 0x7E00);
//   border    : after the interior, (x, 0) <- (N-1-x, 1), (x, N-1) <- (N-1-x, N-2), (0, y) <- (1, N-1-y), (N-1, y) <- (N-2, N-1-y) for
//             1 <= x, y <= N-2, and each corner takes the diagonally opposite interior corner: ddgi.fill_borders.
//
// KERNEL.  One workgroup per probe, one thread per texel of its tile (64 or 256).  The records and the ray directions are staged in
// LDS (7 KB), the finished interior in a third array; a barrier, then the border threads copy.  The left-alone decisions are the
// same for every thread of a workgroup, so all of them leave together, before or between the barriers.  Every address comes from
// the host copy of the descriptor, which the record function checked against the bound textures and the ray buffer's size.
// UNTUNED: correctness came first.  Every interior thread walks all 256 rays; the distance pass's powSoft per ray and texel is its cost.
// Code object (-Rpass-analysis=kernel-resource-usage): radiance 21 VGPRs, occupancy 6 waves per SIMD (64-thread groups), LDS 7424 bytes;
// distance 20 VGPRs, occupancy 8, LDS 8192 bytes; radiance with variability 25 VGPRs, occupancy 6, LDS 7424 bytes; no scratch in any.
#include "ddgi_update.hip.h"

namespace
{

using namespace interop;
using cm::F3;

struct BlendArgs
{
    ddgiu::Block b;
    const float4* rays;                        // t1
    const uint2* data; uint32_t dataW, dataPitch;       // t3 RGBA16_FLOAT array; texels per row and per slice
    uint32_t* tex; uint32_t texW, texPitch;             // u1 R10G10B10A2_UNORM or u2 RG16_FLOAT array
    float* variability;                        // u4 (VARIABILITY only): float[counts.y][6 * counts.z][6 * counts.x]
};

__device__ __forceinline__ float sign_(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
__device__ __forceinline__ float max3(float a, float b, float c) { return cm::max_(cm::max_(a, b), c); }

// tests/ddgi_update_ref.c: ease_radiance
__device__ __forceinline__ F3 easeRadiance(F3 res, F3 prev, const DDGIUpdateConsts& k)
{
    if (prev.x == 0.0f && prev.y == 0.0f && prev.z == 0.0f) return res;
    float h = k.probeHysteresis;
    F3 delta = { res.x - prev.x, res.y - prev.y, res.z - prev.z };
    if (max3(__builtin_fabsf(delta.x), __builtin_fabsf(delta.y), __builtin_fabsf(delta.z)) > k.probeIrradianceThreshold) h = cm::max_(0.0f, h - 0.75f);
    if (cm::sqrt_(cm::dot3(delta, delta)) > k.probeBrightnessThreshold) delta = { delta.x * 0.25f, delta.y * 0.25f, delta.z * 0.25f };
    F3 step = { (1.0f - h) * delta.x, (1.0f - h) * delta.y, (1.0f - h) * delta.z };
    if (max3(prev.x + delta.x, prev.y + delta.y, prev.z + delta.z) < max3(prev.x, prev.y, prev.z)) {
        const float t = 1.0f / 1024.0f;
        step.x = cm::min_(cm::max_(t, __builtin_fabsf(step.x)), __builtin_fabsf(delta.x)) * sign_(step.x);
        step.y = cm::min_(cm::max_(t, __builtin_fabsf(step.y)), __builtin_fabsf(delta.y)) * sign_(step.y);
        step.z = cm::min_(cm::max_(t, __builtin_fabsf(step.z)), __builtin_fabsf(delta.z)) * sign_(step.z);
    }
    return { prev.x + step.x, prev.y + step.y, prev.z + step.z };
}

__device__ __forceinline__ uint32_t unorm10(float v) { return (uint32_t)__builtin_rintf(sp::saturate_(v) * 1023.0f); }

template <bool RADIANCE, bool VARIABILITY>
__global__ __launch_bounds__(RADIANCE ? 64 : 256) void blendKernel(BlendArgs a)
{
    constexpr uint32_t N = (RADIANCE ? kDDGIIrradianceInteriorTexels : kDDGIDistanceInteriorTexels) + 2u, kThreads = N * N, kRays = kDDGIRaysPerProbe;
    __shared__ float4 sRay[kRays];
    __shared__ float sDir[kRays][3];
    __shared__ uint32_t sTile[kThreads];
    const DDGIVolumeDesc& D = a.b.D;
    const DDGIUpdateConsts& k = a.b.k;
    const uint32_t probe = blockIdx.x, tid = threadIdx.x, tx = tid % N, ty = tid / N;
    const ddgiu::I3 c = ddgiu::probeCoords(probe, D);
    if (ddgiu::inactive(D, a.data[(uint64_t)c.y * a.dataPitch + (uint32_t)c.z * a.dataW + (uint32_t)c.x])) return;        // the whole workgroup
    for (uint32_t r = tid; r < kRays; r += kThreads) {
        sRay[r] = a.rays[(uint64_t)probe * kRays + r];
        const F3 d = ddgiu::rayDirection(r, k);
        sDir[r][0] = d.x; sDir[r][1] = d.y; sDir[r][2] = d.z;
    }
    __syncthreads();
    uint32_t back = 0;
    for (uint32_t r = 0; r < kRays; ++r) back += sRay[r].w < 0.0f ? 1u : 0u;
    if (back >= kDDGIBackfaceRayLimit) return;                                                     // the whole workgroup
    uint32_t* tile = a.tex + (uint64_t)c.y * a.texPitch + (uint64_t)((uint32_t)c.z * N) * a.texW + (uint32_t)c.x * N;
    const bool interior = tx >= 1u && tx <= N - 2u && ty >= 1u && ty <= N - 2u;
    if (interior) {
        const F3 texelDir = ddgiu::octDecode(cm::div_((float)(2u * (tx - 1u) + 1u), (float)(N - 2u)) - 1.0f, cm::div_((float)(2u * (ty - 1u) + 1u), (float)(N - 2u)) - 1.0f);
        const uint32_t old = tile[ty * a.texW + tx];
        uint32_t word;
        if constexpr (RADIANCE) {
            F3 sum = { 0.0f, 0.0f, 0.0f };
            float sumW = 0.0f;
            for (uint32_t r = 0; r < kRays; ++r) {
                const float4 rec = sRay[r];
                if (rec.w < 0.0f) continue;
                const float w = cm::max_(0.0f, cm::dot3(texelDir, { sDir[r][0], sDir[r][1], sDir[r][2] }));
                sum.x = sum.x + rec.x * w; sum.y = sum.y + rec.y * w; sum.z = sum.z + rec.z * w;
                sumW = sumW + w;
            }
            const float den = 2.0f * cm::max_(sumW, 1e-9f * 256.0f), invGamma = cm::div_(1.0f, D.probeIrradianceEncodingGamma);
            const F3 res = { ddgi::powSoft(cm::div_(sum.x, den), invGamma), ddgi::powSoft(cm::div_(sum.y, den), invGamma), ddgi::powSoft(cm::div_(sum.z, den), invGamma) };
            const F3 prev = { cm::div_((float)(old & 1023u), 1023.0f), cm::div_((float)((old >> 10) & 1023u), 1023.0f), cm::div_((float)((old >> 20) & 1023u), 1023.0f) };
            const F3 out = easeRadiance(res, prev, k);
            word = unorm10(out.x) | unorm10(out.y) << 10 | unorm10(out.z) << 20 | 3u << 30;
            if constexpr (VARIABILITY) {                                                             // tests/ddgi_variability_ref.c: dv_texel
                const F3 s2 = { (res.x - prev.x) * (res.x - out.x), (res.y - prev.y) * (res.y - out.y), (res.z - prev.z) * (res.z - out.z) };
                const F3 L = { 0.2126f, 0.7152f, 0.0722f };
                const float lumS2 = cm::dot3(s2, L), lumMean = cm::dot3(out, L);
                const float cov = (lumMean <= 1.0f / 1024.0f || !(lumS2 > 0.0f)) ? 0.0f : cm::div_(cm::sqrt_(lumS2), lumMean);
                const uint32_t I = N - 2u, vw = (uint32_t)D.probeCounts[0] * I, vh = (uint32_t)D.probeCounts[2] * I;
                a.variability[((uint64_t)c.y * vh + ((uint32_t)c.z * I + (ty - 1u))) * vw + ((uint32_t)c.x * I + (tx - 1u))] = cov;
            }
        } else {
            const F3 spacing = { D.probeSpacing[0], D.probeSpacing[1], D.probeSpacing[2] };
            const float maxDistance = 1.5f * cm::sqrt_(cm::dot3(spacing, spacing));
            float sx = 0.0f, sy = 0.0f, sumW = 0.0f;
            for (uint32_t r = 0; r < kRays; ++r) {
                const float w = ddgi::powSoft(cm::max_(0.0f, cm::dot3(texelDir, { sDir[r][0], sDir[r][1], sDir[r][2] })), k.probeDistanceExponent);
                const float d = cm::min_(__builtin_fabsf(sRay[r].w), maxDistance);
                sx = sx + d * w; sy = sy + (d * d) * w;
                sumW = sumW + w;
            }
            const float den = 2.0f * cm::max_(sumW, 1e-9f * 256.0f);
            const float rx = cm::div_(sx, den), ry = cm::div_(sy, den);
            const float px = (float)sp::halfOf(old), py = (float)sp::halfOf(old >> 16);
            const float h = (px == 0.0f && py == 0.0f) ? 0.0f : k.probeHysteresis;
            word = sp::halfBits(sp::lerp_(rx, px, h)) | sp::halfBits(sp::lerp_(ry, py, h)) << 16;
        }
        tile[ty * a.texW + tx] = word;
        sTile[tid] = word;
    }
    __syncthreads();
    if (!interior) {
        const bool edgeX = tx == 0u || tx == N - 1u, edgeY = ty == 0u || ty == N - 1u;
        uint32_t sx, sy;
        if (edgeX && edgeY) { sx = tx == 0u ? N - 2u : 1u; sy = ty == 0u ? N - 2u : 1u; }
        else if (edgeY) { sx = N - 1u - tx; sy = ty == 0u ? 1u : N - 2u; }
        else { sx = tx == 0u ? 1u : N - 2u; sy = N - 1u - ty; }
        tile[ty * a.texW + tx] = sTile[sy * N + sx];
    }
}

template <bool RADIANCE>
int recordBlend(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    BlendArgs a = sp::zeroed<BlendArgs>();
    if (const int rc = ddgiu::requireBlock(ctx, a.b)) return rc;
    const DDGIVolumeDesc& D = a.b.D;
    TRHIP_REQUIRE(!ctx.indirect && ctx.gx == (uint32_t)D.probeCounts[0] && ctx.gy == (uint32_t)D.probeCounts[2] && ctx.gz == (uint32_t)D.probeCounts[1],
                  "%s: needs a direct dispatch of (probeCounts.x, probeCounts.z, probeCounts.y) = (%d, %d, %d) groups, one per probe", name, D.probeCounts[0], D.probeCounts[2], D.probeCounts[1]);
    const uint32_t probes = ddgiu::numProbes(D);
    trhip_buffer_t* rays = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 1);
    TRHIP_REQUIRE(rays, "%s: needs StructuredBuffer_SRV t1 = the ray records, float4[numProbes * 256]", name);
    TRHIP_REQUIRE(rays->byteSize == (uint64_t)probes * kDDGIRaysPerProbe * sizeof(float4), "%s: the ray records at t1 hold %llu bytes; %u probes of 256 float4 records are %llu", name,
                  (unsigned long long)rays->byteSize, probes, (unsigned long long)probes * kDDGIRaysPerProbe * sizeof(float4));
    trhip_texture_t *data, *target;
    if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_SRV, 3, TRHIP_FORMAT_RGBA16_FLOAT, 1, "Texture_SRV t3 = the RGBA16_FLOAT array of probe data", D, data)) return rc;
    const bool variability = RADIANCE && (D.flags & kDDGIFlag_Variability) != 0u;
    if (variability) {
        trhip_buffer_t* v = ctx.buffer(TRHIP_BIND_STRUCTURED_UAV, 4);
        const uint64_t bytes = (uint64_t)probes * kDDGIIrradianceInteriorTexels * kDDGIIrradianceInteriorTexels * sizeof(float);
        TRHIP_REQUIRE(v, "%s: DDGIVolumeDesc flags = %u have probe variability on: needs StructuredBuffer_UAV u4 = the probe variability, float[counts.y][6 * counts.z][6 * counts.x]", name, D.flags);
        TRHIP_REQUIRE(v->byteSize == bytes, "%s: the probe variability at u4 holds %llu bytes; %u probes of 36 floats are %llu", name, (unsigned long long)v->byteSize, probes, (unsigned long long)bytes);
        a.variability = (float*)v->ptr;
    }
    if (RADIANCE) {
        if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_UAV, 1, TRHIP_FORMAT_R10G10B10A2_UNORM, kDDGIIrradianceInteriorTexels + 2,
                                                      "Texture_UAV u1 = the R10G10B10A2_UNORM array of probe irradiance", D, target)) return rc;
    } else {
        if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_UAV, 2, TRHIP_FORMAT_RG16_FLOAT, kDDGIDistanceInteriorTexels + 2,
                                                      "Texture_UAV u2 = the RG16_FLOAT array of probe distance", D, target)) return rc;
    }
    a.rays = (const float4*)rays->ptr;
    a.data = (const uint2*)data->ptr; a.dataW = data->width; a.dataPitch = (uint32_t)(data->slicePitch / data->texelBytes);
    a.tex = (uint32_t*)target->ptr; a.texW = target->width; a.texPitch = (uint32_t)(target->slicePitch / target->texelBytes);
    if (variability) sp::launch(ctx, blendKernel<RADIANCE, RADIANCE>, "blendKernel<radiance, variability>", dim3(probes), dim3(64), a);
    else sp::launch(ctx, blendKernel<RADIANCE, false>, RADIANCE ? "blendKernel<radiance>" : "blendKernel<distance>", dim3(probes), dim3(RADIANCE ? 64 : 256), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=1", recordBlend<true>, 1);
trhip::ShaderRegistrar r1("ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=0", recordBlend<false>, 0);

} // namespace
