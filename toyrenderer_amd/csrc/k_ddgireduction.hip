// k_ddgireduction.hip -- "ReductionCS_DDGIReductionCS REDUCTION=1" and "ReductionCS_DDGIExtraReductionCS": the passes of
// GIRenderer::RenderDDGI (source/GIRenderer.cpp:542-573) that average the probe variability (k_giprobeblend.hip, flags bit 2) over
// the volume, down to one element whose .x the host reads back two updates later (csrc/host/DDGIVariability.h).  The RTXGI SDK's
// ReductionCS.hlsl is not part of this project: this is the project's own statement, tests/ddgi_variability_ref.c is the definition
// and the functions below repeat it word for word, THE ORDER OF EVERY ADDITION INCLUDED.
//
// BINDINGS.  Push constants at b1: the SDK's DDGIRootConstants (24 bytes; the three reductionInputSize words are read).
//   first pass : b0 ddgiu::Block (160 bytes: the update's block, whose DDGIVolumeDesc says which probes classification switches off);
//                Texture_SRV t3 the RGBA16_FLOAT array of probe data; StructuredBuffer_SRV t4 the probe variability,
//                float[P][H][W] with W = 6 * counts.x, H = 6 * counts.z, P = counts.y (the push constants must say the same);
//                StructuredBuffer_UAV u5 the averages written, float2[gz][gy][gx];
//   extra pass : StructuredBuffer_SRV t4 the averages read, float2[Z][Y][X] as the push constants say; StructuredBuffer_UAV u5 the
//                averages written, float2[gz][gy][gx], ANOTHER buffer than t4: no workgroup reads what another one of the launch writes.
//   A direct dispatch of ceil(input / (16, 16, 4)) groups, one per output element.
//
// CONVENTION.  One workgroup of 4 x 8 x 4 threads per output element (gx, gy, gz); thread (tx, ty, tz) covers the 4 x 2 inputs
//   x = 16 * gx + 4 * tx + i, y = 16 * gy + 2 * ty + j of plane z = 4 * gz + tz and sums them row-major (j outer, i inner) from 0.0f:
//   first pass : an input out of range contributes nothing.  w = 1.0f, or 0.0f when the texel's probe (x / 6, z, y / 6) is inactive
//                (flags bit 1 and data.w == 1.0f); sumV = sumV + (w != 0.0f ? v : 0.0f) -- a select: the stale value of a switched-off
//                probe, a NaN included, never reaches the sum -- and sumW = sumW + w;
//   extra pass : an element (a, w) out of range contributes nothing; sumV = sumV + a * w (product, then sum); sumW = sumW + w;
//   the group's 128 pairs, indexed t = tx + 4 * ty + 32 * tz, go through the binary tree p[t] = p[t] + p[t + stride] for t < stride,
//   stride = 64, 32, 16, 8, 4, 2, 1, both members alike; the element written is (sumW > 0.0f ? sumV / sumW : 0.0f, sumW) of p[0].
//   sumW counts texels and stays exact: the first pass refuses a volume of more than 2^24 interior texels.
//
// KERNEL.  The tree runs in LDS (1 KB) with a barrier per stride: no atomics, no order that depends on timing or on which wave runs
// first.  UNTUNED: correctness came first; the strides below 64 stay in LDS rather than in cross-lane moves, and next to the trace
// (tens of milliseconds) the passes are microseconds.  Code object (-Rpass-analysis=kernel-resource-usage): first 18 VGPRs,
// extra 14 VGPRs, occupancy 8 waves per SIMD, LDS 1024 bytes; no scratch in either.
#include "ddgi_update.hip.h"

namespace
{

using namespace interop;

constexpr uint32_t kGroupX = kDDGIReductionThreadsX * kDDGIReductionFootprintX, kGroupY = kDDGIReductionThreadsY * kDDGIReductionFootprintY, kGroupZ = kDDGIReductionThreadsZ;
constexpr uint32_t kThreads = kDDGIReductionThreadsX * kDDGIReductionThreadsY * kDDGIReductionThreadsZ;
static_assert(kGroupX == 16 && kGroupY == 16 && kGroupZ == 4 && kThreads == 128, "the reduction's footprint (GIRenderer.cpp:542-543)");

struct ReductionArgs
{
    uint32_t X, Y, Z;                          // the input's extent
    const float* in;                           // t4: float[Z][Y][X] (first) or float2[Z][Y][X] (extra)
    float2* out;                               // u5: float2[gz][gy][gx]
    const uint2* data; uint32_t dataW, dataPitch;       // t3 (first): texels per row and per slice
    uint32_t classification;                   // first: flags bit 1
};

template <bool FIRST>
__global__ __launch_bounds__(kThreads) void reductionKernel(ReductionArgs a)
{
    __shared__ float sV[kThreads], sW[kThreads];
    const uint32_t t = threadIdx.x + kDDGIReductionThreadsX * threadIdx.y + kDDGIReductionThreadsX * kDDGIReductionThreadsY * threadIdx.z;
    const uint32_t x0 = kGroupX * blockIdx.x + kDDGIReductionFootprintX * threadIdx.x, y0 = kGroupY * blockIdx.y + kDDGIReductionFootprintY * threadIdx.y;
    const uint32_t z = kGroupZ * blockIdx.z + threadIdx.z;
    float sumV = 0.0f, sumW = 0.0f;
    if (z < a.Z) {
        for (uint32_t j = 0; j < kDDGIReductionFootprintY; ++j)
            for (uint32_t i = 0; i < kDDGIReductionFootprintX; ++i) {
                const uint32_t x = x0 + i, y = y0 + j;
                if (x >= a.X || y >= a.Y) continue;
                const uint64_t at = ((uint64_t)z * a.Y + y) * a.X + x;
                if constexpr (FIRST) {
                    const uint2 data = a.data[(uint64_t)z * a.dataPitch + (y / kDDGIIrradianceInteriorTexels) * a.dataW + x / kDDGIIrradianceInteriorTexels];
                    const float w = (a.classification && (float)sp::halfOf(data.y >> 16) == 1.0f) ? 0.0f : 1.0f;
                    const float v = a.in[at];
                    sumV = sumV + (w != 0.0f ? v : 0.0f);
                    sumW = sumW + w;
                } else {
                    const float2 e = ((const float2*)a.in)[at];
                    sumV = sumV + e.x * e.y;
                    sumW = sumW + e.y;
                }
            }
    }
    sV[t] = sumV; sW[t] = sumW;
    __syncthreads();
    for (uint32_t stride = kThreads / 2u; stride >= 1u; stride >>= 1) {
        if (t < stride) { sV[t] = sV[t] + sV[t + stride]; sW[t] = sW[t] + sW[t + stride]; }
        __syncthreads();
    }
    if (t == 0u) {
        const float v = sV[0], w = sW[0];
        a.out[((uint64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = make_float2(w > 0.0f ? cm::div_(v, w) : 0.0f, w);
    }
}

template <bool FIRST>
int recordReduction(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    ReductionArgs a = sp::zeroed<ReductionArgs>();
    const DDGIRootConstants* push = (const DDGIRootConstants*)ctx.constants(1, sizeof(DDGIRootConstants));
    TRHIP_REQUIRE(push, "%s: push constants b1 (the 24-byte DDGIRootConstants: three indices, then reductionInputSizeX, Y, Z) missing or short", name);
    a.X = push->reductionInputSizeX; a.Y = push->reductionInputSizeY; a.Z = push->reductionInputSizeZ;
    TRHIP_REQUIRE(a.X >= 1 && a.Y >= 1 && a.Z >= 1 && (uint64_t)a.X * a.Y * a.Z <= (1u << 24), "%s: reductionInputSize (%u, %u, %u): every extent is at least 1 and the product at most 2^24, "
                  "the count a float sums exactly", name, a.X, a.Y, a.Z);
    const uint64_t inputs = (uint64_t)a.X * a.Y * a.Z;
    const uint32_t gx = (a.X + kGroupX - 1) / kGroupX, gy = (a.Y + kGroupY - 1) / kGroupY, gz = (a.Z + kGroupZ - 1) / kGroupZ;
    TRHIP_REQUIRE(!ctx.indirect && ctx.gx == gx && ctx.gy == gy && ctx.gz == gz, "%s: needs a direct dispatch of ceil(reductionInputSize / (16, 16, 4)) = (%u, %u, %u) groups, one per output element",
                  name, gx, gy, gz);
    trhip_buffer_t* in = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 4);
    trhip_buffer_t* out = ctx.buffer(TRHIP_BIND_STRUCTURED_UAV, 5);
    TRHIP_REQUIRE(out, "%s: needs StructuredBuffer_UAV u5 = the averages written, float2[%u][%u][%u]", name, gz, gy, gx);
    TRHIP_REQUIRE(out->byteSize >= (uint64_t)gx * gy * gz * sizeof(float2), "%s: the averages at u5 hold %llu bytes; %u x %u x %u float2 elements are %llu", name,
                  (unsigned long long)out->byteSize, gx, gy, gz, (unsigned long long)gx * gy * gz * sizeof(float2));
    if (FIRST) {
        ddgiu::Block b;
        if (const int rc = ddgiu::requireBlock(ctx, b)) return rc;
        const DDGIVolumeDesc& D = b.D;
        const uint32_t W = (uint32_t)D.probeCounts[0] * kDDGIIrradianceInteriorTexels, H = (uint32_t)D.probeCounts[2] * kDDGIIrradianceInteriorTexels, P = (uint32_t)D.probeCounts[1];
        TRHIP_REQUIRE(a.X == W && a.Y == H && a.Z == P, "%s: reductionInputSize (%u, %u, %u); probeCounts (%d, %d, %d) have (6 * counts.x, 6 * counts.z, counts.y) = (%u, %u, %u) interior texels", name,
                      a.X, a.Y, a.Z, D.probeCounts[0], D.probeCounts[1], D.probeCounts[2], W, H, P);
        TRHIP_REQUIRE(in, "%s: needs StructuredBuffer_SRV t4 = the probe variability, float[counts.y][6 * counts.z][6 * counts.x]", name);
        TRHIP_REQUIRE(in->byteSize == inputs * sizeof(float), "%s: the probe variability at t4 holds %llu bytes; %u probes of 36 floats are %llu", name, (unsigned long long)in->byteSize,
                      ddgiu::numProbes(D), (unsigned long long)inputs * sizeof(float));
        trhip_texture_t* data;
        if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_SRV, 3, TRHIP_FORMAT_RGBA16_FLOAT, 1, "Texture_SRV t3 = the RGBA16_FLOAT array of probe data", D, data)) return rc;
        a.data = (const uint2*)data->ptr; a.dataW = data->width; a.dataPitch = (uint32_t)(data->slicePitch / data->texelBytes);
        a.classification = (D.flags & kDDGIFlag_Classification) ? 1u : 0u;
    } else {
        TRHIP_REQUIRE(in, "%s: needs StructuredBuffer_SRV t4 = the averages read, float2[%u][%u][%u]", name, a.Z, a.Y, a.X);
        TRHIP_REQUIRE(in->byteSize >= inputs * sizeof(float2), "%s: the averages at t4 hold %llu bytes; %u x %u x %u float2 elements are %llu", name, (unsigned long long)in->byteSize, a.X,
                      a.Y, a.Z, (unsigned long long)inputs * sizeof(float2));
    }
    TRHIP_REQUIRE(in->ptr != out->ptr, "%s: t4 and u5 are the same buffer '%s': a workgroup would read what another one of the launch writes", name, in->name.c_str());
    a.in = (const float*)in->ptr;
    a.out = (float2*)out->ptr;
    sp::launch(ctx, reductionKernel<FIRST>, FIRST ? "reductionKernel<first>" : "reductionKernel<extra>", dim3(gx, gy, gz),
               dim3(kDDGIReductionThreadsX, kDDGIReductionThreadsY, kDDGIReductionThreadsZ), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("ReductionCS_DDGIReductionCS REDUCTION=1", recordReduction<true>, 1);
trhip::ShaderRegistrar r1("ReductionCS_DDGIExtraReductionCS", recordReduction<false>, 0);

} // namespace
