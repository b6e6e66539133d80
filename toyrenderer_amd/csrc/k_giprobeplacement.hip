// k_giprobeplacement.hip -- the three passes that place and switch the probes of the DDGI volume, recorded behind the two blends of
// GIRenderer::RenderDDGI (source/GIRenderer.cpp:513-527, switched on at :80-83): "giprobetrace_CS_ProbeTraceFixedRays" (the
// project's own), "ProbeRelocationCS_DDGIProbeRelocationCS" and "ProbeClassificationCS_DDGIProbeClassificationCS".  The RTXGI SDK
// is not part of this project: the passes are the project's own statement of the published algorithm (Majercik et al., JCGT 2019
// and "Scaling Probe-Based Real-Time Dynamic Global Illumination for Production", JCGT 2021), tests/ddgi_placement_ref.c is the
// definition and the functions below repeat it word for word.  The query, the trace and the blends already honour what these
// passes write: data.xyz moves a probe with flags bit 0, data.w == 1 switches it off with flags bit 1.
//
// DEVIATION.  The SDK keeps the first 32 of a probe's rays unrotated for these passes and out of the blend.  Here the
// 256 blended rays stay as they are and the 32 fixed rays are traced by a pass of their own, for EVERY probe, whatever its state:
// that is what lets a switched-off probe wake up (the probe trace writes nothing for it).
//
// BINDINGS.  b0 of all three: ddgiu::Block (160 bytes); probeMinFrontfaceDistance and probeFixedRayBackfaceThreshold are its fields.
//   fixed rays      t0 the 64-byte DDGIVolumeDesc, t1 the RGBA16_FLOAT array of probe data, t4..t6 and t8..t13 the acceleration
//                   structure in the probe trace's slots (no materials), u0 float[numProbes * 32]; a direct dispatch of
//                   ceil(numProbes * 32 / 64) groups of 64: one thread per (ray, probe), a wave holds two probes;
//   relocation, classification: StructuredBuffer_UAV u0 the fixed-ray distances, Texture_UAV u3 the RGBA16_FLOAT data array (the
//                   reference's registers), created with the UAV bit; a direct dispatch of ceil(numProbes / 32) groups; relocation
//                   is refused unless flags bit 0 is set, classification unless bit 1 is.
//
// CONVENTION (binary32, no contraction, fma only in dot3, / and sqrt correctly rounded; S the spacing).
//   fixed ray i     direction ddgiu::fixedRayDirection(i) (32 for 256, no rotation), origin ddgiu::probePosition, TMin 0, TMax
//                   probeMaxRayDistance, rw::closestHit; a miss stores 1e27f, a front face t, a back face -0.2f * t; a probe's state is
//                   not looked at;
//   relocation      o = (half(data.x) * S.x, half(data.y) * S.y, half(data.z) * S.z).  Over the rays 0..31 in order, from closestBack =
//                   closestFront = 1e27f, farthestFront = 0, iBack = iFront = iFar = -1: d < 0: ++back, h = d * -5.0f, h < closestBack
//                   takes (h, i); else d < closestFront takes (d, i) as the closest front; ELSE d > farthestFront takes (d, i) as the
//                   farthest (QUIRK: a new closest ray is not offered as the farthest; a miss is a front face at 1e27f).
//                   A: iBack != -1 and (float)back / 32.0f > probeFixedRayBackfaceThreshold: full = o + dir(iBack) * (closestBack +
//                   probeMinFrontfaceDistance * 0.5f).  B: else closestFront < probeMinFrontfaceDistance: with iFront != -1, iFar != -1 and
//                   dot3(dir(iFront), dir(iFar)) <= 0.5f, full = o + dir(iFar) * fminf(farthestFront, 1.0f) (QUIRK: the 1.0 is in world
//                   units), else no move.  C: else closestFront > probeMinFrontfaceDistance: len = sqrt(dot3(o, o)); len > 0: full = o +
//                   (o * (-1.0f / len)) * fminf(closestFront - probeMinFrontfaceDistance, len), else no move.  Otherwise no move.
//                   A move is taken only when n = full / S has dot3(n, n) < 0.2025f (0.45 of a cell).  The store is data.xyz =
//                   binary16(o / S), nearest even; data.w keeps its bits; a probe that does not move is rewritten;
//   classification  back = the count of d < 0; (float)back / 32.0f > probeFixedRayBackfaceThreshold: state 1.  Otherwise over the rays
//                   with d >= 0 in order: plane = the minimum over the axes a of (|dir.a| == 0 ? 1e27f : S.a / fmaxf(|dir.a|, 1e-6f));
//                   the first ray with d <= plane makes the state 0; if none does, the state is 1.  The store is data.w = binary16 of
//                   the state; xyz keeps its bits.
//
// KERNELS.  The fixed-ray trace is the probe trace without its shading: one rw::closestHit per thread (ray_walk.hip.h states the
// walk, the triangle test and the fetch once for every tracing pass), no shadow ray, no query.
// Relocation and classification run one thread per probe.  The dispatch has the reference's ceil(numProbes / 32) groups; the launch
// packs the probes into workgroups of one full wave, 64 probes each, whose first 32 threads compute the 32 directions once into
// LDS (384 bytes).  A probe reads 128 bytes of distances and one 8-byte texel: the work is tiny next to the traces.  UNTUNED.
// Code objects (-Rpass-analysis=kernel-resource-usage): fixedRayTraceKernel 56 VGPRs, 4 spilled scalar registers, occupancy 7 waves
// per SIMD; placementKernel <relocation> 17 and <classification> 44 VGPRs, occupancy 8, LDS 384 bytes, no spills; no scratch in any.
// MEASURED (tools/ddgi_placement_cost.py, the generated city of 2251 instances, 13 468 probes, one MI355X; profiles/ray_walk/): 10.8
// ms, 9.7 us and 14.6 us per update, next to 45.5 ms for the probe trace of the 8 966 probes still active.  The fixed-ray trace is above an eighth
// of the probe trace: its 6 734 waves are a single resident set, so it lasts as long as its slowest walks (profiles/ddgi/README.md).
#include "ddgi_update.hip.h"

namespace
{

using namespace interop;
using cm::F3;

constexpr uint32_t kWave = 64, kPlacementGroup = 32;      // kPlacementGroup: probes per group of the DISPATCH; the launch uses whole waves

struct FixedRayArgs
{
    ddgiu::Block b;
    rw::SceneArgs scene;
    const uint2* data; uint32_t dataW, dataPitch;      // t1
    float* distances;                                  // u0
    uint32_t numProbes;
};

struct PlacementArgs
{
    ddgiu::Block b;
    const float* distances;                            // u0
    uint2* data; uint32_t dataW, dataPitch;            // u3
    uint32_t numProbes;
};

__global__ __launch_bounds__(kWave) void fixedRayTraceKernel(FixedRayArgs a)
{
    const DDGIVolumeDesc& D = a.b.D;
    const uint32_t gid = blockIdx.x * kWave + threadIdx.x, probe = gid / kDDGIFixedRays, ray = gid % kDDGIFixedRays;
    if (probe >= a.numProbes) return;
    const ddgiu::I3 c = ddgiu::probeCoords(probe, D);
    const uint2 data = a.data[(uint64_t)c.y * a.dataPitch + (uint32_t)c.z * a.dataW + (uint32_t)c.x];
    const rw::Hit hit = rw::closestHit(a.scene, ddgiu::probePosition(D, c, data), ddgiu::fixedRayDirection(ray), 0.0f, a.b.k.probeMaxRayDistance);
    a.distances[(uint64_t)probe * kDDGIFixedRays + ray] = hit.inst == 0xFFFFFFFFu ? 1e27f : (hit.front ? hit.t : -0.2f * hit.t);
}

// tests/ddgi_placement_ref.c: relocate_probe.  dir: the 32 fixed directions; returns the new data.xyz as three binary16 words.
__device__ __forceinline__ void relocateProbe(const DDGIUpdateConsts& k, F3 S, const float* d, const float (*dir)[3], uint32_t h[3])
{
    const float minFront = k.probeMinFrontfaceDistance;
    F3 o = { (float)sp::halfOf(h[0]) * S.x, (float)sp::halfOf(h[1]) * S.y, (float)sp::halfOf(h[2]) * S.z };
    float closestBack = 1e27f, closestFront = 1e27f, farthestFront = 0.0f;
    int iBack = -1, iFront = -1, iFar = -1;
    uint32_t back = 0;
    for (int i = 0; i < (int)kDDGIFixedRays; ++i) {
        const float di = d[i];
        if (di < 0.0f) {
            ++back;
            const float undone = di * -5.0f;
            if (undone < closestBack) { closestBack = undone; iBack = i; }
        }
        else if (di < closestFront) { closestFront = di; iFront = i; }
        else if (di > farthestFront) { farthestFront = di; iFar = i; }
    }
    bool move = false;
    F3 full = o;
    if (iBack != -1 && cm::div_((float)back, (float)kDDGIFixedRays) > k.probeFixedRayBackfaceThreshold) {
        const float s = closestBack + minFront * 0.5f;
        full = { o.x + dir[iBack][0] * s, o.y + dir[iBack][1] * s, o.z + dir[iBack][2] * s };
        move = true;
    } else if (closestFront < minFront) {
        if (iFront != -1 && iFar != -1 && cm::dot3({ dir[iFront][0], dir[iFront][1], dir[iFront][2] }, { dir[iFar][0], dir[iFar][1], dir[iFar][2] }) <= 0.5f) {
            const float s = cm::min_(farthestFront, 1.0f);
            full = { o.x + dir[iFar][0] * s, o.y + dir[iFar][1] * s, o.z + dir[iFar][2] * s };
            move = true;
        }
    } else if (closestFront > minFront) {
        const float len = cm::sqrt_(cm::dot3(o, o));
        if (len > 0.0f) {
            const float inv = cm::div_(-1.0f, len), s = cm::min_(closestFront - minFront, len);
            full = { o.x + (o.x * inv) * s, o.y + (o.y * inv) * s, o.z + (o.z * inv) * s };
            move = true;
        }
    }
    if (move) {
        const F3 n = { cm::div_(full.x, S.x), cm::div_(full.y, S.y), cm::div_(full.z, S.z) };
        if (cm::dot3(n, n) < 0.2025f) o = full;
    }
    h[0] = sp::halfBits(cm::div_(o.x, S.x)); h[1] = sp::halfBits(cm::div_(o.y, S.y)); h[2] = sp::halfBits(cm::div_(o.z, S.z));
}

// tests/ddgi_placement_ref.c: classify_probe.  Returns the state, 0 (active) or 1.
__device__ __forceinline__ float classifyProbe(const DDGIUpdateConsts& k, F3 S, const float* d, const float (*dir)[3])
{
    uint32_t back = 0;
    for (int i = 0; i < (int)kDDGIFixedRays; ++i) back += d[i] < 0.0f ? 1u : 0u;
    if (cm::div_((float)back, (float)kDDGIFixedRays) > k.probeFixedRayBackfaceThreshold) return 1.0f;
    for (int i = 0; i < (int)kDDGIFixedRays; ++i) {
        if (d[i] < 0.0f) continue;
        const float ax = __builtin_fabsf(dir[i][0]), ay = __builtin_fabsf(dir[i][1]), az = __builtin_fabsf(dir[i][2]);
        const float px = ax == 0.0f ? 1e27f : cm::div_(S.x, cm::max_(ax, 1e-6f)), py = ay == 0.0f ? 1e27f : cm::div_(S.y, cm::max_(ay, 1e-6f)),
                    pz = az == 0.0f ? 1e27f : cm::div_(S.z, cm::max_(az, 1e-6f));
        if (d[i] <= cm::min_(cm::min_(px, py), pz)) return 0.0f;
    }
    return 1.0f;
}

template <bool RELOCATE>
__global__ __launch_bounds__(kWave) void placementKernel(PlacementArgs a)
{
    static_assert(kDDGIFixedRays <= kWave, "thread i of a workgroup computes fixed direction i");
    __shared__ float sDir[kDDGIFixedRays][3];
    if (threadIdx.x < kDDGIFixedRays) {
        const F3 mine = ddgiu::fixedRayDirection(threadIdx.x);
        sDir[threadIdx.x][0] = mine.x; sDir[threadIdx.x][1] = mine.y; sDir[threadIdx.x][2] = mine.z;
    }
    __syncthreads();
    const DDGIVolumeDesc& D = a.b.D;
    const uint32_t probe = blockIdx.x * kWave + threadIdx.x;
    if (probe >= a.numProbes) return;
    const ddgiu::I3 c = ddgiu::probeCoords(probe, D);
    uint2* texel = a.data + (uint64_t)c.y * a.dataPitch + (uint32_t)c.z * a.dataW + (uint32_t)c.x;
    const uint2 old = *texel;
    const F3 S = { D.probeSpacing[0], D.probeSpacing[1], D.probeSpacing[2] };
    const float* d = a.distances + (uint64_t)probe * kDDGIFixedRays;
    if constexpr (RELOCATE) {
        uint32_t h[3] = { old.x & 0xFFFFu, old.x >> 16, old.y & 0xFFFFu };
        relocateProbe(a.b.k, S, d, sDir, h);
        *texel = make_uint2(h[0] | h[1] << 16, h[2] | (old.y & 0xFFFF0000u));
    } else {
        *texel = make_uint2(old.x, (old.y & 0xFFFFu) | sp::halfBits(classifyProbe(a.b.k, S, d, sDir)) << 16);
    }
}

int recordFixedRayTrace(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    FixedRayArgs a = sp::zeroed<FixedRayArgs>();
    if (const int rc = ddgiu::requireBlock(ctx, a.b)) return rc;
    const DDGIVolumeDesc& D = a.b.D;
    const uint32_t probes = a.numProbes = ddgiu::numProbes(D);
    if (const int rc = ddgiu::requireLinearDispatch(ctx, (uint64_t)probes * kDDGIFixedRays, kWave, "ceil(numProbes * 32 / 64)")) return rc;
    trhip_buffer_t* descBuffer = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 0);
    TRHIP_REQUIRE(descBuffer && descBuffer->byteSize >= sizeof(DDGIVolumeDesc), "%s: needs StructuredBuffer_SRV t0 = the 64-byte DDGIVolumeDesc", name);
    trhip_texture_t* data;
    if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_SRV, 1, TRHIP_FORMAT_RGBA16_FLOAT, 1, "Texture_SRV t1 = the RGBA16_FLOAT array of probe data", D, data)) return rc;
    if (const int rc = ddgiu::requireFixedRayDistances(ctx, probes, a.distances)) return rc;
    if (const int rc = rw::bindScene(ctx, ddgiu::kSceneSlots, false, a.scene)) return rc;
    a.data = (const uint2*)data->ptr; a.dataW = data->width; a.dataPitch = (uint32_t)(data->slicePitch / data->texelBytes);
    sp::launch(ctx, fixedRayTraceKernel, "fixedRayTraceKernel", dim3((probes * kDDGIFixedRays + kWave - 1) / kWave), dim3(kWave), a);
    return TRHIP_OK;
}

template <bool RELOCATE>
int recordPlacement(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    PlacementArgs a = sp::zeroed<PlacementArgs>();
    if (const int rc = ddgiu::requireBlock(ctx, a.b)) return rc;
    const DDGIVolumeDesc& D = a.b.D;
    TRHIP_REQUIRE(D.flags & (RELOCATE ? kDDGIFlag_Relocation : kDDGIFlag_Classification), "%s: DDGIVolumeDesc flags = %u have %s off: nothing would read what the pass writes", name, D.flags,
                  RELOCATE ? "relocation (bit 0)" : "classification (bit 1)");
    const uint32_t probes = a.numProbes = ddgiu::numProbes(D);
    if (const int rc = ddgiu::requireLinearDispatch(ctx, probes, kPlacementGroup, "ceil(numProbes / 32)")) return rc;
    float* distances;
    if (const int rc = ddgiu::requireFixedRayDistances(ctx, probes, distances)) return rc;
    trhip_texture_t* data;
    if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_UAV, 3, TRHIP_FORMAT_RGBA16_FLOAT, 1, "Texture_UAV u3 = the RGBA16_FLOAT array of probe data", D, data)) return rc;
    a.distances = distances;
    a.data = (uint2*)data->ptr; a.dataW = data->width; a.dataPitch = (uint32_t)(data->slicePitch / data->texelBytes);
    sp::launch(ctx, placementKernel<RELOCATE>, RELOCATE ? "placementKernel<relocation>" : "placementKernel<classification>", dim3((probes + kWave - 1) / kWave),
               dim3(kWave), a);
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("giprobetrace_CS_ProbeTraceFixedRays", recordFixedRayTrace, 0);
trhip::ShaderRegistrar r1("ProbeRelocationCS_DDGIProbeRelocationCS", recordPlacement<true>, 0);
trhip::ShaderRegistrar r2("ProbeClassificationCS_DDGIProbeClassificationCS", recordPlacement<false>, 0);

} // namespace
