// k_pipeline_stats.hip -- pipeline statistics queries (include/trhip.h, nvrhi::PipelineStatisticsQuery): the counters the
// reference's pipeline would have produced for the dispatches recorded between begin and end.
//
// Reference: BasePassRenderers.cpp:178-179, 202-220, 546-549 (a D3D12 PIPELINE_STATISTICS query around RenderBasePass).
// What moves the counters here:
//   * a direct compute dispatch of a counted entry: groups x [numthreads] CS invocations, known at record time and added
//     once by the end command (trhip_cmd_end_pipeline_stats);
//   * an indirect one: one tiny launch right behind it reads its arguments (statsIndirectKernel);
//   * basepass_AS_Main: one launch behind its cull (statsASKernel) adds 32 x G amplification invocations, 96 mesh invocations
//     per visible meshlet and the triangle count of every visible meshlet.  The counts come from a derived array of ONE
//     BYTE per meshlet of the buffer bound at t4 (trhip_buffer_t::triCounts, derived data like the meshlet cull stream:
//     rebuilt on the device when the buffer's version moves): the 32-byte MeshletData of the visible meshlets would be a
//     gather of ~1.8 GB per frame at C3, the bytes are ~36 B per group.
// Sums of integers: the order of the atomics does not matter, the results are exact.
#include <cstring>

#include "meshlet_exact.hip.h"
#include "trhip_internal.h"

using namespace interop;

namespace
{

constexpr uint32_t kStatsBlock = 256;

__global__ __launch_bounds__(64) void statsAddKernel(unsigned long long* counter, unsigned long long value)
{
    if (threadIdx.x == 0) atomicAdd(counter, value);
}

// groups of an indirect dispatch (its 3 x u32 arguments, read when it has been executed) x [numthreads]
__global__ __launch_bounds__(64) void statsIndirectKernel(const uint32_t* args, unsigned long long threads, unsigned long long* counter)
{
    if (threadIdx.x == 0) atomicAdd(counter, (unsigned long long)args[0] * args[1] * args[2] * threads);
}

// triCounts[i] = (m_VertexAndTriangleCount >> 8) & 0xFF of meshlet i
__global__ __launch_bounds__(256) void triCountsKernel(const MeshletData* __restrict__ meshlets, uint64_t n, uint8_t* __restrict__ out)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride)
        out[i] = (uint8_t)((meshlets[i].m_VertexAndTriangleCount >> 8) & 0xFFu);
}

struct StatsASArgs
{
    MeshletCullArgs a;                             // the pass's cull arguments (records, processing order, masks, instance cache)
    const uint8_t* tri;                            // [numMeshlets] triangle counts
    unsigned long long* counters;                  // the open query's trhip_pipeline_statistics
};

// One lane per group: lane e takes position e of the cull's processing order -- the tile-ordered list when the cull used it
// ({record, instance, first meshlet, count} per entry), else the records in order -- reads the group's mask word and, if any
// bit is set, the 32 triangle-count bytes of its meshlets as 9 aligned dwords, and adds the bytes of the set lanes.  (One
// lane per meshlet lane was 174 us at C3: ~100 dependent rounds of entry -> mask -> byte per lane.)
__global__ __launch_bounds__(kStatsBlock) void statsASKernel(StatsASArgs s)
{
    const MeshletCullArgs& a = s.a;
    const uint32_t G = a.listGroups ? a.listGroups[0] : groupCount(a);        // written by the cull: the G of groupCount()
    const bool usePerm = a.permHeader != nullptr && a.permHeader[0] == 1u && a.permHeader[1] == G;   // the cull's own rule
    const uint32_t stride = gridDim.x * kStatsBlock;
    uint32_t visible = 0;
    uint32_t tris = 0;                             // <= 32 x 255 per group, <= 2^8 groups per lane (the grid, statsEmitAS)
    for (uint32_t e = blockIdx.x * kStatsBlock + threadIdx.x; e < G; e += stride) {
        uint32_t g = e;
        uint64_t first = 0;
        uint32_t cnt = 0;
        if (usePerm) { const uint4 ent = a.perm[e]; g = ent.x; first = ent.z; cnt = ent.w; }
        if (g >= a.recordCapacity) continue;
        uint32_t mask = a.visMask[g];
        if (!mask) continue;
        visible += __popc(mask);
        if (!usePerm) {                            // as exactMeshletVisible (meshlet_exact.hip.h) resolves a record
            const MeshletAmplificationData rec = a.records[g];
            const uint32_t cid = rec.m_InstanceConstIdx < a.numInstances ? rec.m_InstanceConstIdx : 0u;
            const uint32_t lodIdx = rec.m_MeshLOD < kMaxNumMeshLODs ? rec.m_MeshLOD : kMaxNumMeshLODs - 1u;
            const uint2 li = a.cache.lod(cid, lodIdx);
            const uint32_t off = rec.m_MeshletGroupOffset;
            cnt = li.x > off ? li.x - off : 0u;
            first = (uint64_t)li.y + off;
        }
        if (first >= a.numMeshlets) continue;
        cnt = cnt < 32u ? cnt : 32u;
        if (first + cnt > a.numMeshlets) cnt = (uint32_t)(a.numMeshlets - first);
        mask &= cnt >= 32u ? 0xFFFFFFFFu : (1u << cnt) - 1u;
        // bytes [first, first + 32) lie in the 9 dwords from first & ~3 (the array is padded: statsEmitAS)
        const uint32_t* w = reinterpret_cast<const uint32_t*>(s.tri) + (first >> 2);
        const uint32_t sh = (uint32_t)(first & 3u);
        uint32_t words[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) words[k] = w[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            uint32_t v = __builtin_amdgcn_alignbyte(words[k + 1], words[k], sh);   // bytes 4k .. 4k + 3 of the group
            const uint32_t m4 = mask >> (4 * k);
            v &= ((m4 & 1u) ? 0xFFu : 0u) | ((m4 & 2u) ? 0xFF00u : 0u) | ((m4 & 4u) ? 0xFF0000u : 0u) | ((m4 & 8u) ? 0xFF000000u : 0u);
            tris += (v & 0xFFu) + ((v >> 8) & 0xFFu) + ((v >> 16) & 0xFFu) + (v >> 24);
        }
    }
    // wave, then workgroup, then one atomic per counter and workgroup
    for (int o = 32; o > 0; o >>= 1) {
        visible += __shfl_xor(visible, o);
        tris += __shfl_xor(tris, o);
    }
    __shared__ uint32_t s_vis[kStatsBlock / 64], s_tri[kStatsBlock / 64];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { s_vis[wave] = visible; s_tri[wave] = tris; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long v = 0, t = 0;
        for (uint32_t w = 0; w < kStatsBlock / 64; ++w) { v += s_vis[w]; t += s_tri[w]; }
        if (v) atomicAdd(s.counters + trhip::kStatMS, 96ull * v);             // kMeshletShaderThreadGroupSize
        if (t) atomicAdd(s.counters + trhip::kStatMSPrim, t);
        if (blockIdx.x == 0 && G) atomicAdd(s.counters + trhip::kStatAS, 32ull * G);   // [numthreads(32)] AS_Main groups
    }
}

// at submission time, on the stream of the stats command: no-op unless the meshlet buffer was written since the array was built
int triCountsLaunchBuild(trhip_buffer_t* meshlets, hipStream_t s)
{
    const trhip::Stamp from = { meshlets->version };
    if (meshlets->triCounts.current(from)) return TRHIP_OK;
    const uint64_t n = meshlets->byteSize / sizeof(MeshletData);
    const uint64_t blocks = (n + 255u) / 256u;
    TRHIP_LAUNCH(triCountsKernel, dim3((uint32_t)(blocks < 65536u ? (blocks ? blocks : 1u) : 65536u)), dim3(256), 0, s,
                 (const MeshletData*)meshlets->ptr, n, (uint8_t*)meshlets->triCounts.ptr);
    meshlets->triCounts.markBuilt(from);
    return trhip::launchStatus("triCountsKernel");
}

bool startsWith(const char* s, const char* prefix) { return strncmp(s, prefix, strlen(prefix)) == 0; }

} // namespace

namespace trhip
{

uint32_t statsCSThreads(const char* name)
{
    if (startsWith(name, "gpuculling_CS_GPUCulling")) return 32;            // [numthreads(kNumThreadsPerWave, 1, 1)]
    if (!strcmp(name, "gpuculling_CS_BuildLateCullIndirectArgs")) return 1;
    if (!strcmp(name, "minmaxdownsample_CS_Main")) return 64;               // [numthreads(8, 8, 1)]
    if (startsWith(name, "ffx_spd_downsample_pass_CS")) return 256;         // SPD's 256-thread groups
    if (startsWith(name, "updateinstanceconsts_")) return 32;
    if (startsWith(name, "giprobevisualization_CS_")) return 32;            // the cull and LoadGIProbes; the draw (_PS_) is no compute shader
    return 0;
}

int statsLaunchAdd(unsigned long long* counter, uint64_t value, hipStream_t s)
{
    TRHIP_LAUNCH(statsAddKernel, dim3(1), dim3(64), 0, s, counter, (unsigned long long)value);
    return launchStatus("statsAddKernel");
}

int statsEmitIndirectCS(trhip_cmdlist_t* cl, trhip_buffer_t* args, uint32_t argsOffset, uint32_t threads)
{
    unsigned long long* counter = cl->openStats->counters + kStatCS;
    const uint32_t* p = (const uint32_t*)((const char*)args->ptr + argsOffset);
    cl->use(args->ptr, cl->ops.size(), false);
    cl->use(cl->openStats->counters, cl->ops.size(), true);
    cl->ops.push_back({ "", [p, threads, counter](hipStream_t s) {
        TRHIP_LAUNCH(statsIndirectKernel, dim3(1), dim3(64), 0, s, p, (unsigned long long)threads, counter);
        return launchStatus("statsIndirectKernel"); } });
    cl->ops.back().kind = "pipeline_stats";
    cl->peephole = trhip_cmdlist_t::Peephole();
    return TRHIP_OK;
}

int statsEmitAS(const DispatchCtx& ctx, const ::MeshletCullArgs& a, trhip_buffer_t* meshlets, trhip_buffer_t* records,
                trhip_buffer_t* instances, trhip_buffer_t* meshData, bool side)
{
    trhip_cmdlist_t* cl = ctx.cl;
    const uint64_t n = meshlets->byteSize / sizeof(MeshletData);
    int rc = meshlets->triCounts.allocate(meshlets->dev, ((n + 255u) & ~uint64_t(255)) + 256u);   // + padding: statsASKernel reads 9 dwords per group
    if (rc != TRHIP_OK) return rc;
    StatsASArgs s;
    memset(&s, 0, sizeof s);
    s.a = a;
    s.tri = (const uint8_t*)meshlets->triCounts.ptr;
    s.counters = cl->openStats->counters;
    uint64_t grid = ((uint64_t)a.recordCapacity + kStatsBlock - 1) / kStatsBlock;
    if (grid > (uint64_t)ctx.computeUnits() * 8u) grid = (uint64_t)ctx.computeUnits() * 8u;
    if (grid == 0) grid = 1;
    const void* recordedMeshlets = meshlets->ptr;
    auto fn = [s, grid, meshlets, recordedMeshlets](hipStream_t st) {
        if (meshlets->ptr != recordedMeshlets)
            return fail(TRHIP_ERR_STATE, "basepass_AS_Main: the meshlet buffer was bound to other memory after this command list was recorded: record it again");
        int brc = triCountsLaunchBuild(meshlets, st);     // no-op unless the meshlet buffer was written since the array was built
        if (brc != TRHIP_OK) return brc;
        TRHIP_LAUNCH(statsASKernel, dim3((uint32_t)grid), dim3(kStatsBlock), 0, st, s);
        return launchStatus("statsASKernel"); };
    if (side && cl->dev->sideStream) {
        // beside the list build: every allocation it reads, so that a later main-stream write waits for it, and the ones it
        // writes, so that the end command (and the next execution's begin) wait for it
        ctx.emitSide("stats", std::move(fn), { { a.listGroups, false }, { a.visMask, false }, { records->ptr, false }, { instances->ptr, false },
                                               { meshData->ptr, false }, { meshlets->ptr, false }, { meshlets->triCounts.ptr, true },
                                               { s.counters, true } });
    } else {
        cl->use(meshlets->triCounts.ptr, cl->ops.size(), true);
        cl->use(s.counters, cl->ops.size(), true);
        ctx.emit("stats", std::move(fn));
    }
    cl->peephole = trhip_cmdlist_t::Peephole();
    return TRHIP_OK;
}

} // namespace trhip
