// trhip_internal.h -- internals of the C-ABI back end (include/trhip.h).  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include <hip/hip_ext.h>

#include "../../include/trhip.h"
#include "ShaderInterop.h"

namespace trhip
{

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int hipfail(hipError_t e, const char* what);

#define TRHIP_HIP(expr)                                                        \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess) return ::trhip::hipfail(_e, #expr);              \
    } while (0)

#define TRHIP_REQUIRE(cond, ...)                                               \
    do {                                                                       \
        if (!(cond)) return ::trhip::fail(TRHIP_ERR_INVALID, __VA_ARGS__);     \
    } while (0)

struct ProfilePending { std::string name; hipEvent_t e0, e1; };
struct ProfileAccum { uint64_t launches = 0; double totalMs = 0; };

} // namespace trhip

struct trhip_device_t;

namespace trhip
{

// What derived data was last built from: the version of its owner (trhip_buffer_t::version) and, for data that also reads a
// second resource (the instance cull cache reads the mesh table), that resource's pointer and version.  Versions start at 1,
// so the zero stamp is never current.
struct Stamp
{
    uint64_t version = 0;
    const void* other = nullptr;
    uint64_t otherVersion = 0;
    bool operator==(const Stamp& s) const { return version == s.version && other == s.other && otherVersion == s.otherVersion; }
};

// Back-end private device memory DERIVED from a buffer or texture the caller owns, and freed with it (freeDerived).  Its size
// is a function of the owner's, which never changes after creation, so it is allocated once, by the first pass that needs it.
// Data rebuilt from the owner's contents is rebuilt exactly when the stamp of its sources is no longer `built`.
struct DerivedData
{
    void* ptr = nullptr;
    uint64_t bytes = 0;
    Stamp built;

    int allocate(const trhip_device_t* dev, uint64_t size);
    bool current(const Stamp& s) const { return built == s; }
    void markBuilt(const Stamp& s) { built = s; }
};

} // namespace trhip

struct trhip_device_t
{
    int index = 0;
    hipStream_t stream = nullptr;
    bool ownsStream = false;
    uint32_t computeUnits = 0;
    uint32_t waveSize = 0;
    uint64_t totalMem = 0;

    // Second stream for work whose results nothing later in the frame consumes (the ordered-list build of
    // a cull pass): it overlaps the passes that follow.  Consecutive side ops form a RUN that ends with an
    // event; a main-stream command that uses memory a run touched first waits for that run's event
    // (execute-time check, trhip_queue_execute), and every host-side synchronisation covers both streams.
    static constexpr uint32_t kSideRuns = 16;
    hipStream_t sideStream = nullptr;
    hipEvent_t evFork = nullptr;
    bool forkSignalled = false;                // evFork already carries the completion of the main stream's last kernel (trhip::LaunchTap)
    hipEvent_t runDone[kSideRuns] = {};
    uint64_t sideRunCounter = 0;               // id of the last finished run (ids start at 1)
    uint64_t mainWaitedUpTo = 0;               // the main stream is ordered after all runs <= this id
    std::unordered_map<const void*, uint64_t> sideWriter;  // allocation -> last run that wrote it
    std::unordered_map<const void*, uint64_t> sideReader;  // allocation -> last run that read it
    int syncAll();                             // host wait for both streams

    std::mutex mutex;
    bool profiling = false;
    std::string profileFilter;              // "" = every named op; else only ops of exactly this name (trhip_profile_filter)
    std::vector<trhip::ProfilePending> pending;
    std::vector<hipEvent_t> eventPool;
    std::map<std::string, trhip::ProfileAccum> accum;
    std::vector<std::string> accumOrder;

    hipEvent_t acquireEvent();
    int drainProfile();

    // The sRGB-to-linear TABLE of SRGBA8_UNORM textures (trhip_srgb_table: 256 floats), on the device from the first texture
    // table on; the textured G-buffer resolve stages it in LDS (material_textures.hip.h).
    trhip::DerivedData srgbTable;
};

struct trhip_heap_t
{
    trhip_device_t* dev = nullptr;
    void* base = nullptr;
    uint64_t bytes = 0;
    std::atomic<int> rc{1};
};

namespace trhip
{

// An owner's release: drains both streams of the device once (commands in flight may still use the data), then frees them.
void freeDerived(trhip_device_t* dev, std::initializer_list<DerivedData*> all);

} // namespace trhip

struct trhip_buffer_t
{
    trhip_device_t* dev = nullptr;
    uint64_t byteSize = 0;
    uint32_t structStride = 0;
    bool canHaveUAVs = false, isDrawIndirectArgs = false, isVirtual = false, isVolatileConstant = false;
    std::string name;
    void* ptr = nullptr;
    bool owns = false;
    trhip_heap_t* heap = nullptr;
    std::vector<uint8_t> shadow; // current version of a volatile constant buffer (record time)
    // Bumped, in SUBMISSION order, by every command that writes the buffer (trhip_queue_execute), by uploads and by
    // bind_memory: the derived data below records the version it was built from (trhip::Stamp).
    std::atomic<uint64_t> version{1};
    // Derived data (trhip::DerivedData); which of it a buffer has depends on what it is bound as.
    // Instance buffers: the INSTANCE CULL CACHE (k_gpuculling.hip), a compact SoA restatement of what the instance cull reads
    // per instance (world-space bounding sphere, max scale, LOD table) -- 88 B instead of the 300 B of AoS instance + mesh
    // records it would otherwise pull through HBM every frame.  Built from this buffer and the mesh table.
    trhip::DerivedData cullCache;
    // Meshlet buffers: the MESHLET CULL STREAM (k_basepass_as.hip), the 20 bytes of each 32-byte MeshletData the cull reads
    // (bounding sphere, cone word) as two dense arrays.
    trhip::DerivedData cullStream;
    // Meshlet buffers, once a pipeline statistics query has covered a basepass_AS_Main dispatch: the TRIANGLE COUNTS, one
    // byte per meshlet ((m_VertexAndTriangleCount >> 8) & 0xFF, k_pipeline_stats.hip).
    trhip::DerivedData triCounts;
    // Amplification record buffers: the screen-tile-sorted PROCESSING ORDER of the records the instance pass wrote into this
    // buffer, which the meshlet cull follows (k_gpuculling.hip / k_basepass_as.hip).  Rewritten by every instance pass: no stamp.
    trhip::DerivedData order;
    // Mask buffers: the list build's GROUP COUNT word, written by the meshlet cull (k_basepass_as.hip).  No stamp.
    trhip::DerivedData listCount;
    std::atomic<int> rc{1};
};

struct trhip_texture_t
{
    trhip_device_t* dev = nullptr;
    uint32_t width = 0, height = 0, mips = 0, format = 0;
    uint32_t texelBytes = 0;
    uint32_t blockBytes = 0;                   // trhip_format_block_bytes(format): nonzero for a block-compressed texture, whose texelBytes is 0
    bool isUAV = false, isVirtual = false;
    // A 2D ARRAY texture (trhip_texture_create_array): arraySize slices of one mip, slice k at byte k * slicePitch (256-byte
    // aligned).  0: not an array.  Only "deferredlighting_PS_Main" / "_Debug" take one, at t6..t8 (recordDispatch refuses the rest).
    uint32_t arraySize = 0;
    uint64_t slicePitch = 0;
    // Texture streaming (include/trhip.h).  A streamable material texture: log2 of its region size (0: not streamable).  A feedback
    // map (TRHIP_SAMPLER_FEEDBACK_FORMAT): `paired` is its material texture, retained; the shifts are that texture's.
    uint32_t regionShiftX = 0, regionShiftY = 0;
    trhip_texture_t* paired = nullptr;
    std::string name;
    uint64_t mipOffset[16] = {};
    uint64_t totalBytes = 0;
    void* ptr = nullptr;
    bool owns = false;
    trhip_heap_t* heap = nullptr;
    // Derived data (trhip::DerivedData) of an R16F min-HZB: the FOOTPRINT-MIN TABLE (k_hzb.hip).  For every mip and
    // every possible bilinear footprint origin (x0,y0) in [-1,w-1]x[-1,h-1] it holds the min of the 2x2
    // edge-clamped footprint, so the meshlet cull kernel resolves SampleLevel(min-reduction) with ONE 2-byte
    // load.  Built from `version` (see trhip_buffer_t::version).
    trhip::DerivedData quad;
    uint32_t quadOffset[16] = {};              // first entry of mip k; mip k has ((w_k >> 3) + 1) * ((h_k >> 3) + 1) blocks of 8 x 8 entries
    uint32_t quadTotal = 0;
    std::atomic<uint64_t> version{1};
    std::atomic<int> rc{1};

    uint32_t mipW(uint32_t k) const { return (width >> k) ? (width >> k) : 1u; }
    uint32_t mipH(uint32_t k) const { return (height >> k) ? (height >> k) : 1u; }
    void* mipPtr(uint32_t k) const { return (char*)ptr + mipOffset[k]; }
    // bytes of level k without its padding: texels, or 4 x 4 blocks of a block-compressed format
    uint64_t mipBytes(uint32_t k) const
    {
        return blockBytes ? (uint64_t)((mipW(k) + 3u) / 4u) * ((mipH(k) + 3u) / 4u) * blockBytes : (uint64_t)mipW(k) * mipH(k) * texelBytes;
    }
};

// The texture table (include/trhip.h): the stand-in of ResourceDescriptorHeap[...].  slots[i] is the retained texture behind
// descriptor index i (nullptr: empty); `entries` its device-side form, capacity x mtex::TableEntry (material_textures.hip.h),
// rewritten entry by entry, synchronously, by trhip_texture_table_set / _clear.
struct trhip_texture_table_t
{
    trhip_device_t* dev = nullptr;
    std::vector<trhip_texture_t*> slots;
    trhip::DerivedData entries;
    uint32_t streamEntries = 0;                // min-mip (R8_UINT) and feedback entries among `slots`: nonzero selects the #streamed resolve
    std::atomic<int> rc{1};
};

struct trhip_timer_t
{
    trhip_device_t* dev = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool began = false, ended = false;
};

struct MeshletCullArgs;                           // meshlet_exact.hip.h

// A pipeline statistics query (include/trhip.h): trhip_pipeline_statistics on the device, zeroed by the begin command and
// added to by the commands recorded up to the end command, whose completion `done` marks.
struct trhip_pipeline_stats_t
{
    trhip_device_t* dev = nullptr;
    unsigned long long* counters = nullptr;      // device: 14 x u64 in the order of trhip_pipeline_statistics
    hipEvent_t done = nullptr;
    bool began = false, ended = false;
};

// A read-back resource (include/trhip.h): `slots` slots of bytesPerSlot pinned host bytes; done[k] is recorded behind slot k's
// last copy, written[k] is what that copy wrote (0: no executed list has written the slot).
struct trhip_readback_t
{
    trhip_device_t* dev = nullptr;
    uint8_t* host = nullptr;
    uint64_t bytesPerSlot = 0;
    std::vector<hipEvent_t> done;
    std::vector<uint64_t> written;
};

namespace trhip
{

// Indices into trhip_pipeline_statistics (the counters a dispatch can move).
enum : uint32_t { kStatCS = 10, kStatAS = 11, kStatMS = 12, kStatMSPrim = 13, kStatWords = 14 };

struct Op
{
    std::string name;                       // profile key ("" = not profiled)
    std::function<int(hipStream_t)> fn;
    const char* kind = "dispatch";          // what the op is, for the host-side submission profile (TRHIP_HOST_PROFILE=1) and the fork rule (LaunchTap)
    uint8_t lane = 0;                       // 0 main stream, 1 side stream (see DispatchCtx::emitSide)
    struct Access { const void* ptr; bool write; };
    std::vector<Access> touched;            // side ops: allocations read / written (base pointers)
};

} // namespace trhip

struct trhip_cmdlist_t
{
    trhip_device_t* dev = nullptr;
    bool open = false;
    std::vector<trhip::Op> ops;
    std::vector<trhip_buffer_t*> heldBuffers;
    std::vector<trhip_texture_t*> heldTextures;
    std::vector<trhip_texture_table_t*> heldTables;
    std::vector<std::string> markers;
    // The pipeline statistics query open in this recording (nullptr: none) and the CS invocations of its direct dispatches,
    // known on the host and added once by the end command.
    trhip_pipeline_stats_t* openStats = nullptr;
    uint64_t statsHostCS = 0;

    struct ScratchBlock { void* ptr; size_t bytes; size_t used; };
    std::vector<ScratchBlock> scratch;

    // Consecutive buffer clears are issued as ONE kernel launch (a frame has ~11 clears of a few bytes
    // each; a launch costs ~5 us on both sides of the queue).
    struct ClearBatch { static constexpr uint32_t kMax = 32; void* ptr[kMax]; uint64_t words[kMax]; uint32_t value[kMax]; uint32_t count = 0; };
    std::shared_ptr<ClearBatch> openClearBatch;    // batch of the LAST op in `ops`, if that op is a clear
    size_t openClearOp = SIZE_MAX;
    // A clear of memory that no earlier command of this recording uses joins the FIRST clear launch of the recording
    // (it is equivalent there, and off the chain of dependent small launches later in the frame); a clear of memory
    // that still holds the value (cleared to it earlier in this recording, not written since) is dropped.
    std::shared_ptr<ClearBatch> firstClearBatch;
    size_t firstClearOp = SIZE_MAX;
    struct ClearedTo { uint32_t value; size_t marks; };       // marks: useMarks.size() right after the clear was noted
    std::unordered_map<const void*, ClearedTo> clearedTo;     // whole allocations, by base pointer
    bool stillClearedTo(const void* ptr, uint32_t value) const
    {
        auto it = clearedTo.find(ptr);
        if (it == clearedTo.end() || it->second.value != value) return false;
        for (size_t i = it->second.marks; i < useMarks.size(); ++i)
            if (useMarks[i].ptr == ptr && useMarks[i].write) return false;
        return true;
    }
    // fresh: the caller guarantees that no earlier command of this recording uses the memory (scratch just allocated)
    int recordClearWords(void* ptr, uint64_t words, uint32_t value, bool fresh = false);
    bool usedSoFar(const void* ptr) const { for (const UseMark& m : useMarks) if (m.ptr == ptr) return true; return false; }

    // Which allocations each command uses (recorded by hold()): checked against the side stream's runs
    // when the list is executed.
    struct UseMark { size_t op; const void* ptr; bool write; std::atomic<uint64_t>* version; };
    std::vector<UseMark> useMarks;
    void use(const void* ptr, size_t op, bool write, std::atomic<uint64_t>* version = nullptr)
    {
        if (!ptr) return;
        useMarks.push_back({ op, ptr, write, version });
    }
    // the command being recorded turned out not to access `ptr` (bound for interface fidelity only): forget its marks
    void forgetUse(const void* ptr, size_t op)
    {
        for (size_t i = useMarks.size(); i-- > 0 && useMarks[i].op >= op;)
            if (useMarks[i].op == op && useMarks[i].ptr == ptr) useMarks.erase(useMarks.begin() + (ptrdiff_t)i);
    }

    // Peephole between two consecutive commands of one recording: a record function may leave a note about the command
    // it just emitted; the next record function may replace that command by a fused one (same command index, so the
    // use marks of both stay attached to it).  Cleared by any other command.
    struct Peephole { size_t op = SIZE_MAX; const char* kind = nullptr; std::shared_ptr<void> data; } peephole;

    void* scratchAlloc(size_t bytes);       // device memory valid until the list is re-opened/released
    void* scratchAllocSide(size_t bytes);   // same, from an arena only side-stream ops use (they are in order among themselves)
    std::vector<ScratchBlock> sideScratch;
    void resetRecording();
    // write: the command writes the resource; op: index of the command that uses it (default: the next one)
    void hold(trhip_buffer_t* b, bool write, size_t op = SIZE_MAX);
    void hold(trhip_texture_t* t, bool write);
};

namespace trhip
{

// What a shader's record function sees of one AddComputePass (Graphic.cpp:893-947).
struct DispatchCtx
{
    trhip_cmdlist_t* cl;
    const char* shaderName;
    int variant;                            // e.g. LATE_CULL / FILTER value of the permutation
    const trhip_binding* bindings; uint32_t numBindings;
    const void* push; uint32_t pushBytes;
    bool indirect; trhip_buffer_t* argsBuffer; uint32_t argsOffset;
    uint32_t gx, gy, gz;

    trhip_buffer_t* buffer(uint32_t type, uint32_t slot) const;
    trhip_texture_t* texture(uint32_t type, uint32_t slot, uint32_t* baseMip = nullptr) const;
    trhip_texture_table_t* textureTable(uint32_t slot) const;
    // Bytes of the constant buffer bound at b<slot> (volatile CB version at record time) or of
    // the push constants; nullptr if absent / wrong size.
    const void* constants(uint32_t slot, size_t bytes) const;
    uint32_t computeUnits() const { return cl->dev->computeUnits; }
    void* scratch(size_t bytes) const { return cl->scratchAlloc(bytes); }
    void* scratchSide(size_t bytes) const { return cl->dev->sideStream ? cl->scratchAllocSide(bytes) : cl->scratchAlloc(bytes); }
    void emit(const char* kernelName, std::function<int(hipStream_t)> fn) const;
    // Same, on the device's side stream, ordered after everything recorded before it.  `touched`: every
    // device allocation the op reads or writes that a later command could also use (base pointers).
    void emitSide(const char* kernelName, std::function<int(hipStream_t)> fn, std::initializer_list<Op::Access> touched) const;
};

// Footprint-min table of an HZB (trhip_texture_t::quad), k_hzb.hip.  ensure: allocate + lay out (record time); launch: rebuild on `s`.
int hzbQuadEnsure(trhip_texture_t* tex);
int hzbQuadLaunchBuild(trhip_texture_t* tex, hipStream_t s);

// Instance cull cache (instance_cache.hip.h, k_gpuculling.hip).  ensure: allocate (record time); launch: rebuild on
// `s` unless it is current -- called while commands are submitted, so every earlier write is counted.
int instanceCacheEnsure(trhip_buffer_t* instances);
int instanceCacheLaunchBuild(trhip_buffer_t* instances, trhip_buffer_t* meshData, hipStream_t s);

// Record capacity (groups) from which the early meshlet cull resolves its HZB lookups through the footprint-min table
// (rebuilt per frame by extra workgroups of the early instance pass's own launches) instead of the texels.  2^17: a rank's
// share of C3 at 8 ranks (390 k groups: 53 instead of 75 us for its early cull); real assets below that keep the texel path.
// TRHIP_TABLE_MIN_GROUPS overrides (tuning); tests/test_gpu_size_boundaries.py reads the default from the line below.
inline uint32_t tableMinGroups()
{
    static const uint32_t v = [] { const char* e = getenv("TRHIP_TABLE_MIN_GROUPS"); return e ? (uint32_t)strtoul(e, nullptr, 0) : (1u << 17); }();
    return v;
}

// Pipeline statistics (k_pipeline_stats.hip).  csThreads: the [numthreads] product of the reference entry behind a shader name
// that counts as CSInvocations (0: none).  emitIndirectCS: a command that adds groups(args) x threads to the open query.
// emitAS: the command that adds a basepass_AS_Main pass's AS / MS invocations and MS primitives to the open query, behind
// its cull (on the side stream when `side`, beside the list build).
uint32_t statsCSThreads(const char* shaderName);
int statsLaunchAdd(unsigned long long* counter, uint64_t value, hipStream_t s);
int statsEmitIndirectCS(trhip_cmdlist_t* cl, trhip_buffer_t* args, uint32_t argsOffset, uint32_t threads);
int statsEmitAS(const DispatchCtx& ctx, const ::MeshletCullArgs& a, trhip_buffer_t* meshlets, trhip_buffer_t* records,
                trhip_buffer_t* instances, trhip_buffer_t* meshData, bool side);

using RecordFn = int (*)(DispatchCtx&);
void registerShader(const char* name, RecordFn fn, int variant);

struct ShaderRegistrar
{
    ShaderRegistrar(const char* name, RecordFn fn, int variant = 0) { registerShader(name, fn, variant); }
};

// FORKS THROUGH THE KERNEL'S COMPLETION SIGNAL.  The side stream continues from a point of the main stream (a fork).
// hipEventRecord there puts a marker packet into the main queue: 2.9 us of the frame's chain of dependent launches, 5.3 us
// with the side stream's wait (tools/sync_cost.hip, profiles/r4/sync_cost.txt).  hipExtLaunchKernelGGL hands the event the
// completion signal of the kernel itself: 1.6 us.  While trhip_queue_execute runs the main-stream command in front of a fork
// it sets a tap; EVERY launch of that command on that stream (every launch of the back end goes through TRHIP_LAUNCH) is
// given the fork event as its stop event -- like a re-recorded event it ends up standing for the last of them (checked by
// tools/sync_cost.hip: two launches, one event, the waiter sees the second one's result).
// THE RULE: a tapped op's last TRHIP_LAUNCH must be its last work on that stream (work behind it is outside the fork).  An op
// that launches nothing (a copy) forks with a marker event, and so does a host callback: the caller's code may launch through
// TRHIP_LAUNCH (trhip_launch_shard_late_info) and then enqueue more, so trhip_queue_execute never taps it.
struct LaunchTap { hipStream_t onStream = nullptr; hipEvent_t stopEvent = nullptr; int launches = 0; };
extern thread_local LaunchTap* g_launchTap;
#define TRHIP_LAUNCH(kernel, grid, block, shmem, stream, ...)                                                       \
    do {                                                                                                            \
        trhip::LaunchTap* tap_ = trhip::g_launchTap;                                                                \
        if (tap_ && tap_->onStream == (stream) && ++tap_->launches)                                              \
            hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, nullptr, tap_->stopEvent, 0, __VA_ARGS__);    \
        else                                                                                                        \
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                                    \
    } while (0)

inline int launchStatus(const char* what)
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRHIP_OK : hipfail(e, what);
}

} // namespace trhip
