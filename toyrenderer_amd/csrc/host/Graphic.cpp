// Graphic.cpp -- see Graphic.h.  Re-authored against the HIP back end; cites are to the reference's
// source/Graphic.cpp and source/GraphicRHI.cpp.
#include <unordered_map>

#include "Graphic.h"
#include "TextureFeedbackManager.h"

#include <algorithm>

#include "HostProfile.h"

#include <chrono>

#include "CommonResources.h"
#include "GraphicConstants.h"
#include "RenderGraph.h"
#include "Scene.h"
#include "../ShaderInterop.h"

// Graphic.cpp:14-20: layouts shared with the kernels must agree
static_assert(sizeof(interop::DispatchIndirectArguments) == 12);
static_assert(GraphicConstants::kMaxThreadGroupsPerDimension == interop::kMaxThreadGroupsPerDimension);

nvrhi::DeviceHandle GraphicRHI::CreateDevice(int deviceIndex, void* externalHipStream)
{
    // GraphicRHI.cpp:56-200: adapter pick + ONE direct queue (:152-177)  ->  one HIP device + one stream.
    trhip_device dev = nullptr;
    if (externalHipStream)
        nvrhi::throwIfFailed(trhip_device_create_on_stream(deviceIndex, externalHipStream, &dev), "GraphicRHI::CreateDevice");
    else
        nvrhi::throwIfFailed(trhip_device_create(deviceIndex, &dev), "GraphicRHI::CreateDevice");
    // Graphic.cpp:84-94 asserts waveLaneCount == kNumThreadsPerWave (32).  gfx950 is wave64-only: one
    // wave runs two reference groups, so the requirement here is 2 * kNumThreadsPerWave.
    uint32_t cus = 0, wave = 0;
    uint64_t mem = 0;
    nvrhi::throwIfFailed(trhip_device_info(dev, &cus, &wave, &mem), "trhip_device_info");
    check(wave == 2 * interop::kNumThreadsPerWave);
    nvrhi::DeviceHandle device(new nvrhi::IDevice(dev));
    device->setDeviceIndex(deviceIndex);
    return device;
}

Graphic& Graphic::GetInstance()
{
    static Graphic s_Instance;
    return s_Instance;
}

void Graphic::Initialize(int deviceIndex, Vector2U renderResolution, void* externalHipStream)
{
    m_RenderResolution = renderResolution;                                   // Graphic.cpp:612
    m_DeviceIndex = deviceIndex;
    m_NVRHIDevice = GraphicRHI::CreateDevice(deviceIndex, externalHipStream); // InitDevice
    // InitShaders (Graphic.cpp:103-251) loads DXIL blobs into a name->shader map; here the kernels are
    // linked into the back end and registered under the same names.
    check(HasShader("gpuculling_CS_GPUCulling LATE_CULL=0"));
    m_CommonResources = std::make_shared<CommonResources>();
    m_CommonResources->Initialize();
    m_Scene = std::make_shared<Scene>();
    m_Scene->Initialize();
    for (IRenderer* renderer : IRenderer::ms_AllRenderers)                    // Graphic.cpp:630-638
        renderer->Initialize();
    ExecuteAllCommandLists();
}

void Graphic::PostSceneLoad()
{
    m_Scene->PostSceneLoad();                                                 // Graphic.cpp:649-662
    for (IRenderer* renderer : IRenderer::ms_AllRenderers)
        renderer->PostSceneLoad();
    ExecuteAllCommandLists();
}

// Texture::LoadFromFile + the SRV's slot in the bindless table (Visual.cpp, Graphic.h:111-113), from decoded texels or from the
// blocks of a block-compressed format: `data` holds the mips back to back, level k of max(width >> k, 1) x max(height >> k, 1) x 4
// bytes, or of ceil(w_k / 4) x ceil(h_k / 4) blocks of 8 (BC1, BC4) or 16 bytes.  Returns the descriptor index.
static uint32_t BlockBytes(nvrhi::Format format)
{
    if (format < nvrhi::Format::BC1_UNORM || format > nvrhi::Format::BC5_UNORM) return 0;
    return format == nvrhi::Format::BC1_UNORM || format == nvrhi::Format::BC1_UNORM_SRGB || format == nvrhi::Format::BC4_UNORM ? 8u : 16u;
}

uint32_t Graphic::CreateMaterialTexture(uint32_t width, uint32_t height, uint32_t mips, nvrhi::Format format, const void* data, uint64_t bytes)
{
    const uint32_t blockBytes = BlockBytes(format);
    if (format != nvrhi::Format::RGBA8_UNORM && format != nvrhi::Format::SRGBA8_UNORM && !blockBytes)
        throw nvrhi::Error("material texture: the format must be RGBA8_UNORM, SRGBA8_UNORM or one of BC1 to BC5 (BC6H and BC7 are not supported)");
    auto levelBytes = [&](uint32_t k) {
        const uint64_t w = std::max(width >> k, 1u), h = std::max(height >> k, 1u);
        return blockBytes ? ((w + 3) / 4) * ((h + 3) / 4) * blockBytes : w * h * 4u;
    };
    if (!width || !height || !mips || mips > 16 || !data) throw nvrhi::Error("material texture: bad dimensions, mip count or data");
    uint64_t need = 0;
    for (uint32_t k = 0; k < mips; ++k) need += levelBytes(k);
    if (bytes != need) throw nvrhi::Error("material texture: " + std::to_string(mips) + " mips of " + std::to_string(width) + " x " + std::to_string(height) + " are " + std::to_string(need) + " bytes, got " + std::to_string(bytes));
    if (m_Textures.size() >= kMaxMaterialTextures) throw nvrhi::Error("material texture: the descriptor table is full");
    if (!m_SrvUavCbvDescriptorTable) m_SrvUavCbvDescriptorTable = m_NVRHIDevice->createDescriptorTable(kMaxMaterialTextures);
    const uint32_t index = (uint32_t)m_Textures.size();
    if (g_TextureFeedbackManager.m_bEnabled) {                                // a streamable texture: tail only, its maps beside it (TextureFeedbackManager.h)
        nvrhi::TextureHandle streamed;
        if (g_TextureFeedbackManager.AddTexture(m_NVRHIDevice, m_SrvUavCbvDescriptorTable, kMaxMaterialTextures, index, width, height, mips, format, blockBytes,
                                                (const uint8_t*)data, streamed)) {
            m_NVRHIDevice->writeDescriptorTable(m_SrvUavCbvDescriptorTable, index, streamed);
            m_Textures.push_back(streamed);
            return index;
        }
    }
    nvrhi::TextureDesc d;
    d.width = width; d.height = height; d.mipLevels = mips; d.format = format;
    d.debugName = "Material Texture " + std::to_string(m_Textures.size());
    d.initialState = nvrhi::ResourceStates::ShaderResource;
    nvrhi::TextureHandle t = m_NVRHIDevice->createTexture(d);
    const uint8_t* p = (const uint8_t*)data;
    for (uint32_t k = 0; k < mips; ++k) {
        const uint64_t n = levelBytes(k);
        nvrhi::throwIfFailed(trhip_texture_upload(t->native(), k, p, n), "material texture upload");
        p += n;
    }
    m_NVRHIDevice->writeDescriptorTable(m_SrvUavCbvDescriptorTable, index, t);
    m_Textures.push_back(t);
    return index;
}

void Graphic::Shutdown()
{
    if (!m_NVRHIDevice) return;
    m_NVRHIDevice->waitForIdle();
    for (IRenderer* renderer : IRenderer::ms_AllRenderers) {
        renderer->m_FrameTimerQuery[0] = nullptr;
        renderer->m_FrameTimerQuery[1] = nullptr;
        renderer->m_Queue = nvrhi::CommandQueue::Graphics;
    }
    m_Scene->Shutdown();
    m_Scene.reset();
    m_CommonResources.reset();
    m_GlobalMeshDataBuffer = nullptr;
    m_GlobalMeshletDataBuffer = nullptr;
    m_GlobalVertexBuffer = nullptr; m_GlobalMeshletVertexOffsetsBuffer = nullptr; m_GlobalMeshletIndicesBuffer = nullptr;
    m_GlobalIndexBuffer = nullptr;                                            // Scene::LoadRaytracing's: left behind, the next session would release it after its device
    m_GlobalMaterialDataBuffer = nullptr;
    m_SrvUavCbvDescriptorTable = nullptr;
    g_TextureFeedbackManager.Shutdown();
    m_Textures.clear();
    m_bAnyMaterialTextured = false;
    m_PendingCommandLists.clear();
    for (auto& pool : m_FreeCommandLists) pool.clear();
    m_AllCommandLists.clear();
    m_NVRHIDevice->destroyQueues();
    m_NVRHIDevice = nullptr;
    m_NumCrossQueueWaits = 0;
    m_FrameCounter = 0;
}

void Graphic::Update()
{
    ++m_FrameCounter;                                                         // Graphic.cpp:706
    const auto t0 = std::chrono::steady_clock::now();
    m_Scene->Update();                                                        // records every pass
    const auto t1 = std::chrono::steady_clock::now();
    ExecuteAllCommandLists();                                                 // the CPU->GPU boundary
    m_NVRHIDevice->runGarbageCollection();                                    // Graphic.cpp:761-765
    const auto t2 = std::chrono::steady_clock::now();
    m_LastRecordMs = std::chrono::duration<float, std::milli>(t1 - t0).count();
    m_LastSubmitMs = std::chrono::duration<float, std::milli>(t2 - t1).count();
}

Vector2 Graphic::ComputeCurrentJitterOffset()
{
    // Graphic.cpp:971-997: the Halton branch (the MSAA-8 table and the white noise are `if constexpr (false)` there)
    auto GetJitterPhaseCount = [](uint32_t renderWidth, uint32_t displayWidth) {
        const float kBasePhaseCount = 8.0f;
        const float ratio = float(displayWidth) / renderWidth;
        return (uint32_t)(kBasePhaseCount * (ratio * ratio));                // pow(x, 2.0f); render = display: 8
    };
    auto VanDerCorput = [](size_t base, size_t index) {
        float ret = 0.0f;
        float denominator = float(base);
        while (index > 0) {
            size_t multiplier = index % base;
            ret += float(multiplier) / denominator;
            index = index / base;
            denominator *= base;
        }
        return ret;
    };
    const uint32_t phaseCount = GetJitterPhaseCount(m_RenderResolution.x, m_RenderResolution.x);
    const uint32_t index = (m_FrameCounter % phaseCount) + 1;
    return Vector2{ VanDerCorput(2, index) - 0.5f, VanDerCorput(3, index) - 0.5f };
}

bool Graphic::HasShader(std::string_view shaderBinName) const
{
    return trhip_shader_exists(std::string(shaderBinName).c_str()) != 0;
}

nvrhi::CommandListHandle Graphic::AllocateCommandList(nvrhi::CommandQueue queueType)
{
    std::lock_guard<std::mutex> lock(m_FreeCommandListsLock);                 // Graphic.cpp:520-555 (one pool per queue type)
    std::deque<nvrhi::CommandListHandle>& pool = m_FreeCommandLists[(size_t)queueType];
    if (!pool.empty()) {
        nvrhi::CommandListHandle cl = pool.front();
        pool.pop_front();
        return cl;
    }
    nvrhi::CommandListHandle cl = m_NVRHIDevice->createCommandList(queueType);
    m_AllCommandLists.push_back(cl);
    return cl;
}

void Graphic::FreeCommandList(nvrhi::CommandListHandle cmdList)
{
    std::lock_guard<std::mutex> lock(m_FreeCommandListsLock);
    m_FreeCommandLists[(size_t)cmdList->m_Queue].push_back(cmdList);
}

void Graphic::BeginCommandList(nvrhi::CommandListHandle cmdList, std::string_view name)
{
    cmdList->open();                                                          // Graphic.cpp:564-583
    cmdList->beginMarker(std::string(name).c_str());
}

void Graphic::EndCommandList(nvrhi::CommandListHandle cmdList, bool bQueueCmdlist, bool bImmediateExecute)
{
    cmdList->endMarker();                                                     // Graphic.cpp:585-606
    cmdList->close();
    if (bQueueCmdlist) QueueCommandList(cmdList);
    if (bImmediateExecute) {
        m_NVRHIDevice->executeCommandList(cmdList);
        FreeCommandList(cmdList);
    }
}

void Graphic::ExecuteAllCommandLists()
{
    std::vector<PendingCommandList> lists;
    {
        std::lock_guard<std::mutex> lock(m_PendingCommandListsLock);
        lists.swap(m_PendingCommandLists);
    }
    if (lists.empty()) return;
    // Graphic.cpp:790 does waitForIdle before every submit (upload-manager versioning).  The streams are
    // in-order and recorded lists own their staging copies, so the wait is not needed for
    // correctness here and would only serialise CPU recording with GPU execution.
    //
    // Lists are submitted in queue order (= pass order); runs of lists of one queue type go down in one call
    // (Graphic.cpp:816).  A list that depends on a list of the OTHER queue (RenderGraph::Compile) first makes its queue
    // wait for that one (nvrhi queueWaitForCommandList).  Frames are joined: whatever the compute queue still runs from
    // the previous submission is awaited by this one's first graphics list and the other way round -- the graph does not
    // see hazards across frames.
    using Q = nvrhi::CommandQueue;
    bool anyCompute = false;
    for (const PendingCommandList& p : lists) anyCompute |= p.m_CommandList->m_Queue == Q::Compute;
    if (anyCompute || m_NVRHIDevice->hasComputeQueue()) {
        if (m_NVRHIDevice->hasComputeQueue() && m_NVRHIDevice->lastInstance(Q::Compute))
            m_NVRHIDevice->queueWaitForCommandList(Q::Graphics, Q::Compute, m_NVRHIDevice->lastInstance(Q::Compute));
        if (anyCompute && m_NVRHIDevice->lastInstance(Q::Graphics))
            m_NVRHIDevice->queueWaitForCommandList(Q::Compute, Q::Graphics, m_NVRHIDevice->lastInstance(Q::Graphics));
    }
    std::unordered_map<const nvrhi::ICommandList*, std::pair<Q, uint64_t>> submitted;     // list -> (queue, instance)
    size_t i = 0;
    while (i < lists.size()) {
        const Q queue = lists[i].m_CommandList->m_Queue;
        for (const nvrhi::ICommandList* dep : lists[i].m_WaitFor) {
            auto it = submitted.find(dep);
            check(it != submitted.end());                                     // dependencies point backwards in queue order
            if (it->second.first != queue) {
                // the producer's queue is in order, so waiting for its LATEST submission covers the one meant
                m_NVRHIDevice->queueWaitForCommandList(queue, it->second.first, m_NVRHIDevice->lastInstance(it->second.first));
                ++m_NumCrossQueueWaits;
            }
        }
        std::vector<nvrhi::ICommandList*> raw{ lists[i].m_CommandList.Get() };
        size_t j = i + 1;
        while (j < lists.size() && lists[j].m_CommandList->m_Queue == queue && lists[j].m_WaitFor.empty()) raw.push_back(lists[j++].m_CommandList.Get());
        const uint64_t instance = m_NVRHIDevice->executeCommandLists(raw.data(), raw.size(), queue);   // Graphic.cpp:816
        for (nvrhi::ICommandList* cl : raw) submitted[cl] = { queue, instance };
        i = j;
    }
    for (auto& p : lists) FreeCommandList(p.m_CommandList);
}

void Graphic::AddComputePass(const ComputePassParams& p)
{
    HOST_PROFILE_SCOPE("Graphic::AddComputePass");
    check(p.m_CommandList);                                                   // Graphic.cpp:895-896
    check(!p.m_ShaderName.empty());
    PROFILE_GPU_SCOPED(p.m_CommandList, p.m_ShaderName.c_str());              // :899

    nvrhi::ComputeState computeState;                                         // :901-921
    check(HasShader(p.m_ShaderName));                                         // GetShader() asserts on unknown names (:276)
    computeState.pipeline = p.m_ShaderName;
    computeState.bindings = p.m_BindingSetDesc;

    if (p.m_IndirectArgsBuffer) {
        // indirect dispatch does not need group size (:923-928)
        check(p.m_DispatchGroupSize.x == 0 && p.m_DispatchGroupSize.y == 0 && p.m_DispatchGroupSize.z == 0);
        computeState.indirectParams = p.m_IndirectArgsBuffer;
    }
    p.m_CommandList->setComputeState(computeState);                           // :930

    if (p.m_PushConstantsData) {                                              // :932-936
        check(p.m_PushConstantsBytes > 0);
        p.m_CommandList->setPushConstants(p.m_PushConstantsData, p.m_PushConstantsBytes);
    }
    if (p.m_IndirectArgsBuffer) {                                             // :938-946
        p.m_CommandList->dispatchIndirect(p.m_IndirectArgsBufferOffsetBytes);
    } else {
        check(p.m_DispatchGroupSize.x != 0 && p.m_DispatchGroupSize.y != 0 && p.m_DispatchGroupSize.z != 0);
        p.m_CommandList->dispatch(p.m_DispatchGroupSize.x, p.m_DispatchGroupSize.y, p.m_DispatchGroupSize.z);
    }
}
