// Scene.cpp -- see Scene.h.  Cites are to the reference's source/Scene.cpp.
#include "Scene.h"
#include "TextureFeedbackManager.h"

#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "HostProfile.h"

#include <cstring>

#include "Graphic.h"
#include "GraphicConstants.h"
#include "../ShaderInterop.h"

extern IRenderer* g_UpdateInstanceConstsRenderer;
extern IRenderer* g_GBufferRenderer;
extern IRenderer* g_AmbientOcclusionRenderer;
extern IRenderer* g_ShadowMaskRenderer;
extern IRenderer* g_DeferredLightingRenderer;
extern IRenderer* g_SkyRenderer;
extern IRenderer* g_BloomRenderer;
extern IRenderer* g_AdaptLuminanceRenderer;
extern IRenderer* g_TAARenderer;
extern IRenderer* g_PostProcessRenderer;
extern IRenderer* g_GIDebugRenderer;
extern IRenderer* g_GIRenderer;

void View::Update()
{
    const bool bTAA = g_Scene->IsTAAEnabled();
    m_PrevJitterOffset = m_CurrentJitterOffset;                               // Scene.cpp:113-114
    m_CurrentJitterOffset = bTAA ? g_Graphic.ComputeCurrentJitterOffset() : Vector2{ 0.0f, 0.0f };
    m_PrevWorldToClip = m_WorldToClip;                                        // :119

    // Scene.cpp:116-118: keep last frame's matrices
    m_PrevWorldToView = m_WorldToView;
    m_PrevViewToClip = m_ViewToClip;
    if (m_bHasPending) m_WorldToView = m_PendingWorldToView;                  // :121-122 (camera from the application)

    if (!m_bUseExplicitProjection) {                                          // :124-125
        const float kKindaBigNumber = 1e10f;
        m_ViewToClip = CreatePerspectiveFieldOfView(m_FOV, m_AspectRatio, m_ZNearP, kKindaBigNumber);
        ModifyPerspectiveMatrix(m_ViewToClip, m_ZNearP, kKindaBigNumber, GraphicConstants::kInversedDepthBuffer, GraphicConstants::kInfiniteDepthBuffer);
    }
    else m_ViewToClip = m_ExplicitViewToClip;                                 // the application's, without last frame's jitter
    if (bTAA) {                                                               // :127-131: m_ViewToClip *= CreateTranslation(2 jx / W, -2 jy / H, 0)
        Matrix pixelOffsetMatrix{};
        for (int i = 0; i < 4; ++i) pixelOffsetMatrix.m[i][i] = 1.0f;
        pixelOffsetMatrix.m[3][0] = 2.0f * m_CurrentJitterOffset.x / g_Graphic.m_RenderResolution.x;
        pixelOffsetMatrix.m[3][1] = -2.0f * m_CurrentJitterOffset.y / g_Graphic.m_RenderResolution.y;
        m_ViewToClip = MultiplyNoFMA(m_ViewToClip, pixelOffsetMatrix);
    }
    m_WorldToClip = MultiplyNoFMA(m_WorldToView, m_ViewToClip);               // :133
    if (!bTAA) m_bHasTAAHistory = false;
    else if (!m_bHasTAAHistory) {                                             // the first frame with TAA on: nothing earlier to refer to
        m_PrevJitterOffset = m_CurrentJitterOffset;
        m_PrevWorldToClip = m_WorldToClip;
        m_bHasTAAHistory = true;
        g_Scene->m_bResetTAAHistory = true;
    }

    for (int j = 0; j < 3; ++j)                                               // m_Eye (:133): see Scene.h; the sum GIRenderer.cpp's constants use
        m_Eye[j] = -(m_WorldToView.m[3][0] * m_WorldToView.m[j][0] + m_WorldToView.m[3][1] * m_WorldToView.m[j][1] + m_WorldToView.m[3][2] * m_WorldToView.m[j][2]);
    m_ClipToWorld = InverseOfProduct(m_WorldToView, m_ViewToClip);            // :135-137

    if (!g_Scene->m_bFreezeCullingCamera) {                                   // :139-144
        m_CullingPrevWorldToView = m_PrevWorldToView;
        m_CullingWorldToView = m_WorldToView;
    }
}

void Scene::Initialize()
{
    m_RenderGraph = std::make_shared<RenderGraph>();
    m_RenderGraph->Initialize();
    m_View.m_AspectRatio = (float)g_Graphic.m_RenderResolution.x / (float)g_Graphic.m_RenderResolution.y;
}

void Scene::LoadFromArrays(const void* instances, uint32_t numInstances, const void* meshData, uint32_t numMeshes,
                           const void* meshlets, uint64_t numMeshlets, const uint32_t* opaqueIds, uint32_t numOpaque,
                           const uint32_t* alphaMaskIds, uint32_t numAlphaMask)
{
    nvrhi::DeviceHandle device = g_Graphic.m_NVRHIDevice;
    auto make = [&](const char* name, uint64_t bytes, uint32_t stride, bool uav) {
        nvrhi::BufferDesc d;
        d.byteSize = bytes ? bytes : stride;
        d.structStride = stride;
        d.debugName = name;
        d.canHaveUAVs = uav;
        d.initialState = nvrhi::ResourceStates::ShaderResource;
        return device->createBuffer(d);
    };
    auto upload = [&](nvrhi::BufferHandle b, const void* src, uint64_t bytes) {
        if (bytes) nvrhi::throwIfFailed(trhip_buffer_upload(b->native(), 0, src, bytes), "Scene upload");
    };
    m_NumPrimitives = numInstances;
    // UpdateInstanceConstsRenderer::CreateInstanceConstsBuffer (BasePassRenderers.cpp:23-62)
    m_InstanceConstsBuffer = make("Instance Consts Buffer", (uint64_t)numInstances * sizeof(interop::BasePassInstanceConstants), sizeof(interop::BasePassInstanceConstants), true);
    upload(m_InstanceConstsBuffer, instances, (uint64_t)numInstances * sizeof(interop::BasePassInstanceConstants));
    // UploadGlobalMeshBuffers (SceneLoading.cpp:1016-1088)
    g_Graphic.m_GlobalMeshDataBuffer = make("GlobalMeshDataBuffer", (uint64_t)numMeshes * sizeof(interop::MeshData), sizeof(interop::MeshData), false);
    upload(g_Graphic.m_GlobalMeshDataBuffer, meshData, (uint64_t)numMeshes * sizeof(interop::MeshData));
    g_Graphic.m_GlobalMeshletDataBuffer = make("GlobalMeshletDataBuffer", numMeshlets * sizeof(interop::MeshletData), sizeof(interop::MeshletData), false);
    if (meshlets) upload(g_Graphic.m_GlobalMeshletDataBuffer, meshlets, numMeshlets * sizeof(interop::MeshletData));   // else: streamed in by the caller
    // Scene::UpdateInstanceIDsBuffers (Scene.cpp:282-362)
    m_OpaquePrimitiveIDs.assign(opaqueIds, opaqueIds + numOpaque);
    m_AlphaMaskPrimitiveIDs.assign(alphaMaskIds, alphaMaskIds + numAlphaMask);
    m_OpaqueInstanceIDsBuffer = make("OpaqueInstanceIDsBuffer", (uint64_t)numOpaque * 4, 4, false);
    upload(m_OpaqueInstanceIDsBuffer, opaqueIds, (uint64_t)numOpaque * 4);
    m_AlphaMaskInstanceIDsBuffer = make("AlphaMaskInstanceIDsBuffer", (uint64_t)numAlphaMask * 4, 4, false);
    upload(m_AlphaMaskInstanceIDsBuffer, alphaMaskIds, (uint64_t)numAlphaMask * 4);
}

void Scene::LoadCachedData(const char* path, const void* instances, uint32_t numInstances, const uint32_t* opaqueIds, uint32_t numOpaque,
                           const uint32_t* alphaMaskIds, uint32_t numAlphaMask)
{
    // SceneLoading.cpp:57-79
    struct Header { uint32_t m_Version, m_MeshOptVersion, m_NumVertices, m_NumIndices, m_NumMeshes, m_NumMeshletVertexIdxOffsets, m_NumMeshletIndices, m_NumMeshletDatas; };
    static_assert(sizeof(Header) == 32, "CachedData::Header");
    constexpr uint32_t kCurrentVersion = 3;
    constexpr size_t kRawVertexFormatBytes = 20, kMeshSpecificDataBytes = 32;
    struct File { FILE* f; ~File() { if (f) fclose(f); } } file{ fopen(path, "rb") };
    if (!file.f) throw std::runtime_error(std::string("cached data: cannot open ") + path);
    Header h{};
    if (fread(&h, sizeof h, 1, file.f) != 1) throw std::runtime_error("cached data: no header");
    if (h.m_Version != kCurrentVersion) throw std::runtime_error("cached data: version " + std::to_string(h.m_Version) + ", this reader handles 3");
    auto take = [&](std::vector<uint8_t>& dst, size_t elemBytes, uint64_t count, const char* what) {     // :728-748, same order
        dst.resize((size_t)(elemBytes * count));
        if (count && fread(dst.data(), elemBytes, (size_t)count, file.f) != count) throw std::runtime_error(std::string("cached data: truncated in ") + what);
    };
    std::vector<uint8_t> vertices, indices, meshData, vertexIds, triangles, meshlets, meshSpecific;
    take(vertices, kRawVertexFormatBytes, h.m_NumVertices, "vertices");
    take(indices, sizeof(uint32_t), h.m_NumIndices, "indices");
    take(meshData, sizeof(interop::MeshData), h.m_NumMeshes, "mesh data");
    take(vertexIds, sizeof(uint32_t), h.m_NumMeshletVertexIdxOffsets, "meshlet vertex ids");
    take(triangles, sizeof(uint32_t), h.m_NumMeshletIndices, "meshlet triangles");
    take(meshlets, sizeof(interop::MeshletData), h.m_NumMeshletDatas, "meshlets");
    take(meshSpecific, kMeshSpecificDataBytes, h.m_NumMeshes, "mesh specific data");
    // the ranges the cull and the mesh shader follow blindly
    const interop::MeshData* md = (const interop::MeshData*)meshData.data();
    for (uint32_t i = 0; i < h.m_NumMeshes; ++i) {
        if (md[i].m_NumLODs < 1 || md[i].m_NumLODs > interop::kMaxNumMeshLODs) throw std::runtime_error("cached data: mesh " + std::to_string(i) + " has a bad LOD count");
        for (uint32_t l = 0; l < md[i].m_NumLODs; ++l)
            if ((uint64_t)md[i].m_MeshLODDatas[l].m_MeshletDataBufferIdx + md[i].m_MeshLODDatas[l].m_NumMeshlets > h.m_NumMeshletDatas)
                throw std::runtime_error("cached data: mesh " + std::to_string(i) + " points past the meshlet buffer");
    }
    const interop::MeshletData* ml = (const interop::MeshletData*)meshlets.data();
    for (uint32_t i = 0; i < h.m_NumMeshletDatas; ++i) {
        const uint32_t nv = ml[i].m_VertexAndTriangleCount & 0xFFu, nt = (ml[i].m_VertexAndTriangleCount >> 8) & 0xFFu;
        if ((uint64_t)ml[i].m_MeshletVertexIDsBufferIdx + nv > h.m_NumMeshletVertexIdxOffsets || (uint64_t)ml[i].m_MeshletIndexIDsBufferIdx + nt > h.m_NumMeshletIndices)
            throw std::runtime_error("cached data: meshlet " + std::to_string(i) + " points past its index buffers");
    }
    LoadFromArrays(instances, numInstances, meshData.data(), h.m_NumMeshes, meshlets.data(), h.m_NumMeshletDatas, opaqueIds, numOpaque, alphaMaskIds, numAlphaMask);
    LoadGeometry(vertices.data(), h.m_NumVertices, (const uint32_t*)vertexIds.data(), h.m_NumMeshletVertexIdxOffsets,
                 (const uint32_t*)triangles.data(), h.m_NumMeshletIndices);
}

void Scene::LoadGeometry(const void* vertices, uint64_t numVertices, const uint32_t* meshletVertexIds, uint64_t numVertexIds,
                         const uint32_t* meshletTriangles, uint64_t numTriangles)
{
    // UploadGlobalMeshBuffers (SceneLoading.cpp:1016-1088): the vertex / meshlet-vertex-id / meshlet-triangle buffers
    nvrhi::DeviceHandle device = g_Graphic.m_NVRHIDevice;
    auto make = [&](const char* name, const void* src, uint64_t bytes, uint32_t stride) {
        nvrhi::BufferDesc d;
        d.byteSize = bytes ? bytes : stride;
        d.structStride = stride;
        d.debugName = name;
        d.initialState = nvrhi::ResourceStates::ShaderResource;
        nvrhi::BufferHandle b = device->createBuffer(d);
        if (bytes) nvrhi::throwIfFailed(trhip_buffer_upload(b->native(), 0, src, bytes), "Scene geometry upload");
        return b;
    };
    g_Graphic.m_GlobalVertexBuffer = make("GlobalVertexBuffer", vertices, numVertices * 20u, 20u);                       // RawVertexFormat (ShaderInterop.h:278-283)
    g_Graphic.m_GlobalMeshletVertexOffsetsBuffer = make("GlobalMeshletVertexOffsetsBuffer", meshletVertexIds, numVertexIds * 4u, 4u);
    g_Graphic.m_GlobalMeshletIndicesBuffer = make("GlobalMeshletIndicesBuffer", meshletTriangles, numTriangles * 4u, 4u);
}

void Scene::LoadRaytracing(const uint32_t* indices, uint64_t numIndices, const uint32_t* indexCounts, uint32_t numMeshes)
{
    // Mesh::BuildBLAS (Visual.cpp:509-542) for every mesh and Scene::CreateAccelerationStructures (Scene.cpp:430-470), through the
    // back end's one builder.  The vertex, mesh and instance tables are read back from their buffers: the scene keeps no host copy.
    if (!g_Graphic.m_GlobalVertexBuffer || !g_Graphic.m_GlobalMeshDataBuffer || !m_InstanceConstsBuffer) throw std::runtime_error("raytracing: load the scene and its geometry first");
    auto readBack = [](nvrhi::BufferHandle b, uint64_t bytes) {
        std::vector<uint8_t> v((size_t)bytes);
        if (bytes) nvrhi::throwIfFailed(trhip_buffer_download(b->native(), 0, v.data(), bytes), "raytracing read-back");
        return v;
    };
    const uint64_t numVertices = g_Graphic.m_GlobalVertexBuffer->getDesc().byteSize / 20u;
    if (g_Graphic.m_GlobalMeshDataBuffer->getDesc().byteSize < (uint64_t)numMeshes * sizeof(interop::MeshData)) throw std::runtime_error("raytracing: more index counts than meshes");
    const std::vector<uint8_t> vertices = readBack(g_Graphic.m_GlobalVertexBuffer, numVertices * 20u);
    const std::vector<uint8_t> meshBytes = readBack(g_Graphic.m_GlobalMeshDataBuffer, (uint64_t)numMeshes * sizeof(interop::MeshData));
    const std::vector<uint8_t> instances = readBack(m_InstanceConstsBuffer, (uint64_t)m_NumPrimitives * sizeof(interop::BasePassInstanceConstants));
    const interop::MeshData* md = (const interop::MeshData*)meshBytes.data();
    std::vector<trhip_blas_header> headers(numMeshes);
    std::vector<trhip_accel_node> blasNodes;
    std::vector<uint32_t> triOrder;
    for (uint32_t m = 0; m < numMeshes; ++m) {
        const uint64_t first = md[m].m_GlobalIndexBufferIdx, count = indexCounts[m], vbase = md[m].m_GlobalVertexBufferIdx;
        if (count % 3 || first + count > numIndices) throw std::runtime_error("raytracing: mesh " + std::to_string(m) + ": its indices are not a list of whole triangles inside the index buffer");
        if (vbase > numVertices) throw std::runtime_error("raytracing: mesh " + std::to_string(m) + ": its first vertex is outside the vertex buffer");
        const uint32_t cap = trhip_accel_max_nodes((uint32_t)(count / 3));
        std::vector<trhip_accel_node> nodes(cap ? cap : 1);
        std::vector<uint32_t> order(count / 3 ? count / 3 : 1);
        uint32_t numNodes = 0, numTris = 0;
        nvrhi::throwIfFailed(trhip_blas_build(vertices.data() + vbase * 20u, 20u, (uint32_t)(numVertices - vbase), indices + first, (uint32_t)count, nodes.data(), cap, order.data(),
                                              &numNodes, &numTris, nullptr), "trhip_blas_build");
        headers[m] = { (uint32_t)blasNodes.size(), numNodes, (uint32_t)triOrder.size(), numTris };
        blasNodes.insert(blasNodes.end(), nodes.begin(), nodes.begin() + numNodes);
        triOrder.insert(triOrder.end(), order.begin(), order.begin() + numTris);
    }
    std::vector<uint32_t> flags(m_NumPrimitives, 0u);                         // Scene.cpp:454
    for (uint32_t id : m_OpaquePrimitiveIDs) if (id < m_NumPrimitives) flags[id] = interop::kTLASInstanceForceOpaque;
    for (uint32_t id : m_AlphaMaskPrimitiveIDs) if (id < m_NumPrimitives) flags[id] = interop::kTLASInstanceForceNonOpaque;
    const uint32_t cap = trhip_accel_max_nodes(m_NumPrimitives);
    std::vector<trhip_accel_node> nodes(cap ? cap : 1);
    std::vector<trhip_tlas_instance> records(m_NumPrimitives ? m_NumPrimitives : 1);
    std::vector<uint32_t> levelNodes(cap ? cap : 1), levelOffsets(trhip_accel_max_depth() + 2, 0u);
    uint32_t numNodes = 0, numLevels = 0;
    nvrhi::throwIfFailed(trhip_tlas_build(instances.data(), m_NumPrimitives, flags.data(), headers.data(), numMeshes, blasNodes.data(), (uint32_t)blasNodes.size(), nodes.data(), cap,
                                          records.data(), levelNodes.data(), levelOffsets.data(), &numNodes, &numLevels), "trhip_tlas_build");
    nvrhi::DeviceHandle device = g_Graphic.m_NVRHIDevice;
    auto make = [&](const char* name, const void* src, uint64_t bytes, uint32_t stride, bool uav) {
        nvrhi::BufferDesc d;
        d.byteSize = bytes ? bytes : stride;
        d.structStride = stride;
        d.debugName = name;
        d.canHaveUAVs = uav;
        d.initialState = nvrhi::ResourceStates::ShaderResource;
        nvrhi::BufferHandle b = device->createBuffer(d);
        if (bytes) nvrhi::throwIfFailed(trhip_buffer_upload(b->native(), 0, src, bytes), "raytracing upload");
        return b;
    };
    auto as = std::make_shared<nvrhi::rt::AccelStruct>();
    as->numNodes = numNodes; as->numLevels = numLevels;
    as->nodes = make("TLAS Nodes", nodes.data(), (uint64_t)numNodes * sizeof(trhip_accel_node), sizeof(trhip_accel_node), true);
    as->instances = make("TLAS Instances", records.data(), (uint64_t)m_NumPrimitives * sizeof(trhip_tlas_instance), sizeof(trhip_tlas_instance), true);
    as->levelNodes = make("TLAS Level Nodes", levelNodes.data(), (uint64_t)(numNodes ? numNodes : 1) * 4u, 4u, false);
    as->levelOffsets = make("TLAS Level Offsets", levelOffsets.data(), levelOffsets.size() * 4u, 4u, false);
    as->blasHeaders = make("BLAS Headers", headers.data(), (uint64_t)numMeshes * sizeof(trhip_blas_header), sizeof(trhip_blas_header), false);
    as->blasNodes = make("BLAS Nodes", blasNodes.data(), blasNodes.size() * sizeof(trhip_accel_node), sizeof(trhip_accel_node), false);
    as->triOrder = make("BLAS Triangle Order", triOrder.data(), triOrder.size() * 4u, 4u, false);
    g_Graphic.m_GlobalIndexBuffer = make("GlobalIndexBuffer", indices, numIndices * 4u, 4u, false);
    m_TLAS = as;
}

void Scene::LoadMaterials(const void* materials, uint32_t numMaterials)
{
    // a textured material: every flagged slot names a loaded texture (trhost_create_material_texture); the two map indices are
    // 0xFFFFFFFF, or -- with streaming on -- name the maps of that very texture, and are filled in for a streamed texture that names none
    std::vector<interop::MaterialData> filled((const interop::MaterialData*)materials, (const interop::MaterialData*)materials + numMaterials);
    interop::MaterialData* m = filled.data();
    materials = filled.data();
    bool anyTextured = false;
    for (uint32_t i = 0; i < numMaterials; ++i) {
        interop::TextureData* slots = &m[i].m_AlbedoTexture;
        for (uint32_t c = 0; c < 4; ++c) {
            if (!(m[i].m_MaterialFlags & (1u << c))) continue;
            if (slots[c].m_DescriptorIndex >= g_Graphic.m_Textures.size())
                throw std::runtime_error("materials: material " + std::to_string(i) + " uses a texture (m_MaterialFlags bit " + std::to_string(c) + ", m_DescriptorIndex " +
                                         std::to_string(slots[c].m_DescriptorIndex) + ") that is not loaded: " + std::to_string(g_Graphic.m_Textures.size()) + " material textures");
            const TextureFeedbackManager::Streamed* streamed = g_TextureFeedbackManager.m_bEnabled ? g_TextureFeedbackManager.Find(slots[c].m_DescriptorIndex) : nullptr;
            const uint32_t fb = slots[c].m_FeedbackTextureDescriptorIndex, mm = slots[c].m_MinMapTextureDescriptorIndex;
            if (!streamed && (fb != 0xFFFFFFFFu || mm != 0xFFFFFFFFu))
                throw std::runtime_error("materials: material " + std::to_string(i) + " names a sampler-feedback or min-mip texture, and its texture is not streamed: texture streaming is "
                                         "on for textures created after trhost_set_texture_streaming only");
            if (streamed) {
                if ((fb != 0xFFFFFFFFu && fb != streamed->m_FeedbackIndex) || (mm != 0xFFFFFFFFu && mm != streamed->m_MinMipIndex))
                    throw std::runtime_error("materials: material " + std::to_string(i) + " names a sampler-feedback or min-mip index that is not the map of its own texture " +
                                             std::to_string(slots[c].m_DescriptorIndex));
                slots[c].m_FeedbackTextureDescriptorIndex = streamed->m_FeedbackIndex;
                slots[c].m_MinMapTextureDescriptorIndex = streamed->m_MinMipIndex;
            }
            anyTextured = true;
        }
    }
    nvrhi::BufferDesc d;
    d.byteSize = numMaterials ? (uint64_t)numMaterials * sizeof(interop::MaterialData) : sizeof(interop::MaterialData);
    d.structStride = sizeof(interop::MaterialData);
    d.debugName = "GlobalMaterialDataBuffer";
    d.initialState = nvrhi::ResourceStates::ShaderResource;
    nvrhi::BufferHandle b = g_Graphic.m_NVRHIDevice->createBuffer(d);
    if (numMaterials) nvrhi::throwIfFailed(trhip_buffer_upload(b->native(), 0, materials, (uint64_t)numMaterials * sizeof(interop::MaterialData)), "Scene material upload");
    g_Graphic.m_GlobalMaterialDataBuffer = b;
    g_Graphic.m_bAnyMaterialTextured = anyTextured;
}

void Scene::LoadNodes(const void* nodes, uint32_t numNodes, const uint32_t* primitiveToNode)
{
    // UpdateInstanceConstsRenderer::CreateNodeTransformsBuffer (BasePassRenderers.cpp:64-104)
    nvrhi::DeviceHandle device = g_Graphic.m_NVRHIDevice;
    m_NumNodes = numNodes;
    m_NodeLocalTransforms.assign((const uint8_t*)nodes, (const uint8_t*)nodes + (size_t)numNodes * sizeof(interop::NodeLocalTransform));
    nvrhi::BufferDesc d;
    d.byteSize = (uint64_t)numNodes * sizeof(interop::NodeLocalTransform);
    d.structStride = sizeof(interop::NodeLocalTransform);
    d.debugName = "Node Transforms Buffer";
    m_NodeLocalTransformsBuffer = device->createBuffer(d);
    nvrhi::BufferDesc p;
    p.byteSize = (uint64_t)m_NumPrimitives * 4;
    p.structStride = 4;
    p.debugName = "PrimitiveIDToNodeID Buffer";
    m_PrimitiveIDToNodeIDBuffer = device->createBuffer(p);
    nvrhi::throwIfFailed(trhip_buffer_upload(m_PrimitiveIDToNodeIDBuffer->native(), 0, primitiveToNode, p.byteSize), "Scene upload");
    m_bUpdateInstanceTransforms = true;
    m_bNodeLocalTransformsDirty = true;
}

void Scene::LoadGIProbes(const float* positions, const float* states, uint32_t numProbes, float probeRadius, bool hideInactive)
{
    nvrhi::DeviceHandle device = g_Graphic.m_NVRHIDevice;
    m_GIProbePositionsBuffer = m_GIProbeStatesBuffer = nullptr;
    m_NumGIProbes = numProbes;
    m_GIProbeRadius = probeRadius;
    m_bHideInactiveGIProbes = hideInactive;
    m_bShowGIProbes = numProbes != 0;
    if (!numProbes) return;
    nvrhi::BufferDesc d;
    d.byteSize = 12ull * numProbes; d.structStride = 12; d.debugName = "GI Probe World Positions";
    m_GIProbePositionsBuffer = device->createBuffer(d);
    nvrhi::throwIfFailed(trhip_buffer_upload(m_GIProbePositionsBuffer->native(), 0, positions, d.byteSize), "Scene::LoadGIProbes");
    d.byteSize = 4ull * numProbes; d.structStride = 4; d.debugName = "GI Probe States";
    m_GIProbeStatesBuffer = device->createBuffer(d);
    nvrhi::throwIfFailed(trhip_buffer_upload(m_GIProbeStatesBuffer->native(), 0, states, d.byteSize), "Scene::LoadGIProbes");
}

void Scene::PostSceneLoad() {}

void Scene::Update()
{
    { HOST_PROFILE_SCOPE("Scene::Update view"); m_View.Update(); }           // Scene.cpp:475

    tf::Taskflow tf;
    { HOST_PROFILE_SCOPE("RenderGraph::InitializeForFrame"); m_RenderGraph->InitializeForFrame(tf); }   // :487
    // pass schedule (:491-512): only the passes of the visibility path exist here
    {
        HOST_PROFILE_SCOPE("RenderGraph::AddRenderer x2 (Setup)");
        m_RenderGraph->AddRenderer(g_UpdateInstanceConstsRenderer);
        m_RenderGraph->AddRenderer(g_GBufferRenderer);
        if (m_bGBuffer && m_bEnableAO) m_RenderGraph->AddRenderer(g_AmbientOcclusionRenderer);   // :499
        if (m_bGBuffer && m_bEnableShadows) m_RenderGraph->AddRenderer(g_ShadowMaskRenderer);    // :500
        if (m_bDeferredLighting && m_bDDGIUpdate) m_RenderGraph->AddRenderer(g_GIRenderer);      // behind the TLAS refit, in front of lighting
        if (m_bDeferredLighting) m_RenderGraph->AddRenderer(g_DeferredLightingRenderer);   // :497, the next pass after the G-buffer
        if (m_bDeferredLighting && m_bEnableSky) m_RenderGraph->AddRenderer(g_SkyRenderer);  // :502
        if (m_bPostProcess && m_bEnableBloom) m_RenderGraph->AddRenderer(g_BloomRenderer);   // :503
        if (m_bPostProcess) {                                                 // :505-507 (the transparents between them are a stub in the reference)
            m_RenderGraph->AddRenderer(g_AdaptLuminanceRenderer);
            m_RenderGraph->AddRenderer(g_TAARenderer);                        // :506; Setup returns false unless IsTAAEnabled()
            m_RenderGraph->AddRenderer(g_PostProcessRenderer);
        }
        m_RenderGraph->AddRenderer(g_GIDebugRenderer);                        // :509 (after the base pass: it reads this frame's HZB)
    }
    { HOST_PROFILE_SCOPE("RenderGraph::Compile"); m_RenderGraph->Compile(); }                            // :515
    { HOST_PROFILE_SCOPE("Executor::corun (Render)"); m_Executor.corun(tf); }                            // :518
}

void Scene::Shutdown()
{
    m_RenderGraph->Shutdown();
    m_RenderGraph.reset();
    m_InstanceConstsBuffer = nullptr;
    m_OpaqueInstanceIDsBuffer = m_AlphaMaskInstanceIDsBuffer = nullptr;
    m_NodeLocalTransformsBuffer = m_PrimitiveIDToNodeIDBuffer = nullptr;
    m_HZB = nullptr;
    m_SyntheticDepth = nullptr;
    m_ShadowMaskTexture = nullptr;
    m_RTDDGIVolume = RTDDGIVolume{};
    m_bEnableDDGI = m_bDDGIUpdate = m_bDDGIProbeRelocation = m_bDDGIProbeClassification = false;
    m_DDGIUpdateCount = 0;
    m_TLAS.reset();
    m_BlueNoise = nullptr;
    m_BloomTexture = nullptr;
    m_LuminanceBuffer = nullptr;
    m_ExposureTexture = nullptr;
    m_GIProbePositionsBuffer = m_GIProbeStatesBuffer = nullptr;
    m_NumGIProbes = 0; m_bShowGIProbes = false;
    m_bDDGIProbeVisualization = false;
}
