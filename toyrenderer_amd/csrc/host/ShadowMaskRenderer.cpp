// ShadowMaskRenderer.cpp -- the reference's renderer between AmbientOcclusionRenderer and DeferredLightingRenderer
// (source/ShadowMaskRenderer.cpp): TraceShadows, "shadowmask_CS_ShadowMask" (csrc/k_shadowmask.hip), one ray
// per pixel towards the sun through the scene's acceleration structure, into the R8_UNORM shadow mask DeferredLightingRenderer binds
// at t4 and the R16_FLOAT linear view depth.  In front of it the renderer records "raytracing_CS_RefitTLAS", this build's stand-in of
// buildTopLevelAccelStructFromBuffer (BasePassRenderers.cpp:159-160): the reference builds the TLAS behind updateinstanceconsts in
// UpdateInstanceConstsRenderer; here the refit is recorded by its one consumer, still behind that pass in the frame.
//
// With Scene::m_bEnableShadowDenoising (trhost_set_shadow_denoising; off by default) Render is TraceShadows followed by DenoiseShadows, as
// in the reference: Setup adds its transient textures (:205-233: the R16_FLOAT penumbra texture, which the trace then writes with
// m_bDoDenoising = 1 in place of the mask, and the R10G10B10A2_UNORM normal roughness texture) and, in place of NRD's pools, the
// denoiser's own (the R8_UINT tiles, two RG16_FLOAT shadow data, two R16_FLOAT histories read and written in turn); PackNormalRoughness
// (:307-335) and the four dispatches of csrc/k_sigma.hip follow the trace (:337-500; NRD is not in the reference's tree: the entry
// names are the ones its loop forms, the passes, their bindings and SigmaConsts are this project's own).  m_DenoisingRange is
// max(100, 2 * scene radius) (:368) with the radius 0: the mirror keeps no bounding sphere.  The history is reset on the first
// frame and on request (trhost_reset_shadow_history).  Out of scope: the ImGui panel.
// The acceleration structure is built by Scene::LoadRaytracing through the back end's builder (trhip_blas_build, trhip_tlas_build).
// One deviation: m_TanSunAngularRadius is tan(radians(d / 2)) evaluated in double and rounded once (the reference calls tanf), so
// that both hosts hand the GPU the same word.  The mask and the depth are kept across frames so that they can be read back.
#include "CommonResources.h"
#include "Graphic.h"
#include "GraphicConstants.h"
#include "RenderGraph.h"
#include "Scene.h"
#include "VisibilityOutputs.h"
#include "../ShaderInterop.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace interop;

constexpr uint32_t kSigmaTile = 16;                  // csrc/k_sigma.hip: the classified tile's side

extern RenderGraph::ResourceHandle g_DepthStencilBufferRDGTextureHandle;

// "raytracing_CS_RefitTLAS" on the instance buffer's current matrices: recorded by the first consumer of the structure in a frame
// (this renderer, or GIRenderer when shadows are off).
void RecordRefitTLAS(nvrhi::CommandListHandle commandList)
{
    using Item = nvrhi::BindingSetItem;
    const nvrhi::rt::AccelStruct& as = *g_Scene->m_TLAS;
    RefitTLASConstants k{ g_Scene->m_NumPrimitives, as.numNodes, as.numLevels };
    Graphic::ComputePassParams p;
    p.m_CommandList = commandList;
    p.m_ShaderName = "raytracing_CS_RefitTLAS";
    p.m_BindingSetDesc.bindings = {
        Item::PushConstants(0, sizeof(k)),
        Item::StructuredBuffer_SRV(0, g_Scene->m_InstanceConstsBuffer),
        Item::StructuredBuffer_SRV(1, as.blasHeaders),
        Item::StructuredBuffer_SRV(2, as.blasNodes),
        Item::StructuredBuffer_SRV(3, as.levelOffsets),
        Item::StructuredBuffer_SRV(4, as.levelNodes),
        Item::StructuredBuffer_UAV(0, as.nodes),
        Item::StructuredBuffer_UAV(1, as.instances),
    };
    p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(g_Scene->m_NumPrimitives, 64);
    p.m_PushConstantsData = &k;
    p.m_PushConstantsBytes = sizeof(k);
    g_Graphic.AddComputePass(p);
}

class ShadowMaskRenderer : public IRenderer
{
public:
    ShadowMaskRenderer() : IRenderer("ShadowMaskRenderer") {}

    nvrhi::TextureHandle m_ShadowMaskTexture;        // R8_UNORM at render resolution, owned here for read-back
    nvrhi::TextureHandle m_LinearViewDepthTexture;   // R16_FLOAT
    ShadowMaskConsts m_LastConsts{};                 // what the last Render uploaded (trhost_get_shadow_mask_consts)
    nvrhi::TextureHandle m_ShadowPenumbraTexture, m_NormalRoughnessTexture, m_ShadowTilesTexture, m_ShadowData[2], m_ShadowHistory[2];   // the denoiser's
    uint32_t m_HistoryWritten = 1;                   // the history texture the last DenoiseShadows wrote
    SigmaConsts m_LastSigmaConsts{};                 // m_Pass 0 (trhost_get_sigma_consts)
    bool m_bDenoisedLastFrame = false;
    bool m_bRanLastFrame = false;
    bool m_bScheduled = false;                       // Setup accepted the current frame: what DeferredLightingRenderer, set up behind it, asks

    bool Setup(RenderGraph& renderGraph) override
    {
        m_bRanLastFrame = m_bScheduled = m_bDenoisedLastFrame = false;
        if (!g_Scene->m_bEnableShadows || !g_Scene->m_bGBuffer || !g_Scene->m_TLAS || !g_Scene->m_BlueNoise || g_Scene->m_NumPrimitives == 0) return false;   // :189-192

        nvrhi::TextureDesc desc;                                              // :194-244
        desc.width = g_Graphic.m_RenderResolution.x;
        desc.height = g_Graphic.m_RenderResolution.y;
        desc.isUAV = true;
        desc.initialState = nvrhi::ResourceStates::ShaderResource;
        if (!m_ShadowMaskTexture) {
            desc.format = GraphicConstants::kShadowMaskFormat;
            desc.debugName = "Shadow Mask Texture";
            m_ShadowMaskTexture = g_Graphic.m_NVRHIDevice->createTexture(desc);
            desc.format = nvrhi::Format::R16_FLOAT;
            desc.debugName = "Linear View Depth";
            m_LinearViewDepthTexture = g_Graphic.m_NVRHIDevice->createTexture(desc);
        }
        if (g_Scene->m_bEnableShadowDenoising && !m_ShadowPenumbraTexture) {  // :205-233
            auto make = [&](nvrhi::Format format, const char* name, uint32_t w, uint32_t h) {
                nvrhi::TextureDesc d = desc;
                d.width = w; d.height = h; d.format = format; d.debugName = name;
                return g_Graphic.m_NVRHIDevice->createTexture(d);
            };
            const uint32_t W = desc.width, H = desc.height;
            m_ShadowPenumbraTexture = make(nvrhi::Format::R16_FLOAT, "Shadow Penumbra Texture", W, H);
            m_NormalRoughnessTexture = make(nvrhi::Format::R10G10B10A2_UNORM, "Normal Roughness Texture", W, H);
            m_ShadowTilesTexture = make(nvrhi::Format::R8_UINT, "Shadow Tiles", (W + kSigmaTile - 1) / kSigmaTile, (H + kSigmaTile - 1) / kSigmaTile);
            m_ShadowData[0] = make(nvrhi::Format::RG16_FLOAT, "Shadow Data 0", W, H);
            m_ShadowData[1] = make(nvrhi::Format::RG16_FLOAT, "Shadow Data 1", W, H);
            m_ShadowHistory[0] = make(nvrhi::Format::R16_FLOAT, "Shadow History 0", W, H);
            m_ShadowHistory[1] = make(nvrhi::Format::R16_FLOAT, "Shadow History 1", W, H);
            m_HistoryWritten = 1;
            g_Scene->m_bResetShadowHistory = true;                            // new textures hold nothing
        }
        CreateGBufferPixelTargets();                                          // GBufferA exists before any Render runs
        renderGraph.AddReadDependency(g_DepthStencilBufferRDGTextureHandle);  // :246-248
        renderGraph.AddExternalReadDependency(GetGBufferA().Get());
        renderGraph.AddExternalReadDependency(g_Scene->m_InstanceConstsBuffer.Get());
        renderGraph.AddExternalWriteDependency(m_ShadowMaskTexture.Get());
        renderGraph.AddExternalWriteDependency(m_LinearViewDepthTexture.Get());
        if (g_Scene->m_bEnableShadowDenoising) {
            renderGraph.AddExternalReadDependency(GetMotionBuffer().Get());   // :248
            renderGraph.AddExternalReadDependency(m_ShadowHistory[m_HistoryWritten].Get());
            renderGraph.AddExternalWriteDependency(m_ShadowHistory[1 - m_HistoryWritten].Get());
        }
        m_bScheduled = true;
        return true;
    }

    void Render(nvrhi::CommandListHandle commandList, const RenderGraph& renderGraph) override
    {
        using Item = nvrhi::BindingSetItem;
        const nvrhi::rt::AccelStruct& as = *g_Scene->m_TLAS;
        RecordRefitTLAS(commandList);                                         // the TLAS of this frame's matrices

        const View& view = g_Scene->m_View;
        ShadowMaskConsts passConstants{};                                     // :264-274
        passConstants.m_ClipToWorld = view.m_ClipToWorld;
        memcpy(passConstants.m_DirectionalLightDirection, g_Scene->m_DirLightVec, sizeof g_Scene->m_DirLightVec);
        passConstants.m_OutputResolution = g_Graphic.m_RenderResolution;
        passConstants.m_NoisePhase = (float)(g_Graphic.m_FrameCounter & 0xff) * 1.61803398875f;   // kGoldenRatio
        passConstants.m_TanSunAngularRadius = g_Scene->m_bEnableSoftShadows ? (float)std::tan((double)g_Scene->m_SunAngularDiameter / 2.0 * (3.14159265358979323846 / 180.0)) : 0.0f;
        memcpy(passConstants.m_CameraPosition, view.m_Eye, sizeof view.m_Eye);
        const bool denoise = g_Scene->m_bEnableShadowDenoising;
        passConstants.m_bDoDenoising = denoise ? 1 : 0;                       // :272
        passConstants.m_RayStartOffset = g_Scene->m_ShadowRayStartOffset;
        m_LastConsts = passConstants;
        m_bRanLastFrame = true;
        nvrhi::BufferHandle passConstantBuffer = g_Graphic.CreateConstantBuffer(commandList, passConstants);

        Graphic::ComputePassParams p;                                         // :278-304
        p.m_CommandList = commandList;
        p.m_ShaderName = "shadowmask_CS_ShadowMask";
        p.m_BindingSetDesc.bindings = {
            Item::ConstantBuffer(0, passConstantBuffer),
            Item::Texture_SRV(0, renderGraph.GetTexture(g_DepthStencilBufferRDGTextureHandle)),
            Item::RayTracingAccelStruct(1, g_Scene->m_TLAS.get()),
            Item::Texture_SRV(2, GetGBufferA()),
            Item::StructuredBuffer_SRV(3, g_Scene->m_InstanceConstsBuffer),
            Item::StructuredBuffer_SRV(4, g_Graphic.m_GlobalVertexBuffer),
            Item::StructuredBuffer_SRV(5, g_Graphic.m_GlobalMaterialDataBuffer),
            Item::StructuredBuffer_SRV(6, g_Graphic.m_GlobalIndexBuffer),
            Item::StructuredBuffer_SRV(7, g_Graphic.m_GlobalMeshDataBuffer),
            Item::Texture_SRV(8, g_Scene->m_BlueNoise),
            Item::Texture_UAV(0, denoise ? m_ShadowPenumbraTexture : m_ShadowMaskTexture),   // :259
            Item::Texture_UAV(1, m_LinearViewDepthTexture),
            Item::StructuredBuffer_SRV(9, as.instances),                      // the structure's other buffers (include/trhip.h)
            Item::StructuredBuffer_SRV(10, as.blasHeaders),
            Item::StructuredBuffer_SRV(11, as.blasNodes),
            Item::StructuredBuffer_SRV(12, as.triOrder),
            Item::Sampler(0, g_CommonResources.LinearClampSampler),           // accepted and ignored (texture-free materials)
            Item::Sampler(1, g_CommonResources.LinearClampSampler),
        };
        if (g_Scene->m_bAlphaTest && g_Graphic.m_bAnyMaterialTextured)        // GetRayHitInstanceGBufferParams samples the albedo texture's alpha (t19)
            p.m_BindingSetDesc.bindings.push_back(Item::DescriptorTable(19, g_Graphic.m_SrvUavCbvDescriptorTable));
        p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(passConstants.m_OutputResolution, 8);
        g_Graphic.AddComputePass(p);
        if (denoise) DenoiseShadows(commandList, renderGraph);
    }

    void DenoiseShadows(nvrhi::CommandListHandle commandList, const RenderGraph& renderGraph)
    {
        using Item = nvrhi::BindingSetItem;
        const View& view = g_Scene->m_View;
        const Vector2U res = g_Graphic.m_RenderResolution;
        {                                                                     // PackNormalRoughness (:307-335)
            PackNormalAndRoughnessConsts k{ res };
            Graphic::ComputePassParams p;
            p.m_CommandList = commandList;
            p.m_ShaderName = "shadowmask_CS_PackNormalAndRoughness";
            p.m_BindingSetDesc.bindings = { Item::PushConstants(0, sizeof(k)), Item::Texture_SRV(2, GetGBufferA()), Item::Texture_UAV(0, m_NormalRoughnessTexture) };
            p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(res, 8);
            p.m_PushConstantsData = &k;
            p.m_PushConstantsBytes = sizeof(k);
            g_Graphic.AddComputePass(p);
        }
        SigmaConsts k{};                                                      // the settings of :345-374 that the project's passes read
        k.m_ClipToWorld = view.m_ClipToWorld;
        k.m_OutputDims = res;
        if (g_Scene->IsTAAEnabled())                                          // TAAConsts' value; (0, 0) without TAA
            k.m_JitterDelta = Vector2{ view.m_PrevJitterOffset.x - view.m_CurrentJitterOffset.x, view.m_PrevJitterOffset.y - view.m_CurrentJitterOffset.y };
        k.m_PixelUnproject = 2.0f / (view.m_ViewToClip.m[1][1] * (float)res.y);
        k.m_DenoisingRange = 100.0f;                                          // max(100, 2 * radius), :368; the mirror keeps no bounding sphere
        k.m_PlaneDistanceSensitivity = g_Scene->m_ShadowPlaneDistanceSensitivity;
        k.m_StabilizationStrength = g_Scene->m_ShadowStabilizationStrength;
        k.m_SigmaScale = g_Scene->m_ShadowSigmaScale;
        k.m_FrameIndex = g_Graphic.m_FrameCounter;                            // :369
        k.m_bResetHistory = g_Scene->m_bResetShadowHistory ? 1 : 0;
        m_LastSigmaConsts = k;
        m_bDenoisedLastFrame = true;
        SigmaConsts k1 = k;
        k1.m_Pass = 1;
        nvrhi::BufferHandle cb0 = g_Graphic.CreateConstantBuffer(commandList, k), cb1 = g_Graphic.CreateConstantBuffer(commandList, k1);
        nvrhi::TextureHandle depth = renderGraph.GetTexture(g_DepthStencilBufferRDGTextureHandle);
        auto pass = [&](const char* name, std::vector<nvrhi::BindingSetItem> bindings, uint32_t side) {
            Graphic::ComputePassParams p;
            p.m_CommandList = commandList;
            p.m_ShaderName = name;
            p.m_BindingSetDesc.bindings = std::move(bindings);
            p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(res, side);
            g_Graphic.AddComputePass(p);
        };
        pass("SIGMA_Shadow_ClassifyTiles.cs", { Item::ConstantBuffer(0, cb0), Item::Texture_SRV(0, m_ShadowPenumbraTexture), Item::Texture_SRV(1, m_LinearViewDepthTexture),
                                                Item::Texture_UAV(0, m_ShadowTilesTexture), Item::Texture_UAV(1, m_ShadowData[0]) }, kSigmaTile);
        for (uint32_t i = 0; i < 2; ++i)
            pass(i ? "SIGMA_Shadow_PostBlur.cs" : "SIGMA_Shadow_Blur.cs",
                 { Item::ConstantBuffer(0, i ? cb1 : cb0), Item::Texture_SRV(0, m_ShadowData[i]), Item::Texture_SRV(1, m_LinearViewDepthTexture), Item::Texture_SRV(2, depth),
                   Item::Texture_SRV(3, m_NormalRoughnessTexture), Item::Texture_SRV(4, m_ShadowTilesTexture), Item::Texture_UAV(0, m_ShadowData[1 - i]) }, 8);
        pass("SIGMA_Shadow_TemporalStabilization.cs",
             { Item::ConstantBuffer(0, cb0), Item::Texture_SRV(0, m_ShadowData[0]), Item::Texture_SRV(1, m_LinearViewDepthTexture), Item::Texture_SRV(2, GetMotionBuffer()),
               Item::Texture_SRV(3, m_ShadowHistory[m_HistoryWritten]), Item::Texture_SRV(4, m_ShadowTilesTexture), Item::Texture_UAV(0, m_ShadowHistory[1 - m_HistoryWritten]),
               Item::Texture_UAV(1, m_ShadowMaskTexture) }, 8);
        m_HistoryWritten = 1 - m_HistoryWritten;
        g_Scene->m_bResetShadowHistory = false;
    }
};
DEFINE_RENDERER(ShadowMaskRenderer);

nvrhi::TextureHandle GetShadowMaskTexture()
{
    const ShadowMaskRenderer* r = static_cast<const ShadowMaskRenderer*>(g_ShadowMaskRenderer);
    return g_Scene->m_bEnableShadows && r->m_bRanLastFrame ? r->m_ShadowMaskTexture : nullptr;
}

// for a renderer set up behind this one in the same frame: the texture this frame's trace writes, or null
nvrhi::TextureHandle GetScheduledShadowMaskTexture()
{
    const ShadowMaskRenderer* r = static_cast<const ShadowMaskRenderer*>(g_ShadowMaskRenderer);
    return g_Scene->m_bEnableShadows && r->m_bScheduled ? r->m_ShadowMaskTexture : nullptr;
}

bool GetLastShadowMaskConsts(void* out112)
{
    const ShadowMaskRenderer* r = static_cast<const ShadowMaskRenderer*>(g_ShadowMaskRenderer);
    if (!g_Scene->m_bEnableShadows || !r->m_bRanLastFrame) return false;
    memcpy(out112, &r->m_LastConsts, sizeof r->m_LastConsts);
    return true;
}

// what the last frame's denoiser left: which 0 the penumbra texture, 1 the tiles, 2 the history it wrote; null if it did not run
nvrhi::TextureHandle GetShadowDenoiserTexture(int which)
{
    const ShadowMaskRenderer* r = static_cast<const ShadowMaskRenderer*>(g_ShadowMaskRenderer);
    if (!g_Scene->m_bEnableShadows || !r->m_bDenoisedLastFrame) return nullptr;
    return which == 0 ? r->m_ShadowPenumbraTexture : which == 1 ? r->m_ShadowTilesTexture : r->m_ShadowHistory[r->m_HistoryWritten];
}

bool GetLastSigmaConsts(void* out112)
{
    const ShadowMaskRenderer* r = static_cast<const ShadowMaskRenderer*>(g_ShadowMaskRenderer);
    if (!g_Scene->m_bEnableShadows || !r->m_bDenoisedLastFrame) return false;
    memcpy(out112, &r->m_LastSigmaConsts, sizeof r->m_LastSigmaConsts);
    return true;
}

void ReleaseShadowMaskOutputs()
{
    ShadowMaskRenderer* r = static_cast<ShadowMaskRenderer*>(g_ShadowMaskRenderer);
    r->m_ShadowPenumbraTexture = r->m_NormalRoughnessTexture = r->m_ShadowTilesTexture = nullptr;
    r->m_ShadowData[0] = r->m_ShadowData[1] = r->m_ShadowHistory[0] = r->m_ShadowHistory[1] = nullptr;
    r->m_HistoryWritten = 1;
    r->m_bDenoisedLastFrame = false;
    r->m_ShadowMaskTexture = nullptr;
    r->m_LinearViewDepthTexture = nullptr;
    r->m_bRanLastFrame = r->m_bScheduled = false;
}
