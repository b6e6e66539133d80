// ShadowMaskRenderer.cpp -- the reference's renderer between AmbientOcclusionRenderer and DeferredLightingRenderer
// (source/ShadowMaskRenderer.cpp): TraceShadows with m_bDoDenoising = 0, "shadowmask_CS_ShadowMask" (csrc/k_shadowmask.hip), one ray
// per pixel towards the sun through the scene's acceleration structure, into the R8_UNORM shadow mask DeferredLightingRenderer binds
// at t4 and the R16_FLOAT linear view depth.  In front of it the renderer records "raytracing_CS_RefitTLAS", this build's stand-in of
// buildTopLevelAccelStructFromBuffer (BasePassRenderers.cpp:159-160): the reference builds the TLAS behind updateinstanceconsts in
// UpdateInstanceConstsRenderer; here the refit is recorded by its one consumer, still behind that pass in the frame.
//
// Out of scope, as in the back end: DenoiseShadows (NRD SIGMA), CS_PackNormalAndRoughness, the penumbra texture, the ImGui panel.
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

using namespace interop;

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
    bool m_bRanLastFrame = false;
    bool m_bScheduled = false;                       // Setup accepted the current frame: what DeferredLightingRenderer, set up behind it, asks

    bool Setup(RenderGraph& renderGraph) override
    {
        m_bRanLastFrame = m_bScheduled = false;
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
        CreateGBufferPixelTargets();                                          // GBufferA exists before any Render runs
        renderGraph.AddReadDependency(g_DepthStencilBufferRDGTextureHandle);  // :246-248
        renderGraph.AddExternalReadDependency(GetGBufferA().Get());
        renderGraph.AddExternalReadDependency(g_Scene->m_InstanceConstsBuffer.Get());
        renderGraph.AddExternalWriteDependency(m_ShadowMaskTexture.Get());
        renderGraph.AddExternalWriteDependency(m_LinearViewDepthTexture.Get());
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
        passConstants.m_bDoDenoising = 0;
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
            Item::Texture_UAV(0, m_ShadowMaskTexture),
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

void ReleaseShadowMaskOutputs()
{
    ShadowMaskRenderer* r = static_cast<ShadowMaskRenderer*>(g_ShadowMaskRenderer);
    r->m_ShadowMaskTexture = nullptr;
    r->m_LinearViewDepthTexture = nullptr;
    r->m_bRanLastFrame = r->m_bScheduled = false;
}
