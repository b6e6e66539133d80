// AmbientOcclusionRenderer.cpp -- the reference's renderer between GBufferRenderer and DeferredLightingRenderer
// (source/AmbientOcclusionRenderer.cpp, extern/xegtao/XeGTAO.h): XeGTAO's three compute passes,
// "ambientocclusion_CS_XeGTAO_PrefilterDepths", "ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0" and
// "ambientocclusion_CS_XeGTAO_Denoise" (csrc/k_ambientocclusion.hip), from the depth buffer and GBufferA into the SSAO texture
// that DeferredLightingRenderer binds at t3.
//
// Out of scope, as in the back end: the debug output texture and its modes (DEBUG_OUTPUT_MODE is always 0), bent normals, the
// ImGui panel.  The 64 x 64 Hilbert table is not created: the main pass computes the index.  The working depth chain, the working
// AO term and the edges are transient resources as in the reference; the SSAO texture is kept across frames so that it can be
// read back (trhost_download_ssao).
#include "CommonResources.h"
#include "Graphic.h"
#include "GraphicConstants.h"
#include "RenderGraph.h"
#include "Scene.h"
#include "VisibilityOutputs.h"
#include "../ShaderInterop.h"

#include <algorithm>
#include <cstring>
#include <utility>

using namespace interop;

extern RenderGraph::ResourceHandle g_DepthStencilBufferRDGTextureHandle;

namespace
{
constexpr uint32_t kDepthMipLevels = 5;              // XE_GTAO_DEPTH_MIP_LEVELS
constexpr uint32_t kNumThreads = 8;                  // XE_GTAO_NUMTHREADS_X / _Y

// XeGTAO::GTAOUpdateConstants (XeGTAO.h:164-198) with rowMajor = true.  Every operation is a float operation in the reference's
// order: toyrenderer_amd/gtao.py does the same and both hand the GPU the same 96 bytes.
void GTAOUpdateConstants(GTAOConstants& consts, int viewportWidth, int viewportHeight, const Scene& settings, const Matrix& projMatrix, unsigned int frameCounter)
{
    consts.ViewportSize[0] = viewportWidth; consts.ViewportSize[1] = viewportHeight;
    consts.ViewportPixelSize = { 1.0f / (float)viewportWidth, 1.0f / (float)viewportHeight };

    float depthLinearizeMul = -projMatrix.m[3][2];
    float depthLinearizeAdd = projMatrix.m[2][2];
    if (depthLinearizeMul * depthLinearizeAdd < 0)   // the handedness flip
        depthLinearizeAdd = -depthLinearizeAdd;
    consts.DepthUnpackConsts = { depthLinearizeMul, depthLinearizeAdd };

    const float tanHalfFOVY = 1.0f / projMatrix.m[1][1];
    const float tanHalfFOVX = 1.0f / projMatrix.m[0][0];
    consts.CameraTanHalfFOV = { tanHalfFOVX, tanHalfFOVY };
    consts.NDCToViewMul = { consts.CameraTanHalfFOV.x * 2.0f, consts.CameraTanHalfFOV.y * -2.0f };
    consts.NDCToViewAdd = { consts.CameraTanHalfFOV.x * -1.0f, consts.CameraTanHalfFOV.y * 1.0f };
    consts.NDCToViewMul_x_PixelSize = { consts.NDCToViewMul.x * consts.ViewportPixelSize.x, consts.NDCToViewMul.y * consts.ViewportPixelSize.y };

    consts.EffectRadius = settings.m_AORadius;
    consts.EffectFalloffRange = settings.m_AOFalloffRange;
    consts.DenoiseBlurBeta = settings.m_AODenoisePasses == 0 ? 1e4f : 1.2f;   // a high value disables the denoise
    consts.RadiusMultiplier = 1.457f;                // the three "default constants": carried, compiled in by the passes
    consts.SampleDistributionPower = 2.0f;
    consts.ThinOccluderCompensation = 0.0f;
    consts.FinalValuePower = settings.m_AOFinalValuePower;
    consts.DepthMIPSamplingOffset = settings.m_AODepthMIPSamplingOffset;
    consts.NoiseIndex = settings.m_AODenoisePasses > 0 ? (int32_t)(frameCounter % 64) : 0;
    consts.Padding0 = 0;
}
}

class AmbientOcclusionRenderer : public IRenderer
{
public:
    AmbientOcclusionRenderer() : IRenderer("AmbientOcclusionRenderer") {}

    RenderGraph::ResourceHandle m_WorkingDepthBufferRDGTextureHandle;
    RenderGraph::ResourceHandle m_WorkingSSAORDGTextureHandle;
    RenderGraph::ResourceHandle m_WorkingEdgesRDGTextureHandle;
    nvrhi::TextureHandle m_SSAOTexture;              // kSSAOOutputFormat (R8_UINT) at render resolution, owned here for read-back
    GTAOConstants m_LastConsts{};                    // what the last Render uploaded (trhost_get_gtao_consts)
    bool m_bRanLastFrame = false;
    bool m_bScheduled = false;                       // Setup accepted the current frame: what DeferredLightingRenderer, set up behind it, asks

    bool Setup(RenderGraph& renderGraph) override
    {
        m_bRanLastFrame = m_bScheduled = false;
        if (!g_Scene->m_bEnableAO || !g_Scene->m_bGBuffer || g_Scene->m_NumPrimitives == 0) return false;   // :87-90

        nvrhi::TextureDesc desc;                                              // :92-113
        desc.width = g_Graphic.m_RenderResolution.x;
        desc.height = g_Graphic.m_RenderResolution.y;
        desc.mipLevels = kDepthMipLevels;
        desc.format = nvrhi::Format::R16_FLOAT;
        desc.debugName = "XeGTAO Working Depth Buffer";
        desc.isUAV = true;
        desc.initialState = nvrhi::ResourceStates::ShaderResource;
        renderGraph.CreateTransientResource(m_WorkingDepthBufferRDGTextureHandle, desc);

        desc.mipLevels = 1;
        desc.format = nvrhi::Format::R8_UINT;
        if (!m_SSAOTexture) {
            desc.debugName = "SSAO Buffer";
            m_SSAOTexture = g_Graphic.m_NVRHIDevice->createTexture(desc);
        }
        desc.debugName = "Working SSAO Texture";
        renderGraph.CreateTransientResource(m_WorkingSSAORDGTextureHandle, desc);

        desc.format = nvrhi::Format::R8_UNORM;
        desc.debugName = "Working Edges Texture";
        renderGraph.CreateTransientResource(m_WorkingEdgesRDGTextureHandle, desc);

        CreateGBufferPixelTargets();                                          // GBufferA exists before any Render runs
        renderGraph.AddExternalReadDependency(GetGBufferA().Get());           // :123-124
        renderGraph.AddReadDependency(g_DepthStencilBufferRDGTextureHandle);
        renderGraph.AddExternalWriteDependency(m_SSAOTexture.Get());
        m_bScheduled = true;
        return true;
    }

    void Render(nvrhi::CommandListHandle commandList, const RenderGraph& renderGraph) override
    {
        using Item = nvrhi::BindingSetItem;
        const Vector2U res = g_Graphic.m_RenderResolution;
        GTAOConstants GTAOconsts{};                                           // :133-138
        const uint32_t frameCounter = g_Graphic.m_FrameCounter % 256;
        GTAOUpdateConstants(GTAOconsts, (int)res.x, (int)res.y, *g_Scene, g_Scene->m_View.m_ViewToClip, frameCounter);
        m_LastConsts = GTAOconsts;
        m_bRanLastFrame = true;
        nvrhi::BufferHandle passConstantBuffer = g_Graphic.CreateConstantBuffer(commandList, GTAOconsts);

        nvrhi::TextureHandle workingDepthBuffer = renderGraph.GetTexture(m_WorkingDepthBufferRDGTextureHandle);
        nvrhi::TextureHandle workingSSAOTexture = renderGraph.GetTexture(m_WorkingSSAORDGTextureHandle);
        nvrhi::TextureHandle workingEdgesTexture = renderGraph.GetTexture(m_WorkingEdgesRDGTextureHandle);
        nvrhi::TextureHandle depthBuffer = renderGraph.GetTexture(g_DepthStencilBufferRDGTextureHandle);

        {                                                                     // generate depth mips, :154-174
            Graphic::ComputePassParams p;
            p.m_CommandList = commandList;
            p.m_ShaderName = "ambientocclusion_CS_XeGTAO_PrefilterDepths";
            p.m_BindingSetDesc.bindings = { Item::ConstantBuffer(0, passConstantBuffer), Item::Texture_SRV(0, depthBuffer) };
            for (uint32_t mip = 0; mip < kDepthMipLevels; ++mip)
                p.m_BindingSetDesc.bindings.push_back(Item::Texture_UAV(mip, workingDepthBuffer, nvrhi::Format::R16_FLOAT, nvrhi::TextureSubresourceSet{ mip, 1, 0, 1 }));
            p.m_BindingSetDesc.bindings.push_back(Item::Sampler(0, g_CommonResources.PointClampSampler));
            p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(res, Vector2U{ 16, 16 });
            g_Graphic.AddComputePass(p);
        }

        {                                                                     // main pass, :177-207
            XeGTAOMainPassConstantBuffer mainPassConsts{};
            mainPassConsts.m_WorldToViewNoTranslate = g_Scene->m_View.m_WorldToView;
            mainPassConsts.m_WorldToViewNoTranslate.m[3][0] = mainPassConsts.m_WorldToViewNoTranslate.m[3][1] = mainPassConsts.m_WorldToViewNoTranslate.m[3][2] = 0.0f;
            mainPassConsts.m_Quality = g_Scene->m_AOQuality;
            Graphic::ComputePassParams p;
            p.m_CommandList = commandList;
            p.m_ShaderName = "ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0";
            p.m_BindingSetDesc.bindings = {
                Item::ConstantBuffer(0, passConstantBuffer),
                Item::PushConstants(1, sizeof(mainPassConsts)),
                Item::Texture_SRV(0, workingDepthBuffer),
                Item::Texture_SRV(2, GetGBufferA()),
                Item::Texture_UAV(0, workingSSAOTexture),
                Item::Texture_UAV(1, workingEdgesTexture),
                Item::Sampler(0, g_CommonResources.PointClampSampler),
            };
            p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(res, Vector2U{ kNumThreads, kNumThreads });
            p.m_PushConstantsData = &mainPassConsts;
            p.m_PushConstantsBytes = sizeof(mainPassConsts);
            g_Graphic.AddComputePass(p);
        }

        nvrhi::TextureHandle pingPongTextures[2] = { workingSSAOTexture, m_SSAOTexture };
        // even without denoising a single last pass writes the term into the output texture
        const uint32_t nbPasses = std::max(1u, g_Scene->m_AODenoisePasses);  // :214
        for (uint32_t i = 0; i < nbPasses; ++i) {                             // :215-247
            XeGTAODenoiseConstants denoiseConsts{};
            denoiseConsts.m_FinalApply = i == nbPasses - 1;
            Graphic::ComputePassParams p;
            p.m_CommandList = commandList;
            p.m_ShaderName = "ambientocclusion_CS_XeGTAO_Denoise";
            p.m_BindingSetDesc.bindings = {
                Item::ConstantBuffer(0, passConstantBuffer),
                Item::PushConstants(1, sizeof(denoiseConsts)),
                Item::Texture_SRV(0, pingPongTextures[0]),
                Item::Texture_SRV(1, workingEdgesTexture),
                Item::Texture_UAV(0, pingPongTextures[1]),
                Item::Sampler(0, g_CommonResources.PointClampSampler),
            };
            p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(res, Vector2U{ kNumThreads * 2, kNumThreads });
            p.m_PushConstantsData = &denoiseConsts;
            p.m_PushConstantsBytes = sizeof(denoiseConsts);
            g_Graphic.AddComputePass(p);
            std::swap(pingPongTextures[0], pingPongTextures[1]);
        }
    }
};
DEFINE_RENDERER(AmbientOcclusionRenderer);

nvrhi::TextureHandle GetSSAOTexture()
{
    const AmbientOcclusionRenderer* r = static_cast<const AmbientOcclusionRenderer*>(g_AmbientOcclusionRenderer);
    return g_Scene->m_bEnableAO && r->m_bRanLastFrame ? r->m_SSAOTexture : nullptr;
}

// for a renderer set up behind this one in the same frame: the texture this frame's AO pass writes, or null
nvrhi::TextureHandle GetScheduledSSAOTexture()
{
    const AmbientOcclusionRenderer* r = static_cast<const AmbientOcclusionRenderer*>(g_AmbientOcclusionRenderer);
    return g_Scene->m_bEnableAO && g_Scene->m_bGBuffer && r->m_bScheduled ? r->m_SSAOTexture : nullptr;
}

bool GetLastGTAOConsts(void* out96)
{
    const AmbientOcclusionRenderer* r = static_cast<const AmbientOcclusionRenderer*>(g_AmbientOcclusionRenderer);
    if (!g_Scene->m_bEnableAO || !r->m_bRanLastFrame) return false;          // off: the renderer is not scheduled, the last frame ran no AO pass
    memcpy(out96, &r->m_LastConsts, sizeof r->m_LastConsts);
    return true;
}

void ReleaseAmbientOcclusionOutputs()
{
    AmbientOcclusionRenderer* r = static_cast<AmbientOcclusionRenderer*>(g_AmbientOcclusionRenderer);
    r->m_SSAOTexture = nullptr;
    r->m_bRanLastFrame = r->m_bScheduled = false;
}
