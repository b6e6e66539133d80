// TAARenderer.cpp -- the place of the reference's TAARenderer (source/TAARenderer.cpp), scheduled between AdaptLuminanceRenderer
// and PostProcessRenderer (Scene.cpp:505-507).  The reference's Render only hands LightingOutput, the depth copy and the motion
// target (:273-275) to DLSS or FSR, and neither SDK is in its tree; here the one dispatch is "taa_CS_TemporalResolve", the
// project's own statement of the published resolve (csrc/k_taa.hip).  What is the reference's is kept: g_AntiAliasedLightingOutput
// in kLightingOutputFormat at render resolution (:263-271), which PostProcessRenderer then reads, and the jitter offsets of
// View::Update.  Render size = display size, no sharpening, no reactive mask (the reference's own TODO).
//
// Owned here and kept across frames: the two RGBA16_FLOAT history textures (xyz the colour, w the accumulated sample count), read
// and written in turn.  The history is reset on the first frame and on request (trhost_reset_taa_history).
#include "Graphic.h"
#include "GraphicConstants.h"
#include "RenderGraph.h"
#include "Scene.h"
#include "VisibilityOutputs.h"
#include "../ShaderInterop.h"

#include <cstring>

using namespace interop;

extern RenderGraph::ResourceHandle g_DepthStencilBufferRDGTextureHandle;

class TAARenderer : public IRenderer
{
public:
    TAARenderer() : IRenderer("TAARenderer") {}

    nvrhi::TextureHandle m_History[2];               // RGBA16_FLOAT at render resolution
    nvrhi::TextureHandle m_AntiAliasedLightingOutput;   // g_AntiAliasedLightingOutput
    uint32_t m_Written = 1;                          // the history texture the last Render wrote
    TAAConsts m_LastConsts{};
    bool m_bRanLastFrame = false;

    bool Setup(RenderGraph& renderGraph) override
    {
        m_bRanLastFrame = false;
        if (!g_Scene->IsTAAEnabled() || !g_Scene->m_bDeferredLighting || g_Scene->m_NumPrimitives == 0) return false;
        auto make = [](nvrhi::Format format, const char* name) {
            nvrhi::TextureDesc desc;
            desc.width = g_Graphic.m_RenderResolution.x;
            desc.height = g_Graphic.m_RenderResolution.y;
            desc.format = format;
            desc.debugName = name;
            desc.isUAV = true;
            desc.initialState = nvrhi::ResourceStates::ShaderResource;
            return g_Graphic.m_NVRHIDevice->createTexture(desc);
        };
        if (!m_AntiAliasedLightingOutput) {                                   // :263-271
            m_AntiAliasedLightingOutput = make(GraphicConstants::kLightingOutputFormat, "Anti-Aliased Lighting Output");
            m_History[0] = make(nvrhi::Format::RGBA16_FLOAT, "TAA History 0");
            m_History[1] = make(nvrhi::Format::RGBA16_FLOAT, "TAA History 1");
            m_Written = 1;
            g_Scene->m_bResetTAAHistory = true;                               // new textures hold nothing
        }
        renderGraph.AddExternalReadDependency(GetLightingOutput().Get());     // :273-275
        renderGraph.AddReadDependency(g_DepthStencilBufferRDGTextureHandle);
        renderGraph.AddExternalReadDependency(GetMotionBuffer().Get());
        renderGraph.AddExternalReadDependency(m_History[m_Written].Get());
        renderGraph.AddExternalWriteDependency(m_History[1 - m_Written].Get());
        renderGraph.AddExternalWriteDependency(m_AntiAliasedLightingOutput.Get());
        return true;
    }

    void Render(nvrhi::CommandListHandle commandList, const RenderGraph& renderGraph) override
    {
        const View& view = g_Scene->m_View;
        TAAConsts passConstants{};
        passConstants.m_OutputDims = g_Graphic.m_RenderResolution;
        passConstants.m_JitterDelta = Vector2{ view.m_PrevJitterOffset.x - view.m_CurrentJitterOffset.x, view.m_PrevJitterOffset.y - view.m_CurrentJitterOffset.y };
        passConstants.m_MinBlend = g_Scene->m_TAAMinBlend;
        passConstants.m_MaxSampleCount = g_Scene->m_TAAMaxSampleCount;
        passConstants.m_bResetHistory = g_Scene->m_bResetTAAHistory ? 1 : 0;
        m_LastConsts = passConstants;
        m_bRanLastFrame = true;

        using Item = nvrhi::BindingSetItem;
        Graphic::ComputePassParams p;
        p.m_CommandList = commandList;
        p.m_ShaderName = "taa_CS_TemporalResolve";
        p.m_BindingSetDesc.bindings = { Item::PushConstants(0, sizeof(passConstants)), Item::Texture_SRV(0, GetLightingOutput()),
                                        Item::Texture_SRV(1, renderGraph.GetTexture(g_DepthStencilBufferRDGTextureHandle)), Item::Texture_SRV(2, GetMotionBuffer()),
                                        Item::Texture_SRV(3, m_History[m_Written]), Item::Texture_UAV(0, m_History[1 - m_Written]),
                                        Item::Texture_UAV(1, m_AntiAliasedLightingOutput) };
        p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(g_Graphic.m_RenderResolution, 8);
        p.m_PushConstantsData = &passConstants;
        p.m_PushConstantsBytes = sizeof(passConstants);
        g_Graphic.AddComputePass(p);
        m_Written = 1 - m_Written;
        g_Scene->m_bResetTAAHistory = false;
    }
};
DEFINE_RENDERER(TAARenderer);

// the frame being set up will run the resolve: PostProcessRenderer reads its output (PostProcessRenderer.cpp:25-27, :52)
nvrhi::TextureHandle GetScheduledAntiAliasedLightingOutput()
{
    return g_Scene->IsTAAEnabled() ? static_cast<TAARenderer*>(g_TAARenderer)->m_AntiAliasedLightingOutput : nullptr;
}

nvrhi::TextureHandle GetAntiAliasedLightingOutput()
{
    const TAARenderer* r = static_cast<const TAARenderer*>(g_TAARenderer);
    return r->m_bRanLastFrame ? r->m_AntiAliasedLightingOutput : nullptr;
}

nvrhi::TextureHandle GetTAAHistory()
{
    const TAARenderer* r = static_cast<const TAARenderer*>(g_TAARenderer);
    return r->m_bRanLastFrame ? r->m_History[r->m_Written] : nullptr;
}

bool GetLastTAAConsts(void* out32, float* currentJitter2, float* prevJitter2)
{
    const TAARenderer* r = static_cast<const TAARenderer*>(g_TAARenderer);
    if (!r->m_bRanLastFrame) return false;
    if (out32) memcpy(out32, &r->m_LastConsts, sizeof r->m_LastConsts);
    const View& view = g_Scene->m_View;
    if (currentJitter2) { currentJitter2[0] = view.m_CurrentJitterOffset.x; currentJitter2[1] = view.m_CurrentJitterOffset.y; }
    if (prevJitter2) { prevJitter2[0] = view.m_PrevJitterOffset.x; prevJitter2[1] = view.m_PrevJitterOffset.y; }
    return true;
}

void ReleaseTAAOutputs()
{
    TAARenderer* r = static_cast<TAARenderer*>(g_TAARenderer);
    r->m_History[0] = r->m_History[1] = r->m_AntiAliasedLightingOutput = nullptr;
    r->m_bRanLastFrame = false;
    r->m_Written = 1;
}
