// DeferredLightingRenderer.cpp -- the reference's next pass after GBufferRenderer (source/DeferredLightingRenderer.cpp): one
// full-screen pass that reads GBufferA, the motion target, the depth buffer and the shadow mask and writes LightingOutput,
// "deferredlighting_PS_Main" or, under a debug view, "deferredlighting_PS_Main_Debug" (csrc/k_deferredlighting.hip).
//
// DDGI: m_bRTDDGIEnabled = g_Scene->IsDDGIEnabled(), as in the reference; the volume (g_Scene->m_RTDDGIVolume: descriptor at t5,
// probe data, irradiance and distance at t6..t8) comes from trhost_upload_ddgi_volume and, with trhost_set_ddgi_update, is filled by
// GIRenderer (GIRenderer.cpp) in front of this pass.  With the volume bound the constant block carries the descriptor's host copy behind the DeferredLightingConsts
// (include/trhip.h).  The shadow mask at t4 is ShadowMaskRenderer's when that pass is scheduled, else an uploaded one
// (trhost_upload_shadow_mask), else t4 stays unbound: 1.0, the reference's WhiteTexture.  The full-screen triangle with its stencil test on the opaque
// bit is a direct dispatch of 8x8 groups here; the kernel writes where depth > 0.
#include "CommonResources.h"
#include "Graphic.h"
#include "GraphicConstants.h"
#include "RenderGraph.h"
#include "Scene.h"
#include "VisibilityOutputs.h"
#include "../ShaderInterop.h"

#include <cstring>

using namespace interop;

extern RenderGraph::ResourceHandle g_DepthStencilBufferRDGTextureHandle;

class DeferredLightingRenderer : public IRenderer
{
public:
    DeferredLightingRenderer() : IRenderer("DeferredLightingRenderer") {}

    nvrhi::TextureHandle m_LightingOutput;           // kLightingOutputFormat at render resolution, owned here for read-back
    nvrhi::TextureHandle m_SSAOTexture;              // AmbientOcclusionRenderer's output in this frame, or null: t3 stays unbound (255)
    nvrhi::TextureHandle m_ShadowMask;               // ShadowMaskRenderer's output in this frame, else the uploaded mask, else null: t4 stays unbound (1.0)
    DeferredLightingConsts m_LastConsts{};           // what the last Render uploaded (trhost_get_deferred_lighting_consts)
    bool m_bHasLastConsts = false;

    bool Setup(RenderGraph& renderGraph) override
    {
        if (!g_Scene->m_bDeferredLighting || g_Scene->m_NumPrimitives == 0) return false;
        if (!m_LightingOutput) {                                              // :25-34 (a transient there; kept across frames here so that it can be read back)
            nvrhi::TextureDesc desc;
            desc.width = g_Graphic.m_RenderResolution.x;
            desc.height = g_Graphic.m_RenderResolution.y;
            desc.format = GraphicConstants::kLightingOutputFormat;
            desc.debugName = "Lighting Output";
            desc.isUAV = true;                       // this build: the pass stores through a UAV
            desc.initialState = nvrhi::ResourceStates::ShaderResource;
            m_LightingOutput = g_Graphic.m_NVRHIDevice->createTexture(desc);
        }
        CreateGBufferPixelTargets();                                          // GBufferA and GBufferMotion exist before any Render runs
        renderGraph.AddExternalReadDependency(GetGBufferA().Get());           // :36-39
        renderGraph.AddExternalReadDependency(GetMotionBuffer().Get());
        renderGraph.AddReadDependency(g_DepthStencilBufferRDGTextureHandle);
        m_SSAOTexture = GetScheduledSSAOTexture();                            // :41-44
        if (m_SSAOTexture) renderGraph.AddExternalReadDependency(m_SSAOTexture.Get());
        m_ShadowMask = GetScheduledShadowMaskTexture();                        // :46-49
        if (!m_ShadowMask) m_ShadowMask = g_Scene->m_ShadowMaskTexture;
        if (m_ShadowMask) renderGraph.AddExternalReadDependency(m_ShadowMask.Get());
        if (g_Scene->m_bDDGIUpdate && g_Scene->m_RTDDGIVolume.IsValid()) {    // GIRenderer, scheduled in front, writes the two textures this pass reads
            renderGraph.AddExternalReadDependency(g_Scene->m_RTDDGIVolume.m_ProbeIrradiance.Get());
            renderGraph.AddExternalReadDependency(g_Scene->m_RTDDGIVolume.m_ProbeDistance.Get());
        }
        renderGraph.AddExternalWriteDependency(m_LightingOutput.Get());
        return true;
    }

    void Render(nvrhi::CommandListHandle commandList, const RenderGraph& renderGraph) override
    {
        const View& view = g_Scene->m_View;
        DeferredLightingConsts passConstants{};                               // :64-72
        passConstants.m_ClipToWorld = view.m_ClipToWorld;
        memcpy(passConstants.m_CameraOrigin, view.m_Eye, sizeof view.m_Eye);
        memcpy(passConstants.m_DirectionalLightVector, g_Scene->m_DirLightVec, sizeof g_Scene->m_DirLightVec);
        passConstants.m_DirectionalLightStrength = g_Scene->m_DirLightStrength;
        passConstants.m_SSAOEnabled = m_SSAOTexture ? 1 : 0;               // :69, m_bEnableAO
        passConstants.m_LightingOutputResolution = g_Graphic.m_RenderResolution;
        passConstants.m_DebugMode = g_Scene->m_DebugViewMode;
        passConstants.m_bRTDDGIEnabled = g_Scene->IsDDGIEnabled() ? 1 : 0;   // :72
        m_LastConsts = passConstants;
        m_bHasLastConsts = true;

        // the reference's per-frame clear of the lighting output (Scene.cpp:42-70): the pass leaves sky texels alone
        commandList->clearTextureFloat(m_LightingOutput, nvrhi::AllSubresources, nvrhi::Color{ 0.0f });

        // the volume's resources are bound whenever there is one (:78-82), its host copy with them; the back end looks at
        // them with the flag or in view 10 only
        const Scene::RTDDGIVolume& volume = g_Scene->m_RTDDGIVolume;
        const bool bindVolume = volume.IsValid();
        struct WithVolume { DeferredLightingConsts consts; DDGIVolumeDesc desc; } withVolume{ passConstants, volume.m_Desc };
        static_assert(sizeof(WithVolume) == 176, "DeferredLightingConsts + DDGIVolumeDesc");

        using Item = nvrhi::BindingSetItem;
        Graphic::ComputePassParams p;                                         // :84-119
        p.m_CommandList = commandList;
        p.m_ShaderName = g_Scene->m_DebugViewMode != 0 ? "deferredlighting_PS_Main_Debug" : "deferredlighting_PS_Main";   // :109-110
        p.m_BindingSetDesc.bindings = {
            Item::ConstantBuffer(0, bindVolume ? g_Graphic.CreateConstantBuffer(commandList, withVolume) : g_Graphic.CreateConstantBuffer(commandList, passConstants)),
            Item::Texture_SRV(0, GetGBufferA()),
            Item::Texture_SRV(1, GetMotionBuffer()),
            Item::Texture_SRV(2, renderGraph.GetTexture(g_DepthStencilBufferRDGTextureHandle)),
            Item::Texture_UAV(0, m_LightingOutput),
        };
        if (m_SSAOTexture) p.m_BindingSetDesc.bindings.push_back(Item::Texture_SRV(3, m_SSAOTexture));   // :77
        if (m_ShadowMask) p.m_BindingSetDesc.bindings.push_back(Item::Texture_SRV(4, m_ShadowMask));
        if (bindVolume) {
            p.m_BindingSetDesc.bindings.push_back(Item::StructuredBuffer_SRV(5, volume.m_DescBuffer));
            p.m_BindingSetDesc.bindings.push_back(Item::Texture_SRV(6, volume.m_ProbeData));
            p.m_BindingSetDesc.bindings.push_back(Item::Texture_SRV(7, volume.m_ProbeIrradiance));
            p.m_BindingSetDesc.bindings.push_back(Item::Texture_SRV(8, volume.m_ProbeDistance));
        }
        p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(g_Graphic.m_RenderResolution, 8);
        g_Graphic.AddComputePass(p);
    }
};
DEFINE_RENDERER(DeferredLightingRenderer);

nvrhi::TextureHandle GetLightingOutput() { return static_cast<DeferredLightingRenderer*>(g_DeferredLightingRenderer)->m_LightingOutput; }

bool GetLastDeferredLightingConsts(void* out112)
{
    const DeferredLightingRenderer* r = static_cast<const DeferredLightingRenderer*>(g_DeferredLightingRenderer);
    if (!r->m_bHasLastConsts) return false;
    memcpy(out112, &r->m_LastConsts, sizeof r->m_LastConsts);
    return true;
}

void ReleaseDeferredLightingOutputs()
{
    DeferredLightingRenderer* r = static_cast<DeferredLightingRenderer*>(g_DeferredLightingRenderer);
    r->m_LightingOutput = nullptr;
    r->m_SSAOTexture = nullptr;
    r->m_ShadowMask = nullptr;
    r->m_bHasLastConsts = false;
}
