// PostProcessRenderer.cpp -- the reference's last pass before the swap chain (source/PostProcessRenderer.cpp): exposure,
// PBRNeutralToneMapping and LinearToSRGB from LightingOutput into the RGBA8_UNORM back buffer, "postprocess_PS_PostProcess"
// (csrc/k_postprocess.hip).
//
// The input at t0 is TAARenderer's g_AntiAliasedLightingOutput when TAA is enabled, else LightingOutput (:25-27, :52).  The bloom texture at t2 is BloomRenderer's when
// generation is on (trhost_set_bloom), else the uploaded one (trhost_upload_bloom); without either t2 stays unbound: black, the
// reference's BlackTexture, and the strength is 0.  There is no
// swap chain: the back buffer is a texture owned here, read back by trhost_download_back_buffer.  The full-screen triangle is a
// direct dispatch of 8x8 groups.
#include "Graphic.h"
#include "GraphicConstants.h"
#include "RenderGraph.h"
#include "Scene.h"
#include "VisibilityOutputs.h"
#include "../ShaderInterop.h"

#include <cstring>

using namespace interop;

void GetLastAdaptLuminanceParams(void* histogram16, void* adapt20, int* adaptRan);   // AdaptLuminanceRenderer.cpp
void ReleaseAdaptLuminanceOutputs();

class PostProcessRenderer : public IRenderer
{
public:
    PostProcessRenderer() : IRenderer("PostProcessRenderer") {}

    nvrhi::TextureHandle m_BackBuffer;               // kBackBufferFormat at render resolution
    PostProcessParameters m_LastParams{};
    bool m_bHasLastParams = false;

    nvrhi::TextureHandle m_Input;                    // this frame's t0
    static nvrhi::TextureHandle BloomTexture() { return g_Scene->m_bEnableBloom ? GetGeneratedBloomTexture() : g_Scene->m_BloomTexture; }

    bool Setup(RenderGraph& renderGraph) override
    {
        if (!g_Scene->m_bPostProcess || g_Scene->m_NumPrimitives == 0) return false;
        if (!m_BackBuffer) {
            nvrhi::TextureDesc desc;
            desc.width = g_Graphic.m_RenderResolution.x;
            desc.height = g_Graphic.m_RenderResolution.y;
            desc.format = GraphicConstants::kBackBufferFormat;
            desc.debugName = "Back Buffer";
            desc.isUAV = true;                       // this build: the pass stores through a UAV
            m_BackBuffer = g_Graphic.m_NVRHIDevice->createTexture(desc);
        }
        if (BloomTexture()) renderGraph.AddExternalReadDependency(BloomTexture().Get());   // :20-23
        m_Input = GetScheduledAntiAliasedLightingOutput();                    // :25-27: g_Scene->IsTAAEnabled() ? g_AntiAliasedLightingOutput : g_LightingOutput
        if (!m_Input) m_Input = GetLightingOutput();
        renderGraph.AddExternalReadDependency(m_Input.Get());                 // :29-32
        renderGraph.AddExternalReadDependency(g_Scene->m_LuminanceBuffer.Get());
        renderGraph.AddExternalWriteDependency(m_BackBuffer.Get());
        return true;
    }

    void Render(nvrhi::CommandListHandle commandList, const RenderGraph&) override
    {
        const nvrhi::TextureHandle bloomTexture = BloomTexture();
        const bool bloom = bloomTexture != nullptr;
        PostProcessParameters passParameters{};                               // :46-50
        passParameters.m_OutputDims = g_Graphic.m_RenderResolution;
        passParameters.m_ManualExposure = g_Scene->m_ManualExposureOverride;
        passParameters.m_MiddleGray = g_Scene->m_MiddleGray;
        passParameters.m_BloomStrength = bloom ? g_Scene->m_BloomStrength : 0.0f;
        m_LastParams = passParameters;
        m_bHasLastParams = true;

        using Item = nvrhi::BindingSetItem;
        Graphic::ComputePassParams p;                                         // :55-73
        p.m_CommandList = commandList;
        p.m_ShaderName = "postprocess_PS_PostProcess";
        p.m_BindingSetDesc.bindings = { Item::PushConstants(0, sizeof(passParameters)), Item::Texture_SRV(0, m_Input),
                                        Item::StructuredBuffer_SRV(1, g_Scene->m_LuminanceBuffer), Item::Texture_UAV(0, m_BackBuffer) };
        if (bloom) p.m_BindingSetDesc.bindings.push_back(Item::Texture_SRV(2, bloomTexture));
        p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(g_Graphic.m_RenderResolution, 8);
        p.m_PushConstantsData = &passParameters;
        p.m_PushConstantsBytes = sizeof(passParameters);
        g_Graphic.AddComputePass(p);
    }
};
DEFINE_RENDERER(PostProcessRenderer);

nvrhi::TextureHandle GetBackBuffer() { return static_cast<PostProcessRenderer*>(g_PostProcessRenderer)->m_BackBuffer; }

bool GetLastPostProcessConsts(void* histogram16, void* adapt20, void* post24, int* adaptRan)
{
    const PostProcessRenderer* r = static_cast<const PostProcessRenderer*>(g_PostProcessRenderer);
    if (!r->m_bHasLastParams) return false;
    GetLastAdaptLuminanceParams(histogram16, adapt20, adaptRan);
    if (post24) memcpy(post24, &r->m_LastParams, sizeof r->m_LastParams);
    return true;
}

void ReleasePostProcessOutputs()
{
    PostProcessRenderer* r = static_cast<PostProcessRenderer*>(g_PostProcessRenderer);
    r->m_BackBuffer = r->m_Input = nullptr;
    r->m_bHasLastParams = false;
    ReleaseAdaptLuminanceOutputs();
}
