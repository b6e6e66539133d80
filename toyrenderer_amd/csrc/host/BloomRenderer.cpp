// BloomRenderer.cpp -- the reference's bloom pass (source/BloomRenderer.cpp), scheduled between DeferredLightingRenderer and
// AdaptLuminanceRenderer (Scene.cpp:503): m_NbBloomMips - 1 downsamples of "bloom_PS_Downsample" from LightingOutput down the
// mips of the bloom texture, then as many "bloom_PS_Upsample" passes back up, each overwriting its destination mip
// (BlendOpaque).  PostProcessRenderer reads mip 0 at t2.  The kernels and their arithmetic: csrc/k_bloom.hip.
//
// As with the other image passes here, the full-screen triangle with its viewport is a direct dispatch of 8x8 groups over the
// destination mip, which is bound as a UAV; the texture is a transient in the reference and kept across frames here so that it
// can be read back (trhost_download_bloom).  The reference leaves the BloomConsts fields a pass does not read uninitialised;
// they are zero here.
#include "CommonResources.h"
#include "Graphic.h"
#include "GraphicConstants.h"
#include "RenderGraph.h"
#include "Scene.h"
#include "VisibilityOutputs.h"
#include "../ShaderInterop.h"

#include <cstring>
#include <vector>

using namespace interop;

class BloomRenderer : public IRenderer
{
public:
    BloomRenderer() : IRenderer("BloomRenderer") {}

    nvrhi::TextureHandle m_BloomTexture;             // kLightingOutputFormat at render resolution, m_NbBloomMips mips
    std::vector<BloomConsts> m_LastConsts;           // of the last Render, downsamples first (trhost_get_bloom_consts)

    bool Setup(RenderGraph& renderGraph) override
    {
        if (!g_Scene->m_bEnableBloom || !g_Scene->m_bPostProcess || g_Scene->m_NumPrimitives == 0) return false;   // :36-39
        if (m_BloomTexture && m_BloomTexture->getDesc().mipLevels != g_Scene->m_NbBloomMips) m_BloomTexture = nullptr;
        if (!m_BloomTexture) {                                                // :41-50
            nvrhi::TextureDesc desc;
            desc.width = g_Graphic.m_RenderResolution.x;
            desc.height = g_Graphic.m_RenderResolution.y;
            desc.format = GraphicConstants::kLightingOutputFormat;
            desc.debugName = "Bloom Texture";
            desc.mipLevels = g_Scene->m_NbBloomMips;
            desc.isRenderTarget = true;
            desc.isUAV = true;                       // this build: the passes store through a UAV
            desc.initialState = nvrhi::ResourceStates::ShaderResource;
            m_BloomTexture = g_Graphic.m_NVRHIDevice->createTexture(desc);
        }
        renderGraph.AddExternalReadDependency(GetLightingOutput().Get());     // :52
        renderGraph.AddExternalWriteDependency(m_BloomTexture.Get());
        return true;
    }

    void AddPass(nvrhi::CommandListHandle commandList, const char* shaderName, const BloomConsts& bloomConsts, nvrhi::TextureHandle srcTexture,
                 uint32_t srcMip, uint32_t destMip, Vector2U destRes)
    {
        using Item = nvrhi::BindingSetItem;
        Graphic::ComputePassParams p;
        p.m_CommandList = commandList;
        p.m_ShaderName = shaderName;
        p.m_BindingSetDesc.bindings = {
            Item::PushConstants(0, sizeof(bloomConsts)),
            Item::Texture_SRV(0, srcTexture, nvrhi::Format::UNKNOWN, nvrhi::TextureSubresourceSet{ srcMip, 1, 0, 1 }),
            Item::Sampler(0, g_CommonResources.LinearClampSampler),
            Item::Texture_UAV(0, m_BloomTexture, nvrhi::Format::UNKNOWN, nvrhi::TextureSubresourceSet{ destMip, 1, 0, 1 }),   // the colour attachment
        };
        p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(destRes, 8);   // the viewport
        p.m_PushConstantsData = &bloomConsts;
        p.m_PushConstantsBytes = sizeof(bloomConsts);
        g_Graphic.AddComputePass(p);
        m_LastConsts.push_back(bloomConsts);
    }

    void Render(nvrhi::CommandListHandle commandList, const RenderGraph&) override
    {
        const uint32_t nbPasses = g_Scene->m_NbBloomMips - 1;
        nvrhi::TextureHandle lightingOutput = GetLightingOutput();
        const nvrhi::TextureDesc& textureDesc = lightingOutput->getDesc();
        m_LastConsts.clear();

        for (uint32_t i = 0; i < nbPasses; ++i) {                             // downsample, :69-105
            const bool bIsFirstPass = (i == 0);
            const uint32_t srcMip = i, destMip = srcMip + 1;
            const Vector2U srcRes{ textureDesc.width >> srcMip, textureDesc.height >> srcMip };
            const Vector2U destRes{ textureDesc.width >> destMip, textureDesc.height >> destMip };
            BloomConsts bloomConsts{};
            bloomConsts.m_bIsFirstDownsample = bIsFirstPass;
            bloomConsts.m_InvSourceResolution = Vector2{ 1.0f / srcRes.x, 1.0f / srcRes.y };
            AddPass(commandList, "bloom_PS_Downsample", bloomConsts, bIsFirstPass ? lightingOutput : m_BloomTexture, srcMip, destMip, destRes);
        }
        for (uint32_t i = 0; i < nbPasses; ++i) {                             // upsample, :108-140
            const uint32_t srcMip = nbPasses - i, destMip = srcMip - 1;
            const Vector2U destRes{ textureDesc.width >> destMip, textureDesc.height >> destMip };
            BloomConsts bloomConsts{};
            bloomConsts.m_FilterRadius = g_Scene->m_BloomFilterRadius;
            AddPass(commandList, "bloom_PS_Upsample", bloomConsts, m_BloomTexture, srcMip, destMip, destRes);
        }
    }
};
DEFINE_RENDERER(BloomRenderer);

nvrhi::TextureHandle GetGeneratedBloomTexture() { return static_cast<BloomRenderer*>(g_BloomRenderer)->m_BloomTexture; }

bool GetLastBloomConsts(uint32_t pass, void* out16)
{
    const BloomRenderer* r = static_cast<const BloomRenderer*>(g_BloomRenderer);
    if (!g_Scene->m_bEnableBloom || pass >= r->m_LastConsts.size()) return false;   // off: the last frame ran no bloom pass
    memcpy(out16, &r->m_LastConsts[pass], sizeof(BloomConsts));
    return true;
}

void ReleaseBloomOutputs()
{
    BloomRenderer* r = static_cast<BloomRenderer*>(g_BloomRenderer);
    r->m_BloomTexture = nullptr;
    r->m_LastConsts.clear();
}
