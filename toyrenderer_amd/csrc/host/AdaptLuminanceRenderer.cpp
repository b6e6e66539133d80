// AdaptLuminanceRenderer.cpp -- the reference's auto exposure (source/AdaptLuminanceRenderer.cpp): a 256-bin histogram of the
// log luminance of LightingOutput, "adaptluminance_CS_GenerateLuminanceHistogram", and its weighted average eased into the
// one-float luminance buffer and the 1 x 1 exposure texture, "adaptluminance_CS_AdaptExposure" (csrc/k_postprocess.hip).
//
// Differences from the reference, all on the host side: the luminance limits, the speed and the frame time live in Scene where
// the facade sets them (the reference's are members behind ImGui and Engine's clock); the histogram buffer is kept across frames
// so that it can be read back (a transient there); the luminance buffer and the exposure texture are created by the first Setup
// (the reference's Initialize); and the reference's two-frame-late CPU read-backs of luminance and exposure for its ImGui text
// (:123-147) are NOT modelled: trhost_get_scene_luminance waits for the device and reads the current values.  With a manual
// exposure the reference's Setup returns false, so that its write of the override into the luminance buffer (:149-153) never
// runs; here the pass is scheduled and does that write, as FrameDriver does, so that the buffer always holds what the post pass
// used.  log2 of the limits: in double precision, rounded once (interop.log_luminance_range does the same two operations).
#include "Graphic.h"
#include "RenderGraph.h"
#include "Scene.h"
#include "VisibilityOutputs.h"
#include "../ShaderInterop.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace interop;

class AdaptLuminanceRenderer : public IRenderer
{
public:
    AdaptLuminanceRenderer() : IRenderer("AdaptLuminanceRenderer") {}

    nvrhi::BufferHandle m_LuminanceHistogram;        // 256 x uint32
    GenerateLuminanceHistogramParameters m_LastHistogramParams{};
    AdaptExposureParameters m_LastAdaptParams{};
    bool m_bAdaptRan = false;

    bool Setup(RenderGraph& renderGraph) override
    {
        if (!g_Scene->m_bPostProcess || g_Scene->m_NumPrimitives == 0) return false;
        nvrhi::DeviceHandle device = g_Graphic.m_NVRHIDevice;
        if (!g_Scene->m_LuminanceBuffer) {                                    // :54-76
            nvrhi::BufferDesc desc;
            desc.byteSize = sizeof(float);
            desc.structStride = sizeof(float);
            desc.debugName = "Exposure Buffer";
            desc.canHaveUAVs = true;
            g_Scene->m_LuminanceBuffer = device->createBuffer(desc);
            nvrhi::TextureDesc textureDesc;
            textureDesc.format = nvrhi::Format::R32_FLOAT;
            textureDesc.isUAV = true;
            textureDesc.debugName = "Exposure Texture";
            g_Scene->m_ExposureTexture = device->createTexture(textureDesc);
            ResetExposure();
        }
        if (!m_LuminanceHistogram) {                                          // :106-112
            nvrhi::BufferDesc desc;
            desc.byteSize = sizeof(uint32_t) * 256;
            desc.structStride = sizeof(uint32_t);
            desc.debugName = "Luminance Histogram";
            desc.canHaveUAVs = true;
            m_LuminanceHistogram = device->createBuffer(desc);
        }
        renderGraph.AddExternalReadDependency(GetLightingOutput().Get());     // :114
        renderGraph.AddExternalWriteDependency(g_Scene->m_LuminanceBuffer.Get());
        renderGraph.AddExternalWriteDependency(g_Scene->m_ExposureTexture.Get());
        return true;
    }

    void Render(nvrhi::CommandListHandle commandList, const RenderGraph&) override
    {
        m_bAdaptRan = false;
        if (g_Scene->m_ManualExposureOverride > 0.0f) {                       // :149-153
            commandList->writeBuffer(g_Scene->m_LuminanceBuffer, &g_Scene->m_ManualExposureOverride, sizeof(float));
            return;
        }
        const float minLogLum = (float)std::log2((double)g_Scene->m_MinimumLuminance);   // :155-156
        const float maxLogLum = (float)std::log2((double)g_Scene->m_MaximumLuminance);
        using Item = nvrhi::BindingSetItem;
        {                                                                     // :161-186
            commandList->clearBufferUInt(m_LuminanceHistogram, 0);
            GenerateLuminanceHistogramParameters passParameters{};
            passParameters.m_SrcColorDims = g_Graphic.m_RenderResolution;
            passParameters.m_MinLogLuminance = minLogLum;
            passParameters.m_InverseLogLuminanceRange = 1.0f / (maxLogLum - minLogLum);
            m_LastHistogramParams = passParameters;
            Graphic::ComputePassParams p;
            p.m_CommandList = commandList;
            p.m_ShaderName = "adaptluminance_CS_GenerateLuminanceHistogram";
            p.m_BindingSetDesc.bindings = { Item::PushConstants(0, sizeof(passParameters)), Item::Texture_SRV(0, GetLightingOutput()),
                                            Item::StructuredBuffer_UAV(0, m_LuminanceHistogram) };
            p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(passParameters.m_SrcColorDims, 16);
            p.m_PushConstantsData = &passParameters;
            p.m_PushConstantsBytes = sizeof(passParameters);
            g_Graphic.AddComputePass(p);
        }
        {                                                                     // :188-214
            AdaptExposureParameters passParameters{};
            passParameters.m_AdaptationSpeed = std::clamp(g_Scene->m_AutoExposureSpeed * g_Scene->m_CPUCappedFrameTimeMs, 0.0f, 1.0f);
            passParameters.m_MinLogLuminance = minLogLum;
            passParameters.m_LogLuminanceRange = maxLogLum - minLogLum;
            passParameters.m_NbPixels = g_Graphic.m_RenderResolution.x * g_Graphic.m_RenderResolution.y;
            passParameters.m_MiddleGray = g_Scene->m_MiddleGray;
            m_LastAdaptParams = passParameters;
            Graphic::ComputePassParams p;
            p.m_CommandList = commandList;
            p.m_ShaderName = "adaptluminance_CS_AdaptExposure";
            p.m_BindingSetDesc.bindings = { Item::PushConstants(0, sizeof(passParameters)), Item::StructuredBuffer_SRV(0, m_LuminanceHistogram),
                                            Item::StructuredBuffer_UAV(0, g_Scene->m_LuminanceBuffer), Item::Texture_UAV(1, g_Scene->m_ExposureTexture) };
            p.m_DispatchGroupSize = Vector3U{ 1, 1, 1 };
            p.m_PushConstantsData = &passParameters;
            p.m_PushConstantsBytes = sizeof(passParameters);
            g_Graphic.AddComputePass(p);
        }
        m_bAdaptRan = true;
    }
};
DEFINE_RENDERER(AdaptLuminanceRenderer);

void ResetExposure()
{
    if (!g_Scene->m_LuminanceBuffer) return;                                  // created with 1.0 by the first frame
    g_Graphic.m_NVRHIDevice->waitForIdle();
    const float kInitialExposure = 1.0f;                                      // :65
    nvrhi::throwIfFailed(trhip_buffer_upload(g_Scene->m_LuminanceBuffer->native(), 0, &kInitialExposure, sizeof(float)), "ResetExposure");
    nvrhi::throwIfFailed(trhip_texture_upload(g_Scene->m_ExposureTexture->native(), 0, &kInitialExposure, sizeof(float)), "ResetExposure");
}

void GetLastAdaptLuminanceParams(void* histogram16, void* adapt20, int* adaptRan)
{
    const AdaptLuminanceRenderer* r = static_cast<const AdaptLuminanceRenderer*>(g_AdaptLuminanceRenderer);
    if (histogram16) memcpy(histogram16, &r->m_LastHistogramParams, sizeof r->m_LastHistogramParams);
    if (adapt20) memcpy(adapt20, &r->m_LastAdaptParams, sizeof r->m_LastAdaptParams);
    if (adaptRan) *adaptRan = r->m_bAdaptRan ? 1 : 0;
}

void ReleaseAdaptLuminanceOutputs()
{
    AdaptLuminanceRenderer* r = static_cast<AdaptLuminanceRenderer*>(g_AdaptLuminanceRenderer);
    r->m_LuminanceHistogram = nullptr;
    r->m_bAdaptRan = false;
}
