// SkyRenderer.cpp -- the reference's sky pass (source/SkyRenderer.cpp), scheduled between DeferredLightingRenderer and
// BloomRenderer (Scene.cpp:502): HosekWilkieHelper::CalculateSkyParameters on the host, then one full-screen pass,
// "sky_PS_HosekWilkieSky" (csrc/k_sky.hip), that fills every texel of LightingOutput the base pass did not draw.
//
// As with the other image passes here, the full-screen triangle at kFarDepth with its GreaterOrEqual depth test is a direct
// dispatch of 8x8 groups; the read-only depth attachment is bound at t0 and the colour attachment as a UAV at u0, and the kernel
// writes where depth <= 0.  The reference declares LightingOutput as a read dependency (it is an attachment there); the pass
// stores into it, so this build's cross-queue hazard tracking is told of the write.
//
// THE DATASET IS AN INPUT (trhost_load_sky_dataset): the model's RGB tables are not part of this library.
//
// THE 30 FLOATS are, bit for bit, those of toyrenderer_amd/sky.py and tests/sky_ref.c: the operations and types are the
// reference's, with its roundings to float (sun_theta, std::max<float>, 1.f / 3.0f, turbidityK, the (float) of each Evaluate).
// acos and cos are the C library's double functions rounded once to float, and pow is called through a pointer so that the
// compiler folds none of its calls (pow(x, 1), pow(x, 2)): every side then runs the same library function on the same doubles.
// ROW 9: DirectXMath is not in the tree and its polynomial XMVectorExp (an alias of XMVectorExp2: base two) and XMVectorPow cannot
// be restated, so the normalisation helper is evaluated in double from the 30 rounded floats (2^x as pow(2, x), pow(b, 1.5), the
// luminance dot left to right) and row 9 is rounded once; it agrees with a run of the reference only to the accuracy of
// DirectXMath's approximations.  The helper's quirks are kept: it is not the shader's function.
#include "CommonResources.h"
#include "Graphic.h"
#include "GraphicConstants.h"
#include "RenderGraph.h"
#include "Scene.h"
#include "VisibilityOutputs.h"
#include "../ShaderInterop.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>

using namespace interop;

extern RenderGraph::ResourceHandle g_DepthStencilBufferRDGTextureHandle;

namespace HosekWilkieHelper
{
    using SkyParameters = std::array<std::array<float, 3>, 10>;                // rows A B C D E F G H I Z

    static double Pow(double a, double b) { double (*volatile f)(double, double) = pow; return f(a, b); }

    static double EvaluateSpline(double const* spline, size_t stride, double value)   // :41-50
    {
        return
            1  * Pow(1.0 - value, 5)                 * spline[0 * stride] +
            5  * Pow(1.0 - value, 4) * Pow(value, 1) * spline[1 * stride] +
            10 * Pow(1.0 - value, 3) * Pow(value, 2) * spline[2 * stride] +
            10 * Pow(1.0 - value, 2) * Pow(value, 3) * spline[3 * stride] +
            5  * Pow(1.0 - value, 1) * Pow(value, 4) * spline[4 * stride] +
            1                        * Pow(value, 5) * spline[5 * stride];
    }

    static double Evaluate(double const* dataset, size_t stride, float turbidity, float albedo, float sun_theta)   // :52-71
    {
        // splines are functions of elevation^1/3
        double elevationK = Pow(std::max<float>(0.f, (float)(1.f - sun_theta / (3.14159265358979323846 * 0.5f))), 1.f / 3.0f);

        // table has values for turbidity 1..10
        int turbidity0 = std::clamp(static_cast<int>(turbidity), 1, 10);
        int turbidity1 = std::min(turbidity0 + 1, 10);
        float turbidityK = std::clamp(turbidity - turbidity0, 0.f, 1.f);

        double const* datasetA0 = dataset;
        double const* datasetA1 = dataset + stride * 6 * 10;

        double a0t0 = EvaluateSpline(datasetA0 + stride * 6 * (turbidity0 - 1), stride, elevationK);
        double a1t0 = EvaluateSpline(datasetA1 + stride * 6 * (turbidity0 - 1), stride, elevationK);
        double a0t1 = EvaluateSpline(datasetA0 + stride * 6 * (turbidity1 - 1), stride, elevationK);
        double a1t1 = EvaluateSpline(datasetA1 + stride * 6 * (turbidity1 - 1), stride, elevationK);

        return a0t0 * (1.0f - albedo) * (1.0f - turbidityK) + a1t0 * albedo * (1.0f - turbidityK) + a0t1 * (1.0f - albedo) * turbidityK + a1t1 * albedo * turbidityK;
    }

    // :73-95 of one channel, in double from the rounded rows
    static double HosekWilkie(float cos_theta, float gamma, float cos_gamma, const SkyParameters& p, int c)
    {
        const double A = p[0][c], B = p[1][c], C = p[2][c], D = p[3][c], E = p[4][c], F = p[5][c], G = p[6][c], H = p[7][c], I = p[8][c];
        const double chi = (double)(1.f + cos_gamma * cos_gamma) / Pow(H * H + 1.0 - H * (double)(2.0f * cos_gamma), 1.5);
        const double temp1 = A * Pow(2.0, B * (double)(1.0f / (cos_theta + 0.01f)));
        const double temp2 = C + D * Pow(2.0, E * (double)gamma) + F * (double)(gamma * gamma) + chi * G + I * (double)(float)sqrt((double)std::max(0.f, cos_theta));
        return temp1 * temp2;
    }

    // rgb: 3 x 1080, rad: 3 x 120
    static SkyParameters CalculateSkyParameters(const double* rgb, const double* rad, float turbidity, const float albedo[3], const float sun_direction[3])   // :97-129
    {
        float sun_theta = (float)acos((double)std::clamp(sun_direction[1], 0.f, 1.f));

        SkyParameters params{};
        for (uint32_t i = 0; i < 3; ++i)
        {
            const double* dataset = rgb + 1080 * i;
            for (uint32_t r = 0; r < 7; ++r)
                params[r][i] = (float)Evaluate(dataset + r, 9, turbidity, albedo[i], sun_theta);

            // data values are swapped
            params[7][i] = (float)Evaluate(dataset + 8, 9, turbidity, albedo[i], sun_theta);
            params[8][i] = (float)Evaluate(dataset + 7, 9, turbidity, albedo[i], sun_theta);

            // Z value thing
            params[9][i] = (float)Evaluate(rad + 120 * i, 1, turbidity, albedo[i], sun_theta);
        }

        const float cos_theta = (float)cos((double)sun_theta);
        double S[3];
        for (int i = 0; i < 3; ++i) S[i] = HosekWilkie(cos_theta, 0.0f, 1.0f, params, i) * (double)params[9][i];
        const double lum = S[0] * (double)0.2126f + S[1] * (double)0.7152f + S[2] * (double)0.0722f;
        for (int i = 0; i < 3; ++i) params[9][i] = (float)((double)params[9][i] / lum);

        return params;
    }
}

class SkyRenderer : public IRenderer
{
public:
    SkyRenderer() : IRenderer("SkyRenderer") {}

    SkyPassParameters m_LastConsts{};                // what the last Render uploaded (trhost_get_sky_consts)
    bool m_bRanLastFrame = false;

    bool Setup(RenderGraph& renderGraph) override
    {
        m_bRanLastFrame = false;
        if (!g_Scene->m_bEnableSky || !g_Scene->m_bDeferredLighting || g_Scene->m_SkyDataset.empty() || g_Scene->m_NumPrimitives == 0) return false;   // :152-155
        if (!GetLightingOutput()) return false;                               // DeferredLightingRenderer::Setup creates it, and is scheduled first
        renderGraph.AddExternalWriteDependency(GetLightingOutput().Get());    // :157-158
        renderGraph.AddReadDependency(g_DepthStencilBufferRDGTextureHandle);
        return true;
    }

    void Render(nvrhi::CommandListHandle commandList, const RenderGraph& renderGraph) override
    {
        const double* data = g_Scene->m_SkyDataset.data();
        SkyPassParameters skyPassParameters{};                                // :178-187
        skyPassParameters.m_ClipToWorld = g_Scene->m_View.m_ClipToWorld;
        memcpy(skyPassParameters.m_SunLightDir, g_Scene->m_DirLightVec, sizeof g_Scene->m_DirLightVec);
        memcpy(skyPassParameters.m_CameraPosition, g_Scene->m_View.m_Eye, sizeof g_Scene->m_View.m_Eye);
        const HosekWilkieHelper::SkyParameters skyParams =
            HosekWilkieHelper::CalculateSkyParameters(data, data + 3 * 1080, g_Scene->m_SkyTurbidity, g_Scene->m_GroundAlbedo, g_Scene->m_DirLightVec);
        for (uint32_t i = 0; i < skyParams.size(); ++i)
            skyPassParameters.m_HosekParams.m_Params[i] = Vector4{ skyParams[i][0], skyParams[i][1], skyParams[i][2], 0.0f };
        m_LastConsts = skyPassParameters;
        m_bRanLastFrame = true;

        using Item = nvrhi::BindingSetItem;
        Graphic::ComputePassParams p;                                         // :189-207
        p.m_CommandList = commandList;
        p.m_ShaderName = "sky_PS_HosekWilkieSky";
        p.m_BindingSetDesc.bindings = {
            Item::ConstantBuffer(0, g_Graphic.CreateConstantBuffer(commandList, skyPassParameters)),
            Item::Texture_SRV(0, renderGraph.GetTexture(g_DepthStencilBufferRDGTextureHandle)),   // the read-only depth attachment
            Item::Texture_UAV(0, GetLightingOutput()),                                            // the colour attachment
        };
        p.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(g_Graphic.m_RenderResolution, 8);
        g_Graphic.AddComputePass(p);
    }
};
DEFINE_RENDERER(SkyRenderer);

bool GetLastSkyConsts(void* out256)
{
    const SkyRenderer* r = static_cast<const SkyRenderer*>(g_SkyRenderer);
    if (!g_Scene->m_bEnableSky || !g_Scene->m_bDeferredLighting || !r->m_bRanLastFrame) return false;   // off: the renderer is not scheduled, the last frame ran no sky pass
    memcpy(out256, &r->m_LastConsts, sizeof r->m_LastConsts);
    return true;
}

void ReleaseSkyOutputs() { static_cast<SkyRenderer*>(g_SkyRenderer)->m_bRanLastFrame = false; }
