// GIRenderer.cpp -- the reference's GI debug renderer, GIDebugRenderer (source/GIRenderer.cpp:598-808; Setup :612-657,
// RenderDDGIDebug :672-808): the probe culling dispatch, the second consumer of FrustumCull / OcclusionCull and of compaction into
// indirect draw arguments, and the draw of the unit spheres that consumes those arguments (:737-806).
//
// Two paths.  With trhost_set_ddgi_probe_visualization the renderer works on Scene::m_RTDDGIVolume as it is on the device this
// frame: "giprobevisualization_CS_LoadGIProbes" (the project's own: the reference reads the volume inline through SDK functions)
// writes every probe's position and state into two transient buffers, the cull takes them at t10 / t11, and
// "giprobevisualization_PS_VisualizeGIProbes" (csrc/k_giprobedraw.hip) draws the survivors into PostProcessRenderer's back buffer
// and the frame's depth buffer; m_IndexCount is the unit sphere's 468.  With Scene::LoadGIProbes alone the positions and states are
// two supplied buffers, the cull is the one dispatch, its arguments carry 2880 and nothing is drawn.
//
// And GIRenderer (source/GIRenderer.cpp: RenderDDGI): the probe update of Scene::m_RTDDGIVolume, "giprobetrace_CS_ProbeTrace" and
// the two "ProbeBlendingCS_DDGIProbeBlendingCS" passes (csrc/k_giprobetrace.hip, csrc/k_giprobeblend.hip), behind the TLAS refit and
// in front of DeferredLightingRenderer.  The RTXGI SDK is not part of this project: the passes are the project's own, with one
// constant block (DDGIUpdateConsts, the descriptor's host copy behind it).  With trhost_set_ddgi_probe_placement the reference's
// relocation and classification (:513-527) follow the blends: "giprobetrace_CS_ProbeTraceFixedRays", the project's own trace of 32
// unrotated rays from every probe, then "ProbeRelocationCS_DDGIProbeRelocationCS" and "ProbeClassificationCS_DDGIProbeClassificationCS"
// (csrc/k_giprobeplacement.hip).  With trhost_set_ddgi_probe_variability the reference's probe variability (:158-190, :466-470, :529-576): the
// radiance blend also writes a coefficient of variation per interior texel (u4), "ReductionCS_DDGIReductionCS REDUCTION=1" and
// "ReductionCS_DDGIExtraReductionCS" (csrc/k_ddgireduction.hip) average it over the active probes, element 0 goes into one of two
// read-back slots, the slot written two updates earlier feeds the ring of DDGIVariability.h, and an update that finds the ring
// converged records nothing.  The frame's ray rotation is a uniformly distributed rotation (Shoemake's three-uniform form) from a splitmix64 stream
// keyed by (seed, update count), evaluated in double and rounded once; trhost_get_ddgi_update_consts shows the block that ran.
#include "CommonResources.h"
#include "Graphic.h"
#include "MathUtilities.h"
#include "RenderGraph.h"
#include "Scene.h"
#include "VisibilityOutputs.h"
#include "../ShaderInterop.h"

#include <cmath>
#include <cstring>

using namespace interop;

extern RenderGraph::ResourceHandle g_DepthStencilBufferRDGTextureHandle;

class GIDebugRenderer : public IRenderer
{
    // the pass's three transient outputs (GIRenderer.cpp:618-650), described once
    struct Output
    {
        const char* debugName;
        uint32_t stride;
        bool perProbe;                 // one element per probe, else a single element
        bool indirectArgs;
        RenderGraph::ResourceHandle handle;
        nvrhi::BufferHandle last;      // what the last frame wrote (trhost_gi_probe_buffers)
    };
    enum { kPositions, kDrawArgs, kInstanceToProbe, kNumOutputs };
    Output m_Outputs[kNumOutputs] = {
        { "Probe Positions", sizeof(float) * 3, true, false, {}, nullptr },
        { "Probe Draw Indirect Args", sizeof(DrawIndexedIndirectArguments), false, true, {}, nullptr },
        { "Instance ID to Probe Index", sizeof(uint32_t), true, false, {}, nullptr },
    };

    // the live path's two inputs of the cull, written by LoadGIProbes
    RenderGraph::ResourceHandle m_LivePositions, m_LiveStates;
    bool m_bLive = false;

    static uint32_t LiveProbeCount(const Scene& scene)
    {
        const DDGIVolumeDesc& d = scene.m_RTDDGIVolume.m_Desc;
        return (uint32_t)d.probeCounts[0] * (uint32_t)d.probeCounts[1] * (uint32_t)d.probeCounts[2];
    }

    static GIProbeVisualizationUpdateConsts ConstantsOf(const Scene& scene, bool live)     // :687-708
    {
        const View& view = scene.m_View;
        GIProbeVisualizationUpdateConsts k{};
        k.m_NumProbes = live ? LiveProbeCount(scene) : scene.m_NumGIProbes;
        // :701 m_CameraOrigin = m_View.m_Eye.  This mirror takes the camera as a world-to-view matrix (Scene.h, View::SetCamera):
        // the eye is the point that maps to the view-space origin, -t * R^T for the rigid transform [R | t] a camera is.
        // (The culling shader does not read the field; it is filled so that the uploaded block equals the reference's.)
        for (int j = 0; j < 3; ++j)
            k.m_CameraOrigin[j] = -(view.m_WorldToView.m[3][0] * view.m_WorldToView.m[j][0] + view.m_WorldToView.m[3][1] * view.m_WorldToView.m[j][1] +
                                    view.m_WorldToView.m[3][2] * view.m_WorldToView.m[j][2]);
        k.m_Frustum = CullingFrustumOf(view.m_ViewToClip);
        k.m_WorldToView = view.m_WorldToView;
        k.m_HZBDimensions = Vector2U{ scene.m_HZB->getDesc().width, scene.m_HZB->getDesc().height };
        k.m_P00 = view.m_ViewToClip.m[0][0];
        k.m_P11 = view.m_ViewToClip.m[1][1];
        k.m_NearPlane = view.m_ZNearP;
        k.m_ProbeRadius = live ? scene.m_DDGIProbeVisualizationRadius : scene.m_GIProbeRadius;
        k.m_bHideInactiveProbes = live ? scene.m_bDDGIProbeVisualizationHideInactive : scene.m_bHideInactiveGIProbes;
        return k;
    }

public:
    GIDebugRenderer() : IRenderer("GIDebugRenderer") {}

    GIProbeVisualizationConsts m_LastDrawConsts{};
    bool m_bDrewLastFrame = false;

    nvrhi::BufferHandle LastOutput(int which) const { return m_Outputs[which].last; }
    void DropLastOutputs() { for (Output& o : m_Outputs) o.last = nullptr; }

    bool Setup(RenderGraph& renderGraph) override
    {
        m_bDrewLastFrame = false;
        // trhost_frame has refused a frame with the switch on and no volume or no post-processing (CheckDDGIProbeVisualization)
        m_bLive = g_Scene->m_bDDGIProbeVisualization && g_Scene->m_RTDDGIVolume.IsValid() && g_Scene->m_bPostProcess && g_Scene->m_NumPrimitives != 0;
        const uint32_t numProbes = m_bLive ? LiveProbeCount(*g_Scene) : g_Scene->m_NumGIProbes;
        if (numProbes == 0 || !(m_bLive || g_Scene->m_bShowGIProbes)) return false;   // :661-670: only with DDGI and the debug view on
        renderGraph.AddExternalReadDependency(g_Scene->m_HZB.Get());            // where the reference declares the volume descriptors (:652)
        if (m_bLive) {
            const Scene::RTDDGIVolume& volume = g_Scene->m_RTDDGIVolume;
            renderGraph.AddExternalReadDependency(volume.m_ProbeData.Get());    // GIRenderer, scheduled in front, may have rewritten all three
            renderGraph.AddExternalReadDependency(volume.m_ProbeIrradiance.Get());
            renderGraph.AddExternalReadDependency(volume.m_ProbeDistance.Get());
            renderGraph.AddExternalWriteDependency(GetBackBuffer().Get());      // PostProcessRenderer::Setup, scheduled in front, has created it
            renderGraph.AddWriteDependency(g_DepthStencilBufferRDGTextureHandle);
            nvrhi::BufferDesc desc;
            desc.canHaveUAVs = true;
            desc.initialState = nvrhi::ResourceStates::ShaderResource;
            desc.debugName = "GI Probe World Positions"; desc.structStride = sizeof(float) * 3; desc.byteSize = (uint64_t)desc.structStride * numProbes;
            renderGraph.CreateTransientResource(m_LivePositions, desc);
            desc.debugName = "GI Probe States"; desc.structStride = sizeof(float); desc.byteSize = (uint64_t)desc.structStride * numProbes;
            renderGraph.CreateTransientResource(m_LiveStates, desc);
        }
        for (Output& o : m_Outputs) {
            nvrhi::BufferDesc desc;
            desc.debugName = o.debugName;
            desc.structStride = o.stride;
            desc.byteSize = (uint64_t)o.stride * (o.perProbe ? numProbes : 1u);
            desc.canHaveUAVs = true;
            desc.isDrawIndirectArgs = o.indirectArgs;
            desc.initialState = o.indirectArgs ? nvrhi::ResourceStates::IndirectArgument : nvrhi::ResourceStates::ShaderResource;
            renderGraph.CreateTransientResource(o.handle, desc);
        }
        return true;
    }

    void Render(nvrhi::CommandListHandle commandList, const RenderGraph& renderGraph) override
    {
        nvrhi::BufferHandle out[kNumOutputs];
        for (int i = 0; i < kNumOutputs; ++i) out[i] = renderGraph.GetBuffer(m_Outputs[i].handle);      // :678-681

        using Item = nvrhi::BindingSetItem;
        const Scene::RTDDGIVolume& volume = g_Scene->m_RTDDGIVolume;
        nvrhi::BufferHandle positions = g_Scene->m_GIProbePositionsBuffer, states = g_Scene->m_GIProbeStatesBuffer;
        if (m_bLive) {                                                          // where the reference calls DDGILoadProbeState / DDGIGetProbeWorldPosition (:29-37)
            positions = renderGraph.GetBuffer(m_LivePositions);
            states = renderGraph.GetBuffer(m_LiveStates);
            Graphic::ComputePassParams load;
            load.m_CommandList = commandList;
            load.m_ShaderName = "giprobevisualization_CS_LoadGIProbes";
            load.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(LiveProbeCount(*g_Scene), kNumThreadsPerWave);
            load.m_BindingSetDesc.bindings = {
                Item::ConstantBuffer(0, g_Graphic.CreateConstantBuffer(commandList, volume.m_Desc)),
                Item::StructuredBuffer_SRV(0, volume.m_DescBuffer),
                Item::Texture_SRV(1, volume.m_ProbeData),
                Item::StructuredBuffer_UAV(0, positions),
                Item::StructuredBuffer_UAV(1, states),
            };
            g_Graphic.AddComputePass(load);
        }

        // the draw the culling feeds: unit-sphere indices, instance count 0 until the shader has counted (:683-685)
        DrawIndexedIndirectArguments sphereDraw{};
        sphereDraw.m_IndexCount = m_bLive ? g_CommonResources.UnitSphere.m_NumIndices : g_Scene->m_GIProbeSphereIndexCount;
        commandList->writeBuffer(out[kDrawArgs], &sphereDraw, sizeof sphereDraw);

        const GIProbeVisualizationUpdateConsts consts = ConstantsOf(*g_Scene, m_bLive);
        Graphic::ComputePassParams pass;                                        // :710-733
        pass.m_CommandList = commandList;
        pass.m_ShaderName = "giprobevisualization_CS_VisualizeGIProbesCulling";
        pass.m_DispatchGroupSize = ComputeShaderUtils::GetGroupCount(consts.m_NumProbes, kNumThreadsPerWave);
        pass.m_BindingSetDesc.bindings = {
            Item::ConstantBuffer(0, g_Graphic.CreateConstantBuffer(commandList, consts)),
            Item::Texture_SRV(0, g_Scene->m_HZB),
            Item::Sampler(0, g_CommonResources.LinearClampMinReductionSampler),
            // t10 / t11: probe positions and states, where the reference binds the DDGI volume descriptors (t10) and
            // the probe-data texture array (u10)
            Item::StructuredBuffer_SRV(10, positions),
            Item::StructuredBuffer_SRV(11, states),
            Item::StructuredBuffer_UAV(0, out[kPositions]),
            Item::StructuredBuffer_UAV(1, out[kDrawArgs]),
            Item::StructuredBuffer_UAV(2, out[kInstanceToProbe]),
        };
        g_Graphic.AddComputePass(pass);

        for (int i = 0; i < kNumOutputs; ++i) m_Outputs[i].last = out[i];
        if (!m_bLive) return;

        struct Block { GIProbeVisualizationConsts k; DDGIVolumeDesc desc; } block{};    // :745-752
        static_assert(sizeof(Block) == 160, "GIProbeVisualizationConsts + DDGIVolumeDesc");
        const View& view = g_Scene->m_View;
        block.k.m_WorldToClip = MultiplyNoFMA(view.m_WorldToView, view.m_ViewToClip);
        for (int j = 0; j < 3; ++j) block.k.m_CameraDirection[j] = -view.m_WorldToView.m[j][2];     // the view looks down -Z; the draw does not read it
        block.k.m_ProbeRadius = g_Scene->m_DDGIProbeVisualizationRadius;
        block.k.m_NearPlane = view.m_ZNearP;
        block.desc = volume.m_Desc;
        m_LastDrawConsts = block.k;
        m_bDrewLastFrame = true;
        Graphic::ComputePassParams draw;                                        // :754-806
        draw.m_CommandList = commandList;
        draw.m_ShaderName = "giprobevisualization_PS_VisualizeGIProbes";
        draw.m_DispatchGroupSize = Vector3U{ 1, 1, 1 };                        // the launches size themselves
        draw.m_BindingSetDesc.bindings = {
            Item::ConstantBuffer(0, g_Graphic.CreateConstantBuffer(commandList, block)),
            Item::StructuredBuffer_SRV(0, out[kPositions]),
            Item::Texture_SRV(1, volume.m_ProbeData),
            Item::Texture_SRV(2, volume.m_ProbeIrradiance),
            Item::Texture_SRV(3, volume.m_ProbeDistance),
            Item::StructuredBuffer_SRV(4, volume.m_DescBuffer),
            Item::StructuredBuffer_SRV(5, out[kInstanceToProbe]),
            Item::StructuredBuffer_SRV(6, out[kDrawArgs]),                      // the project's own slots from here (include/trhip.h)
            Item::StructuredBuffer_SRV(7, g_CommonResources.UnitSphere.m_VertexBuffer),
            Item::StructuredBuffer_SRV(8, g_CommonResources.UnitSphere.m_IndexBuffer),
            Item::Texture_UAV(0, renderGraph.GetTexture(g_DepthStencilBufferRDGTextureHandle)),
            Item::Texture_UAV(1, GetBackBuffer()),
            Item::Sampler(0, g_CommonResources.LinearClampSampler),             // the reference's g_LinearWrapSampler: accepted and ignored
        };
        g_Graphic.AddComputePass(draw);
    }

    enum { Positions = kPositions, DrawArgs = kDrawArgs, InstanceToProbe = kInstanceToProbe };
};
DEFINE_RENDERER(GIDebugRenderer);

class GIRenderer : public IRenderer
{
    static double Uniform(uint64_t& state)                                     // splitmix64, 53 bits
    {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return (double)((z ^ (z >> 31)) >> 11) * (1.0 / 9007199254740992.0);
    }

    static void RandomRotation(uint32_t seed, uint32_t count, float rows[3][4])
    {
        uint64_t state = (uint64_t)seed << 32 | count;
        const double kTwoPi = 6.28318530717958647692;
        const double u1 = Uniform(state), u2 = Uniform(state), u3 = Uniform(state);
        const double a = std::sqrt(1.0 - u1), b = std::sqrt(u1);
        const double x = a * std::sin(kTwoPi * u2), y = a * std::cos(kTwoPi * u2), z = b * std::sin(kTwoPi * u3), w = b * std::cos(kTwoPi * u3);
        const double m[3][3] = { { 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w) },
                                 { 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w) },
                                 { 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y) } };
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) rows[i][j] = (float)m[i][j];
            rows[i][3] = 0.0f;
        }
    }

public:
    GIRenderer() : IRenderer("GIRenderer") {}

    DDGIUpdateConsts m_LastConsts{};
    bool m_bRanLastFrame = false;

    bool Setup(RenderGraph& renderGraph) override
    {
        m_bRanLastFrame = false;
        const Scene::RTDDGIVolume& volume = g_Scene->m_RTDDGIVolume;
        if (!g_Scene->m_bDDGIUpdate || !g_Scene->m_bDeferredLighting || !volume.IsValid() || !volume.m_RayData || !g_Scene->m_TLAS || g_Scene->m_NumPrimitives == 0) return false;
        renderGraph.AddExternalReadDependency(g_Scene->m_InstanceConstsBuffer.Get());
        renderGraph.AddExternalWriteDependency(volume.m_ProbeIrradiance.Get());
        renderGraph.AddExternalWriteDependency(volume.m_ProbeDistance.Get());
        if (g_Scene->m_bDDGIProbeRelocation || g_Scene->m_bDDGIProbeClassification) renderGraph.AddExternalWriteDependency(volume.m_ProbeData.Get());
        return true;
    }

    void Render(nvrhi::CommandListHandle commandList, const RenderGraph&) override
    {
        using Item = nvrhi::BindingSetItem;
        Scene::RTDDGIVolume& volume = g_Scene->m_RTDDGIVolume;
        const nvrhi::rt::AccelStruct& as = *g_Scene->m_TLAS;
        DDGIVariability& tracker = volume.m_Variability;
        const bool variability = tracker.m_bProbeVariabilityEnabled;
        uint32_t call = 0;                                                    // this update call's number since the last reset
        if (variability) {                                                    // :464-470
            tracker.Update();
            call = volume.m_NumUpdateCalls++;
            if (tracker.bIsConverged) {                                       // nothing of the update is recorded, the refit included
                ++volume.m_NumUpdatesSkipped;
                return;
            }
        }
        if (!GetScheduledShadowMaskTexture()) RecordRefitTLAS(commandList);   // ShadowMaskRenderer, scheduled in front, refits otherwise

        struct Block { DDGIUpdateConsts k; DDGIVolumeDesc desc; } block{};
        static_assert(sizeof(Block) == 160, "DDGIUpdateConsts + DDGIVolumeDesc");
        DDGIUpdateConsts& k = block.k;
        memcpy(k.m_DirectionalLightVector, g_Scene->m_DirLightVec, sizeof g_Scene->m_DirLightVec);   // GIRenderer.cpp: GIProbeTraceConsts
        k.m_DirectionalLightStrength = g_Scene->m_DirLightStrength;
        RandomRotation(g_Scene->m_DDGIUpdateSeed, g_Scene->m_DDGIUpdateCount++, k.rayRotation);
        k.probeMaxRayDistance = 1e10f;                                        // :79 passes the scene's bounding radius; this mirror has none
        k.probeHysteresis = 0.5f;                                             // :115
        k.probeDistanceExponent = 50.0f;                                      // :118
        k.probeIrradianceThreshold = 0.2f;                                    // :111
        k.probeBrightnessThreshold = 0.1f;                                    // :112
        const bool placement = g_Scene->m_bDDGIProbeRelocation || g_Scene->m_bDDGIProbeClassification;
        if (placement) {                                                      // both stay 0 when neither pass runs
            k.probeMinFrontfaceDistance = g_Scene->m_DDGIMinFrontfaceDistance;
            k.probeFixedRayBackfaceThreshold = g_Scene->m_DDGIFixedRayBackfaceThreshold;
        }
        block.desc = volume.m_Desc;
        m_LastConsts = k;
        m_bRanLastFrame = true;
        nvrhi::BufferHandle cb = g_Graphic.CreateConstantBuffer(commandList, block);
        const uint32_t cx = (uint32_t)volume.m_Desc.probeCounts[0], cy = (uint32_t)volume.m_Desc.probeCounts[1], cz = (uint32_t)volume.m_Desc.probeCounts[2];

        Graphic::ComputePassParams trace;
        trace.m_CommandList = commandList;
        trace.m_ShaderName = "giprobetrace_CS_ProbeTrace";
        trace.m_BindingSetDesc.bindings = {
            Item::ConstantBuffer(0, cb),
            Item::StructuredBuffer_SRV(0, volume.m_DescBuffer),
            Item::Texture_SRV(1, volume.m_ProbeData),
            Item::Texture_SRV(2, volume.m_ProbeIrradiance),
            Item::Texture_SRV(3, volume.m_ProbeDistance),
            Item::RayTracingAccelStruct(4, g_Scene->m_TLAS.get()),
            Item::StructuredBuffer_SRV(5, g_Scene->m_InstanceConstsBuffer),
            Item::StructuredBuffer_SRV(6, g_Graphic.m_GlobalVertexBuffer),
            Item::StructuredBuffer_SRV(7, g_Graphic.m_GlobalMaterialDataBuffer),
            Item::StructuredBuffer_SRV(8, g_Graphic.m_GlobalIndexBuffer),
            Item::StructuredBuffer_SRV(9, g_Graphic.m_GlobalMeshDataBuffer),
            Item::StructuredBuffer_SRV(10, as.instances),                     // the structure's other buffers (include/trhip.h)
            Item::StructuredBuffer_SRV(11, as.blasHeaders),
            Item::StructuredBuffer_SRV(12, as.blasNodes),
            Item::StructuredBuffer_SRV(13, as.triOrder),
            Item::StructuredBuffer_UAV(0, volume.m_RayData),
            Item::Sampler(0, g_CommonResources.LinearClampSampler),           // accepted and ignored
            Item::Sampler(1, g_CommonResources.LinearClampSampler),
            Item::Sampler(2, g_CommonResources.LinearClampSampler),
        };
        trace.m_DispatchGroupSize = Vector3U{ kDDGIRaysPerProbe / 64, cx * cz, cy };          // groups of 64 rays: the pass's wave
        g_Graphic.AddComputePass(trace);

        for (int radiance = 1; radiance >= 0; --radiance) {
            Graphic::ComputePassParams blend;
            blend.m_CommandList = commandList;
            blend.m_ShaderName = radiance ? "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=1" : "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=0";
            blend.m_BindingSetDesc.bindings = {
                Item::ConstantBuffer(0, cb),
                Item::StructuredBuffer_SRV(1, volume.m_RayData),
                Item::Texture_SRV(3, volume.m_ProbeData),
                radiance ? Item::Texture_UAV(1, volume.m_ProbeIrradiance) : Item::Texture_UAV(2, volume.m_ProbeDistance),
            };
            if (radiance && variability) blend.m_BindingSetDesc.bindings.push_back(Item::StructuredBuffer_UAV(4, volume.m_ProbeVariability));
            blend.m_DispatchGroupSize = Vector3U{ cx, cz, cy };
            g_Graphic.AddComputePass(blend);
        }
        if (placement) RecordPlacement(commandList, cb, cx, cy, cz);
        if (variability) RecordVariability(commandList, cb, call, cx, cy, cz);
    }

    void RecordPlacement(nvrhi::CommandListHandle commandList, nvrhi::BufferHandle cb, uint32_t cx, uint32_t cy, uint32_t cz)
    {
        using Item = nvrhi::BindingSetItem;
        const Scene::RTDDGIVolume& volume = g_Scene->m_RTDDGIVolume;
        const nvrhi::rt::AccelStruct& as = *g_Scene->m_TLAS;
        const uint32_t numProbes = cx * cy * cz;                              // :513-527: relocation and classification behind the blends
        Graphic::ComputePassParams fixed;
        fixed.m_CommandList = commandList;
        fixed.m_ShaderName = "giprobetrace_CS_ProbeTraceFixedRays";
        fixed.m_BindingSetDesc.bindings = {
            Item::ConstantBuffer(0, cb),
            Item::StructuredBuffer_SRV(0, volume.m_DescBuffer),
            Item::Texture_SRV(1, volume.m_ProbeData),
            Item::RayTracingAccelStruct(4, g_Scene->m_TLAS.get()),
            Item::StructuredBuffer_SRV(5, g_Scene->m_InstanceConstsBuffer),
            Item::StructuredBuffer_SRV(6, g_Graphic.m_GlobalVertexBuffer),
            Item::StructuredBuffer_SRV(8, g_Graphic.m_GlobalIndexBuffer),
            Item::StructuredBuffer_SRV(9, g_Graphic.m_GlobalMeshDataBuffer),
            Item::StructuredBuffer_SRV(10, as.instances),
            Item::StructuredBuffer_SRV(11, as.blasHeaders),
            Item::StructuredBuffer_SRV(12, as.blasNodes),
            Item::StructuredBuffer_SRV(13, as.triOrder),
            Item::StructuredBuffer_UAV(0, volume.m_FixedRayData),
        };
        fixed.m_DispatchGroupSize = Vector3U{ (numProbes * kDDGIFixedRays + 63) / 64, 1, 1 };
        g_Graphic.AddComputePass(fixed);
        for (int relocation = 1; relocation >= 0; --relocation) {
            if (!(relocation ? g_Scene->m_bDDGIProbeRelocation : g_Scene->m_bDDGIProbeClassification)) continue;
            Graphic::ComputePassParams place;
            place.m_CommandList = commandList;
            place.m_ShaderName = relocation ? "ProbeRelocationCS_DDGIProbeRelocationCS" : "ProbeClassificationCS_DDGIProbeClassificationCS";
            place.m_BindingSetDesc.bindings = {
                Item::ConstantBuffer(0, cb),
                Item::StructuredBuffer_UAV(0, volume.m_FixedRayData),
                Item::Texture_UAV(3, volume.m_ProbeData),
            };
            place.m_DispatchGroupSize = Vector3U{ (numProbes + 31) / 32, 1, 1 };   // the reference's group count
            g_Graphic.AddComputePass(place);
        }
    }

    // :529-576: the sample of two update calls ago goes into the ring, then this call's reductions and the copy of their result
    void RecordVariability(nvrhi::CommandListHandle commandList, nvrhi::BufferHandle cb, uint32_t call, uint32_t cx, uint32_t cy, uint32_t cz)
    {
        using Item = nvrhi::BindingSetItem;
        Scene::RTDDGIVolume& volume = g_Scene->m_RTDDGIVolume;
        const uint32_t slot = call % 2;                                       // g_Graphic.m_FrameCounter % 2
        float readback = 0.0f;                                                // a slot never written reads 0
        g_Graphic.m_NVRHIDevice->readStagingBuffer(volume.m_ProbeVariabilityReadback, slot, &readback, sizeof readback);
        volume.m_Variability.m_AverageVariability = readback;
        volume.m_Variability.SetVariabilityForCurrentFrame(readback);

        const Vector3U kNumThreadsInGroup = { kDDGIReductionThreadsX, kDDGIReductionThreadsY, kDDGIReductionThreadsZ };
        const Vector2U kThreadSampleFootprint = { kDDGIReductionFootprintX, kDDGIReductionFootprintY };
        uint32_t inputTexelsX = cx * kDDGIIrradianceInteriorTexels, inputTexelsY = cz * kDDGIIrradianceInteriorTexels, inputTexelsZ = cy;
        DDGIRootConstants rootConsts{};
        bool bIsFirstPass = true;
        uint32_t numPasses = 0;
        while (inputTexelsX > 1 || inputTexelsY > 1 || inputTexelsZ > 1) {
            const uint32_t outputTexelsX = (inputTexelsX + kNumThreadsInGroup.x * kThreadSampleFootprint.x - 1) / (kNumThreadsInGroup.x * kThreadSampleFootprint.x);
            const uint32_t outputTexelsY = (inputTexelsY + kNumThreadsInGroup.y * kThreadSampleFootprint.y - 1) / (kNumThreadsInGroup.y * kThreadSampleFootprint.y);
            const uint32_t outputTexelsZ = (inputTexelsZ + kNumThreadsInGroup.z - 1) / kNumThreadsInGroup.z;
            rootConsts.reductionInputSizeX = inputTexelsX;
            rootConsts.reductionInputSizeY = inputTexelsY;
            rootConsts.reductionInputSizeZ = inputTexelsZ;
            Graphic::ComputePassParams reduce;
            reduce.m_CommandList = commandList;
            reduce.m_ShaderName = bIsFirstPass ? "ReductionCS_DDGIReductionCS REDUCTION=1" : "ReductionCS_DDGIExtraReductionCS";
            reduce.m_BindingSetDesc.bindings = {                              // the averages ping-pong: a pass never reads the buffer it writes
                Item::PushConstants(1, sizeof rootConsts),
                Item::StructuredBuffer_SRV(4, bIsFirstPass ? volume.m_ProbeVariability : volume.m_ProbeVariabilityAverage[(numPasses + 1) % 2]),
                Item::StructuredBuffer_UAV(5, volume.m_ProbeVariabilityAverage[numPasses % 2]),
            };
            if (bIsFirstPass) {                                               // which probes classification has switched off
                reduce.m_BindingSetDesc.bindings.push_back(Item::ConstantBuffer(0, cb));
                reduce.m_BindingSetDesc.bindings.push_back(Item::Texture_SRV(3, volume.m_ProbeData));
            }
            reduce.m_PushConstantsData = &rootConsts;
            reduce.m_PushConstantsBytes = sizeof rootConsts;
            reduce.m_DispatchGroupSize = Vector3U{ outputTexelsX, outputTexelsY, outputTexelsZ };
            g_Graphic.AddComputePass(reduce);
            inputTexelsX = outputTexelsX; inputTexelsY = outputTexelsY; inputTexelsZ = outputTexelsZ;
            bIsFirstPass = false;
            ++numPasses;
        }
        commandList->copyToStagingBuffer(volume.m_ProbeVariabilityReadback, slot, volume.m_ProbeVariabilityAverage[(numPasses + 1) % 2], 0, sizeof(float));
    }
};
DEFINE_RENDERER(GIRenderer);

bool GetLastDDGIUpdateConsts(void* out96)
{
    const GIRenderer* r = static_cast<const GIRenderer*>(g_GIRenderer);
    if (!g_Scene->m_bDDGIUpdate || !r->m_bRanLastFrame) return false;
    memcpy(out96, &r->m_LastConsts, sizeof r->m_LastConsts);
    return true;
}

bool GetLastDDGIProbeVisualizationConsts(void* out96)
{
    const GIDebugRenderer* r = static_cast<const GIDebugRenderer*>(g_GIDebugRenderer);
    if (!r->m_bDrewLastFrame) return false;
    memcpy(out96, &r->m_LastDrawConsts, sizeof r->m_LastDrawConsts);
    return true;
}

bool GetGIProbeCullBuffers(nvrhi::BufferHandle* positions, nvrhi::BufferHandle* drawArgs, nvrhi::BufferHandle* instanceToProbe)
{
    const GIDebugRenderer* r = static_cast<const GIDebugRenderer*>(g_GIDebugRenderer);
    if (!r->LastOutput(GIDebugRenderer::DrawArgs)) return false;
    *positions = r->LastOutput(GIDebugRenderer::Positions);
    *drawArgs = r->LastOutput(GIDebugRenderer::DrawArgs);
    *instanceToProbe = r->LastOutput(GIDebugRenderer::InstanceToProbe);
    return true;
}

void ReleaseGIProbeCullBuffers() { static_cast<GIDebugRenderer*>(g_GIDebugRenderer)->DropLastOutputs(); }
