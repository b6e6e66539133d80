// Scene.h -- the part of the reference's Scene / View (source/Scene.h:44-179, source/Scene.cpp) that
// feeds the visibility path: culling matrices, culling toggles, the GPU buffers the passes bind, and
// the per-frame pass schedule.  Camera controls, animation, ImGui, TLAS and lighting are out of scope.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "../ShaderInterop.h"
#include "DDGIVariability.h"
#include "MathUtilities.h"
#include "RenderGraph.h"
#include "nvrhi_lite.h"
#include "tf_lite.h"

// Scene.h:44-74
class View
{
public:
    void Update();                                   // Scene.cpp:109-145

    float m_ZNearP = 0.1f;                           // Scene.h:50
    float m_FOV = 0.785398163f;                      // 45 deg, Scene.h:52
    float m_AspectRatio = 16.0f / 9.0f;

    Matrix m_WorldToView{}, m_PrevWorldToView{};
    Matrix m_ViewToClip{}, m_PrevViewToClip{};
    Matrix m_CullingWorldToView{}, m_CullingPrevWorldToView{};   // frozen by m_bFreezeCullingCamera
    // Scene.h:60-66, what DeferredLightingRenderer reads.  m_Eye: the point m_WorldToView maps to the view-space origin,
    // -t * R^T of the rigid transform [R | t] (the camera arrives as a matrix here, not as eye + orientation);
    // m_ClipToWorld: the inverse of m_WorldToView * m_ViewToClip, in double precision, rounded once (MathUtilities.h).
    float m_Eye[3] = { 0.0f, 0.0f, 0.0f };
    Matrix m_ClipToWorld{};

    // The reference derives m_WorldToView from eye/orientation with DirectXMath (absent here) in
    // View::Update; this build takes the camera matrix from the application instead.
    void SetCamera(const Matrix& worldToView) { m_PendingWorldToView = worldToView; m_bHasPending = true; }
    // Tests need an explicit previous-frame matrix for frame 0.
    void SetPrevCamera(const Matrix& prevWorldToView) { m_WorldToView = prevWorldToView; }
    bool m_bUseExplicitProjection = false;           // keep m_ViewToClip as set by the application
    Matrix m_ExplicitViewToClip{};                   // that projection, unjittered: what Update starts from every frame

    // Temporal anti-aliasing (Scene.h:57-58, Scene.cpp:113-119, :127-131), kept while Scene::IsTAAEnabled(): the jitter offsets in
    // pixels and the jittered world-to-clip of this frame and the last.  On the first such frame the previous ones are this frame's.
    Vector2 m_PrevJitterOffset{ 0.0f, 0.0f }, m_CurrentJitterOffset{ 0.0f, 0.0f };
    Matrix m_WorldToClip{}, m_PrevWorldToClip{};
    bool m_bHasTAAHistory = false;                   // a frame ran with TAA on since it was switched on

private:
    Matrix m_PendingWorldToView{};
    bool m_bHasPending = false;
};

class Scene
{
public:
    void Initialize();
    void PostSceneLoad();                            // Scene.cpp:662-681
    void Update();                                   // Scene.cpp:468-521
    void Shutdown();

    // Scene content as flat arrays = what SceneLoading.cpp:203-224,1016-1088 produces
    // (global mesh / meshlet buffers) plus the primitive table of Scene.cpp:282-362.
    void LoadFromArrays(const void* instances, uint32_t numInstances,
                        const void* meshData, uint32_t numMeshes,
                        const void* meshlets, uint64_t numMeshlets,
                        const uint32_t* opaqueIds, uint32_t numOpaque,
                        const uint32_t* alphaMaskIds, uint32_t numAlphaMask);
    void LoadNodes(const void* nodeLocalTransforms, uint32_t numNodes, const uint32_t* primitiveToNode);

    View m_View;

    // Scene.h:128-132
    bool m_bEnableFrustumCulling = true;
    bool m_bEnableOcclusionCulling = true;
    bool m_bEnableMeshletConeCulling = true;
    bool m_bFreezeCullingCamera = false;
    int32_t m_ForceMeshLOD = -1;
    bool m_bUpdateInstanceTransforms = false;        // run UpdateInstanceConstsRenderer (animated scenes)
    // multi-GPU (not in the reference): the instances whose transforms this rank updates every frame -- the contiguous range its
    // id lists cover (trhost_set_instance_update_range); the whole (replicated) table by default
    uint32_t m_InstanceUpdateFirst = 0, m_InstanceUpdateCount = 0xFFFFFFFFu;

    uint32_t m_NumPrimitives = 0;
    std::vector<uint32_t> m_OpaquePrimitiveIDs, m_AlphaMaskPrimitiveIDs;
    std::vector<uint8_t> m_NodeLocalTransforms;      // NodeLocalTransform[] (host copy, uploaded every frame)
    uint32_t m_NumNodes = 0;
    bool m_bNodeLocalTransformsDirty = false;        // the host copy changed since UpdateInstanceConstsRenderer last uploaded it

    // Scene.h:152-162
    nvrhi::BufferHandle m_InstanceConstsBuffer;
    nvrhi::BufferHandle m_OpaqueInstanceIDsBuffer, m_AlphaMaskInstanceIDsBuffer;
    nvrhi::BufferHandle m_NodeLocalTransformsBuffer, m_PrimitiveIDToNodeIDBuffer;
    nvrhi::TextureHandle m_HZB;
    // stand-in for the rasteriser's output (RenderInstances' pixel work is out of scope): the depth
    // image that GenerateHZB consumes is copied from here into the transient depth buffer.
    nvrhi::TextureHandle m_SyntheticDepth;
    // Instead of the stand-in: every pass rasterises the depth of its visible meshlets ("basepass_MS_Main_depth", the
    // compute replacement of MS_Main + depth test) into the depth buffer, cleared at the start of the base pass.
    bool m_bRasterDepth = false;
    // Visibility buffer + motion target (trhost_set_visibility_buffer; implies m_bRasterDepth): every pass rasterises through
    // "basepass_MS_Main_visibility" into GBufferRenderer's VisibilityBuffer, and "basepass_PS_Main_motion" resolves
    // GBufferMotion once after the last pass.
    bool m_bVisibilityBuffer = false;
    // GBufferA (trhost_set_gbuffer; implies m_bVisibilityBuffer): "basepass_PS_Main_GBuffer" resolves GBufferA and
    // GBufferMotion in one dispatch in the place of "basepass_PS_Main_motion".  Needs LoadMaterials.
    bool m_bGBuffer = false;
    // ALPHA_MASK_MODE's discard (trhost_set_alpha_test; needs m_bRasterDepth and LoadMaterials): the alpha-mask pass slots draw
    // through "basepass_MS_Main_depth ALPHA_MASK_MODE=1" / "basepass_MS_Main_visibility ALPHA_MASK_MODE=1" (BasePassRenderers.cpp:489),
    // and ShadowMaskRenderer binds the texture table.  Off: alpha-mask instances are drawn as solid triangles.
    bool m_bAlphaTest = false;
    uint32_t m_DebugViewMode = 0;                    // Scene.h: feeds BasePassConstants::m_DebugMode (BasePassRenderers.cpp:455) and DeferredLightingConsts::m_DebugMode
    // Deferred lighting (trhost_set_deferred_lighting; implies m_bGBuffer): DeferredLightingRenderer runs after GBufferRenderer,
    // "deferredlighting_PS_Main" or, with m_DebugViewMode != 0, "deferredlighting_PS_Main_Debug", into its LightingOutput.
    bool m_bDeferredLighting = false;
    float m_DirLightVec[3] = { 0.0f, -1.0f, 0.0f };  // Scene.h:134-136: used as given (the reference derives it from two angles)
    float m_DirLightStrength = 1.0f;
    nvrhi::TextureHandle m_ShadowMaskTexture;        // R8_UNORM at render resolution, or null: the pass reads 1.0 (the reference's WhiteTexture)
    // The DDGI volume DeferredLightingRenderer consumes (Scene.h: m_RTDDGIVolume, GIRenderer's in the reference).
    // trhost_upload_ddgi_volume supplies the descriptor and the three array textures; with trhost_set_ddgi_update GIRenderer
    // (GIRenderer.cpp) traces and blends the probes into them every frame, from what they hold.
    struct RTDDGIVolume
    {
        interop::DDGIVolumeDesc m_Desc{};            // the host copy, appended to the pass's constant block
        nvrhi::BufferHandle m_DescBuffer;            // t5
        nvrhi::TextureHandle m_ProbeData, m_ProbeIrradiance, m_ProbeDistance;   // t6, t7, t8
        nvrhi::BufferHandle m_RayData;               // float4[numProbes * 256]: the trace's u0, the blends' t1
        nvrhi::BufferHandle m_FixedRayData;          // float[numProbes * 32]: u0 of the fixed-ray trace, of relocation and of classification
        // Probe variability (trhost_set_ddgi_probe_variability; GIRenderer.cpp:158-190, :529-576): the radiance blend's u4,
        // float[counts.y][6 * counts.z][6 * counts.x], zero on creation and after a reset; the reductions' two average buffers
        // (float2 per workgroup, ping-pong); the two-slot read-back of element 0; and the convergence rule with its counters.
        nvrhi::BufferHandle m_ProbeVariability, m_ProbeVariabilityAverage[2];
        nvrhi::StagingBufferHandle m_ProbeVariabilityReadback;
        DDGIVariability m_Variability;
        uint32_t m_NumUpdateCalls = 0;               // update calls since the last reset: the read-back slot is this % 2
        uint32_t m_NumUpdatesSkipped = 0;            // of them, the converged ones, which recorded nothing
        bool IsValid() const { return m_DescBuffer && m_ProbeData && m_ProbeIrradiance && m_ProbeDistance; }
    } m_RTDDGIVolume;
    // GIRenderer::RenderDDGI (trhost_set_ddgi_update; needs the volume, m_TLAS and m_bDeferredLighting): frame n's ray rotation
    // comes from (m_DDGIUpdateSeed, m_DDGIUpdateCount = n); the settings are GIRenderer.cpp:111-118's.
    bool m_bDDGIUpdate = false;
    uint32_t m_DDGIUpdateSeed = 0, m_DDGIUpdateCount = 0;
    // trhost_set_ddgi_probe_placement: GIRenderer.cpp:513-527's relocation and classification behind the blends (off by default; the
    // reference's :80-83 switch both on), with probeMinFrontfaceDistance (:98, :106) and probeFixedRayBackfaceThreshold (:121).
    bool m_bDDGIProbeRelocation = false, m_bDDGIProbeClassification = false;
    float m_DDGIMinFrontfaceDistance = 0.3f, m_DDGIFixedRayBackfaceThreshold = 0.25f;
    bool m_bEnableDDGI = false;                      // trhost_set_ddgi
    bool IsDDGIEnabled() const { return m_bEnableDDGI && m_RTDDGIVolume.IsValid(); }
    // Auto exposure and tone mapping (trhost_set_post_process; implies m_bDeferredLighting): AdaptLuminanceRenderer and
    // PostProcessRenderer run after DeferredLightingRenderer and turn LightingOutput into the RGBA8_UNORM back buffer.
    bool m_bPostProcess = false;
    float m_ManualExposureOverride = 0.0f;           // Scene.h: > 0 switches the histogram and the adaptation off
    float m_MiddleGray = 0.18f;
    // AdaptLuminanceRenderer.cpp:19-21 (members of the renderer there; here where the facade can set them)
    float m_MinimumLuminance = 0.004f, m_MaximumLuminance = 12.0f, m_AutoExposureSpeed = 0.0025f;
    float m_CPUCappedFrameTimeMs = 16.0f;            // Engine::m_CPUCappedFrameTimeMs: set by the application (trhost_set_frame_time_ms), no clock here
    nvrhi::TextureHandle m_BloomTexture;             // R11G11B10_FLOAT at render resolution, or null: the pass reads black (the reference's BlackTexture)
    float m_BloomStrength = 0.0f;
    // Bloom generation (trhost_set_bloom; needs m_bPostProcess, excludes an uploaded m_BloomTexture): BloomRenderer runs between
    // DeferredLightingRenderer and AdaptLuminanceRenderer and PostProcessRenderer binds its texture.  The mip count and the
    // radius are members of the renderer in the reference (BloomRenderer.cpp:16-17, defaults 6 and 0.005f).
    // Temporal anti-aliasing (trhost_set_taa; needs m_bPostProcess): View::Update jitters the projection and TAARenderer runs between
    // AdaptLuminanceRenderer and PostProcessRenderer, which then reads its g_AntiAliasedLightingOutput (Scene.cpp:505-507).
    bool m_bEnableTAA = false;
    float m_TAAMinBlend = 0.1f, m_TAAMaxSampleCount = 64.0f;
    bool m_bResetTAAHistory = true;                  // the next frame's resolve starts every texel again (the first frame; trhost_reset_taa_history)
    bool IsTAAEnabled() const { return m_bEnableTAA && m_bPostProcess; }
    bool m_bEnableBloom = false;
    uint32_t m_NbBloomMips = 6;
    float m_BloomFilterRadius = 0.005f;
    // The sky pass (trhost_set_sky; needs m_bDeferredLighting and a dataset from trhost_load_sky_dataset): SkyRenderer runs between
    // DeferredLightingRenderer and BloomRenderer and fills the texels of LightingOutput whose depth is <= 0.  Turbidity and ground
    // albedo are members of the renderer in the reference (SkyRenderer.cpp:135-136, the defaults below).
    bool m_bEnableSky = false;
    float m_SkyTurbidity = 2.0f;
    float m_GroundAlbedo[3] = { 0.1f, 0.1f, 0.1f };
    std::vector<double> m_SkyDataset;                // 3 x 1080 RGB coefficients, then 3 x 120 radiance coefficients; empty: none loaded
    // Ambient occlusion (trhost_set_ambient_occlusion; needs m_bGBuffer): AmbientOcclusionRenderer runs between GBufferRenderer and
    // DeferredLightingRenderer, which then binds its SSAO texture at t3 with m_SSAOEnabled = 1.  The settings are members of the
    // renderer in the reference (AmbientOcclusionRenderer.cpp:22, :36-37; XeGTAO::GTAOSettings' defaults below).
    bool m_bEnableAO = false;
    uint32_t m_AOQuality = 3, m_AODenoisePasses = 3;
    float m_AORadius = 0.5f, m_AOFalloffRange = 0.615f, m_AOFinalValuePower = 2.2f, m_AODepthMIPSamplingOffset = 3.3f;
    // Ray-traced sun shadows (trhost_load_raytracing, trhost_upload_blue_noise, trhost_set_shadow_mask; needs m_bGBuffer, excludes an
    // uploaded m_ShadowMaskTexture): ShadowMaskRenderer runs between AmbientOcclusionRenderer and DeferredLightingRenderer, which
    // then binds its mask at t4.  m_TLAS (Scene.h:157) holds the whole structure; the settings are members of the renderer in the
    // reference (ShadowMaskRenderer.cpp:87-89), the ray start offset is its 0.01 / 0.1 by the scene's bounding radius (:274).
    void LoadRaytracing(const uint32_t* indices, uint64_t numIndices, const uint32_t* indexCounts, uint32_t numMeshes);
    nvrhi::rt::AccelStructHandle m_TLAS;
    nvrhi::TextureHandle m_BlueNoise;                // CommonResources::BlueNoise: RGBA8_UNORM 128 x 128, an input
    bool m_bEnableShadows = false, m_bEnableSoftShadows = true;
    float m_SunAngularDiameter = 0.533f, m_ShadowRayStartOffset = 0.1f;
    // The shadow denoiser (trhost_set_shadow_denoising; needs m_bEnableShadows; the reference's m_bEnableShadowDenoising): ShadowMaskRenderer
    // then runs DenoiseShadows behind the trace.  The first two defaults are NRD's, the third this project's (csrc/k_sigma.hip, SETTINGS).
    bool m_bEnableShadowDenoising = false;
    float m_ShadowPlaneDistanceSensitivity = 0.02f, m_ShadowStabilizationStrength = 5.0f / 6.0f, m_ShadowSigmaScale = 2.0f;
    bool m_bResetShadowHistory = true;               // the next frame's stabilisation reads no history (the first frame; trhost_reset_shadow_history)
    nvrhi::BufferHandle m_LuminanceBuffer;           // Scene.h: one float, the adapted luminance; survives across frames
    nvrhi::TextureHandle m_ExposureTexture;          // 1 x 1 R32_FLOAT
    // SceneLoader's m_GlobalMaterialData upload (SceneLoading.cpp:516-537, 1016-1088); a textured material names textures of Graphic::CreateMaterialTexture.
    void LoadMaterials(const void* materials, uint32_t numMaterials);
    // `<scene>_CachedData.bin` version 3 (SceneLoading.cpp:57-79 layout, :706-781 LoadCachedData): meshes, meshlets and
    // the mesh-shader geometry come from the file, instances and id lists from the caller (the glTF side of the reference).
    void LoadCachedData(const char* path, const void* instances, uint32_t numInstances, const uint32_t* opaqueIds, uint32_t numOpaque,
                        const uint32_t* alphaMaskIds, uint32_t numAlphaMask);
    void LoadGeometry(const void* vertices, uint64_t numVertices, const uint32_t* meshletVertexIds, uint64_t numVertexIds,
                      const uint32_t* meshletTriangles, uint64_t numTriangles);

    // GI debug view (GIRenderer.cpp:598-808), from supplied buffers: the probes' world positions and states as a DDGI volume would
    // give them, culled every frame by GIDebugRenderer when m_bShowGIProbes is set.  This path has no draw (the buffers belong to no
    // volume whose irradiance could shade the spheres); trhost_set_ddgi_probe_visualization below is the whole pass.
    void LoadGIProbes(const float* positions, const float* states, uint32_t numProbes, float probeRadius, bool hideInactive);
    nvrhi::BufferHandle m_GIProbePositionsBuffer, m_GIProbeStatesBuffer;
    uint32_t m_NumGIProbes = 0;
    float m_GIProbeRadius = 0.1f;
    bool m_bHideInactiveGIProbes = false, m_bShowGIProbes = false;
    uint32_t m_GIProbeSphereIndexCount = 2880;       // m_IndexCount the supplied-buffer path writes (its arguments have no consumer); the live path writes UnitSphere's 468
    // trhost_set_ddgi_probe_visualization: GIDebugRenderer on m_RTDDGIVolume as it is on the device this frame -- "giprobevisualization_
    // CS_LoadGIProbes", the cull, then "giprobevisualization_PS_VisualizeGIProbes" into PostProcessRenderer's back buffer and the
    // frame's depth buffer (csrc/k_giprobedraw.hip).  Needs the volume and m_bPostProcess: a frame without either fails and says which.
    bool m_bDDGIProbeVisualization = false, m_bDDGIProbeVisualizationHideInactive = false;
    float m_DDGIProbeVisualizationRadius = 0.1f;

    std::shared_ptr<RenderGraph> m_RenderGraph;
    tf::Executor m_Executor{ 4 };                    // Engine.cpp:19,110-116 (default 12 workers)
};
#define g_Scene (Graphic::GetInstance().m_Scene)
