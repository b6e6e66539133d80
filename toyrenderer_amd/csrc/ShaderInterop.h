// ShaderInterop.h -- wire formats of the meshlet-visibility path, shared by the C++ host mirror
// and the HIP kernels.  Restates the layouts of the reference's shared C++/HLSL header
// source/shaders/ShaderInterop.h (only the structs on the hot path); every
// size/offset the HLSL side relies on is pinned by a static_assert.
#pragma once

#include <cstddef>
#include <cstdint>

namespace interop
{

// ShaderInterop.h:6-7
static constexpr uint32_t kNumThreadsPerWave = 32;              // reference group width (D3D wave32); a gfx950 wave64 runs two groups
static constexpr uint32_t kMaxThreadGroupsPerDimension = 65535;

// ShaderInterop.h:15-17
static constexpr uint32_t kCullingFlagFrustumCullingEnable = (1u << 0);
static constexpr uint32_t kCullingFlagOcclusionCullingEnable = (1u << 1);
static constexpr uint32_t kCullingFlagMeshletConeCullingEnable = (1u << 2);

// ShaderInterop.h:10-13
static constexpr uint32_t MaterialFlag_UseAlbedoTexture = (1u << 0);
static constexpr uint32_t MaterialFlag_UseNormalTexture = (1u << 1);
static constexpr uint32_t MaterialFlag_UseMetallicRoughnessTexture = (1u << 2);
static constexpr uint32_t MaterialFlag_UseEmissiveTexture = (1u << 3);
static constexpr uint32_t kMaterialFlagAnyTexture = 0xFu;

// ShaderInterop.h:26-38 (2, 3 and 12 also write GBufferA's debug byte; 10 needs the DDGI volume and is refused)
static constexpr uint32_t kDeferredLightingDebugMode_LightingOnly = 1;
static constexpr uint32_t kDeferredLightingDebugMode_ColorizeInstances = 2;
static constexpr uint32_t kDeferredLightingDebugMode_ColorizeMeshlets = 3;
static constexpr uint32_t kDeferredLightingDebugMode_Albedo = 4;
static constexpr uint32_t kDeferredLightingDebugMode_Normal = 5;
static constexpr uint32_t kDeferredLightingDebugMode_Emissive = 6;
static constexpr uint32_t kDeferredLightingDebugMode_Metalness = 7;
static constexpr uint32_t kDeferredLightingDebugMode_Roughness = 8;
static constexpr uint32_t kDeferredLightingDebugMode_AmbientOcclusion = 9;
static constexpr uint32_t kDeferredLightingDebugMode_Ambient = 10;
static constexpr uint32_t kDeferredLightingDebugMode_ShadowMask = 11;
static constexpr uint32_t kDeferredLightingDebugMode_MeshLOD = 12;
static constexpr uint32_t kDeferredLightingDebugMode_MotionVectors = 13;

// ShaderInterop.h:19-24
static constexpr uint32_t kMaxMeshletVertices = 64;
static constexpr uint32_t kMaxMeshletTriangles = 96;
static constexpr uint32_t kMaxNumMeshLODs = 8;
static constexpr uint32_t kInvalidMeshLOD = 0xFF;

struct Vector2 { float x, y; };
struct Vector2U { uint32_t x, y; };
struct Vector3U { uint32_t x, y, z; };
struct Vector4 { float x, y, z, w; };
struct Matrix { float m[4][4]; }; // row-major, row vectors (compileallshaders.bat:73 --matrixRowMajor)

// ShaderInterop.h:49-68
struct BasePassConstants
{
    Matrix m_WorldToClip;
    Matrix m_PrevWorldToClip;
    Matrix m_WorldToView;
    Vector4 m_Frustum;
    Vector2U m_HZBDimensions;
    float m_P00;
    float m_P11;
    float m_NearPlane;
    uint32_t m_CullingFlags;
    uint32_t m_DebugMode;
    uint32_t PAD0;
    Vector2U m_OutputResolution;
    uint32_t m_bVisualizeMinMipTilesOnAlbedoOutput;
    uint32_t m_bWriteSamplerFeedback;
};

// ShaderInterop.h:70-77
struct BasePassInstanceConstants
{
    Matrix m_WorldMatrix;
    Matrix m_PrevWorldMatrix;
    uint32_t m_MeshDataIdx;
    uint32_t m_MaterialDataIdx;
    float PAD0[2];
};

// ShaderInterop.h:150-158
struct TextureData
{
    uint32_t m_GlobalIndex;
    uint32_t m_IsWrapSampler;
    uint32_t m_DescriptorIndex;
    uint32_t m_FeedbackTextureDescriptorIndex;
    uint32_t m_MinMapTextureDescriptorIndex;
};

// ShaderInterop.h:160-172.  The G-buffer resolve (k_gbuffer.hip) reads the first 32 bytes only: texture-free materials.
struct MaterialData
{
    Vector4 m_ConstAlbedo;
    float m_ConstEmissive[3];
    float m_AlphaCutoff;
    TextureData m_AlbedoTexture;
    TextureData m_NormalTexture;
    TextureData m_MetallicRoughnessTexture;
    TextureData m_EmissiveTexture;
    uint32_t m_MaterialFlags;
    float m_ConstRoughness;                  // Q13: never read by the reference's shader (roughness 1, metallic 0 without a texture)
    float m_ConstMetallic;
};
// The four TextureData members are indexed as an array, slot c behind flag bit c (visibility_resolve.hip.h, host/Scene.cpp).
static_assert(offsetof(MaterialData, m_NormalTexture) == offsetof(MaterialData, m_AlbedoTexture) + sizeof(TextureData) &&
              offsetof(MaterialData, m_MetallicRoughnessTexture) == offsetof(MaterialData, m_AlbedoTexture) + 2 * sizeof(TextureData) &&
              offsetof(MaterialData, m_EmissiveTexture) == offsetof(MaterialData, m_AlbedoTexture) + 3 * sizeof(TextureData),
              "MaterialData: albedo, normal, metallic-roughness, emissive TextureData back to back");
static_assert(MaterialFlag_UseAlbedoTexture == 1u << 0 && MaterialFlag_UseNormalTexture == 1u << 1 && MaterialFlag_UseMetallicRoughnessTexture == 1u << 2 &&
              MaterialFlag_UseEmissiveTexture == 1u << 3, "MaterialData: flag bit c belongs to texture slot c");


// ShaderInterop.h:86-98
struct DeferredLightingConsts
{
    Matrix m_ClipToWorld;
    float m_CameraOrigin[3];
    uint32_t m_SSAOEnabled;
    uint32_t m_DebugMode;
    float m_DirectionalLightVector[3];
    float m_DirectionalLightStrength;
    Vector2U m_LightingOutputResolution;
    uint32_t m_bRTDDGIEnabled;
};
static_assert(sizeof(DeferredLightingConsts) == 112 && offsetof(DeferredLightingConsts, m_CameraOrigin) == 64 && offsetof(DeferredLightingConsts, m_SSAOEnabled) == 76, "DeferredLightingConsts");
static_assert(offsetof(DeferredLightingConsts, m_DebugMode) == 80 && offsetof(DeferredLightingConsts, m_DirectionalLightVector) == 84, "DeferredLightingConsts");
static_assert(offsetof(DeferredLightingConsts, m_DirectionalLightStrength) == 96 && offsetof(DeferredLightingConsts, m_LightingOutputResolution) == 100 &&
              offsetof(DeferredLightingConsts, m_bRTDDGIEnabled) == 108, "DeferredLightingConsts");

// The project's own: the DDGI volume as "deferredlighting_PS_Main" reads it at t5 (k_deferredlighting.hip, ddgi_irradiance.hip.h).
// It stands in for the RTXGI SDK's DDGIVolumeDescGPUPacked, whose layout this project cannot check; INTEGRATION.md names the SDK
// field behind each member.  No rotation and no scrolling (the reference's volume has neither, GIRenderer.cpp:71, :90);
// coordinate system 0 (left-handed, Y up): a probe's tile sits at texel (x * N, z * N) of slice y, N = interior + 2.
struct DDGIVolumeDesc
{
    float origin[3];
    float probeNormalBias;
    float probeSpacing[3];
    float probeViewBias;
    int32_t probeCounts[3];
    float probeIrradianceEncodingGamma;
    uint32_t numIrradianceInteriorTexels;    // 6 in the reference
    uint32_t numDistanceInteriorTexels;      // 14 in the reference
    uint32_t flags;                          // bit 0 relocation enabled, bit 1 classification enabled, bit 2 probe variability (the radiance blend writes u4)
    uint32_t pad;
};
static_assert(sizeof(DDGIVolumeDesc) == 64 && offsetof(DDGIVolumeDesc, probeSpacing) == 16 && offsetof(DDGIVolumeDesc, probeCounts) == 32 &&
              offsetof(DDGIVolumeDesc, numIrradianceInteriorTexels) == 48 && offsetof(DDGIVolumeDesc, flags) == 56, "DDGIVolumeDesc");
static constexpr uint32_t kDDGIFlag_Relocation = 1u, kDDGIFlag_Classification = 2u, kDDGIFlag_Variability = 4u;
static constexpr uint32_t kDDGIIrradianceInteriorTexels = 6, kDDGIDistanceInteriorTexels = 14, kDDGIMaxProbeCount = 1024;

// The project's own: b0 of "giprobetrace_CS_ProbeTrace", of the two "ProbeBlendingCS_DDGIProbeBlendingCS" passes and of the three
// placement passes (k_giprobetrace.hip, k_giprobeblend.hip, k_giprobeplacement.hip).  It begins with the reference's GIProbeTraceConsts (ShaderInterop.h:243-247) and
// goes on with what the SDK keeps in its volume descriptor and this project's 64-byte DDGIVolumeDesc does not hold: the frame's
// ray rotation (rows of a 3 x 3 matrix, rotated = (dot3(row0, d), dot3(row1, d), dot3(row2, d))) and the update's settings.
// Defaults: GIRenderer.cpp:79 (the scene's bounding radius), :111-118.  The passes read the volume's descriptor from a host copy
// that follows this block in b0 (160 bytes together), as the lighting pass does.
struct DDGIUpdateConsts
{
    float m_DirectionalLightVector[3];
    float m_DirectionalLightStrength;
    float rayRotation[3][4];                 // three rows; the fourth column is padding
    float probeMaxRayDistance;
    float probeHysteresis;                   // 0.5
    float probeDistanceExponent;             // 50
    float probeIrradianceThreshold;          // 0.2
    float probeBrightnessThreshold;          // 0.1
    float probeMinFrontfaceDistance;         // relocation and classification (k_giprobeplacement.hip): 0.1 for a scene radius below 3, else 0.3
    float probeFixedRayBackfaceThreshold;    // 0.25 (GIRenderer.cpp:121); both are 0 when neither of the two passes is on
    uint32_t pad;
};
static_assert(sizeof(DDGIUpdateConsts) == 96 && offsetof(DDGIUpdateConsts, rayRotation) == 16 && offsetof(DDGIUpdateConsts, probeMaxRayDistance) == 64 &&
              offsetof(DDGIUpdateConsts, probeBrightnessThreshold) == 80 && offsetof(DDGIUpdateConsts, probeMinFrontfaceDistance) == 84 &&
              offsetof(DDGIUpdateConsts, probeFixedRayBackfaceThreshold) == 88, "DDGIUpdateConsts");
static constexpr uint32_t kDDGIRaysPerProbe = 256;              // RTXGI_DDGI_BLEND_RAYS_PER_PROBE
static constexpr uint32_t kDDGIBackfaceRayLimit = 25;           // (uint)(256 * probeRandomRayBackfaceThreshold), 0.1f: GIRenderer.cpp:120
static constexpr uint32_t kDDGIFixedRays = 32;                  // RTXGI_DDGI_NUM_FIXED_RAYS: the unrotated rays of relocation and classification

// The RTXGI SDK's DDGIRootConstants (rtxgi/ddgi/DDGIRootConstants.h; GIRenderer.cpp:483, :553-555): push constants of the two
// reduction passes (k_ddgireduction.hip), which read the three input sizes; the three indices are accepted and ignored.
struct DDGIRootConstants
{
    uint32_t volumeIndex;
    uint32_t volumeConstantsIndex;
    uint32_t volumeResourceIndicesIndex;
    uint32_t reductionInputSizeX;
    uint32_t reductionInputSizeY;
    uint32_t reductionInputSizeZ;
};
static_assert(sizeof(DDGIRootConstants) == 24 && offsetof(DDGIRootConstants, reductionInputSizeX) == 12, "DDGIRootConstants");
// Probe variability (GIRenderer.cpp:158-190, :542-573): the ring's length, and the reduction's group and per-thread footprint
static constexpr uint32_t kDDGIMinimumVariabilitySamples = 16;
static constexpr uint32_t kDDGIReductionThreadsX = 4, kDDGIReductionThreadsY = 8, kDDGIReductionThreadsZ = 4, kDDGIReductionFootprintX = 4, kDDGIReductionFootprintY = 2;

// ShaderInterop.h:124-129: push constants of "adaptluminance_CS_GenerateLuminanceHistogram"
struct GenerateLuminanceHistogramParameters
{
    Vector2U m_SrcColorDims;
    float m_MinLogLuminance;                // log2 of the luminance that maps to bin 1
    float m_InverseLogLuminanceRange;       // 1 / (log2 max - log2 min)
};
static_assert(sizeof(GenerateLuminanceHistogramParameters) == 16 && offsetof(GenerateLuminanceHistogramParameters, m_MinLogLuminance) == 8, "GenerateLuminanceHistogramParameters");

// ShaderInterop.h:40-47: push constants of "adaptluminance_CS_AdaptExposure"
struct AdaptExposureParameters
{
    float m_MinLogLuminance;
    float m_LogLuminanceRange;
    float m_AdaptationSpeed;                // already clamped to [0, 1]: speed per ms times the frame time
    uint32_t m_NbPixels;
    float m_MiddleGray;
};
static_assert(sizeof(AdaptExposureParameters) == 20 && offsetof(AdaptExposureParameters, m_NbPixels) == 12 && offsetof(AdaptExposureParameters, m_MiddleGray) == 16, "AdaptExposureParameters");

// ShaderInterop.h:234-241: push constants of "postprocess_PS_PostProcess"
struct PostProcessParameters
{
    Vector2U m_OutputDims;
    float m_ManualExposure;                 // 0: the scene luminance comes from the luminance buffer
    float m_MiddleGray;
    float m_WhitePoint;                     // not read by the entry
    float m_BloomStrength;
};
static_assert(sizeof(PostProcessParameters) == 24 && offsetof(PostProcessParameters, m_ManualExposure) == 8 && offsetof(PostProcessParameters, m_BloomStrength) == 20, "PostProcessParameters");

// ShaderInterop.h:79-84: push constants (or b0) of "bloom_PS_Downsample" and "bloom_PS_Upsample"
struct BloomConsts
{
    Vector2 m_InvSourceResolution;          // downsample: 1 / (W >> i, H >> i) of the mip read
    float m_FilterRadius;                   // upsample: the tap distance in UV
    uint32_t m_bIsFirstDownsample;          // downsample: the Karis-weighted branch
};
static_assert(sizeof(BloomConsts) == 16 && offsetof(BloomConsts, m_InvSourceResolution) == 0 && offsetof(BloomConsts, m_FilterRadius) == 8 && offsetof(BloomConsts, m_bIsFirstDownsample) == 12, "BloomConsts");

// Push constants (or b0) of "taa_CS_TemporalResolve" (k_taa.hip).  The project's own: the reference's TAARenderer hands its
// parameters to the DLSS / FSR SDKs, which are not in its tree.
struct TAAConsts
{
    Vector2U m_OutputDims;
    Vector2 m_JitterDelta;                  // previous minus current jitter offset, in pixels
    float m_MinBlend;                       // the least weight of the current colour
    float m_MaxSampleCount;                 // the accumulated count's cap
    uint32_t m_bResetHistory;               // 1: no texel's history is valid
    uint32_t PAD0;
};
static_assert(sizeof(TAAConsts) == 32 && offsetof(TAAConsts, m_JitterDelta) == 8 && offsetof(TAAConsts, m_MinBlend) == 16 && offsetof(TAAConsts, m_bResetHistory) == 24, "TAAConsts");

// ShaderInterop.h:146-149, 297-305: the constant buffer b0 of "sky_PS_HosekWilkieSky".  Rows A B C D E F G H I Z; the shader
// reads .xyz, .w is written as 0.
struct HosekWilkieSkyParameters
{
    Vector4 m_Params[10];
};
struct SkyPassParameters
{
    Matrix m_ClipToWorld;
    float m_SunLightDir[3];
    uint32_t PAD0;
    float m_CameraPosition[3];
    uint32_t PAD1;
    HosekWilkieSkyParameters m_HosekParams;
};
static_assert(sizeof(SkyPassParameters) == 256 && offsetof(SkyPassParameters, m_SunLightDir) == 64 && offsetof(SkyPassParameters, m_CameraPosition) == 80 &&
              offsetof(SkyPassParameters, m_HosekParams) == 96, "SkyPassParameters");

// extern/xegtao/XeGTAO.h:59-83: the constant buffer b0 of the three "ambientocclusion_CS_XeGTAO_*" passes, filled by
// GTAOUpdateConstants (csrc/host/AmbientOcclusionRenderer.cpp, toyrenderer_amd/gtao.py)
struct GTAOConstants
{
    int32_t ViewportSize[2];
    Vector2 ViewportPixelSize;              // 1 / ViewportSize
    Vector2 DepthUnpackConsts;
    Vector2 CameraTanHalfFOV;
    Vector2 NDCToViewMul;
    Vector2 NDCToViewAdd;
    Vector2 NDCToViewMul_x_PixelSize;
    float EffectRadius;
    float EffectFalloffRange;
    float RadiusMultiplier;                 // the four "default constants" are carried but not read: the passes compile them in
    float Padding0;
    float FinalValuePower;
    float DenoiseBlurBeta;
    float SampleDistributionPower;
    float ThinOccluderCompensation;
    float DepthMIPSamplingOffset;
    int32_t NoiseIndex;
};
static_assert(sizeof(GTAOConstants) == 96 && offsetof(GTAOConstants, DepthUnpackConsts) == 16 && offsetof(GTAOConstants, EffectRadius) == 56 &&
              offsetof(GTAOConstants, FinalValuePower) == 72 && offsetof(GTAOConstants, NoiseIndex) == 92, "GTAOConstants");

// ShaderInterop.h:322-331: the push constants b1 of the main pass and of the denoise pass
struct XeGTAOMainPassConstantBuffer
{
    Matrix m_WorldToViewNoTranslate;
    uint32_t m_Quality;
};
struct XeGTAODenoiseConstants
{
    uint32_t m_FinalApply;
};
static_assert(sizeof(XeGTAOMainPassConstantBuffer) == 68 && offsetof(XeGTAOMainPassConstantBuffer, m_Quality) == 64, "XeGTAOMainPassConstantBuffer");
static_assert(sizeof(XeGTAODenoiseConstants) == 4, "XeGTAODenoiseConstants");

// ShaderInterop.h:285-295: the constant buffer b0 of "shadowmask_CS_ShadowMask" (csrc/host/ShadowMaskRenderer.cpp, toyrenderer_amd/frame.py)
struct ShadowMaskConsts
{
    Matrix m_ClipToWorld;
    float m_DirectionalLightDirection[3];
    float m_NoisePhase;                     // (frame counter & 0xff) * 1.61803398875f
    float m_CameraPosition[3];
    float m_TanSunAngularRadius;            // 0: hard shadows
    Vector2U m_OutputResolution;
    uint32_t m_bDoDenoising;                // != 0: u0 is the R16_FLOAT penumbra texture that the shadow denoiser reads (k_sigma.hip)
    float m_RayStartOffset;                 // the origin's offset along the normal, and TMin
};
static_assert(sizeof(ShadowMaskConsts) == 112 && offsetof(ShadowMaskConsts, m_DirectionalLightDirection) == 64 && offsetof(ShadowMaskConsts, m_NoisePhase) == 76 &&
              offsetof(ShadowMaskConsts, m_CameraPosition) == 80 && offsetof(ShadowMaskConsts, m_TanSunAngularRadius) == 92 &&
              offsetof(ShadowMaskConsts, m_OutputResolution) == 96 && offsetof(ShadowMaskConsts, m_bDoDenoising) == 104 &&
              offsetof(ShadowMaskConsts, m_RayStartOffset) == 108, "ShadowMaskConsts");

// ShaderInterop.h:229-232: push constants (or b0) of "shadowmask_CS_PackNormalAndRoughness" (k_shadowmask.hip)
struct PackNormalAndRoughnessConsts
{
    Vector2U m_OutputResolution;
};
static_assert(sizeof(PackNormalAndRoughnessConsts) == 8, "PackNormalAndRoughnessConsts");

// b0 (or push constants) of the three shadow denoiser entries "SIGMA_Shadow_*" (k_sigma.hip).  The project's own: the reference
// hands its settings to NRD, which is not in its tree.
struct SigmaConsts
{
    Matrix m_ClipToWorld;
    Vector2U m_OutputDims;
    Vector2 m_JitterDelta;                  // previous minus current jitter offset in pixels (TAAConsts carries the same); (0, 0) without TAA
    float m_PixelUnproject;                 // the world size of one pixel at unit distance, from m_ViewToClip
    float m_DenoisingRange;                 // max(100, 2 * scene radius): a texel at or beyond it is sky
    float m_PlaneDistanceSensitivity;
    float m_StabilizationStrength;          // the history's weight
    float m_SigmaScale;                     // the history clamp's half width in standard deviations
    uint32_t m_FrameIndex;                  // turns the tap rotation
    uint32_t m_Pass;                        // 0: Blur, 1: PostBlur; the other entries ignore it
    uint32_t m_bResetHistory;               // 1: no texel's history is valid
};
static_assert(sizeof(SigmaConsts) == 112 && offsetof(SigmaConsts, m_OutputDims) == 64 && offsetof(SigmaConsts, m_JitterDelta) == 72 &&
              offsetof(SigmaConsts, m_PixelUnproject) == 80 && offsetof(SigmaConsts, m_DenoisingRange) == 84 && offsetof(SigmaConsts, m_PlaneDistanceSensitivity) == 88 &&
              offsetof(SigmaConsts, m_StabilizationStrength) == 92 && offsetof(SigmaConsts, m_SigmaScale) == 96 && offsetof(SigmaConsts, m_FrameIndex) == 100 &&
              offsetof(SigmaConsts, m_Pass) == 104 && offsetof(SigmaConsts, m_bResetHistory) == 108, "SigmaConsts");

// this build's own (not in the reference): push constants of "raytracing_CS_RefitTLAS" (include/trhip.h, "acceleration structure")
struct RefitTLASConstants
{
    uint32_t m_NumInstances;
    uint32_t m_NumNodes;
    uint32_t m_NumLevels;
};
static_assert(sizeof(RefitTLASConstants) == 12, "RefitTLASConstants");
static constexpr uint32_t kBlueNoiseSize = 128;                 // CommonResources::BlueNoise: RGBA8_UNORM, 128 x 128
static constexpr uint32_t kAccelInner = 0xFFFFFFFFu;            // trhip_accel_node::leaf of an inner node
static constexpr uint32_t kTLASInstanceForceOpaque = 1, kTLASInstanceForceNonOpaque = 2;   // trhip_tlas_instance::flags

// ShaderInterop.h:117-122
struct DispatchIndirectArguments
{
    uint32_t m_ThreadGroupCountX;
    uint32_t m_ThreadGroupCountY;
    uint32_t m_ThreadGroupCountZ;
};

// ShaderInterop.h:131-144
struct GPUCullingPassConstants
{
    uint32_t m_NbInstances;
    uint32_t m_CullingFlags;
    Vector2U m_HZBDimensions;
    Vector4 m_Frustum;
    Matrix m_WorldToView;
    Matrix m_PrevWorldToView;
    float m_NearPlane;
    float m_P00;
    float m_P11;
    uint32_t m_ForcedMeshLOD;
    float m_MeshLODTarget;
};

// ShaderInterop.h:174-180
struct MeshLODData
{
    uint32_t m_MeshletDataBufferIdx;
    uint32_t m_NumMeshlets;
    float m_Error;
    uint32_t PAD0;
};

// ShaderInterop.h:182-189
struct MeshData
{
    Vector4 m_BoundingSphere;
    MeshLODData m_MeshLODDatas[kMaxNumMeshLODs];
    uint32_t m_NumLODs;
    uint32_t m_GlobalVertexBufferIdx;
    uint32_t m_GlobalIndexBufferIdx;
};

// ShaderInterop.h:191-198
struct MeshletData
{
    Vector4 m_BoundingSphere;
    uint32_t m_ConeAxisAndCutoff; // 4x u8: axis xyz mapped [0,255] -> [-1,1], cutoff /255
    uint32_t m_MeshletVertexIDsBufferIdx;
    uint32_t m_MeshletIndexIDsBufferIdx;
    uint32_t m_VertexAndTriangleCount;
};

// ShaderInterop.h:200-205 (Q9: 64 slots, at most 32 written)
struct MeshletPayload
{
    uint32_t m_MeshletIndices[64];
    uint32_t m_InstanceConstIdx;
    uint32_t m_MeshLOD;
};

// ShaderInterop.h:207-212
struct MeshletAmplificationData
{
    uint32_t m_InstanceConstIdx;
    uint32_t m_MeshLOD;
    uint32_t m_MeshletGroupOffset;
};

// ShaderInterop.h:278-283: the global vertex buffer.  The mesh stage (mesh_stage.hip.h) reads the position; the G-buffer
// resolve also reads the normal.
struct RawVertexFormat
{
    float m_Position[3];
    uint32_t m_PackedNormal;                 // R10G10B10A2
    uint16_t m_TexCoord[2];                  // half2
};
static_assert(sizeof(RawVertexFormat) == 20 && offsetof(RawVertexFormat, m_PackedNormal) == 12, "RawVertexFormat");

// ShaderInterop.h:108-115
struct DrawIndexedIndirectArguments
{
    uint32_t m_IndexCount;
    uint32_t m_InstanceCount;
    uint32_t m_StartIndexLocation;
    int32_t  m_BaseVertexLocation;
    uint32_t m_StartInstanceLocation;
};
static_assert(sizeof(DrawIndexedIndirectArguments) == 20, "DrawIndexedIndirectArguments");

// ShaderInterop.h:249-261
struct GIProbeVisualizationUpdateConsts
{
    uint32_t m_NumProbes;
    float m_CameraOrigin[3];
    Vector4 m_Frustum;
    Matrix m_WorldToView;
    Vector2U m_HZBDimensions;
    float m_P00;
    float m_P11;
    float m_NearPlane;
    float m_ProbeRadius;
    uint32_t m_bHideInactiveProbes;
};
static_assert(sizeof(GIProbeVisualizationUpdateConsts) == 124 && offsetof(GIProbeVisualizationUpdateConsts, m_WorldToView) == 32, "GIProbeVisualizationUpdateConsts");

// ShaderInterop.h:263-268, b0 of "giprobevisualization_PS_VisualizeGIProbes" (k_giprobedraw.hip): the reference's 80 bytes, layout
// unchanged, then the project's own near plane (the raster drops a triangle with a vertex at w <= near) and padding.  The
// descriptor's host copy follows the block in b0 (160 bytes together), as it follows the constants of the other DDGI passes.
struct GIProbeVisualizationConsts
{
    Matrix m_WorldToClip;
    float m_CameraDirection[3];
    float m_ProbeRadius;
    float m_NearPlane;                       // the project's own from here
    uint32_t pad[3];
};
static_assert(sizeof(GIProbeVisualizationConsts) == 96 && offsetof(GIProbeVisualizationConsts, m_CameraDirection) == 64 && offsetof(GIProbeVisualizationConsts, m_ProbeRadius) == 76 &&
              offsetof(GIProbeVisualizationConsts, m_NearPlane) == 80, "GIProbeVisualizationConsts");

// ShaderInterop.h:270-276: the vertex of the unit sphere (CommonResources.cpp:40-102), 91 of them with 468 indices (uint32_t)
struct UncompressedRawVertexFormat
{
    float m_Position[3];
    float m_Normal[3];
    float m_TexCoord[2];
};
static_assert(sizeof(UncompressedRawVertexFormat) == 32 && offsetof(UncompressedRawVertexFormat, m_Normal) == 12, "UncompressedRawVertexFormat");
static constexpr uint32_t kUnitSphereVertices = 91, kUnitSphereIndices = 468;

// ShaderInterop.h:214-218
struct MinMaxDownsampleConsts
{
    Vector2U m_OutputDimensions;
    uint32_t m_bDownsampleMax;
};

// ShaderInterop.h:220-227
struct NodeLocalTransform
{
    uint32_t m_ParentNodeIdx;
    float m_Position[3];
    float m_Rotation[4];
    float m_Scale[3];
    uint32_t PAD0;
};

// ShaderInterop.h:317-320
struct UpdateInstanceConstsPassConstants
{
    uint32_t m_NumInstances;
};
// this build's extension (not in the reference): the same pass over the instance range [m_FirstInstance, + m_NumInstances) --
// a rank of a sharded scene updates the instances it culls (csrc/host/BasePassRenderers.cpp, Scene::m_InstanceUpdate*)
struct UpdateInstanceConstsShardConstants
{
    uint32_t m_NumInstances;
    uint32_t m_FirstInstance;
};

// FFXHelpers.cpp:15-23 (push constants of the SPD pass)
struct SPDConstants
{
    uint32_t mips;
    uint32_t numWorkGroups;
    uint32_t workGroupOffset[2];
    float invInputSize[2]; // only used for linear sampling mode
    float padding[2];
};

// ---- extension of this build (documented in DESIGN.md) --------------------------------------
// The meshlet-dispatch argument buffer may be 16 bytes: the 4th word receives the number of
// leading amplification records that are defined (Q2: everything from the first dropped
// instance on is undefined in the reference).  A 12-byte buffer keeps the reference layout.
struct DispatchIndirectArgumentsEx
{
    DispatchIndirectArguments m_Args;
    uint32_t m_ValidRecords;
};

static_assert(sizeof(Matrix) == 64);
static_assert(sizeof(BasePassConstants) == 256);
static_assert(offsetof(BasePassConstants, m_WorldToView) == 128);
static_assert(offsetof(BasePassConstants, m_Frustum) == 192);
static_assert(offsetof(BasePassConstants, m_HZBDimensions) == 208);
static_assert(offsetof(BasePassConstants, m_NearPlane) == 224);
static_assert(offsetof(BasePassConstants, m_CullingFlags) == 228);
static_assert(sizeof(BasePassInstanceConstants) == 144);
static_assert(offsetof(BasePassInstanceConstants, m_MeshDataIdx) == 128);
static_assert(sizeof(TextureData) == 20);
static_assert(sizeof(MaterialData) == 124);
static_assert(offsetof(MaterialData, m_ConstEmissive) == 16 && offsetof(MaterialData, m_AlphaCutoff) == 28);
static_assert(offsetof(MaterialData, m_AlbedoTexture) == 32 && offsetof(MaterialData, m_MaterialFlags) == 112);
static_assert(sizeof(DispatchIndirectArguments) == 12);
static_assert(sizeof(GPUCullingPassConstants) == 180);
static_assert(offsetof(GPUCullingPassConstants, m_Frustum) == 16);
static_assert(offsetof(GPUCullingPassConstants, m_WorldToView) == 32);
static_assert(offsetof(GPUCullingPassConstants, m_PrevWorldToView) == 96);
static_assert(offsetof(GPUCullingPassConstants, m_NearPlane) == 160);
static_assert(offsetof(GPUCullingPassConstants, m_MeshLODTarget) == 176);
static_assert(sizeof(MeshLODData) == 16);
static_assert(sizeof(MeshData) == 156);
static_assert(offsetof(MeshData, m_MeshLODDatas) == 16);
static_assert(offsetof(MeshData, m_NumLODs) == 144);
static_assert(sizeof(MeshletData) == 32);
static_assert(offsetof(MeshletData, m_ConeAxisAndCutoff) == 16);
static_assert(sizeof(MeshletPayload) == 264);
static_assert(sizeof(MeshletAmplificationData) == 12);
static_assert(sizeof(MinMaxDownsampleConsts) == 12);
static_assert(sizeof(NodeLocalTransform) == 48);
static_assert(sizeof(SPDConstants) == 32);
static_assert(sizeof(DispatchIndirectArgumentsEx) == 16);

} // namespace interop
