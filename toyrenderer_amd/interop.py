"""numpy mirrors of the wire formats on the meshlet-visibility path.

Layouts follow the reference's shared C++/HLSL header source/shaders/ShaderInterop.h
(BasePassInstanceConstants :70-77, MeshLODData :174-180, MeshData :182-189, MeshletData :191-198,
MeshletAmplificationData :207-212, DispatchIndirectArguments :117-122, GPUCullingPassConstants
:131-144, BasePassConstants :49-68, MinMaxDownsampleConsts :214-218, NodeLocalTransform :220-227).
The C++ mirror with static_asserts is toyrenderer_amd/csrc/ShaderInterop.h.
"""
import numpy as np

kNumThreadsPerWave = 32
kMaxThreadGroupsPerDimension = 65535
kCullingFlagFrustumCullingEnable = 1
kCullingFlagOcclusionCullingEnable = 2
kCullingFlagMeshletConeCullingEnable = 4
kMaxNumMeshLODs = 8
kInvalidMeshLOD = 0xFF
MaterialFlag_UseAlbedoTexture = 1 << 0                      # ShaderInterop.h:10-13
MaterialFlag_UseNormalTexture = 1 << 1
MaterialFlag_UseMetallicRoughnessTexture = 1 << 2
MaterialFlag_UseEmissiveTexture = 1 << 3
kMaterialFlagAnyTexture = 0xF
kDeferredLightingDebugMode_ColorizeInstances = 2            # ShaderInterop.h:27-37: the views that write GBufferA's debug byte
kDeferredLightingDebugMode_ColorizeMeshlets = 3
kDeferredLightingDebugMode_MeshLOD = 12
kDeferredLightingDebugMode_Ambient = 10                     # needs the DDGI volume: refused by the lighting pass without one

BasePassInstanceConstants = np.dtype([
    ("m_WorldMatrix", np.float32, (4, 4)), ("m_PrevWorldMatrix", np.float32, (4, 4)),
    ("m_MeshDataIdx", np.uint32), ("m_MaterialDataIdx", np.uint32), ("PAD0", np.float32, (2,))])
MeshLODData = np.dtype([
    ("m_MeshletDataBufferIdx", np.uint32), ("m_NumMeshlets", np.uint32), ("m_Error", np.float32), ("PAD0", np.uint32)])
MeshData = np.dtype([
    ("m_BoundingSphere", np.float32, (4,)), ("m_MeshLODDatas", MeshLODData, (kMaxNumMeshLODs,)),
    ("m_NumLODs", np.uint32), ("m_GlobalVertexBufferIdx", np.uint32), ("m_GlobalIndexBufferIdx", np.uint32)])
MeshletData = np.dtype([
    ("m_BoundingSphere", np.float32, (4,)), ("m_ConeAxisAndCutoff", np.uint32),
    ("m_MeshletVertexIDsBufferIdx", np.uint32), ("m_MeshletIndexIDsBufferIdx", np.uint32),
    ("m_VertexAndTriangleCount", np.uint32)])
MeshletAmplificationData = np.dtype([
    ("m_InstanceConstIdx", np.uint32), ("m_MeshLOD", np.uint32), ("m_MeshletGroupOffset", np.uint32)])
DispatchIndirectArguments = np.dtype([
    ("m_ThreadGroupCountX", np.uint32), ("m_ThreadGroupCountY", np.uint32), ("m_ThreadGroupCountZ", np.uint32)])
GPUCullingPassConstants = np.dtype([
    ("m_NbInstances", np.uint32), ("m_CullingFlags", np.uint32), ("m_HZBDimensions", np.uint32, (2,)),
    ("m_Frustum", np.float32, (4,)), ("m_WorldToView", np.float32, (4, 4)), ("m_PrevWorldToView", np.float32, (4, 4)),
    ("m_NearPlane", np.float32), ("m_P00", np.float32), ("m_P11", np.float32), ("m_ForcedMeshLOD", np.uint32),
    ("m_MeshLODTarget", np.float32)])
BasePassConstants = np.dtype([
    ("m_WorldToClip", np.float32, (4, 4)), ("m_PrevWorldToClip", np.float32, (4, 4)), ("m_WorldToView", np.float32, (4, 4)),
    ("m_Frustum", np.float32, (4,)), ("m_HZBDimensions", np.uint32, (2,)), ("m_P00", np.float32), ("m_P11", np.float32),
    ("m_NearPlane", np.float32), ("m_CullingFlags", np.uint32), ("m_DebugMode", np.uint32), ("PAD0", np.uint32),
    ("m_OutputResolution", np.uint32, (2,)), ("m_bVisualizeMinMipTilesOnAlbedoOutput", np.uint32),
    ("m_bWriteSamplerFeedback", np.uint32)])
MinMaxDownsampleConsts = np.dtype([("m_OutputDimensions", np.uint32, (2,)), ("m_bDownsampleMax", np.uint32)])
DrawIndexedIndirectArguments = np.dtype([("m_IndexCount", np.uint32), ("m_InstanceCount", np.uint32), ("m_StartIndexLocation", np.uint32),
                                         ("m_BaseVertexLocation", np.int32), ("m_StartInstanceLocation", np.uint32)])     # ShaderInterop.h:108-115
GIProbeVisualizationUpdateConsts = np.dtype([                                                                              # ShaderInterop.h:249-261
    ("m_NumProbes", np.uint32), ("m_CameraOrigin", np.float32, (3,)), ("m_Frustum", np.float32, (4,)), ("m_WorldToView", np.float32, (4, 4)),
    ("m_HZBDimensions", np.uint32, (2,)), ("m_P00", np.float32), ("m_P11", np.float32), ("m_NearPlane", np.float32), ("m_ProbeRadius", np.float32),
    ("m_bHideInactiveProbes", np.uint32)])
GIProbeVisualizationConsts = np.dtype([                                                                                    # ShaderInterop.h:263-268, then the project's own
    ("m_WorldToClip", np.float32, (4, 4)), ("m_CameraDirection", np.float32, (3,)), ("m_ProbeRadius", np.float32), ("m_NearPlane", np.float32),
    ("pad", np.uint32, (3,))])
UncompressedRawVertexFormat = np.dtype([("m_Position", np.float32, (3,)), ("m_Normal", np.float32, (3,)), ("m_TexCoord", np.float32, (2,))])   # ShaderInterop.h:270-276
kUnitSphereVertices, kUnitSphereIndices = 91, 468
NodeLocalTransform = np.dtype([
    ("m_ParentNodeIdx", np.uint32), ("m_Position", np.float32, (3,)), ("m_Rotation", np.float32, (4,)),
    ("m_Scale", np.float32, (3,)), ("PAD0", np.uint32)])
TextureData = np.dtype([                                                                                                   # ShaderInterop.h:150-158
    ("m_GlobalIndex", np.uint32), ("m_IsWrapSampler", np.uint32), ("m_DescriptorIndex", np.uint32),
    ("m_FeedbackTextureDescriptorIndex", np.uint32), ("m_MinMapTextureDescriptorIndex", np.uint32)])
MaterialData = np.dtype([                                                                                                  # ShaderInterop.h:160-172
    ("m_ConstAlbedo", np.float32, (4,)), ("m_ConstEmissive", np.float32, (3,)), ("m_AlphaCutoff", np.float32),
    ("m_AlbedoTexture", TextureData), ("m_NormalTexture", TextureData), ("m_MetallicRoughnessTexture", TextureData),
    ("m_EmissiveTexture", TextureData), ("m_MaterialFlags", np.uint32), ("m_ConstRoughness", np.float32), ("m_ConstMetallic", np.float32)])
UpdateInstanceConstsPassConstants = np.dtype([("m_NumInstances", np.uint32)])
DeferredLightingConsts = np.dtype([                                                                                        # ShaderInterop.h:86-98
    ("m_ClipToWorld", np.float32, (4, 4)), ("m_CameraOrigin", np.float32, (3,)), ("m_SSAOEnabled", np.uint32), ("m_DebugMode", np.uint32),
    ("m_DirectionalLightVector", np.float32, (3,)), ("m_DirectionalLightStrength", np.float32), ("m_LightingOutputResolution", np.uint32, (2,)),
    ("m_bRTDDGIEnabled", np.uint32)])
GenerateLuminanceHistogramParameters = np.dtype([                                                                          # ShaderInterop.h:124-129
    ("m_SrcColorDims", np.uint32, (2,)), ("m_MinLogLuminance", np.float32), ("m_InverseLogLuminanceRange", np.float32)])
AdaptExposureParameters = np.dtype([                                                                                       # ShaderInterop.h:40-47
    ("m_MinLogLuminance", np.float32), ("m_LogLuminanceRange", np.float32), ("m_AdaptationSpeed", np.float32), ("m_NbPixels", np.uint32),
    ("m_MiddleGray", np.float32)])
PostProcessParameters = np.dtype([                                                                                         # ShaderInterop.h:234-241
    ("m_OutputDims", np.uint32, (2,)), ("m_ManualExposure", np.float32), ("m_MiddleGray", np.float32), ("m_WhitePoint", np.float32),
    ("m_BloomStrength", np.float32)])
BloomConsts = np.dtype([("m_InvSourceResolution", np.float32, (2,)), ("m_FilterRadius", np.float32), ("m_bIsFirstDownsample", np.uint32)])   # ShaderInterop.h:79-84
TAAConsts = np.dtype([("m_OutputDims", np.uint32, (2,)), ("m_JitterDelta", np.float32, (2,)), ("m_MinBlend", np.float32), ("m_MaxSampleCount", np.float32),   # the project's own (csrc/k_taa.hip)
                      ("m_bResetHistory", np.uint32), ("PAD0", np.uint32)])
HosekWilkieSkyParameters = np.dtype([("m_Params", np.float32, (10, 4))])                                                    # ShaderInterop.h:146-149
SkyPassParameters = np.dtype([                                                                                             # ShaderInterop.h:297-305
    ("m_ClipToWorld", np.float32, (4, 4)), ("m_SunLightDir", np.float32, (3,)), ("PAD0", np.uint32), ("m_CameraPosition", np.float32, (3,)),
    ("PAD1", np.uint32), ("m_HosekParams", HosekWilkieSkyParameters)])
GTAOConstants = np.dtype([                                                                                                 # extern/xegtao/XeGTAO.h:59-83
    ("ViewportSize", np.int32, (2,)), ("ViewportPixelSize", np.float32, (2,)), ("DepthUnpackConsts", np.float32, (2,)),
    ("CameraTanHalfFOV", np.float32, (2,)), ("NDCToViewMul", np.float32, (2,)), ("NDCToViewAdd", np.float32, (2,)),
    ("NDCToViewMul_x_PixelSize", np.float32, (2,)), ("EffectRadius", np.float32), ("EffectFalloffRange", np.float32),
    ("RadiusMultiplier", np.float32), ("Padding0", np.float32), ("FinalValuePower", np.float32), ("DenoiseBlurBeta", np.float32),
    ("SampleDistributionPower", np.float32), ("ThinOccluderCompensation", np.float32), ("DepthMIPSamplingOffset", np.float32),
    ("NoiseIndex", np.int32)])
XeGTAOMainPassConstantBuffer = np.dtype([("m_WorldToViewNoTranslate", np.float32, (4, 4)), ("m_Quality", np.uint32)])          # ShaderInterop.h:322-326
XeGTAODenoiseConstants = np.dtype([("m_FinalApply", np.uint32)])                                                             # ShaderInterop.h:328-331
ShadowMaskConsts = np.dtype([                                                                                              # ShaderInterop.h:285-295
    ("m_ClipToWorld", np.float32, (4, 4)), ("m_DirectionalLightDirection", np.float32, (3,)), ("m_NoisePhase", np.float32),
    ("m_CameraPosition", np.float32, (3,)), ("m_TanSunAngularRadius", np.float32), ("m_OutputResolution", np.uint32, (2,)),
    ("m_bDoDenoising", np.uint32), ("m_RayStartOffset", np.float32)])
PackNormalAndRoughnessConsts = np.dtype([("m_OutputResolution", np.uint32, (2,))])                                        # ShaderInterop.h:229-232
SigmaConsts = np.dtype([                                                                                                   # the project's own (csrc/k_sigma.hip)
    ("m_ClipToWorld", np.float32, (4, 4)), ("m_OutputDims", np.uint32, (2,)), ("m_JitterDelta", np.float32, (2,)), ("m_PixelUnproject", np.float32),
    ("m_DenoisingRange", np.float32), ("m_PlaneDistanceSensitivity", np.float32), ("m_StabilizationStrength", np.float32), ("m_SigmaScale", np.float32),
    ("m_FrameIndex", np.uint32), ("m_Pass", np.uint32), ("m_bResetHistory", np.uint32)])
# this build's acceleration structure (include/trhip.h, "acceleration structure")
RefitTLASConstants = np.dtype([("m_NumInstances", np.uint32), ("m_NumNodes", np.uint32), ("m_NumLevels", np.uint32)])
AccelNode = np.dtype([("lo", np.float32, (3,)), ("skip", np.uint32), ("hi", np.float32, (3,)), ("leaf", np.uint32)])
BLASHeader = np.dtype([("node_offset", np.uint32), ("num_nodes", np.uint32), ("tri_offset", np.uint32), ("num_tris", np.uint32)])
TLASInstance = np.dtype([("object_from_world", np.float32, (4, 3)), ("flags", np.uint32), ("leaf_node", np.uint32), ("reserved", np.uint32, (2,))])
kAccelInner = 0xFFFFFFFF
kTLASInstanceForceOpaque, kTLASInstanceForceNonOpaque = 1, 2
kBlueNoiseSize = 128
kDeferredLightingDebugMode_ShadowMask = 11
# csrc/ShaderInterop.h: the project's own 64-byte DDGI volume descriptor ("deferredlighting_PS_Main" t5)
DDGIVolumeDesc = np.dtype([("origin", np.float32, (3,)), ("probeNormalBias", np.float32), ("probeSpacing", np.float32, (3,)), ("probeViewBias", np.float32),
                           ("probeCounts", np.int32, (3,)), ("probeIrradianceEncodingGamma", np.float32), ("numIrradianceInteriorTexels", np.uint32),
                           ("numDistanceInteriorTexels", np.uint32), ("flags", np.uint32), ("pad", np.uint32)])
kDDGIFlag_Relocation, kDDGIFlag_Classification, kDDGIFlag_Variability = 1, 2, 4
kDDGIIrradianceInteriorTexels, kDDGIDistanceInteriorTexels, kDDGIMaxProbeCount = 6, 14, 1024
# csrc/ShaderInterop.h: the project's own b0 of the probe trace and the two probe blends; the DDGIVolumeDesc follows it in b0
DDGIUpdateConsts = np.dtype([("m_DirectionalLightVector", np.float32, (3,)), ("m_DirectionalLightStrength", np.float32), ("rayRotation", np.float32, (3, 4)),
                             ("probeMaxRayDistance", np.float32), ("probeHysteresis", np.float32), ("probeDistanceExponent", np.float32),
                             ("probeIrradianceThreshold", np.float32), ("probeBrightnessThreshold", np.float32), ("probeMinFrontfaceDistance", np.float32),
                             ("probeFixedRayBackfaceThreshold", np.float32), ("pad", np.uint32)])
kDDGIRaysPerProbe, kDDGIBackfaceRayLimit, kDDGIFixedRays = 256, 25, 32
# csrc/ShaderInterop.h: the SDK's DDGIRootConstants, push constants of the two reduction passes (csrc/k_ddgireduction.hip)
DDGIRootConstants = np.dtype([("volumeIndex", np.uint32), ("volumeConstantsIndex", np.uint32), ("volumeResourceIndicesIndex", np.uint32),
                              ("reductionInputSizeX", np.uint32), ("reductionInputSizeY", np.uint32), ("reductionInputSizeZ", np.uint32)])
kDDGIMinimumVariabilitySamples = 16
kDDGIReductionGroup = (16, 16, 4)                 # inputs per workgroup: 4 x 8 x 4 threads of 4 x 2 inputs each

SIZES = {
    "BasePassInstanceConstants": 144, "MeshLODData": 16, "MeshData": 156, "MeshletData": 32,
    "MeshletAmplificationData": 12, "DispatchIndirectArguments": 12, "GPUCullingPassConstants": 180,
    "BasePassConstants": 256, "MinMaxDownsampleConsts": 12, "NodeLocalTransform": 48,
    "TextureData": 20, "MaterialData": 124, "DeferredLightingConsts": 112,
    "GenerateLuminanceHistogramParameters": 16, "AdaptExposureParameters": 20, "PostProcessParameters": 24,
    "BloomConsts": 16, "TAAConsts": 32, "HosekWilkieSkyParameters": 160, "SkyPassParameters": 256,
    "GTAOConstants": 96, "XeGTAOMainPassConstantBuffer": 68, "XeGTAODenoiseConstants": 4,
    "ShadowMaskConsts": 112, "PackNormalAndRoughnessConsts": 8, "SigmaConsts": 112, "DDGIVolumeDesc": 64, "DDGIUpdateConsts": 96, "DDGIRootConstants": 24, "GIProbeVisualizationConsts": 96, "UncompressedRawVertexFormat": 32, "RefitTLASConstants": 12, "AccelNode": 32, "BLASHeader": 16, "TLASInstance": 64,
}
for _n, _s in SIZES.items():
    assert globals()[_n].itemsize == _s, (_n, globals()[_n].itemsize, _s)


RawVertexFormat = np.dtype([("m_Position", np.float32, (3,)), ("m_PackedNormal", np.uint32), ("m_TexCoord", np.uint16, (2,))])   # ShaderInterop.h:278-283
assert RawVertexFormat.itemsize == 20


def world_to_clip(world_to_view, view_to_clip) -> np.ndarray:
    """m_WorldToClip = WorldToView * ViewToClip in float32, summed left to right without fused multiply-add: the
    one definition used by every host side of this repo (Python and csrc/host/MathUtilities), so that the oracle
    and the GPU are handed the same 16 numbers."""
    a = np.asarray(world_to_view, np.float32).reshape(4, 4)
    b = np.asarray(view_to_clip, np.float32).reshape(4, 4)
    out = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            acc = np.float32(a[i, 0] * b[0, j])
            for k_ in (1, 2, 3):
                acc = np.float32(acc + np.float32(a[i, k_] * b[k_, j]))
            out[i, j] = acc
    return out


def clip_to_world(world_to_view, view_to_clip) -> np.ndarray:
    """m_ClipToWorld: the inverse of WorldToView * ViewToClip in float64, every element rounded once to float32 (the reference
    uses DirectXMath's float32 inverse, absent here).  The operation order is part of the definition and is the one of
    csrc/host/MathUtilities.cpp InverseOfProduct, so that both host sides hand the GPU the same 16 numbers: the product summed
    left to right, cofactors as 3x3 determinants, the determinant along row 0, cofactor / determinant + 0.0.  A camera's
    structural zeros come out as exact zeros (a LAPACK inverse leaves 1e-17 there)."""
    a = np.asarray(world_to_view, np.float32).reshape(4, 4).astype(np.float64)
    b = np.asarray(view_to_clip, np.float32).reshape(4, 4).astype(np.float64)
    m = [[((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) + a[i, 3] * b[3, j] for j in range(4)] for i in range(4)]
    cof = [[None] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            r, c = [k for k in range(4) if k != i], [k for k in range(4) if k != j]
            e = lambda y, x: m[r[y]][c[x]]                                                          # noqa: E731
            d = (e(0, 0) * (e(1, 1) * e(2, 2) - e(1, 2) * e(2, 1)) - e(0, 1) * (e(1, 0) * e(2, 2) - e(1, 2) * e(2, 0))) + e(0, 2) * (e(1, 0) * e(2, 1) - e(1, 1) * e(2, 0))
            cof[i][j] = -d if (i + j) & 1 else d
    det = ((m[0][0] * cof[0][0] + m[0][1] * cof[0][1]) + m[0][2] * cof[0][2]) + m[0][3] * cof[0][3]
    out = np.zeros((4, 4), np.float32)
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                out[j, i] = np.float32(cof[i][j] / det + np.float64(0.0))
    return out


def log_luminance_range(min_luminance, max_luminance):
    """(minLogLum, maxLogLum) of AdaptLuminanceRenderer.cpp:155-156: log2 of the float32 luminance in float64, rounded once to
    float32.  One definition for both host sides (csrc/host does the same two operations), so that the GPU is handed the same
    words.  The pass constants derived from them are float32 operations: range = max - min, inverse = 1.0f / range."""
    import math
    lo = np.float32(math.log2(float(np.float32(min_luminance))))
    hi = np.float32(math.log2(float(np.float32(max_luminance))))
    return lo, hi


def get_next_pow2(x: int) -> int:
    """MathUtilities.h:47-61"""
    if x == 0:
        return 1
    x -= 1
    for s in (1, 2, 4, 8, 16):
        x |= x >> s
    return (x + 1) & 0xFFFFFFFF


def compute_nb_mips(w: int, h: int) -> int:
    """Graphic.h:227-231 (std::bit_width of the larger dimension)"""
    return int(max(w, h)).bit_length()


def hzb_dims(render_w: int, render_h: int):
    """BasePassRenderers.cpp:601-602"""
    return get_next_pow2(render_w) >> 1, get_next_pow2(render_h) >> 1


def groups8(w: int, h: int):
    """The group counts of a dispatch of 8 x 8 threads per group over w x h texels."""
    return (w + 7) // 8, (h + 7) // 8, 1


def hzb_layout(w: int, h: int):
    """Linear R16F mip chain used on the HIP side and by the oracle: mip k = max(w>>k,1) x
    max(h>>k,1) texels, row-major, mips packed back to back.  Returns (mips, offsets, total)."""
    mips = compute_nb_mips(w, h)
    offs, off = [], 0
    for k in range(mips):
        offs.append(off)
        off += max(w >> k, 1) * max(h >> k, 1)
    return mips, offs, off


def fmaf(a, b, c) -> np.float32:
    """Exact scalar float32 fused multiply-add (std::fmaf): the product is exact in float64, the
    float64 sum is rounded to odd, then rounded once to float32."""
    a, b, c = np.float64(np.float32(a)), np.float64(np.float32(b)), np.float64(np.float32(c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    if err != 0 and np.isfinite(s) and (np.float64(s).view(np.int64) & 1) == 0:
        s = np.nextafter(s, np.inf if err > 0 else -np.inf)
    return np.float32(s)


def srgb_to_linear(c):
    """The sRGB transfer function (float64): what SRGBA8_UNORM texels are decoded with (rhi.srgb_table rounds it to float)."""
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def linear_to_srgb(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.0031308, x * 12.92, 1.055 * np.maximum(x, 0.0) ** (1.0 / 2.4) - 0.055)


def make_mips(image, srgb: bool, levels: int | None = None):
    """The mip chain of a uint8 [h, w, 4] image, level k of max(w >> k, 1) x max(h >> k, 1) texels (the back end's rule), down to
    1 x 1 or `levels` levels: a 2 x 2 box in linear light, in float64, rounded once per level (half to even).  Texel (x, y) of a
    level averages columns 2x and min(2x + 1, w - 1) and rows 2y and min(2y + 1, h - 1) of the level above, itself kept in
    float64 (an odd last column or row is dropped, a 1-texel axis is repeated).  srgb: R, G and B are decoded with the sRGB
    transfer function before the box and encoded after it; alpha is linear.  The reference ships its mips inside its DDS
    files; an application with its own mips passes them instead."""
    img = np.ascontiguousarray(image, np.uint8)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("image: uint8 [h, w, 4]")
    lin = img.astype(np.float64) / 255.0
    if srgb:
        lin[..., :3] = srgb_to_linear(lin[..., :3])
    out = [img.copy()]
    while (lin.shape[0] > 1 or lin.shape[1] > 1) and (levels is None or len(out) < levels):
        h, w = lin.shape[:2]
        nh, nw = max(h >> 1, 1), max(w >> 1, 1)
        y0, x0 = 2 * np.arange(nh), 2 * np.arange(nw)
        y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
        lin = ((lin[y0][:, x0] + lin[y0][:, x1]) + (lin[y1][:, x0] + lin[y1][:, x1])) * 0.25
        enc = lin.copy()
        if srgb:
            enc[..., :3] = linear_to_srgb(enc[..., :3])
        out.append(np.rint(np.clip(enc, 0.0, 1.0) * 255.0).astype(np.uint8))
    return out


# ----------------------------------------------------------------------------------------------- block-compressed textures
_FORMAT_RGBA8_UNORM, _FORMAT_SRGBA8_UNORM = 10, 11            # rhi.FORMAT_*
_BC1, _BC1_SRGB, _BC2, _BC2_SRGB, _BC3, _BC3_SRGB, _BC4, _BC5 = range(14, 22)
_BC_BLOCK_BYTES = {_BC1: 8, _BC1_SRGB: 8, _BC2: 16, _BC2_SRGB: 16, _BC3: 16, _BC3_SRGB: 16, _BC4: 8, _BC5: 16}


class BlockMips(list):
    """The mip chain of a block-compressed texture: a list of the levels' raw block bytes (bytes or uint8 arrays; level k holds
    ceil(w_k / 4) x ceil(h_k / 4) blocks, row-major, w_k = max(width >> k, 1)) that also carries the size of level 0 in texels,
    which the bytes alone do not tell.  What rhi.Device.create_sampled_texture, GpuScene.set_textures and
    host.Renderer.load_textures take as `mips` for one of rhi.BC_FORMATS.  There is no encoder: the blocks come from parse_dds
    or from another tool."""
    def __init__(self, levels, width: int, height: int):
        super().__init__(levels)
        self.width, self.height = int(width), int(height)
        if self.width < 1 or self.height < 1 or len(self) == 0:
            raise ValueError("BlockMips: at least one level, width and height >= 1")


def bc_level_bytes(w: int, h: int, fmt: int, level: int = 0) -> int:
    """Bytes of level `level` of a w x h texture of a block-compressed format."""
    mw, mh = max(w >> level, 1), max(h >> level, 1)
    return ((mw + 3) // 4) * ((mh + 3) // 4) * _BC_BLOCK_BYTES[fmt]


def _bc_colour(blk, bc1: bool):
    """uint8 [n, 8] colour blocks -> uint8 [n, 16, 4]."""
    b = blk.astype(np.uint32)
    c0, c1 = b[:, 0] | b[:, 1] << 8, b[:, 2] | b[:, 3] << 8
    idx = b[:, 4] | b[:, 5] << 8 | b[:, 6] << 16 | b[:, 7] << 24
    k = (idx[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3

    def ends(c):
        r, g, bl = c >> 11, (c >> 5) & 63, c & 31
        return np.stack([r << 3 | r >> 2, g << 2 | g >> 4, bl << 3 | bl >> 2], 1)
    p0, p1 = ends(c0), ends(c1)
    four = ((c0 > c1) | (not bc1))[:, None]
    pal = np.zeros((len(b), 4, 4), np.uint32)
    pal[:, 0, :3], pal[:, 1, :3] = p0, p1
    pal[:, 2, :3] = np.where(four, (2 * p0 + p1) // 3, (p0 + p1) // 2)
    pal[:, 3, :3] = np.where(four, (p0 + 2 * p1) // 3, 0)
    pal[:, :3, 3] = 255
    pal[:, 3, 3] = np.where(four[:, 0], 255, 0)
    return np.take_along_axis(pal, np.broadcast_to(k[:, :, None], (len(b), 16, 4)), 1).astype(np.uint8)


def _bc_alpha(blk):
    """uint8 [n, 8] alpha blocks -> uint8 [n, 16]."""
    b = blk.astype(np.uint64)
    a0, a1 = b[:, 0].astype(np.uint32), b[:, 1].astype(np.uint32)
    bits = sum(b[:, 2 + j] << np.uint64(8 * j) for j in range(6))
    k = ((bits[:, None] >> (3 * np.arange(16, dtype=np.uint64))[None, :]) & np.uint64(7)).astype(np.intp)
    pal = np.zeros((len(b), 8), np.uint32)
    pal[:, 0], pal[:, 1] = a0, a1
    eight = a0 > a1
    for j in range(2, 8):
        short = ((6 - j) * a0 + (j - 1) * a1) // 5 if j < 6 else np.full(len(b), 0 if j == 6 else 255, np.uint32)
        pal[:, j] = np.where(eight, ((8 - j) * a0 + (j - 1) * a1) // 7, short)
    return np.take_along_axis(pal, k, 1).astype(np.uint8)


def bc_decode(blocks, w: int, h: int, fmt: int) -> np.ndarray:
    """uint8 [h, w, 4] (R, G, B, A) of one level of a block-compressed texture: `blocks` are its ceil(w / 4) x ceil(h / 4) blocks,
    row-major (bytes or a uint8 array), fmt one of rhi.BC_FORMATS (a _SRGB variant decodes to the same bytes as its UNORM twin).
    A vectorised statement of the decode csrc/material_textures.hip.h performs per texel (integer, truncating divisions; BC4 gives
    (R, 0, 0, 255), BC5 (R, G, 0, 255)), for viewing and for tools/material_texture_cost.py: the product samples the blocks on the
    GPU and has no CPU fallback.  There is no encoder."""
    if fmt not in _BC_BLOCK_BYTES:
        raise ValueError(f"bc_decode: format {fmt} is not block-compressed")
    nb = _BC_BLOCK_BYTES[fmt]
    bw, bh = (w + 3) // 4, (h + 3) // 4
    raw = np.frombuffer(blocks, np.uint8) if isinstance(blocks, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blocks, np.uint8).reshape(-1)
    if w < 1 or h < 1 or raw.size != bw * bh * nb:
        raise ValueError(f"bc_decode: {w} x {h} texels of format {fmt} are {bw * bh * nb} bytes, got {raw.size}")
    blk = raw.reshape(bw * bh, nb)
    out = np.zeros((bw * bh, 16, 4), np.uint8)
    out[..., 3] = 255
    if fmt in (_BC1, _BC1_SRGB):
        out = _bc_colour(blk, True)
    elif fmt in (_BC2, _BC2_SRGB, _BC3, _BC3_SRGB):
        out = _bc_colour(blk[:, 8:], False)
        if fmt in (_BC2, _BC2_SRGB):
            nib = np.stack([blk[:, :8] & 15, blk[:, :8] >> 4], 2).reshape(-1, 16)
            out[..., 3] = nib * 17
        else:
            out[..., 3] = _bc_alpha(blk[:, :8])
    else:
        out[..., 0] = _bc_alpha(blk[:, :8])
        if fmt == _BC5:
            out[..., 1] = _bc_alpha(blk[:, 8:])
    img = out.reshape(bh, bw, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(bh * 4, bw * 4, 4)
    return np.ascontiguousarray(img[:h, :w])


def bc_decode_mips(mips: BlockMips, fmt: int):
    """The decoded twin of a BlockMips: its levels as uint8 [h_k, w_k, 4] arrays (bc_decode per level)."""
    return [bc_decode(m, max(mips.width >> k, 1), max(mips.height >> k, 1), fmt) for k, m in enumerate(mips)]


def parse_dds(data):
    """(mips, format, width, height) of the bytes of a .dds file, through trhip_dds_parse (include/trhip.h: what is accepted and
    refused; raises rhi.TrhipError with the parser's message).  format is the rhi.FORMAT_* the file states; the sRGB choice by
    material slot is the loader's (gltf_lite.load, trhost_create_material_texture_dds).  mips: a BlockMips of the levels' block
    bytes for a block-compressed format, uint8 [h_k, w_k, 4] arrays for RGBA8.  Nothing is decoded or encoded here."""
    from . import rhi
    data = bytes(data)
    info = rhi.dds_parse(data)
    levels = [data[int(info.levelOffset[k]):int(info.levelOffset[k]) + int(info.levelBytes[k])] for k in range(info.mipLevels)]
    w, h, fmt = int(info.width), int(info.height), int(info.format)
    if fmt in _BC_BLOCK_BYTES:
        return BlockMips(levels, w, h), fmt, w, h
    mips = [np.frombuffer(m, np.uint8).reshape(max(h >> k, 1), max(w >> k, 1), 4).copy() for k, m in enumerate(levels)]
    return mips, fmt, w, h


def srgb_variant(fmt: int, srgb: bool) -> int:
    """The format of the pair (RGBA8, BC1, BC2, BC3: UNORM / _SRGB) that a material slot wants; BC4 and BC5 have one form."""
    if fmt in (_FORMAT_RGBA8_UNORM, _FORMAT_SRGBA8_UNORM) or _BC1 <= fmt <= _BC3_SRGB:
        return ((fmt - _FORMAT_RGBA8_UNORM) & ~1) + _FORMAT_RGBA8_UNORM + int(bool(srgb))
    return fmt
