// VisibilityOutputs.h -- where a consumer (software rasteriser, multi-GPU gather, tests) finds the
// buffers the last recorded frame's cull passes wrote.  New in this build: in the reference the
// mesh-shader stage consumes the amplification payload on chip and nothing is exposed.
#pragma once

#include "nvrhi_lite.h"

struct VisibilityPassBuffers
{
    bool m_bRan = false;
    nvrhi::BufferHandle m_MeshletAmplificationDataBuffer;   // MeshletAmplificationData[G]
    nvrhi::BufferHandle m_MeshletDispatchArgumentsBuffer;   // {G,1,1, validRecords}
    nvrhi::BufferHandle m_MeshletVisibilityMaskBuffer;      // uint32 per group: lane-visibility ballot
    nvrhi::BufferHandle m_VisibleMeshletListBuffer;         // (g << 5) | lane, canonical order
    nvrhi::BufferHandle m_VisibleMeshletDrawArgsBuffer;     // {numVisible,1,1}
    nvrhi::BufferHandle m_LateCullInstanceCountBuffer, m_LateCullDispatchIndirectArgsBuffer;
};

// slot: 0 early-opaque, 1 late-opaque, 2 early-alpha-mask, 3 late-alpha-mask
bool GetVisibilityPassBuffers(uint32_t slot, VisibilityPassBuffers* out);
void ReleaseVisibilityPassBuffers();

// Multi-GPU (instance list sharded over ranks; trhost.h trhost_set_shard_late_exchange): called while
// the frame is submitted: after each early instance cull (phase 0) and before each late one (phase 1).
using ShardLateFn = void (*)(void* user, void* hipStream, void* lateCount, void* shardInfo, int bucket, int phase);
// listPresenceMask: bit 0 = some rank holds opaque ids, bit 1 = some rank holds alpha-mask ids (0: this rank's own lists);
// every rank posts the in-frame collective of exactly those buckets.  depthFn (may be null): element-wise MAX of the depth
// words over all ranks, enqueued on hipStream -- required when the frame rasterises its own depth (m_bRasterDepth).
using ShardDepthFn = int (*)(void* user, void* depthWords, uint64_t countWords, void* hipStream);
void SetShardLateExchange(ShardLateFn fn, void* user, uint32_t listPresenceMask = 0, ShardDepthFn depthFn = nullptr, void* depthUser = nullptr);

// Outputs of the last GI probe culling dispatch (GIRenderer.cpp; false before the first one).
bool GetGIProbeCullBuffers(nvrhi::BufferHandle* positions, nvrhi::BufferHandle* drawArgs, nvrhi::BufferHandle* instanceToProbe);
void ReleaseGIProbeCullBuffers();

// Depth attachment of the last recorded base pass (read-back for tests; null before the first frame).
nvrhi::TextureHandle GetLastDepthBuffer();
// GBufferRenderer's visibility buffer (RG32_UINT) and motion target (RG16_FLOAT); null until a frame ran with them on.
nvrhi::TextureHandle GetVisibilityBuffer();
nvrhi::TextureHandle GetMotionBuffer();
// GBufferRenderer's GBufferA (RGBA32_UINT); null until a frame ran with the G-buffer on.
nvrhi::TextureHandle GetGBufferA();
// Creates GBufferRenderer's per-pixel targets that the scene's flags ask for and that do not exist yet (Setup phase only).
void CreateGBufferPixelTargets();
// DeferredLightingRenderer's LightingOutput (R11G11B10_FLOAT) and the DeferredLightingConsts of the last recorded frame; null /
// false until a frame ran with deferred lighting on.
nvrhi::TextureHandle GetLightingOutput();
bool GetLastDeferredLightingConsts(void* out112);
void ReleaseDeferredLightingOutputs();

// PostProcessRenderer's back buffer (RGBA8_UNORM), AdaptLuminanceRenderer's histogram and the three parameter structs of the last
// recorded frame (adaptRan: the two adapt dispatches were recorded, i.e. no manual exposure); null / false until a frame ran
// with post-processing on.  ResetExposure writes 1.0 into the luminance buffer and the exposure texel (kInitialExposure).
nvrhi::TextureHandle GetBackBuffer();
bool GetLastPostProcessConsts(void* histogram16, void* adapt20, void* post24, int* adaptRan);
void ResetExposure();
void ReleasePostProcessOutputs();
// BloomRenderer's texture (R11G11B10_FLOAT, Scene::m_NbBloomMips mips) and the BloomConsts of pass `pass` of the last recorded
// frame (downsamples first); null / false until a frame ran with bloom generation on.
nvrhi::TextureHandle GetGeneratedBloomTexture();
bool GetLastBloomConsts(uint32_t pass, void* out16);
void ReleaseBloomOutputs();
// TAARenderer: g_AntiAliasedLightingOutput of the last frame and the history texture it wrote (null if the resolve did not run in it),
// the output the frame being set up will write (null if TAA is off), the TAAConsts the last frame ran with and View's jitter offsets.
nvrhi::TextureHandle GetAntiAliasedLightingOutput();
nvrhi::TextureHandle GetScheduledAntiAliasedLightingOutput();
nvrhi::TextureHandle GetTAAHistory();
bool GetLastTAAConsts(void* out32, float* currentJitter2, float* prevJitter2);
void ReleaseTAAOutputs();
// AmbientOcclusionRenderer: the SSAO texture of the last frame (null if the pass did not run in it), the one the frame being set
// up will write (null if the pass is not scheduled in it), and the GTAOConstants the last frame uploaded.
nvrhi::TextureHandle GetSSAOTexture();
nvrhi::TextureHandle GetScheduledSSAOTexture();
bool GetLastGTAOConsts(void* out96);
void ReleaseAmbientOcclusionOutputs();
// ShadowMaskRenderer: the mask of the last frame (null if the pass did not run in it), the one the frame being set up will write
// (null if the pass is not scheduled in it), and the ShadowMaskConsts the last frame uploaded.
nvrhi::TextureHandle GetShadowMaskTexture();
nvrhi::TextureHandle GetScheduledShadowMaskTexture();
bool GetLastShadowMaskConsts(void* out112);
// the shadow denoiser's outputs of the last frame (which 0: the penumbra texture, 1: the tiles, 2: the history written) and its
// SigmaConsts (m_Pass 0); null / false if it did not run
nvrhi::TextureHandle GetShadowDenoiserTexture(int which);
bool GetLastSigmaConsts(void* out112);
void ReleaseShadowMaskOutputs();
// the TLAS refit, recorded by the structure's first consumer in a frame (ShadowMaskRenderer.cpp)
void RecordRefitTLAS(nvrhi::CommandListHandle commandList);
// GIRenderer: the 96 bytes of DDGIUpdateConsts the last frame's probe update ran with (false if it did not run in it)
bool GetLastDDGIUpdateConsts(void* out96);
bool GetLastDDGIProbeVisualizationConsts(void* out96);   // GIDebugRenderer: the 96-byte GIProbeVisualizationConsts of the last frame's draw
// The SkyPassParameters SkyRenderer uploaded in the last frame; false if the pass did not run in it.
bool GetLastSkyConsts(void* out256);
void ReleaseSkyOutputs();
// the base pass's pipeline statistics: the value its frame N showed (the query of frame N - 2) and the last executed frame's (waits)
void GetBasePassPipelineStatistics(nvrhi::PipelineStatistics* lastShown, nvrhi::PipelineStatistics* latest);

// Native per-frame driver of the multi-GPU exchange (ShardExchange.cpp; C facade in trhost.h).
struct trhost_exchange_desc;
void ShardExchangeCreate(const trhost_exchange_desc& desc);
void ShardExchangeRun();
void ShardExchangeWait();
void ShardExchangeOutputs(uint32_t slot, void** records, void** masks, void** list, void** args);
void ShardExchangeDestroy();
