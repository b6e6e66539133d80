/*
 * trhip.h -- C ABI of the MI355X (gfx950 / HIP) compute back end that replaces the NVRHI/D3D12
 * compute dispatch under ToyRenderer's GPU-driven visibility path.
 *
 * Plain C: opaque handles, plain pointers and sizes, int status returns (0 = ok, <0 = error,
 * text via trhip_last_error()).  No torch / C++ types cross this boundary.  The reference never
 * returns errors (everything asserts: PCH.h:42 check(), GraphicRHI.cpp:18-38); the C++ wrapper
 * above this ABI (toyrenderer_amd/csrc/host) re-creates the assert-on-failure behaviour.
 *
 * Each entry point cites the reference interface it replaces (paths relative to
 * /root/reference/source; nvrhi = the renderer's RHI, used by the reference as cited).
 *
 * Threading: distinct command lists may be recorded concurrently from
 * different threads; trhip_queue_execute is called from one thread at a time.  Nothing is
 * enqueued on the HIP stream before trhip_queue_execute (Graphic.cpp:786-830).
 */
#ifndef TRHIP_H_
#define TRHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRHIP_ABI_VERSION 1

typedef struct trhip_device_t*  trhip_device;
typedef struct trhip_heap_t*    trhip_heap;
typedef struct trhip_buffer_t*  trhip_buffer;
typedef struct trhip_texture_t* trhip_texture;
typedef struct trhip_cmdlist_t* trhip_cmdlist;
typedef struct trhip_timer_t*   trhip_timer;
typedef struct trhip_pipeline_stats_t* trhip_pipeline_stats;
typedef struct trhip_texture_table_t* trhip_texture_table;
typedef struct trhip_readback_t* trhip_readback;

enum {
    TRHIP_OK = 0,
    TRHIP_ERR_INVALID = -1,      /* bad argument / binding / shape                       */
    TRHIP_ERR_HIP = -2,          /* a HIP runtime call failed                            */
    TRHIP_ERR_UNKNOWN_SHADER = -3,
    TRHIP_ERR_STATE = -4,        /* e.g. recording into a closed command list            */
    TRHIP_ERR_NO_DEVICE = -5
};

/* nvrhi::Format subset used on the path (GraphicConstants.h:25-28).  RG32_UINT (the visibility buffer: each texel one
 * little-endian u64), RG16_FLOAT (the motion target, GBufferMotion) and RGBA32_UINT (GBufferA, GraphicConstants.h:24: 16 bytes per
 * texel, little-endian words x, y, z, w) have one mip only.  So do the deferred lighting pass's formats (with one exception: an
 * R11G11B10_FLOAT texture created as a render target, isUAV & TRHIP_TEXTURE_RENDER_TARGET, may have a mip chain: the bloom
 * texture of BloomRenderer.cpp:41-50, whose mips "bloom_PS_Downsample" / "bloom_PS_Upsample" write): R11G11B10_FLOAT
 * (LightingOutput, GraphicConstants::kLightingOutputFormat: 4 bytes per texel, R in bits 0-10, G in bits 11-21, B in bits 22-31;
 * unsigned floats of 5 exponent bits with 6, 6 and 5 mantissa bits), R8_UNORM (the shadow mask) and R8_UINT (the SSAO texture),
 * one byte per texel each.  RGBA8_UNORM (the back buffer, GraphicRHI.cpp:214: 4 bytes per texel, R in the low byte, one mip) is
 * created, uploaded, downloaded and copied; both clears refuse it, because "postprocess_PS_PostProcess" writes every texel.
 * Its value is 10, not 9: 9 is not a format and stays refused with "unsupported format".
 * SRGBA8_UNORM (11) has RGBA8_UNORM's layout; a sampling pass decodes R, G and B through the sRGB transfer function before
 * filtering (trhip_srgb_table), alpha stays linear.  An RGBA8_UNORM or SRGBA8_UNORM texture created WITHOUT the UAV and
 * render-target bits (isUAV == 0: a material texture, sampled only) may have a mip chain, uploaded per mip through
 * trhip_texture_upload; one that a pass writes keeps one mip.
 * R10G10B10A2_UNORM (12: the DDGI probe irradiance; 4 bytes per texel, R in bits 0-9, G in bits 10-19, B in bits 20-29, A in bits
 * 30-31) and RGBA16_FLOAT (13: the DDGI probe data; 8 bytes per texel, four binary16 x, y, z, w) have one mip; they are created,
 * uploaded and downloaded, and both clears refuse them.
 * BLOCK-COMPRESSED formats (14..21: BC1, BC2, BC3 with their _SRGB variants, BC4, BC5; all UNORM) are material textures only: created
 * with isUAV == 0, with up to a full mip chain, never as an array.  Level k of max(w >> k, 1) x max(h >> k, 1) texels is stored as
 * ceil(w_k / 4) x ceil(h_k / 4) blocks of trhip_format_block_bytes(format) bytes, row-major, at the 256-byte aligned offset
 * trhip_texture_mip_info answers; any width and height >= 1 are accepted, and the texels of an edge block beyond the level's size
 * are never read.  trhip_texture_upload / _download move the block bytes of one whole level.  Such a texture reaches a kernel
 * through the texture table only: both clears, a copy to a texture of another format and every Texture_SRV / Texture_UAV binding
 * refuse it.  A sampling pass decodes one texel per fetch, byte-exactly (csrc/material_textures.hip.h states the decode, DESIGN.md
 * 3 restates it); the _SRGB variants send the decoded R, G and B through trhip_srgb_table, alpha stays linear.  BC4 decodes to
 * (R, 0, 0, 255), BC5 to (R, G, 0, 255).  There is no encoder, and BC6H, BC7 and the SNORM variants are not supported. */
enum { TRHIP_FORMAT_R16_FLOAT = 1, TRHIP_FORMAT_R32_FLOAT = 2, TRHIP_FORMAT_RG32_UINT = 3, TRHIP_FORMAT_RG16_FLOAT = 4,
       TRHIP_FORMAT_RGBA32_UINT = 5, TRHIP_FORMAT_R11G11B10_FLOAT = 6, TRHIP_FORMAT_R8_UNORM = 7, TRHIP_FORMAT_R8_UINT = 8,
       TRHIP_SAMPLER_FEEDBACK_FORMAT = 9,   /* opaque: made by trhip_sampler_feedback_create only */
       TRHIP_FORMAT_RGBA8_UNORM = 10, TRHIP_FORMAT_SRGBA8_UNORM = 11, TRHIP_FORMAT_R10G10B10A2_UNORM = 12, TRHIP_FORMAT_RGBA16_FLOAT = 13,
       TRHIP_FORMAT_BC1_UNORM = 14, TRHIP_FORMAT_BC1_UNORM_SRGB = 15, TRHIP_FORMAT_BC2_UNORM = 16, TRHIP_FORMAT_BC2_UNORM_SRGB = 17,
       TRHIP_FORMAT_BC3_UNORM = 18, TRHIP_FORMAT_BC3_UNORM_SRGB = 19, TRHIP_FORMAT_BC4_UNORM = 20, TRHIP_FORMAT_BC5_UNORM = 21 };
/* Bytes of one 4 x 4 block: 8 (BC1, BC4) or 16 (BC2, BC3, BC5); 0 for every format that is not block-compressed.  No device needed. */
uint32_t    trhip_format_block_bytes(uint32_t format);

/* ---- error / introspection ---------------------------------------------------------------- */
const char* trhip_last_error(void);          /* thread-local text of the last failure          */
uint32_t    trhip_abi_version(void);
/* Kernel registry keyed by the reference's shader-name strings (Graphic.cpp:159-171,246,270-278;
 * ShadersToCompile.txt): "gpuculling_CS_GPUCulling LATE_CULL=0", "... LATE_CULL=1",
 * "gpuculling_CS_BuildLateCullIndirectArgs", "minmaxdownsample_CS_Main",
 * "ffx_spd_downsample_pass_CS FFX_SPD_OPTION_DOWNSAMPLE_FILTER=1|2",
 * "updateinstanceconsts_CS_UpdateInstanceConstsAndBuildTLAS", and the compute replacement of the
 * amplification shader: "basepass_AS_Main LATE_CULL=0|1" (alias "basepass_AS_Main_cull").
 * "basepass_MS_Main_depth" (basepass.hlsl:124-188 + raster + depth test, depth only): b0 BasePassConstants,
 * t0 instances, t1 vertices (RawVertexFormat, 20 B), t2 mesh data, t4 meshlets, t5 meshlet vertex ids,
 * t6 packed meshlet triangles, t7 amplification records, t9 visible list, u0 (texture) R32_FLOAT depth;
 * dispatched indirectly on the visible list's draw args.
 * "basepass_MS_Main_visibility": the same bindings, plus u1 (texture) RG32_UINT visibility buffer (render resolution, mip 0) and
 * push constants {uint32 passSlot} (0..3); each covered sample also max-merges (depthBits << 32) | passSlot << 30 |
 * listPosition << 7 | triangle into u1 (equal depth: the larger payload wins).  Visible-list capacity at most 2^23 entries.
 * "basepass_MS_Main_depth ALPHA_MASK_MODE=1" and "basepass_MS_Main_visibility ALPHA_MASK_MODE=1" (the permutation the reference
 * draws alpha-mask primitives with, BasePassRenderers.cpp:489; basepass.hlsl:210-215): the bindings of the plain shader, plus t3
 * MaterialData (124-byte stride, required) and t19 the texture table (TRHIP_BIND_TEXTURE_TABLE, optional).  A covered sample is
 * discarded iff m_ConstAlbedo.w, times the alpha of the albedo texture (sampled as the resolve samples it, derivatives from the
 * triangle's plane) when MaterialFlag_UseAlbedoTexture is set, is below m_AlphaCutoff; a NaN is kept.  Nothing of a triangle is
 * drawn when its m_MaterialDataIdx is past the buffer, or the flag is set and no table is bound, the descriptor index is past the
 * table, the entry is empty or of another format.  Refused at record time: t3 missing; a table that holds a texture created with
 * the UAV or render-target bit.  The convention is stated in csrc/k_raster.hip and tests/alpha_test_ref.c.
 * "basepass_PS_Main_motion" (basepass.hlsl:226-237, GBufferMotion): a direct dispatch of [numthreads(8, 8, 1)] groups over
 * the screen; b0 BasePassConstants (m_PrevWorldToClip set), t0 t1 t2 t4 t5 t6 as above, t10..t13 the four slots' records,
 * t14..t17 their visible lists, t18 (texture) the visibility buffer, u0 (texture) RG16_FLOAT motion target: the screen-space
 * motion to the previous frame, in pixels, of every pixel with a nonzero visibility texel (others are left as they are).
 * "basepass_PS_Main_GBuffer" (basepass.hlsl:231-253, both targets of the reference's pixel shader, texture-free materials):
 * dispatched as the motion shader, same bindings, plus t3 MaterialData (124-byte stride; the first 32 bytes are read, the
 * texture flags ignored), u0 (texture) RGBA32_UINT GBufferA and u1 (texture) the RG16_FLOAT motion target, both required.
 * Per pixel with a nonzero texel: u0 = PackGBuffer(albedo + debug byte by m_DebugMode 2 / 3 / 12, interpolated vertex
 * normal, emissive, roughness 1, metallic 0), u1 = the words "basepass_PS_Main_motion" writes.  A pixel whose chain of
 * indices leaves a bound buffer (m_MaterialDataIdx included) is left as it is in both targets.
 * With a texture table bound at t19 (TRHIP_BIND_TEXTURE_TABLE, the stand-in of ResourceDescriptorHeap[...]; optional) the same
 * shader name records the TEXTURED kernel ("basepass_PS_Main_GBuffer#textured" in the profile, "#main" without a table): all
 * 124 bytes of MaterialData are read, and each slot flagged in m_MaterialFlags (albedo, normal, metallic-roughness, emissive) is
 * sampled through its m_DescriptorIndex with the 16x anisotropic wrap or clamp sampler (m_IsWrapSampler) in software:
 * GetCommonGBufferParams (lightingcommon.hlsli:435-493) with derivatives from the triangle's plane, tangent-free normal mapping,
 * u0.w = PackRGBA8(roughness, metallic, 0, 0).  The convention is stated in csrc/material_textures.hip.h and
 * csrc/visibility_resolve.hip.h.  A flagged slot whose descriptor index is at or past the table's capacity, names an empty entry
 * or an entry of a format other than RGBA8_UNORM / SRGBA8_UNORM / the BC formats leaves the pixel as it is in both targets.  Refused at record
 * time: a table that holds a texture created with the UAV or render-target bit.
 * That check covers the table's contents when the dispatch is recorded: trhip_texture_table_set rewrites an entry in place, so a
 * UAV-capable texture set AFTERWARDS is sampled by the lists already recorded (read only; nothing is written through the table)
 * and is refused by the next recording.  A texture table bound to a shader other than this one, the two ALPHA_MASK_MODE=1 rasters
 * and "shadowmask_CS_ShadowMask", or at another slot, is refused.
 * "deferredlighting_PS_Main" and "deferredlighting_PS_Main_Debug" (deferredlighting.hlsl, DeferredLightingRenderer.cpp: the
 * directional light, the DDGI ambient term from a SUPPLIED probe volume, and the debug views): a direct dispatch of
 * [numthreads(8, 8, 1)] groups over the screen; b0 DeferredLightingConsts (112 bytes), t0 (texture) RGBA32_UINT
 * GBufferA, t1 RG16_FLOAT GBufferMotion (required by _Debug only), t2 R32_FLOAT depth, t3 R8_UINT SSAO (optional: unbound
 * reads 255), t4 R8_UNORM shadow mask (optional: unbound reads 1.0), u0 (texture) R11G11B10_FLOAT LightingOutput; every
 * texture of the size m_LightingOutputResolution; samplers are accepted and ignored.  A pixel is
 * written iff its depth is > 0.0f (the stand-in for the reference's stencil test on the opaque bit); every other texel of u0
 * keeps its value.  The arithmetic convention is stated in csrc/k_deferredlighting.hip.
 * DDGI (m_bRTDDGIEnabled != 0 in PS_Main: lighting += albedo / pi * irradiance, times ssao / 255 when m_SSAOEnabled; or
 * m_DebugMode 10 in _Debug: the irradiance itself): t5 a structured buffer of at least 64 bytes holding a DDGIVolumeDesc
 * (csrc/ShaderInterop.h: the project's own 64-byte descriptor, INTEGRATION.md names the SDK field behind each member), t6 the
 * probe data (RGBA16_FLOAT array, counts.x x counts.z, counts.y slices), t7 the probe irradiance (R10G10B10A2_UNORM array,
 * counts.x * 8 x counts.z * 8), t8 the probe distance (RG16_FLOAT array, counts.x * 16 x counts.z * 16), and b0 grows to 176
 * bytes: the DeferredLightingConsts followed by a HOST COPY of the descriptor.  The record function checks the host copy
 * (counts 1..1024, interior texel counts 6 and 14, spacing positive and finite, the three textures' formats, sizes and slice
 * counts); the kernel reads t5.  It is the caller's promise that the two agree; where they do not, every fetch still stays
 * inside the bound textures and the value is unspecified.  The query is csrc/ddgi_irradiance.hip.h's (tests/ddgi_ref.c).
 * With m_bRTDDGIEnabled == 0 and another mode, bindings at t5..t8 and a longer b0 are accepted and ignored.
 *
 * "giprobetrace_CS_ProbeTrace", "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=1" and "... =0"
 * (GIRenderer::RenderDDGI: the probe update that fills that volume; csrc/k_giprobetrace.hip, csrc/k_giprobeblend.hip, which state
 * the bindings and the arithmetic; tests/ddgi_update_ref.c is the definition).  b0 of all three: the 96-byte DDGIUpdateConsts
 * (csrc/ShaderInterop.h) with the DDGIVolumeDesc's host copy behind it, 160 bytes.  Trace: t0 the descriptor, t1..t3 the probe
 * textures, t4..t13 the scene and its acceleration structure, u0 a structured buffer float4[numProbes * 256] of ray records; a
 * direct dispatch of (4, counts.x * counts.z, counts.y) groups.  Blends: t1 the ray records, t3 the probe data, u1 the
 * irradiance (radiance blend) or u2 the distance (distance blend) array, created with the UAV bit; (counts.x, counts.z,
 * counts.y) groups.  An array texture is accepted only at a binding that a pass declares, in the declared format.
 * With the descriptor's flags bit 2 (kDDGIFlag_Variability) the radiance blend also writes u4, a structured buffer
 * float[counts.y][6 * counts.z][6 * counts.x] of probe variability (a coefficient of variation per interior texel), and
 * "ReductionCS_DDGIReductionCS REDUCTION=1" / "ReductionCS_DDGIExtraReductionCS" (GIRenderer.cpp:542-573; csrc/k_ddgireduction.hip
 * states the bindings and the order of every addition, tests/ddgi_variability_ref.c is the definition) average it: push constants
 * b1 the SDK's 24-byte DDGIRootConstants, t4 the input, u5 a structured buffer of float2 (average, weight) per workgroup, a direct
 * dispatch of ceil(input / (16, 16, 4)) groups; the first pass also takes b0 (the same 160 bytes) and t3 the probe data.  Every
 * other pass accepts bit 2 and ignores it.
 * "giprobetrace_CS_ProbeTraceFixedRays", "ProbeRelocationCS_DDGIProbeRelocationCS" and
 * "ProbeClassificationCS_DDGIProbeClassificationCS" (GIRenderer.cpp:513-527: probe relocation and classification behind the blends;
 * csrc/k_giprobeplacement.hip states the bindings and the arithmetic, tests/ddgi_placement_ref.c is the definition).  b0 of all
 * three: the same 160 bytes.  Fixed rays: t0 the descriptor, t1 the probe data, t4..t6 and t8..t13 the scene and its structure in
 * the trace's slots (no materials), u0 a structured buffer float[numProbes * 32]; a direct dispatch of ceil(numProbes * 32 / 64)
 * groups.  Relocation, classification: u0 those distances, u3 (texture) the RGBA16_FLOAT data array, created with the UAV bit; a
 * direct dispatch of ceil(numProbes / 32) groups; refused unless the descriptor's flags have bit 0 (relocation) or bit 1
 * (classification).
 * "giprobevisualization_CS_LoadGIProbes" and "giprobevisualization_PS_VisualizeGIProbes" (GIDebugRenderer: the probes of that volume
 * drawn as spheres behind the cull "giprobevisualization_CS_VisualizeGIProbesCulling"; csrc/k_giprobedraw.hip states the rules,
 * tests/ddgi_probe_draw_ref.c is the definition).  LoadGIProbes, the project's own: b0 the 64-byte DDGIVolumeDesc (the host copy the
 * record function checks), t0 the descriptor, t1 the probe data, u0 a structured buffer float3[numProbes] of positions, u1
 * float[numProbes] of states (data.w when the flags have bit 1, else 0); a direct dispatch of ceil(numProbes / 32) groups; a probe
 * count larger than either output is refused.  The cull takes u0 and u1 at its t10 and t11.  The draw: b0 the 96-byte
 * GIProbeVisualizationConsts (the reference's 80 bytes, then m_NearPlane) with the descriptor's host copy behind it, 160 bytes; the
 * reference's registers t0 the culled positions, t1 / t2 / t3 the probe data / irradiance / distance arrays (the distance is not
 * read), t4 the descriptor, t5 instance -> probe index; and the project's own: t6 the DrawIndexedIndirectArguments (m_InstanceCount
 * is read on the device and clamped to the capacities of t0 and t5; m_IndexCount is not read), t7 the unit sphere's vertices
 * (UncompressedRawVertexFormat, 32 bytes; at most 128), t8 its indices (uint32; at most 256 triangles), u0 (texture) the R32_FLOAT
 * depth buffer, read and written, u1 (texture) the RGBA8_UNORM back buffer of the same size, and optionally u2 (texture) an RG32_UINT
 * texture of that size that then holds the per-texel winner words (depth bits << 32 | instance << 8 | triangle; 0: no sphere)
 * instead of the list's scratch.  Any direct dispatch: the two launches size themselves.  Texels no sphere wins keep colour and depth.
 * "adaptluminance_CS_GenerateLuminanceHistogram" (adaptluminance.hlsl, AdaptLuminanceRenderer.cpp): a direct dispatch of
 * [numthreads(16, 16, 1)] groups covering m_SrcColorDims; push constants GenerateLuminanceHistogramParameters (16 bytes), t0
 * (texture) the R11G11B10_FLOAT colour, u0 a structured UAV of at least 256 uint32.  It ADDS to u0: the caller clears it.
 * "adaptluminance_CS_AdaptExposure": a dispatch of (1, 1, 1); push constants AdaptExposureParameters (20 bytes), t0 the
 * histogram, u0 the one-float luminance buffer (read and written), u1 (texture) the 1 x 1 R32_FLOAT exposure texture.
 * "postprocess_PS_PostProcess" (postprocess.hlsl, PostProcessRenderer.cpp): a direct dispatch of [numthreads(8, 8, 1)] groups
 * over m_OutputDims; b0 or push constants PostProcessParameters (24 bytes), t0 (texture) the R11G11B10_FLOAT colour, t1 the
 * luminance buffer (required only when m_ManualExposure == 0), t2 (texture) R11G11B10_FLOAT bloom (optional: unbound reads
 * (0, 0, 0)), u0 (texture) the RGBA8_UNORM target; samplers are accepted and ignored.  Every texel is written, alpha 255.
 * A t2 with a mip chain (the generated bloom texture) is read at mip 0.
 * The arithmetic convention of the three is stated in csrc/k_postprocess.hip.
 * "sky_PS_HosekWilkieSky" (sky.hlsl, SkyRenderer.cpp; the stand-in of the full-screen pass at kFarDepth with its GreaterOrEqual
 * depth test): a direct dispatch of [numthreads(8, 8, 1)] groups covering the target; b0 SkyPassParameters (256 bytes, a constant
 * buffer), t0 (texture) the R32_FLOAT depth (the read-only depth attachment), u0 (texture) the R11G11B10_FLOAT target at mip 0,
 * whose size is the resolution; samplers are accepted and ignored.  A texel is written iff its depth is <= 0.0f (NaN is skipped):
 * the complement of the lighting pass.  Refused at record time: a missing or short b0, another format at t0 or u0, a missing
 * binding, a mip other than 0, depth and target of different size.  The arithmetic convention is stated in csrc/k_sky.hip.
 * "ambientocclusion_CS_XeGTAO_PrefilterDepths", "ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0" and
 * "ambientocclusion_CS_XeGTAO_Denoise" (ambientocclusion.hlsl, XeGTAO.hlsli, AmbientOcclusionRenderer.cpp): direct dispatches.
 * Prefilter: ceil(W / 16) x ceil(H / 16) groups; b0 GTAOConstants (96 bytes, a constant buffer), t0 (texture) the R32_FLOAT depth,
 * u0..u4 mips 0..4 of one R16_FLOAT texture with exactly 5 mips at the depth's size.  Main: ceil(W / 8) x ceil(H / 8) groups; b0,
 * b1 push constants XeGTAOMainPassConstantBuffer (68 bytes), t0 that chain, t2 GBufferA (RGBA32_UINT), u0 the working AO term
 * (R8_UINT), u1 the edges (R8_UNORM); the reference's t1 (Hilbert table) and u2 (debug texture) are not read.  Denoise:
 * ceil(W / 16) x ceil(H / 8) groups; b0, b1 push constants XeGTAODenoiseConstants (4 bytes), t0 the AO term (R8_UINT), t1 the
 * edges, u0 the output (R8_UINT, another texture than t0).  Samplers are accepted and ignored.  Refused at record time: a missing
 * binding, another format or size, a depth chain without 5 mips or u<k> not its mip k, a constant block of another size, groups
 * that do not cover the target, an indirect dispatch.  The arithmetic convention is tests/gtao_ref.c's (csrc/k_ambientocclusion.hip).
 * "raytracing_CS_RefitTLAS" (the back end's own name; stands in for buildTopLevelAccelStructFromBuffer, BasePassRenderers.cpp:159-160)
 * and "shadowmask_CS_ShadowMask" (shadowmask.hlsl, ShadowMaskRenderer::TraceShadows without denoising): see "acceleration
 * structure" below for the buffers and the bindings.  The arithmetic convention is tests/shadowmask_ref.c's (csrc/k_shadowmask.hip).
 * "bloom_PS_Downsample" and "bloom_PS_Upsample" (bloom.hlsl, BloomRenderer.cpp; the stand-ins of the full-screen passes of
 * Graphic.cpp:832-860): a direct dispatch of [numthreads(8, 8, 1)] groups covering the destination mip; b0 or push constants
 * BloomConsts (16 bytes: the downsample reads m_InvSourceResolution and m_bIsFirstDownsample, the upsample m_FilterRadius), t0
 * (texture) the R11G11B10_FLOAT source, read at the binding's baseMip, u0 (texture) the R11G11B10_FLOAT destination at its
 * baseMip, whose size is the viewport; samplers are accepted and ignored (linear clamp, filtered in software, is the only
 * behaviour).  Every texel of the destination mip is written and no other (the upsample overwrites: BlendOpaque).  Refused at
 * record time: another format at t0 or u0, a missing binding, a mip out of range, t0 and u0 naming the same mip of one texture.
 * The arithmetic convention is stated in csrc/k_bloom.hip. */
uint32_t    trhip_shader_count(void);
const char* trhip_shader_name(uint32_t index);
int         trhip_shader_exists(const char* name);

/* ---- device: replaces GraphicRHI::CreateDevice / nvrhi::IDevice (GraphicRHI.cpp:56-200) ----- */
int  trhip_device_create(int device_index, trhip_device* out);
/* Same, but submissions go to a caller-owned hipStream_t (e.g. torch's current stream). */
int  trhip_device_create_on_stream(int device_index, void* hip_stream, trhip_device* out);
void trhip_device_destroy(trhip_device dev);
int  trhip_device_wait_idle(trhip_device dev);                 /* nvrhi waitForIdle, Graphic.cpp:790 */
/* Orders the device's stream after everything its lists have put on the back end's internal side stream so far: an event
 * recorded on trhip_device_stream() afterwards covers ALL work of the lists executed before (what another queue waits
 * for: nvrhi queueWaitForCommandList). */
int  trhip_device_join_side_stream(trhip_device dev);
int  trhip_device_info(trhip_device dev, uint32_t* compute_units, uint32_t* wave_size, uint64_t* total_mem);
void* trhip_device_stream(trhip_device dev);                   /* the hipStream_t in use            */

/* ---- memory: replaces nvrhi heaps / createBuffer / createTexture / bind*Memory
 *      (RenderGraph.cpp:137-221,431-441; BasePassRenderers.cpp:236-291,596-616) --------------- */
typedef struct {
    uint64_t    byteSize;
    uint32_t    structStride;
    uint32_t    canHaveUAVs;
    uint32_t    isDrawIndirectArgs;
    uint32_t    isVirtual;          /* 1: no memory until trhip_buffer_bind_memory (placed)    */
    uint32_t    isVolatileConstant; /* nvrhi volatile constant buffer (Graphic.h:66-72)        */
    const char* debugName;
} trhip_buffer_desc;

typedef struct {
    uint32_t    width, height, mipLevels;
    uint32_t    format;             /* TRHIP_FORMAT_*                                          */
    uint32_t    isUAV;              /* bit 0: UAV; bit 1: TRHIP_TEXTURE_RENDER_TARGET                */
    uint32_t    isVirtual;
    const char* debugName;
} trhip_texture_desc;
/* nvrhi::TextureDesc::isRenderTarget, or'ed into isUAV: the texture's mips are the targets of full-screen passes, which this
 * back end writes through Texture_UAV bindings.  Only such a texture of R11G11B10_FLOAT may have more than one mip. */
#define TRHIP_TEXTURE_RENDER_TARGET 2u

int  trhip_heap_create(trhip_device dev, uint64_t bytes, trhip_heap* out);     /* nvrhi createHeap */
void trhip_heap_release(trhip_heap heap);

int  trhip_buffer_create(trhip_device dev, const trhip_buffer_desc* desc, trhip_buffer* out);
/* Wrap caller-owned device memory (e.g. a torch tensor's data_ptr) as a buffer; never freed here. */
int  trhip_buffer_wrap(trhip_device dev, void* device_ptr, const trhip_buffer_desc* desc, trhip_buffer* out);
int  trhip_buffer_memory_requirements(trhip_buffer buf, uint64_t* size, uint64_t* alignment);
int  trhip_buffer_bind_memory(trhip_buffer buf, trhip_heap heap, uint64_t offset);
void trhip_buffer_retain(trhip_buffer buf);
void trhip_buffer_release(trhip_buffer buf);
void* trhip_buffer_device_ptr(trhip_buffer buf);
uint64_t trhip_buffer_size(trhip_buffer buf);

int  trhip_texture_create(trhip_device dev, const trhip_texture_desc* desc, trhip_texture* out);
/* A 2D ARRAY texture (Texture2DArray: the DDGI probe textures of RTXGI, GIRenderer.cpp): `arraySize` (1..2048) slices of
 * desc's size and format, one mip.  trhip_texture_desc stays as it is.  Formats: R10G10B10A2_UNORM, RG16_FLOAT, RGBA16_FLOAT.
 * Slice k is row-major at byte k * trhip_texture_slice_pitch(tex) of the allocation; the pitch is width * height * texel bytes
 * rounded up to 256.  trhip_texture_array_size is 0 for a texture that is not an array (one of a single slice is still an
 * array).  An array texture is uploaded and downloaded per slice (the mip calls refuse it); it cannot be a texture table
 * entry, and every shader refuses one at any binding, naming itself, except "deferredlighting_PS_Main" / "_Debug" at t6..t8. */
int  trhip_texture_create_array(trhip_device dev, const trhip_texture_desc* desc, uint32_t arraySize, trhip_texture* out);
uint32_t trhip_texture_array_size(trhip_texture tex);
uint64_t trhip_texture_slice_pitch(trhip_texture tex);
int  trhip_texture_upload_slice(trhip_texture tex, uint32_t slice, const void* src, uint64_t bytes);
int  trhip_texture_download_slice(trhip_texture tex, uint32_t slice, void* dst, uint64_t bytes);
int  trhip_texture_memory_requirements(trhip_texture tex, uint64_t* size, uint64_t* alignment);
int  trhip_texture_bind_memory(trhip_texture tex, trhip_heap heap, uint64_t offset);
void trhip_texture_retain(trhip_texture tex);
void trhip_texture_release(trhip_texture tex);
void* trhip_texture_device_ptr(trhip_texture tex);
/* Layout in HBM: one linear allocation, mip k row-major max(w>>k,1) x max(h>>k,1) texels at
 * byte offset mip_offset(k); offsets are 256-byte aligned.  A block-compressed texture answers the same sizes in texels; its
 * level k holds ceil(w_k / 4) x ceil(h_k / 4) blocks, row-major. */
int  trhip_texture_mip_info(trhip_texture tex, uint32_t mip, uint32_t* w, uint32_t* h, uint64_t* byte_offset);
uint64_t trhip_texture_size(trhip_texture tex);

/* Synchronous host access (scene upload, test read-back; the reference's equivalents are
 * writeBuffer on an init command list, SceneLoading.cpp:1016-1088, and no read-back at all). */
int  trhip_buffer_upload(trhip_buffer buf, uint64_t dst_offset, const void* src, uint64_t bytes);
int  trhip_buffer_download(trhip_buffer buf, uint64_t src_offset, void* dst, uint64_t bytes);
int  trhip_texture_upload(trhip_texture tex, uint32_t mip, const void* src, uint64_t bytes);
int  trhip_texture_download(trhip_texture tex, uint32_t mip, void* dst, uint64_t bytes);

/* ---- texture table: the stand-in of the bindless ResourceDescriptorHeap[descriptorIndex] (lightingcommon.hlsli:345) --------
 * A device object of `capacity` entries; entry i maps descriptor index i to a texture's base pointer, width, height, mip count,
 * format and per-mip offsets.  set / clear rewrite one entry synchronously (they wait for the device first, like the uploads); the
 * table retains the textures it names until they are replaced, cleared or the table is released.  A texture of any format may
 * be set (the shader that indexes the table decides what it can sample); it needs memory bound, and an entry is NOT refreshed by
 * a later trhip_texture_bind_memory: set it again.  Bound as TRHIP_BIND_TEXTURE_TABLE; a command list retains the table. */
int  trhip_texture_table_create(trhip_device dev, uint32_t capacity, trhip_texture_table* out);
void trhip_texture_table_retain(trhip_texture_table table);
void trhip_texture_table_release(trhip_texture_table table);
uint32_t trhip_texture_table_capacity(trhip_texture_table table);
int  trhip_texture_table_set(trhip_texture_table table, uint32_t index, trhip_texture tex);
int  trhip_texture_table_clear(trhip_texture_table table, uint32_t index);
/* The 256-entry sRGB-to-linear table of SRGBA8_UNORM (no device needed): out[i] = the sRGB transfer function of i / 255 evaluated
 * in double precision (c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4)), rounded once to float.  The device keeps a
 * copy from its first texture table on. */
int  trhip_srgb_table(float* out);

/* ---- texture streaming: the min-mip clamp and sampler feedback of SampleMaterialValue (lightingcommon.hlsli:358-406) -----------
 * OPT-IN: a table without a min-mip or feedback entry records exactly the launches it always did.
 *
 * A material texture (RGBA8_UNORM, SRGBA8_UNORM or block-compressed, no UAV bit) becomes STREAMABLE by
 * trhip_texture_set_streaming_region: region_w x region_h texels, both powers of two >= 4 (a BC block never straddles a region),
 * both dividing the size of mip 0.  0 x 0 asks for D3D's 64 KB tile shape of the format: 128 x 128 (RGBA8), 512 x 256 (BC1, BC4),
 * 256 x 256 (BC2, BC3, BC5).  A texture that the region does not divide is refused: it is "not tiled", stays fully resident and
 * takes no maps.  Level k is STANDARD when it and every finer level are whole tiles, that is when (w >> j) and (h >> j) are
 * multiples (>= 1) of the region for every j <= k (a size that is no power of two stops early: 24 x 24 with 8 x 8 has one standard
 * level, 48 x 32 two), and k is not the last level: the levels after the last standard one are the PACKED TAIL, which is always
 * resident and always holds at least the last level.  The region is part of the texture's table entry: set it before trhip_texture_table_set.
 *
 * MIN-MIP MAP: an ordinary R8_UINT texture of (w / region_w) x (h / region_h) texels, one per mip-0 region, set into the same
 * table; a material names it in TextureData::m_MinMapTextureDescriptorIndex.  The resolve reads the texel of the region that holds
 * the mip-0 texel under uv (point, wrapped or clamped as the slot's sampler) and samples at
 * fmin(fmax(lod, (float)minMip), mips - 1); the tap count and the tap positions do not change.
 *
 * FEEDBACK MAP: an opaque texture (TRHIP_SAMPLER_FEEDBACK_FORMAT; one 32-bit word per region, 0xFFFFFFFF = never sampled) made
 * by trhip_sampler_feedback_create against its streamable material texture, set into the table and named by
 * m_FeedbackTextureDescriptorIndex.  With BasePassConstants::m_bWriteSamplerFeedback != 0 the resolve lowers, for every sample
 * of the slot, the word of every region that the UNCLAMPED sample would read to the finest level it would read it at (atomic
 * min; material_textures.hip.h states the marks).  trhip_cmd_clear_sampler_feedback resets every word,
 * trhip_cmd_decode_sampler_feedback writes one byte per region (row-major; the level, 0xFF = never sampled) into a buffer, from
 * where trhip_cmd_copy_to_readback takes it to the host.
 *
 * A flagged slot whose min-mip or feedback index is not 0xFFFFFFFF and names no such map of that very texture (past the table,
 * empty, another format, another size, a texture that is not streamable) ends the pixel untouched, like every other broken chain.
 * "basepass_PS_Main_GBuffer" records its #streamed kernel iff the bound table holds at least one R8_UINT or feedback entry.
 *
 * trhip_cmd_write_texture_region (writeTexture with a TextureSlice): a rectangle of one mip of a sampled material texture (or of an
 * R8_UINT min-mip map created without the UAV bit), in texels; for a block-compressed texture x, y, w and h are multiples of 4 (w and h may instead end at the level's edge) and src
 * holds the rectangle's blocks.  src is row-major without padding and is copied when the command is recorded. */
int  trhip_texture_set_streaming_region(trhip_texture tex, uint32_t region_w, uint32_t region_h);
int  trhip_texture_streaming_region(trhip_texture tex, uint32_t* region_w, uint32_t* region_h);   /* 0 x 0: not streamable */
int  trhip_sampler_feedback_create(trhip_device dev, trhip_texture paired, const char* debug_name, trhip_texture* out);
int  trhip_cmd_clear_sampler_feedback(trhip_cmdlist cl, trhip_texture feedback);
int  trhip_cmd_decode_sampler_feedback(trhip_cmdlist cl, trhip_buffer dst, uint64_t dst_offset, trhip_texture feedback);
int  trhip_cmd_write_texture_region(trhip_cmdlist cl, trhip_texture tex, uint32_t mip, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                    const void* src, uint64_t bytes);

/* ---- DDS container (no device needed; written from the public description of the format) ---------------------------------------
 * trhip_dds_parse reads the header of a .dds file held in memory and answers what the file says: size, mip count, format, and
 * where each level's bytes lie in the file (levels follow the header back to back, without padding; a level of a block format
 * is ceil(w_k / 4) * ceil(h_k / 4) blocks, one of RGBA8 is w_k * h_k * 4 bytes).  Accepted: the legacy fourCCs DXT1 (BC1), DXT2
 * and DXT3 (BC2), DXT4 and DXT5 (BC3), ATI1 and BC4U (BC4), ATI2 and BC5U (BC5), and a DX10 header with DXGI format 71 / 72
 * (BC1 / BC1_SRGB), 74 / 75 (BC2), 77 / 78 (BC3), 80 (BC4), 83 (BC5), 28 / 29 (RGBA8_UNORM / SRGBA8_UNORM).  Refused, each with
 * a message that names it: a bad magic or header size, mipMapCount == 0, more than 16 levels, an array size other than 1, cube
 * and volume textures, the SNORM variants, BC6H and BC7, every other pixel format, a file shorter than its levels.  A legacy
 * fourCC says nothing about sRGB: the loaders choose the variant by material slot (trhost_create_material_texture_dds,
 * gltf_lite.load), where the reference forces every BC1 file to sRGB. */
typedef struct {
    uint32_t width, height, mipLevels, format;                 /* format: TRHIP_FORMAT_* */
    uint64_t levelOffset[16], levelBytes[16];                  /* from the start of the file */
} trhip_dds_info;
int  trhip_dds_parse(const void* file, uint64_t bytes, trhip_dds_info* out);

/* Contents changed behind the back end's back.  The back end keeps derived, private copies of some bound resources (the
 * instance cull cache, the meshlet cull stream of the buffer bound at t4 of basepass_AS_Main and, once a pipeline statistics
 * query has covered that pass, its triangle-count bytes, an HZB's footprint-min table)
 * and rebuilds them when the source's version counter moves.  The counter moves for every write the back end SEES:
 * trhip_*_upload, a UAV use in an executed command list, trhip_*_bind_memory.  A write it cannot see -- through the raw
 * pointer of trhip_buffer_wrap / trhip_*_device_ptr (a torch kernel, hipMemcpy), through a second wrap of the same memory,
 * through another virtual resource aliased on the same heap range -- MUST be followed by this call (any thread; ordered by
 * the caller before the next trhip_queue_execute that reads the resource), or later culls use the old contents.
 * nvrhi has no counterpart: D3D12 shaders read the buffers themselves. */
int  trhip_buffer_mark_written(trhip_buffer buf);
int  trhip_texture_mark_written(trhip_texture tex);

/* ---- command lists: replaces nvrhi::ICommandList (Graphic.cpp:520-606,893-947) --------------- */
typedef enum {
    TRHIP_BIND_CONSTANT_BUFFER = 0,  /* nvrhi::BindingSetItem::ConstantBuffer(slot, buf)        */
    TRHIP_BIND_PUSH_CONSTANTS  = 1,  /* ::PushConstants(slot, bytes); data via push_constants   */
    TRHIP_BIND_STRUCTURED_SRV  = 2,  /* ::StructuredBuffer_SRV(slot, buf)   register(tN)        */
    TRHIP_BIND_STRUCTURED_UAV  = 3,  /* ::StructuredBuffer_UAV(slot, buf)   register(uN)        */
    TRHIP_BIND_TEXTURE_SRV     = 4,  /* ::Texture_SRV(slot, tex)            register(tN)        */
    TRHIP_BIND_TEXTURE_UAV     = 5,  /* ::Texture_UAV(slot, tex, fmt, {baseMip,1,0,1}) (uN)     */
    TRHIP_BIND_SAMPLER         = 6,  /* ::Sampler(slot, s): accepted and ignored (sampling is
                                        done in software, see DESIGN.md "HZB sampling")         */
    TRHIP_BIND_TEXTURE_TABLE   = 7   /* a trhip_texture_table at register(tN): what the shader
                                        indexes as ResourceDescriptorHeap[...]; t19 of
                                        "basepass_PS_Main_GBuffer", the first slot after t18     */
} trhip_binding_type;

typedef struct {
    uint32_t type;       /* trhip_binding_type                                                  */
    uint32_t slot;
    void*    resource;   /* trhip_buffer, trhip_texture or trhip_texture_table (NULL for push constants / sampler) */
    uint32_t baseMip;    /* Texture_UAV subresource; Texture_SRV: read by bloom_PS_* only       */
    uint32_t reserved;
} trhip_binding;

int  trhip_cmd_create(trhip_device dev, trhip_cmdlist* out);          /* AllocateCommandList    */
void trhip_cmd_release(trhip_cmdlist cl);
int  trhip_cmd_open(trhip_cmdlist cl);                                /* ICommandList::open     */
int  trhip_cmd_close(trhip_cmdlist cl);                               /* ::close                */
/* ::writeBuffer -- the source bytes are copied at record time (nvrhi upload manager semantics).
 * On a volatile constant buffer this sets the version later dispatches in this list see. */
int  trhip_cmd_write_buffer(trhip_cmdlist cl, trhip_buffer buf, uint64_t dst_offset, const void* src, uint64_t bytes);
int  trhip_cmd_clear_buffer_u32(trhip_cmdlist cl, trhip_buffer buf, uint32_t value);   /* ::clearBufferUInt   */
int  trhip_cmd_clear_texture_f32(trhip_cmdlist cl, trhip_texture tex, float value);    /* ::clearTextureFloat (16-bit formats: the fp16 of value, RNE; R11G11B10_FLOAT: the pack of value in all three channels; R8_UNORM: round(saturate(value) * 255); not the UINT formats) */
int  trhip_cmd_clear_texture_u32(trhip_cmdlist cl, trhip_texture tex, uint32_t value); /* ::clearTextureUInt: RG32_UINT / RGBA32_UINT, value in every 32-bit channel word; R8_UINT, the low byte */
int  trhip_cmd_copy_buffer(trhip_cmdlist cl, trhip_buffer dst, uint64_t dst_offset, trhip_buffer src, uint64_t src_offset, uint64_t bytes); /* ::copyBuffer */
/* Multi-GPU hook (no counterpart in the reference, which is single-GPU: GraphicRHI.cpp:165).
 * fn(user, hip_stream) is called on the submitting thread while the list is executed, in order with
 * the surrounding commands: whatever fn enqueues on hip_stream runs after everything recorded before
 * it and before everything recorded after it.  fn must not execute lists on / wait for this device. */
typedef void (*trhip_host_fn)(void* user, void* hip_stream);
int  trhip_cmd_host_callback(trhip_cmdlist cl, trhip_host_fn fn, void* user);
/* ::copyTexture, whole mip chain; both textures must have identical dimensions, mips and format. */
int  trhip_cmd_copy_texture(trhip_cmdlist cl, trhip_texture dst, trhip_texture src);
/* ::setComputeState + ::setPushConstants + ::dispatch(gx,gy,gz) (Graphic.cpp:893-947).
 * Group counts keep the reference's meaning (groups of the HLSL [numthreads]); the HIP launch
 * shape behind a shader name is the back end's business. */
int  trhip_cmd_dispatch(trhip_cmdlist cl, const char* shader_name,
                        const trhip_binding* bindings, uint32_t num_bindings,
                        const void* push_constants, uint32_t push_bytes,
                        uint32_t gx, uint32_t gy, uint32_t gz);
/* ::dispatchIndirect(offset): the 3 x u32 group counts are read ON THE DEVICE at execution. */
int  trhip_cmd_dispatch_indirect(trhip_cmdlist cl, const char* shader_name,
                                 const trhip_binding* bindings, uint32_t num_bindings,
                                 const void* push_constants, uint32_t push_bytes,
                                 trhip_buffer args_buffer, uint32_t args_offset_bytes);
int  trhip_cmd_begin_timer(trhip_cmdlist cl, trhip_timer t);          /* ::beginTimerQuery      */
int  trhip_cmd_end_timer(trhip_cmdlist cl, trhip_timer t);            /* ::endTimerQuery        */
int  trhip_cmd_begin_marker(trhip_cmdlist cl, const char* name);      /* ::beginMarker          */
int  trhip_cmd_end_marker(trhip_cmdlist cl);                          /* ::endMarker            */

/* nvrhi executeCommandLists (Graphic.cpp:786-830): enqueue the recorded lists, in order, on the
 * device stream.  Asynchronous; a list may be executed more than once without re-recording. */
int  trhip_queue_execute(trhip_device dev, const trhip_cmdlist* lists, uint32_t num_lists);

/* ---- timer queries: nvrhi::TimerQuery (RenderGraph.cpp:269-285) ----------------------------- */
int  trhip_timer_create(trhip_device dev, trhip_timer* out);
void trhip_timer_release(trhip_timer t);
int  trhip_timer_get_ms(trhip_timer t, float* ms);   /* waits for the end event (getTimerQueryTime) */

/* ---- pipeline statistics queries: nvrhi::PipelineStatisticsQuery (BasePassRenderers.cpp:178-179,202-207,546-549) ------
 * 14 counters in the field order of D3D12_QUERY_DATA_PIPELINE_STATISTICS1 (112 bytes).  They count what the reference's
 * pipeline would have invoked for the dispatches recorded between begin and end, not what HIP launched:
 *   ASInvocations  basepass_AS_Main LATE_CULL=*: 32 x G, G = min(X, validRecords, record capacity) (X read on the device)
 *   MSInvocations  the same dispatch: 96 (kMeshletShaderThreadGroupSize) x visible meshlets (its draw args word 0)
 *   MSPrimitives   the same dispatch: sum over its visible meshlets of (m_VertexAndTriangleCount >> 8) & 0xFF
 *   CSInvocations  groups x the reference entry's [numthreads]: gpuculling_CS_GPUCulling 32 (the late pass is indirect: its
 *                  groups are read on the device), gpuculling_CS_BuildLateCullIndirectArgs 1, minmaxdownsample_CS_Main 64,
 *                  ffx_spd_downsample_pass_CS * 256, updateinstanceconsts_* 32, giprobevisualization_CS_* 32
 *   all others     0: no fixed-function stage is modelled; basepass_MS_Main_depth adds nothing (its mesh work is counted by
 *                  the AS dispatch that fed it), nor do the back end's own visibility_CS_* shaders.
 * Begin zeroes the counters when it executes, so a list executed twice yields the same values again.  Begin and end must be
 * recorded into the same command list, which holds at most one open query (else TRHIP_ERR_STATE; closing a list with a
 * query open is TRHIP_ERR_STATE too).  With several devices each counts the dispatches of its own lists. */
typedef struct {
    uint64_t IAVertices, IAPrimitives, VSInvocations, GSInvocations, GSPrimitives, CInvocations, CPrimitives, PSInvocations,
             HSInvocations, DSInvocations, CSInvocations, ASInvocations, MSInvocations, MSPrimitives;
} trhip_pipeline_statistics;

int  trhip_pipeline_stats_create(trhip_device dev, trhip_pipeline_stats* out);   /* createPipelineStatisticsQuery */
void trhip_pipeline_stats_release(trhip_pipeline_stats q);
int  trhip_cmd_begin_pipeline_stats(trhip_cmdlist cl, trhip_pipeline_stats q);   /* ::beginPipelineStatisticsQuery */
int  trhip_cmd_end_pipeline_stats(trhip_cmdlist cl, trhip_pipeline_stats q);     /* ::endPipelineStatisticsQuery   */
/* getPipelineStatistics: waits for the end of the last executed end; TRHIP_ERR_STATE if the query was never ended in an
 * executed list. */
int  trhip_pipeline_stats_get(trhip_pipeline_stats q, trhip_pipeline_statistics* out);

/* ---- read-back: nvrhi::StagingTexture / a CpuAccessMode::Read buffer (GIRenderer.cpp:531-540, :575) ----------------------
 * Pinned host memory of `slots` slots of bytes_per_slot bytes, one event per slot.  trhip_cmd_copy_to_readback records an
 * asynchronous device-to-host copy of `bytes` (<= bytes_per_slot) from src_buffer at src_offset into the slot, on the list's
 * stream, and the slot's event behind it.  trhip_readback_read (mapStagingTexture) waits for THAT SLOT'S event only -- never for
 * the device, so a frame that reads what it copied two frames ago does not wait for the frame in flight -- and copies
 * min(bytes, what the slot's last executed copy wrote) to dst; *written receives that count.  A slot that no executed list has
 * written yet gives *written = 0 and `bytes` zero bytes in dst.  A slot is the caller's to pace: a copy into a slot that is
 * being read is not ordered against the read.  trhip_readback_reset waits for the device and marks every slot as never
 * written (the events and the memory stay, so a recorded list that names the resource stays valid).  Release waits for the
 * device; a recorded list holds the source buffer but NOT the read-back resource: every list that names it must have been
 * re-opened or released before it is released. */
int  trhip_readback_create(trhip_device dev, uint64_t bytes_per_slot, uint32_t slots, trhip_readback* out);
void trhip_readback_release(trhip_readback rb);
int  trhip_readback_reset(trhip_readback rb);
int  trhip_cmd_copy_to_readback(trhip_cmdlist cl, trhip_readback rb, uint32_t slot, trhip_buffer src_buffer, uint64_t src_offset, uint64_t bytes);
int  trhip_readback_read(trhip_readback rb, uint32_t slot, void* dst, uint64_t bytes, uint64_t* written);
/* Never waits: *ready = 1 when trhip_readback_read of that slot would return at once (its last copy has completed, or no executed
 * list has written it), else 0. */
int  trhip_readback_poll(trhip_readback rb, uint32_t slot, int* ready);

/* ---- acceleration structure: nvrhi::rt::AccelStruct (Visual.cpp:509-542 Mesh::BuildBLAS, Scene.cpp:430-470 the TLAS) ----------
 * DXR's structure is opaque; this one is the project's own and lives in ordinary structured buffers that the caller creates,
 * fills from the two host-side builders below (no device needed) and binds.  DESIGN.md 13 has the reasoning.
 *
 * NODES (trhip_accel_node, 32 bytes), both levels: a binary tree in depth-first preorder.  Node i's first child is i + 1, its
 * second child is nodes[i + 1].skip, nodes[i].skip is the first node behind i's subtree (the node count for the last), so a
 * walk needs no stack: box hit on an inner node -> i + 1, else -> skip.  leaf = 0xFFFFFFFF: inner.  BLAS leaf: first | (count - 1)
 * << 30, `count` (1..4) entries of the mesh's triangle order from `first`.  TLAS leaf: the instance index (one instance per leaf).
 * Depth <= trhip_accel_max_depth() = 56 for every input (median split where the midpoint split degenerates).
 * BLAS, per mesh, object space, built once: trhip_blas_build over the mesh's LOD-0 index list (indices relative to the mesh's first
 * vertex, as m_GlobalIndexBufferIdx addresses them).  tri_order receives the triangle ids (index / 3) in leaf order; a triangle
 * with a non-finite vertex is in no leaf and is never hit.  Every box is moved outward by 2^-16 times the mesh's largest
 * |coordinate|.  All meshes' nodes and orders are concatenated; trhip_blas_header (16 bytes) per mesh says where: node_offset
 * (skip and child indices are relative to it), num_nodes (0: nothing to hit), tri_offset, num_tris.  Same input, same bytes.
 * TLAS, per scene: trhip_tlas_build makes the topology from the instances' rest transforms (m_WorldMatrix of the 144-byte
 * records) and flags[i] (0: not in the structure, 1: ForceOpaque, 2: ForceNonOpaque; Scene.cpp:454), fills one trhip_tlas_instance
 * (64 bytes) per instance (flags, leaf_node or 0xFFFFFFFF, the matrix zero) and lists the inner nodes by height: level_nodes
 * [level_offsets[h - 1], level_offsets[h]) are the nodes of height h = 1..num_levels (level_offsets: trhip_accel_max_depth() + 2
 * words; level_nodes: as many words as nodes).
 * "raytracing_CS_RefitTLAS", recorded every frame behind "updateinstanceconsts_*": a direct dispatch of 64-thread groups covering
 * m_NumInstances; push constants { m_NumInstances, m_NumNodes, m_NumLevels } (12 bytes); t0 instances, t1 BLAS headers, t2 BLAS
 * nodes, t3 level_offsets, t4 level_nodes, u0 the TLAS nodes, u1 the TLAS instances.  Per instance in the structure it writes the
 * object-from-world 3x4 (rows of p_object = (p_world, 1) * M) and the leaf's box: the BLAS root box's 8 corners through
 * m_WorldMatrix, moved outward by 2^-12 times the largest |coordinate|; then every inner box, height by height.
 * "shadowmask_CS_ShadowMask": a direct dispatch of [numthreads(8, 8, 1)] groups covering m_OutputResolution; b0 ShadowMaskConsts
 * (112 bytes, a constant buffer; m_bDoDenoising: see the shadow denoiser below), t0 (texture) R32_FLOAT depth, t1 the TLAS nodes, t2 (texture) GBufferA,
 * t3 instances, t4 vertices, t5 materials, t6 indices, t7 mesh data, t8 (texture) RGBA8_UNORM 128 x 128 blue noise, u0 (texture)
 * R8_UNORM mask, u1 (texture) R16_FLOAT linear view depth, and the structure's other buffers: t9 TLAS instances, t10 BLAS
 * headers, t11 BLAS nodes, t12 triangle order, and optionally t19 the texture table: with it ("#textured" in the profile) a
 * candidate on a ForceNonOpaque instance whose material has MaterialFlag_UseAlbedoTexture counts iff m_ConstAlbedo.w times the
 * albedo texture's alpha at the hit (one bilinear fetch of mip 0 at InterpolateVertex's uv; a broken descriptor: it does not
 * count) is at least m_AlphaCutoff; without it, and for texture-free materials, iff m_ConstAlbedo.w >= m_AlphaCutoff.
 * Samplers are accepted and ignored.  A texel of depth 0.0f gets u1 = 65504 and
 * keeps u0; any other gets u0 = 0 (occluded) or 255 and u1 = fp16(|worldPosition - m_CameraPosition|).  An index read on the
 * device that leaves its buffer ends that instance's (or triangle's) test; it is never followed.
 * THE SHADOW DENOISER (ShadowMaskRenderer::DenoiseShadows; csrc/k_sigma.hip states every rule, tests/sigma_ref.c defines them).
 * "shadowmask_CS_ShadowMask" with m_bDoDenoising != 0: u0 is an R16_FLOAT penumbra texture (the R8_UNORM mask there is refused): no
 * occluder 65504, else min(0.5 * t * m_TanSunAngularRadius, 32768) of the CLOSEST committing candidate; "#penumbra" /
 * "#textured_penumbra" in the profile; u1 and far texels as above.  "shadowmask_CS_PackNormalAndRoughness": groups of 8 x 8 covering
 * m_OutputResolution; b0 or push constants { m_OutputResolution } (8 bytes), t2 GBufferA, u0 an R10G10B10A2_UNORM texture: the
 * octahedral normal in x and y, roughness in z, w = 0, every texel.  The four entries behind them share b0 or push constants
 * SigmaConsts (112 bytes, csrc/ShaderInterop.h) and an R8_UINT tile texture of ceil(W / 16) x ceil(H / 16):
 * "SIGMA_Shadow_ClassifyTiles.cs" (groups of 16 x 16): t0 penumbra, t1 R16_FLOAT linear view depth, u0 tiles, u1 RG16_FLOAT shadow data;
 * "SIGMA_Shadow_Blur.cs" (m_Pass 0) and "SIGMA_Shadow_PostBlur.cs" (m_Pass 1), groups of 8 x 8: t0 shadow data in, t1 linear view
 * depth, t2 R32_FLOAT depth, t3 the normal roughness texture, t4 tiles, u0 shadow data out (another texture than t0);
 * "SIGMA_Shadow_TemporalStabilization.cs" (8 x 8): t0 shadow data, t1 linear view depth, t2 the RG16_FLOAT motion target, t3 the previous
 * R16_FLOAT history, t4 tiles, u0 the new history (another texture than t3), u1 the R8_UNORM shadow mask the lighting pass binds.
 * All textures one mip at m_OutputDims; every dispatch direct; each refusal happens at record time. */
typedef struct { float lo[3]; uint32_t skip; float hi[3]; uint32_t leaf; } trhip_accel_node;
typedef struct { uint32_t node_offset, num_nodes, tri_offset, num_tris; } trhip_blas_header;
typedef struct { float object_from_world[12]; uint32_t flags, leaf_node, reserved[2]; } trhip_tlas_instance;
uint32_t trhip_accel_max_depth(void);
uint32_t trhip_blas_leaf_capacity(void);
uint32_t trhip_accel_max_nodes(uint32_t num_primitives);     /* 2 n - 1: the node capacity a build of n primitives needs */
int  trhip_blas_build(const void* vertices, uint32_t vertex_stride, uint32_t num_vertices, const uint32_t* indices, uint32_t num_indices,
                      trhip_accel_node* nodes, uint32_t node_capacity, uint32_t* tri_order, uint32_t* num_nodes, uint32_t* num_tris, uint32_t* depth);
int  trhip_tlas_build(const void* instances, uint32_t num_instances, const uint32_t* flags, const trhip_blas_header* headers, uint32_t num_meshes,
                      const trhip_accel_node* blas_nodes, uint32_t num_blas_nodes, trhip_accel_node* nodes, uint32_t node_capacity,
                      trhip_tlas_instance* records, uint32_t* level_nodes, uint32_t* level_offsets, uint32_t* num_nodes, uint32_t* num_levels);

/* ---- per-shader GPU profile: PROFILE_GPU_SCOPED in AddComputePass (Graphic.cpp:899) ----------
 * When enabled, every dispatch executed is bracketed by HIP events on the device stream and
 * accumulated under its shader name (sub-kernels under "name#kernel").  Off by default. */
int  trhip_profile_enable(trhip_device dev, int enabled);
/* Bracket only the dispatches accumulated under exactly `name` ("shader#kernel"); NULL or "" = all of them.  One event pair
 * per frame instead of one per launch: the frame keeps its steady-state overlap and clocks while one kernel is timed. */
int  trhip_profile_filter(trhip_device dev, const char* name);
int  trhip_profile_reset(trhip_device dev);
int  trhip_profile_count(trhip_device dev, uint32_t* n);
int  trhip_profile_entry(trhip_device dev, uint32_t index, const char** name, uint64_t* launches, double* total_ms);

/* Streams and events for callers that order work across streams themselves (the multi-GPU exchange runs on its own
 * streams next to the renderer's).  Plain wrappers: hipStreamCreateWithFlags(NonBlocking), hipEventCreateWithFlags
 * (DisableTiming), hipEventRecord, hipStreamWaitEvent, hipStreamSynchronize. */
int  trhip_stream_create(int device_index, void** out_hip_stream);
/* priority_class < 0: the device's highest stream priority, 0: default, > 0: lowest (hipStreamCreateWithPriority).
 * Streams of different priority classes never share a hardware queue; streams of one class may (HIP multiplexes them
 * round robin onto GPU_MAX_HW_QUEUES queues) and then run one after the other. */
int  trhip_stream_create_priority(int device_index, int priority_class, void** out_hip_stream);
void trhip_stream_destroy(void* hip_stream);
int  trhip_stream_synchronize(void* hip_stream);
int  trhip_event_create(int device_index, void** out_hip_event);
void trhip_event_destroy(void* hip_event);
int  trhip_event_record(void* hip_event, void* hip_stream);
int  trhip_stream_wait_event(void* hip_stream, void* hip_event);

/* Multi-GPU late phase.  The reference sizes the late instance cull from the late-list length
 * (gpuculling.hlsl:182-195, Q1: ceil(count/64) groups of 32 threads).  With the instance list sharded
 * over ranks that rule has to see the WHOLE scene's late list: every rank all-gathers its late count,
 * then this kernel writes info = { sum of counts[0..rank), sum of counts[0..world) } on hip_stream.
 * The late "gpuculling_CS_GPUCulling LATE_CULL=1" dispatch reads it from an optional SRV t4 and
 * processes exactly the entries the single-GPU dispatch would. */
int  trhip_launch_shard_late_info(void* hip_stream, const uint32_t* gathered_counts, uint32_t world, uint32_t rank, uint32_t* info);

#ifdef __cplusplus
}
#endif
#endif /* TRHIP_H_ */
