/*
 * trhost.h -- C entry points of the C++ host mirror (toyrenderer_amd/csrc/host): the reference's
 * frame loop for the visibility path (Graphic::Update -> Scene::Update -> RenderGraph::AddRenderer /
 * Compile -> UpdateInstanceConstsRenderer / GBufferRenderer -> Graphic::AddComputePass) behind a
 * plain-C facade, for callers that cannot link C++ (Python tests, bench.py).  A C++ application
 * uses the classes directly.
 *
 * All functions return 0 on success, -1 on failure (text: trhost_last_error()).  One context per
 * process (the reference's Graphic / Scene are singletons: Graphic.h:43, Scene.h:179).
 */
#ifndef TRHOST_H_
#define TRHOST_H_

#include <stdint.h>

#include "trhip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* trhost_last_error(void);

/* Graphic::Initialize (Graphic.cpp:608-647): device, shaders(kernels), common resources, renderers'
 * Initialize() (HZB creation, BasePassRenderers.cpp:596-616).  external_hip_stream may be NULL. */
int  trhost_initialize(int device_index, uint32_t render_width, uint32_t render_height, void* external_hip_stream);
void trhost_shutdown(void);

/* Scene content as flat arrays in the wire formats of ShaderInterop.h (what SceneLoading.cpp:203-224,
 * 1016-1088 and Scene.cpp:282-362 produce); followed by Graphic::PostSceneLoad. */
int  trhost_load_scene(const void* instances, uint32_t num_instances, const void* mesh_data, uint32_t num_meshes,
                       const void* meshlets, uint64_t num_meshlets, const uint32_t* opaque_ids, uint32_t num_opaque,
                       const uint32_t* alpha_mask_ids, uint32_t num_alpha_mask);
/* Same, with meshes, meshlets and the mesh-shader geometry read from a `<scene>_CachedData.bin` version 3, the
 * reference's mesh-processing cache (SceneLoading.cpp:57-79 layout, :706-781 LoadCachedData); instances and id lists
 * come from the caller (the glTF side).  Fails on another version, a truncated file or dangling ranges. */
int  trhost_load_scene_cached(const char* cached_data_path, const void* instances, uint32_t num_instances, const uint32_t* opaque_ids, uint32_t num_opaque,
                              const uint32_t* alpha_mask_ids, uint32_t num_alpha_mask);
/* Large scenes: pass meshlets = NULL to trhost_load_scene (allocation only) and stream the meshlet
 * buffer in with this call. */
int  trhost_upload_meshlets(uint64_t first_meshlet, const void* meshlets, uint64_t count);
/* Node hierarchy for UpdateInstanceConstsRenderer (BasePassRenderers.cpp:64-104); enables the pass. */
int  trhost_load_nodes(const void* node_local_transforms, uint32_t num_nodes, const uint32_t* primitive_to_node);
int  trhost_set_node_transforms(const void* node_local_transforms, uint32_t num_nodes);
/* Multi-GPU (not in the reference, which updates every instance it renders): UpdateInstanceConstsRenderer rebuilds the
 * transforms of instances [first, first + count) only -- the range a rank's id lists cover; the rest of the replicated
 * instance table is never read by its passes.  Default: the whole table. */
int  trhost_set_instance_update_range(uint32_t first, uint32_t count);

/* View (Scene.cpp:109-145): row-major 4x4, row vectors.  prev_world_to_view / view_to_clip may be NULL
 * (previous = last frame's; projection = RH reverse-Z infinite from fov/aspect/near). */
int  trhost_set_camera(const float* world_to_view, const float* prev_world_to_view, const float* view_to_clip, float near_plane);
/* Scene.h:128-132 toggles; force_mesh_lod < 0 = automatic. */
int  trhost_set_culling(int frustum, int occlusion, int cone, int freeze_culling_camera, int force_mesh_lod);
/* Capacity of the amplification-record buffer (kMaxThreadGroupsPerDimension = 65535 in the reference)
 * and the per-resource cap of the render graph (1 GB in the reference); 0 keeps the current value. */
int  trhost_set_limits(uint32_t max_meshlet_groups, uint64_t max_transient_resource_bytes);
/* Per-renderer GPU timer queries (RenderGraph.cpp:262-281, read back by trhost_renderer_times).  On by default like
 * the reference; each query is two timestamped barrier packets on the stream. */
int  trhost_set_gpu_timers(int enable);

/* Depth image the next frames' GenerateHZB will consume (stand-in for the rasteriser). */
int  trhost_upload_depth(const float* depth, uint32_t width, uint32_t height);
/* Instead of the stand-in: the frame rasterises the depth of its own visible meshlets ("basepass_MS_Main_depth", the
 * compute replacement of MS_Main + depth test, basepass.hlsl:124-188) after every cull pass, from the buffers the mesh
 * shader reads (SceneLoading.cpp:1016-1088): RawVertexFormat vertices (20 B), meshlet vertex ids, packed meshlet
 * triangles.  trhost_download_depth: the depth buffer of the last frame (float32, render resolution), after wait_idle. */
int  trhost_load_geometry(const void* vertices, uint64_t num_vertices, const uint32_t* meshlet_vertex_ids, uint64_t num_vertex_ids,
                          const uint32_t* meshlet_triangles, uint64_t num_triangles);
int  trhost_set_raster_depth(int enable);
/* Per-pixel visibility buffer and motion target (implies raster depth): every pass rasterises through
 * "basepass_MS_Main_visibility" into GBufferRenderer's VisibilityBuffer (RG32_UINT: per texel one u64,
 * depthBits << 32 | passSlot << 30 | listPosition << 7 | triangle, 0 = nothing drawn), and "basepass_PS_Main_motion" resolves
 * GBufferMotion (RG16_FLOAT: previous position minus pixel centre, pixels) once after the last pass, with
 * m_PrevWorldToClip = the last frame's raster camera.  Refused with max_meshlet_groups above 2^18 and with a shard exchange.
 * The downloads read the last frame's targets (render resolution; 8 and 4 bytes per texel), after wait_idle. */
int  trhost_set_visibility_buffer(int enable);
int  trhost_download_visibility(uint64_t* texels, uint64_t bytes);
int  trhost_download_motion(uint16_t* halves, uint64_t bytes);
/* GBufferA for texture-free materials (implies the visibility buffer, same refusals): "basepass_PS_Main_GBuffer" resolves
 * GBufferRenderer's GBufferA (RGBA32_UINT: PackGBuffer's x, y, z, w per texel, 16 bytes; 0 = nothing drawn) and GBufferMotion
 * in one dispatch in the place of "basepass_PS_Main_motion".  trhost_load_materials uploads MaterialData[count] (124-byte
 * stride, Graphic::m_GlobalMaterialDataBuffer; BasePassInstanceConstants::m_MaterialDataIdx indexes it) and refuses a material
 * whose m_MaterialFlags names a texture that is not loaded (see trhost_create_material_texture); it comes before trhost_set_gbuffer(1).  trhost_set_debug_view_mode sets
 * Scene::m_DebugViewMode -> m_DebugMode (2 ColorizeInstances, 3 ColorizeMeshlets, 12 MeshLOD fill GBufferA's debug byte). */
int  trhost_load_materials(const void* materials, uint32_t count);
/* Textured materials.  trhost_create_material_texture uploads one material texture (format TRHIP_FORMAT_RGBA8_UNORM or
 * TRHIP_FORMAT_SRGBA8_UNORM; `data`: the mips back to back, level k of max(width >> k, 1) x max(height >> k, 1) texels of 4 bytes
 * R, G, B, A; `bytes` their sum; or one of TRHIP_FORMAT_BC1_UNORM .. TRHIP_FORMAT_BC5_UNORM: level k is then ceil(w_k / 4) x
 * ceil(h_k / 4) blocks of trhip_format_block_bytes(format) bytes, `bytes` the sum of the levels' block bytes) and returns its descriptor index (0, 1, ... in call order; -1 and trhost_last_error on failure):
 * the value a flagged TextureData::m_DescriptorIndex names.  The host owns the texture table (the stand-in of the bindless heap,
 * 4096 entries) and binds it at t19 of "basepass_PS_Main_GBuffer" whenever a loaded material has a texture flag; the resolve then
 * samples (include/trhip.h).  trhost_load_materials accepts a textured material when every flagged slot's m_DescriptorIndex names a
 * texture created before it and its m_FeedbackTextureDescriptorIndex and m_MinMapTextureDescriptorIndex are 0xFFFFFFFF; otherwise
 * it fails with a message containing "texture".  The textures live until trhost_shutdown. */
int  trhost_create_material_texture(uint32_t width, uint32_t height, uint32_t mips, uint32_t format, const void* data, uint64_t bytes);
/* Texture::LoadFromFile (TextureLoading.cpp) for a .dds file held in memory: trhip_dds_parse, then trhost_create_material_texture
 * on the file's levels; returns the descriptor index, or -1 (the parser's message in trhost_last_error).  `srgb` is the material
 * slot's choice (base colour and emissive: 1; normal and metallic-roughness: 0): it picks between a format and its _SRGB twin
 * whatever the file says, and is ignored for BC4 and BC5.  The reference instead forces every BC1 file to sRGB. */
int  trhost_create_material_texture_dds(const void* file, uint64_t bytes, int srgb);
int  trhost_set_gbuffer(int enable);
/* ALPHA_MASK_MODE's discard (basepass.hlsl:210-215), default 0 = off: alpha-mask primitives are drawn as solid triangles, as before.
 * With 1 (needs the rasters: trhost_set_raster_depth, trhost_set_visibility_buffer or anything that implies them, and
 * trhost_load_materials; fails otherwise) the alpha-mask pass slots draw through "basepass_MS_Main_depth ALPHA_MASK_MODE=1" or
 * "basepass_MS_Main_visibility ALPHA_MASK_MODE=1" (include/trhip.h) with the materials at t3 and, when a loaded material is
 * textured, the texture table at t19: a sample whose m_ConstAlbedo.w times its albedo texture's alpha is below m_AlphaCutoff is
 * not drawn.  ShadowMaskRenderer then binds the table as well, and a textured cut-out casts the shadow of its kept texels. */
int  trhost_set_alpha_test(int enabled);
int  trhost_set_debug_view_mode(uint32_t mode);
int  trhost_download_gbuffer_a(uint32_t* words, uint64_t bytes);
/* Deferred lighting from GBufferA (DeferredLightingRenderer.cpp; implies the G-buffer, same refusals): after GBufferRenderer one
 * "deferredlighting_PS_Main" dispatch ("deferredlighting_PS_Main_Debug" while trhost_set_debug_view_mode is not 0; mode 10 needs
 * the DDGI volume, trhost_upload_ddgi_volume below, and is refused without it) writes LightingOutput (R11G11B10_FLOAT at render resolution, 4 bytes per texel, cleared to
 * 0 every frame; written where depth > 0).  trhost_set_directional_light sets Scene::m_DirLightVec, used as given, and
 * m_DirLightStrength (default (0, -1, 0), 1).  trhost_upload_shadow_mask uploads the R8_UNORM mask at render resolution
 * (width * height bytes); NULL means white.  trhost_get_deferred_lighting_consts copies the 112 bytes of DeferredLightingConsts
 * the last frame uploaded (m_ClipToWorld = the inverse of m_WorldToView * m_ViewToClip in double precision, rounded once;
 * m_CameraOrigin = the eye of m_WorldToView). */
int  trhost_set_deferred_lighting(int enable);
int  trhost_set_directional_light(const float vec[3], float strength);
int  trhost_upload_shadow_mask(const uint8_t* texels, uint64_t bytes);
int  trhost_download_lighting_output(uint32_t* words, uint64_t bytes);
int  trhost_get_deferred_lighting_consts(void* out112);
/* The DDGI ambient term from a SUPPLIED probe volume (Scene::m_RTDDGIVolume; trhost_set_ddgi_update below lets it fill itself).
 * trhost_upload_ddgi_volume creates and fills the volume: desc64 is the 64-byte DDGIVolumeDesc (csrc/ShaderInterop.h), the three
 * arrays are dense, slice (probe y) after slice: irradiance R10G10B10A2_UNORM words [counts.y][counts.z * 8][counts.x * 8],
 * distance binary16 pairs [counts.y][counts.z * 16][counts.x * 16][2], data binary16 quadruples [counts.y][counts.z][counts.x][4];
 * the byte sizes must match the counts.  desc64 = NULL drops the volume and switches DDGI off.  From then on the lighting pass
 * binds the volume at t5..t8.  trhost_set_ddgi(1) makes Scene::IsDDGIEnabled() true: m_bRTDDGIEnabled = 1 in the consts
 * trhost_get_deferred_lighting_consts shows, and LightingOutput gains albedo / pi * irradiance (times the SSAO texture when
 * ambient occlusion is on).  Debug view 10 (Ambient) shows the irradiance, whatever trhost_set_ddgi says.  Without an uploaded
 * volume trhost_set_ddgi(1) and view 10 are refused ("DDGI", "Ambient" in the text). */
int  trhost_upload_ddgi_volume(const void* desc64, const uint32_t* irradiance, uint64_t irradiance_bytes, const uint16_t* distance, uint64_t distance_bytes,
                               const uint16_t* data, uint64_t data_bytes);
int  trhost_set_ddgi(int enable);
/* The probe update, GIRenderer::RenderDDGI (csrc/host/GIRenderer.cpp): with trhost_set_ddgi_update(1, seed) every frame with
 * deferred lighting on records, behind the TLAS refit (which then runs with or without trhost_set_shadow_mask) and in front of
 * DeferredLightingRenderer, "giprobetrace_CS_ProbeTrace" and the two "ProbeBlendingCS_DDGIProbeBlendingCS" passes on the uploaded
 * volume, which so fills itself from what it holds; the n-th update after the call takes its ray rotation from (seed, n).  It
 * needs trhost_upload_ddgi_volume and trhost_load_raytracing and is refused without them; dropping the volume switches it off.
 * The settings are the reference's (hysteresis 0.5, distance exponent 50, thresholds 0.2 and 0.1; probeMaxRayDistance 1e10).
 * trhost_reset_ddgi_volume clears irradiance and distance to zero words, the reference's start (GIRenderer.cpp:457-458);
 * trhost_download_ddgi_volume reads the three textures back in trhost_upload_ddgi_volume's layout;
 * trhost_get_ddgi_update_consts copies the 96 bytes of DDGIUpdateConsts (csrc/ShaderInterop.h) the last frame's update ran with,
 * the rotation among them, and fails if no update ran in it.
 * trhost_set_ddgi_probe_placement(relocation, classification, min_frontface_distance, fixed_ray_backface_threshold): the reference's
 * probe relocation and classification (GIRenderer.cpp:80-83, :513-527), off by default here.  With either on, every update records
 * behind the blends "giprobetrace_CS_ProbeTraceFixedRays" (32 unrotated rays from every probe, active or not) and then
 * "ProbeRelocationCS_DDGIProbeRelocationCS" and / or "ProbeClassificationCS_DDGIProbeClassificationCS", which rewrite the data
 * texture's xyz (offsets in units of the spacing) and w (1: switched off); the lighting pass of the same frame reads the new data.
 * The reference's values are 0.1 (scene radius below 3) or 0.3, and 0.25; they show in trhost_get_ddgi_update_consts' bytes 84..91,
 * which are 0 while both passes are off.  It needs the volume, and each pass its flag in the volume's descriptor; uploading a
 * volume whose flags do not allow what was set switches both off. */
int  trhost_set_ddgi_update(int enabled, uint32_t seed);
int  trhost_set_ddgi_probe_placement(int relocation, int classification, float min_frontface_distance, float fixed_ray_backface_threshold);
int  trhost_reset_ddgi_volume(void);
int  trhost_download_ddgi_volume(uint32_t* irradiance, uint64_t irradiance_bytes, uint16_t* distance, uint64_t distance_bytes, uint16_t* data, uint64_t data_bytes);
int  trhost_get_ddgi_update_consts(void* out96);
/* Probe variability, the reference's convergence early-out (GIRenderer.cpp:84, :158-190, :466-470, :529-576;
 * csrc/host/DDGIVariability.h is the rule, DESIGN.md 12's eighteenth amendment the reasoning).  An option, off by default.
 * trhost_set_ddgi_probe_variability(enable, stddev_threshold) needs the probe update on (refused without it) and a threshold that
 * is finite and >= 0 (the reference's is 0.001).  On, the volume's descriptor gains flags bit 2 on the host and on the device,
 * the radiance blend writes a coefficient of variation per interior texel, the reduction passes average it over the active
 * probes, and the average goes into one of two read-back slots; every update call first runs the rule on the ring of the last
 * 16 averages (the one read is two calls old, 0 before that) and, once the ring's standard deviation is below the threshold
 * -- on the 18th call at the earliest --, records NOTHING: no refit, trace, blend, placement, reduction or copy.  Lighting goes
 * on reading the volume.  A converged volume never wakes by itself, as in the reference; waking on a light or transform change
 * is not built: trhost_reset_ddgi_variability re-arms it (the whole tracker and the variability buffer start again), and so do
 * trhost_reset_ddgi_volume and every call of trhost_set_ddgi_probe_variability.  trhost_upload_ddgi_volume installs a fresh volume
 * with the option OFF (it strips flags bit 2 from the descriptor it is given): call trhost_set_ddgi_probe_variability again.  A skipped update does not advance
 * the ray rotation's count.  trhost_get_ddgi_variability: the last average read, the ring's standard deviation, the verdict, the
 * rule's sample count and the number of skipped updates (any pointer may be null).
 * trhost_ddgi_variability_run touches no device: it runs the rule over averages[0..n) from a fresh tracker -- per element one
 * Update and, unless that Update found the ring converged (the driver then records nothing and stores nothing), one
 * SetVariabilityForCurrentFrame -- and writes the verdict and the deviation after each Update.
 * trhost_download_ddgi_variability reads the variability buffer back (counts.y x 6 counts.z x 6 counts.x floats; it waits for the
 * device, so it is for tests and tools, not for the frame path). */
int  trhost_set_ddgi_probe_variability(int enable, float stddev_threshold);
int  trhost_get_ddgi_variability(float* average, float* stddev, int* converged, uint32_t* samples, uint32_t* skipped);
int  trhost_reset_ddgi_variability(void);
int  trhost_ddgi_variability_run(const float* averages, uint32_t n, float threshold, uint8_t* converged, float* stddev);
int  trhost_download_ddgi_variability(float* variability, uint64_t variability_bytes);

/* The probe visualisation: GIDebugRenderer (source/GIRenderer.cpp:598-808) on the DDGI volume as it is on the device this frame.
 * trhost_set_ddgi_probe_visualization(enable, probe_radius, hide_inactive): off by default.  On, every frame records behind
 * PostProcessRenderer "giprobevisualization_CS_LoadGIProbes" (every probe's position and state from the live volume),
 * "giprobevisualization_CS_VisualizeGIProbesCulling" on what it wrote, and "giprobevisualization_PS_VisualizeGIProbes", which draws
 * the surviving probes as spheres of probe_radius shaded with their own irradiance into the back buffer, depth-tested against the
 * frame's depth buffer, which it also writes (include/trhip.h).  hide_inactive: the cull drops probes whose state is 1 (honoured only
 * when the volume's classification flag is set).  It needs a volume (trhost_upload_ddgi_volume) and post-processing
 * (trhost_set_post_process): with either missing, trhost_frame fails and says which.  trhost_gi_probe_buffers reads the cull's three
 * outputs as for trhost_load_gi_probes, whose supplied-buffer path keeps its single dispatch and draws nothing; m_IndexCount is 468 here.
 * trhost_get_ddgi_probe_visualization_consts copies the 96 bytes of GIProbeVisualizationConsts (csrc/ShaderInterop.h) the last
 * frame's draw ran with.  trhost_unit_sphere copies the sphere that is drawn, CommonResources' UnitSphere: 91 vertices of 32 bytes
 * (position, normal, texcoord) and 468 uint32 indices; it needs no device. */
int  trhost_set_ddgi_probe_visualization(int enable, float probe_radius, int hide_inactive);
int  trhost_get_ddgi_probe_visualization_consts(void* out96);
int  trhost_unit_sphere(void* vertices, uint64_t vertices_bytes, uint32_t* indices, uint64_t indices_bytes);
/* Auto exposure and tone mapping (AdaptLuminanceRenderer.cpp, PostProcessRenderer.cpp; implies deferred lighting, same refusals):
 * after DeferredLightingRenderer the frame clears the luminance histogram and runs "adaptluminance_CS_GenerateLuminanceHistogram"
 * and "adaptluminance_CS_AdaptExposure" (with a manual exposure > 0: one write of it into the luminance buffer instead), then
 * "postprocess_PS_PostProcess" into the back buffer (RGBA8_UNORM at render resolution, 4 bytes per texel, R in the low byte).
 * trhost_set_exposure: Scene::m_ManualExposureOverride and m_MiddleGray (defaults 0, 0.18).  trhost_set_auto_exposure: the
 * luminance limits and the speed per millisecond (defaults 0.004, 12, 0.0025); trhost_set_frame_time_ms: the mirror of
 * Engine::m_CPUCappedFrameTimeMs (default 16; there is no clock here); m_AdaptationSpeed = clamp(speed * ms, 0, 1) is formed in the
 * renderer.  trhost_upload_bloom: the R11G11B10_FLOAT bloom texture at render resolution and its strength; NULL switches bloom
 * off.  trhost_get_scene_luminance waits for the device and reads the adapted luminance and the exposure texel as they are now
 * (the reference's two-frame-late read-backs are not modelled); trhost_reset_exposure sets both back to 1.0.
 * trhost_get_post_process_consts copies the parameter structs of the last frame: 16 bytes GenerateLuminanceHistogramParameters,
 * 20 bytes AdaptExposureParameters (both as of the last frame that adapted; *adapt_ran tells whether the last one did) and 24
 * bytes PostProcessParameters; any pointer may be NULL.
 * Bloom generation (BloomRenderer.cpp; off by default): trhost_set_bloom(1, nbMips, filterRadius, strength) schedules
 * BloomRenderer between DeferredLightingRenderer and AdaptLuminanceRenderer: nbMips - 1 "bloom_PS_Downsample" and as many
 * "bloom_PS_Upsample" dispatches over an R11G11B10_FLOAT texture of nbMips mips, which "postprocess_PS_PostProcess" then reads
 * at t2 with `strength` (the reference's defaults: 6, 0.005, 0.1).  Refused: post-processing off; nbMips < 2 or above
 * floor(log2(min(W, H))) + 1; a radius that is negative or not finite; an uploaded bloom texture still set -- and while
 * generation is on trhost_upload_bloom refuses a texture.  trhost_set_bloom(0, ...) switches it off.  trhost_download_bloom
 * waits and copies one mip ((W >> mip) x (H >> mip) words); trhost_get_bloom_consts copies the 16 bytes of BloomConsts of pass
 * `pass` < 2 * (nbMips - 1) of the last frame, downsamples first.
 * Temporal anti-aliasing (TAARenderer.cpp; off by default).  trhost_set_taa(1, minBlend, maxSampleCount) (0.1 and 64 are usual)
 * makes View::Update jitter the projection by Graphic::ComputeCurrentJitterOffset's Halton offset (Scene.cpp:113-131) and schedules
 * TAARenderer between AdaptLuminanceRenderer and PostProcessRenderer: one "taa_CS_TemporalResolve" dispatch (csrc/k_taa.hip) from
 * LightingOutput, the depth buffer, the motion target and the history of the frame before into the other history texture and
 * g_AntiAliasedLightingOutput, which "postprocess_PS_PostProcess" then reads at t0; bloom and the histogram keep reading
 * LightingOutput.  m_PrevWorldToClip is then last frame's jittered world-to-clip.  The first frame with it on resets the history,
 * and so does the frame after trhost_reset_taa_history.  Refused: post-processing off; minBlend outside [0, 1]; maxSampleCount
 * outside [1, 65504].  trhost_set_taa(0, ...) switches it off.  trhost_download_anti_aliased_output waits and copies the W x H
 * words, trhost_download_taa_history the W x H x 4 binary16 of the history texture written last (xyz colour, w sample count),
 * trhost_get_taa_consts the 32 bytes of TAAConsts of the last frame and its current and previous jitter offsets in pixels (2 floats
 * each; any pointer may be NULL); all three refuse if the resolve did not run in the last frame.
 * The sky pass (SkyRenderer.cpp; off by default).  trhost_load_sky_dataset copies the Hosek-Wilkie RGB dataset, an input and not
 * part of this library: rgb = 3 x 1080 doubles (per channel 2 albedos x 10 turbidities x 6 control points x 9 parameters), rad =
 * 3 x 120 doubles; NULL unloads it and switches the pass off.  trhost_set_sky(1, turbidity, groundAlbedo) schedules SkyRenderer
 * between DeferredLightingRenderer and BloomRenderer: one "sky_PS_HosekWilkieSky" dispatch that fills every texel of
 * LightingOutput whose depth is <= 0 (the reference's defaults: 2.0 and (0.1, 0.1, 0.1)); the sun direction is the directional
 * light vector as given.  Refused: no dataset loaded; deferred lighting off; a turbidity that is not finite or outside [1, 10];
 * an albedo outside [0, 1].  trhost_set_sky(0, ...) switches it off.  trhost_get_sky_consts copies the 256 bytes of
 * SkyPassParameters of the last frame and refuses if the pass did not run in it.
 * Ambient occlusion (AmbientOcclusionRenderer.cpp, XeGTAO; off by default).  trhost_set_ambient_occlusion(1, quality,
 * denoisePasses, radius, falloffRange, finalValuePower, depthMipSamplingOffset) schedules AmbientOcclusionRenderer between
 * GBufferRenderer and DeferredLightingRenderer (the reference's defaults: 3, 3, 0.5, 0.615, 2.2, 3.3): the prefilter, the main
 * pass and max(1, denoisePasses) denoise dispatches into the SSAO texture, which the lighting pass then binds at t3 with
 * m_SSAOEnabled = 1 (only debug view 9 shows it).  Refused: the G-buffer off; quality or passes above 3; a radius that is negative
 * or not finite; another setting that is not finite.  trhost_set_ambient_occlusion(0, ...) switches it off.  trhost_download_ssao
 * waits and copies the W x H bytes of the SSAO texture; trhost_get_gtao_consts copies the 96 bytes of GTAOConstants of the last
 * frame; both refuse if the pass did not run in it.
 * Ray-traced sun shadows (ShadowMaskRenderer.cpp TraceShadows without denoising; off by default).  trhost_load_raytracing(indices,
 * numIndices, indexCounts, numMeshes), after the scene, its geometry and its materials: the global index buffer (each mesh's LOD-0
 * list at m_GlobalIndexBufferIdx, relative to its first vertex) and one index count per mesh (MeshSpecificData); it builds every
 * mesh's BLAS and the TLAS topology from the instance buffer's current matrices (include/trhip.h, "acceleration structure").
 * trhost_upload_blue_noise: the 128 x 128 RGBA8 image (65536 bytes), an input.  trhost_set_shadow_mask(1, soft, sunAngularDiameter,
 * rayStartOffset) schedules ShadowMaskRenderer between AmbientOcclusionRenderer and DeferredLightingRenderer (the reference's
 * defaults: 1, 0.533 degrees, 0.01 below a scene radius of 3 and 0.1 above): the TLAS refit and the trace into the shadow mask,
 * which the lighting pass then binds at t4.  Refused: the G-buffer off; no structure; no noise; an uploaded shadow mask; a diameter
 * outside [0, 180) or an offset that is negative or not finite.  trhost_set_shadow_mask(0, ...) switches it off.
 * trhost_download_shadow_mask waits and copies the W x H bytes of the mask; trhost_get_shadow_mask_consts copies the 112 bytes of
 * ShadowMaskConsts of the last frame; both refuse if the pass did not run in it. */
int  trhost_set_post_process(int enable);
int  trhost_set_exposure(float manual, float middle_gray);
int  trhost_set_auto_exposure(float min_lum, float max_lum, float speed_per_ms);
int  trhost_set_frame_time_ms(float ms);
int  trhost_upload_bloom(const uint32_t* words, uint64_t bytes, float strength);
int  trhost_set_bloom(int enable, uint32_t nb_mips, float filter_radius, float strength);
int  trhost_download_bloom(uint32_t mip, uint32_t* words, uint64_t bytes);
int  trhost_get_bloom_consts(uint32_t pass, void* out16);
int  trhost_set_taa(int enable, float min_blend, float max_sample_count);
int  trhost_reset_taa_history(void);
int  trhost_download_anti_aliased_output(uint32_t* words, uint64_t bytes);
int  trhost_download_taa_history(void* halves, uint64_t bytes);
int  trhost_get_taa_consts(void* out32, float* current_jitter, float* prev_jitter);
int  trhost_load_sky_dataset(const double* rgb, const double* rad);
int  trhost_set_sky(int enable, float turbidity, const float ground_albedo[3]);
int  trhost_get_sky_consts(void* out256);
int  trhost_set_ambient_occlusion(int enable, uint32_t quality, uint32_t denoise_passes, float radius, float falloff_range, float final_value_power,
                                  float depth_mip_sampling_offset);
int  trhost_download_ssao(uint8_t* bytes, uint64_t size);
int  trhost_get_gtao_consts(void* out96);
int  trhost_load_raytracing(const uint32_t* indices, uint64_t num_indices, const uint32_t* index_counts, uint32_t num_meshes);
int  trhost_upload_blue_noise(const uint8_t* rgba, uint64_t bytes);
int  trhost_set_shadow_mask(int enable, int soft, float sun_angular_diameter, float ray_start_offset);
int  trhost_download_shadow_mask(uint8_t* bytes, uint64_t size);
int  trhost_get_shadow_mask_consts(void* out112);
/* The shadow denoiser (ShadowMaskRenderer::DenoiseShadows; csrc/k_sigma.hip; off by default).  trhost_set_shadow_denoising(1,
 * plane_distance_sensitivity, stabilization_strength, sigma_scale) (0.02 and 5/6: NRD's defaults; 2: this project's choice): the
 * trace then writes the penumbra texture, and "shadowmask_CS_PackNormalAndRoughness" and the four "SIGMA_Shadow_*" dispatches turn it
 * into the mask the lighting pass binds.  Refused: the shadow mask off; a sensitivity that is not finite and > 0, a strength outside
 * [0, 1], a scale that is not finite and >= 0.  trhost_set_shadow_mask(0, ...) switches it off too.  The first frame, the first after
 * it was switched on and the one after trhost_reset_shadow_history run with m_bResetHistory = 1.  The downloads wait and copy the
 * W x H binary16 words of the penumbra texture, the ceil(W / 16) x ceil(H / 16) tile bytes and the W x H binary16 words of the
 * history the last frame wrote; trhost_get_sigma_consts copies the 112 bytes of SigmaConsts (m_Pass 0) of the last frame; all
 * refuse if the denoiser did not run in it.  m_DenoisingRange is 100: the mirror keeps no bounding sphere. */
int  trhost_set_shadow_denoising(int enable, float plane_distance_sensitivity, float stabilization_strength, float sigma_scale);
int  trhost_reset_shadow_history(void);
int  trhost_download_shadow_penumbra(void* halves, uint64_t bytes);
int  trhost_download_shadow_tiles(uint8_t* tiles, uint64_t bytes);
int  trhost_download_shadow_history(void* halves, uint64_t bytes);
int  trhost_get_sigma_consts(void* out112);
int  trhost_download_back_buffer(uint32_t* words, uint64_t bytes);
int  trhost_get_scene_luminance(float* luminance, float* exposure);
int  trhost_reset_exposure(void);
int  trhost_get_post_process_consts(void* histogram16, void* adapt20, void* post24, int* adapt_ran);
int  trhost_download_depth(float* depth, uint64_t bytes);
int  trhost_upload_hzb_mip(uint32_t mip, const uint16_t* texels, uint64_t bytes);
int  trhost_download_hzb_mip(uint32_t mip, uint16_t* texels, uint64_t bytes);
int  trhost_hzb_info(uint32_t* width, uint32_t* height, uint32_t* mips);

/* GI debug view (GIDebugRenderer, GIRenderer.cpp:598-808): probe world positions (3 floats each) and states (1 float each,
 * 1 = RTXGI_DDGI_PROBE_STATE_INACTIVE) as the DDGI volume would provide them; from then on every frame runs
 * "giprobevisualization_CS_VisualizeGIProbesCulling" after the base pass.  num_probes = 0 switches it off.
 * trhost_gi_probe_buffers: trhip_buffer handles of the last dispatch's outputs (positions, DrawIndexedIndirectArguments,
 * instance -> probe index). */
int  trhost_load_gi_probes(const float* positions, const float* states, uint32_t num_probes, float probe_radius, int hide_inactive);
int  trhost_gi_probe_buffers(void** positions, void** draw_args, void** instance_to_probe);

/* Pipeline statistics of the base pass (BasePassRenderers.cpp:178-220,546-549; counters: include/trhip.h).  Off by default;
 * once on, every frame's RenderBasePass brackets itself with one of two queries and first reads the query of two frames
 * earlier, as the reference does.  trhost_pipeline_statistics: last_shown = that value of the last frame (the reference's
 * m_LastPipelineStatistics: frame N - 2, zeros in the first two frames); latest = the last executed frame's own query
 * (waits for it; zeros if no frame has recorded one).  Either pointer may be NULL.  Per device: each rank counts its own. */
int  trhost_set_pipeline_statistics(int enable);
int  trhost_pipeline_statistics(trhip_pipeline_statistics* last_shown, trhip_pipeline_statistics* latest);

int  trhost_frame(void);       /* Graphic::Update: record every pass, submit, (asynchronous)       */
int  trhost_wait_idle(void);

typedef struct {
    int   ran;
    void* records;        /* trhip_buffer handles (include/trhip.h) of the pass slot's outputs      */
    void* dispatch_args;
    void* vis_mask;
    void* visible_list;
    void* draw_args;
    void* late_count;
    void* late_args;
} trhost_pass_buffers_t;
/* slot: 0 early-opaque, 1 late-opaque, 2 early-alpha-mask, 3 late-alpha-mask */
int  trhost_pass_buffers(uint32_t slot, trhost_pass_buffers_t* out);
int  trhost_instance_buffer(void** buffer);
/* Lengths of this process' opaque / alpha-mask id lists (Scene.cpp:282-362). */
int  trhost_scene_list_sizes(uint32_t* num_opaque, uint32_t* num_alpha_mask);
void* trhost_device(void);     /* the trhip_device in use                                           */

/* Multi-GPU (one process per GPU, instance list sharded; not in the reference).  When set, fn(user, hip_stream,
 * late_count, shard_info, bucket, phase) is called on the thread inside trhost_frame while the frame is submitted,
 * twice per bucket (0 opaque, 1 alpha mask):
 *   phase 0  right after the EARLY instance cull: late_count (device address of this rank's late-list length, 1 x u32)
 *            is final from this point of hip_stream on.  Start the exchange -- typically on another stream, after an
 *            event recorded on hip_stream: all-gather late_count, then trhip_launch_shard_late_info fills shard_info
 *            (2 x u32) with {late entries of the lower ranks, late entries of all ranks}.  It has the whole early
 *            meshlet cull and the HZB build to complete.
 *   phase 1  right before the LATE instance cull: make hip_stream wait for shard_info (event wait).
 * The late dispatch then covers exactly the entries the single-GPU dispatch would (gpuculling.hlsl:182-195).
 * fn = NULL removes the hook. */
typedef void (*trhost_shard_late_fn)(void* user, void* hip_stream, void* late_count, void* shard_info, int bucket, int phase);
int  trhost_set_shard_late_exchange(trhost_shard_late_fn fn, void* user);

/* Native per-frame driver of the multi-GPU exchange (protocol: toyrenderer_amd/gather.py).
 * The collectives are callbacks so that the library needs no RCCL at link time: all-gather `count_words` 32-bit words
 * from `send` of every rank into `recv` (rank-major), enqueued on `hip_stream`; return 0 on success.
 * trhost_rccl_allgather is the ready-made binding: user = void*[2] { address of ncclAllGather, the ncclComm_t }. */
typedef int (*trhost_allgather_fn)(void* user, const void* send, void* recv, uint64_t count_words, void* hip_stream);
int  trhost_rccl_allgather(void* user, const void* send, void* recv, uint64_t count_words, void* hip_stream);
int  trhost_rccl_allreduce_max_u32(void* user, void* words, uint64_t count_words, void* hip_stream);   /* user = void*[2] { address of ncclAllReduce, the ncclComm_t } */
typedef struct trhost_exchange_desc {
    uint32_t world, rank;
    uint32_t slot_groups;            /* groups one rank's shard slot holds (the same on every rank)                 */
    uint32_t group_capacity;         /* whole-scene outputs, groups (0: world * slot_groups)                        */
    uint64_t list_capacity;          /* whole-scene visible list, entries (0: 32 * group_capacity)                  */
    uint32_t pass_slot_mask;         /* bit s: gather pass slot s (0 early-opaque, 1 late-opaque, 2/3 alpha mask)   */
    int      overlap;                /* 1: gather + unpack on their own stream, overlapping the next frame          */
    trhost_allgather_fn slots_allgather; void* slots_user;     /* shard slots, once per frame                       */
    trhost_allgather_fn late_allgather;  void* late_user;      /* late-list lengths, inside the frame (1 word)      */
    /* bit 0: SOME rank holds opaque ids, bit 1: some rank holds alpha-mask ids (an all-reduce of trhost_scene_list_sizes
     * at set-up).  Every rank posts the in-frame late-count collective of exactly these buckets, whether its own
     * list is empty or not (an empty list contributes 0), so the collectives match on all ranks.  0 = this rank's
     * own lists (only right when every rank holds the same kinds of lists). */
    uint32_t list_presence_mask;
    /* 1: every rank rasterises only its shard's visible meshlets (trhost_set_raster_depth), so before each
     * GenerateHZB the depth buffers are combined across ranks with `depth_allreduce_max` (element-wise MAX of the
     * reverse-Z depth words; positive floats order like their bit patterns).  Without the callback the combination
     * exchange + raster depth is rejected: per-rank HZBs would make the late and next-frame culls diverge from the
     * single-GPU frame. */
    int (*depth_allreduce_max)(void* user, void* depth_words, uint64_t count_words, void* hip_stream); void* depth_user;
    /* run entries one rank's shard slot holds (the same on every rank): a run = the consecutive records of one
     * submitted instance, so the number of id-list entries of the largest shard bounds it.  0: slot_groups (always
     * enough).  Slot size = 16 + 4 * slot_runs + slot_groups words. */
    uint32_t slot_runs;
    /* Q2 (gpuculling.hlsl:64-74) made global.  > 0: the group capacity (max_groups) of the single-GPU run this exchange
     * reproduces; every rank must run its passes with that same capacity.  The unpack then cuts the rank-major
     * concatenation in front of the first instance the single-GPU pass would drop (its position follows from the ranks'
     * dispatch counters in the slot headers; protocol: toyrenderer_amd/gather.py) and reports {sum of the counters, 1, 1,
     * validRecords}.  0: a rank that drops groups only raises status bit 8 in the whole-scene arguments. */
    uint32_t global_group_capacity;
} trhost_exchange_desc;
int  trhost_exchange_create(const trhost_exchange_desc* desc);   /* also installs the in-frame late-count hook      */
int  trhost_exchange_run(void);                                  /* after trhost_frame: pack, gather, unpack (async) */
int  trhost_exchange_wait(void);                                 /* until the last run's results are complete; fails if the unpack flagged a
                                                                  * pass slot (status word 7 of its arguments: slot overflow, capacity, header, drop) */
/* trhip_buffer handles of the whole-scene results of a pass slot: records, lane masks, ordered visible list,
 * args (8 words: {G,1,1,G}, {V,1,1}, status bits as in gather.py). */
int  trhost_exchange_outputs(uint32_t pass_slot, void** records, void** masks, void** list, void** args);
int  trhost_exchange_destroy(void);

/* Async compute (RenderGraph.cpp:251 "TODO: compute queue" in the reference): which queue a renderer records for --
 * 0 graphics (default), 1 compute = a second stream; the render graph derives the cross-queue waits from the passes'
 * declared resource accesses.  renderer_name: "UpdateInstanceConstsRenderer", "GBufferRenderer", "GIDebugRenderer". */
int  trhost_set_renderer_queue(const char* renderer_name, int queue);
/* Of the last frame: passes on the compute queue, cross-queue waits placed, bytes of live transient resources and what
 * an allocator that aliases non-overlapping pass lifetimes would need for them. */
int  trhost_render_graph_frame_stats(uint32_t* compute_queue_passes, uint32_t* cross_queue_waits, uint64_t* transient_bytes, uint64_t* aliased_bytes);
int  trhost_render_graph_stats(uint32_t* num_heaps, uint64_t* bytes_reserved, uint64_t* bytes_used, uint32_t* num_passes);
/* renderer_name "<frame>": host milliseconds the last trhost_frame spent recording (cpu_ms) and submitting (gpu_ms). */
int  trhost_renderer_times(const char* renderer_name, float* cpu_ms, float* gpu_ms);

/* Test hook (no GPU): drives RenderGraph::Heap's free-list allocator (RenderGraph.cpp:443-580).
 * ops[i] > 0: Allocate(ops[i]) -> results[i] = offset (UINT64_MAX = no fit);
 * ops[i] < 0: Free(results[-ops[i]-1]). */
int  trhost_heap_sim(uint64_t heap_size, const int64_t* ops, uint32_t num_ops, uint64_t* results, uint64_t* used, uint64_t* peak, uint32_t* num_blocks);

/* TEXTURE STREAMING (csrc/host/TextureFeedbackManager.h; include/trhip.h "texture streaming"; opt-in, off by default).  Switched on
 * BEFORE the first trhost_create_material_texture: a texture created afterwards whose size is a multiple of the region (default: D3D's
 * 64 KB tile shape of its format; trhost_set_texture_streaming_region gives another, and then a size that is no multiple is refused)
 * keeps its mips on the host and only its packed tail on the device, with the rest filled with 0xFF00FFFF when poison != 0;
 * trhost_load_materials fills the two map indices of its slots in, accepts them when they name the maps of that very texture and
 * refuses anything else.  Every frame with the G-buffer resolve then runs TextureFeedbackManager::BeginFrame (what earlier frames
 * decoded and has arrived -- polled, never waited for --, the residency rule, tile uploads, min-mip rewrites, round-robin over
 * textures_per_frame textures, clear) and EndFrame (decode, copy to the read-back).  A tile that none of the last evict_after
 * processed feedbacks of its texture required is unmapped.  Refused together with trhost_set_alpha_test.
 * stats: tiles total, tiles resident, tiles uploaded by the last frame, bytes uploaded by the last frame, textures processed by it.
 * trhost_download_min_mip: the device's min-mip map of a streamed texture (one byte per region, row-major); dst NULL asks for the
 * size alone. */
int  trhost_set_texture_streaming(int enable, uint32_t textures_per_frame, uint32_t evict_after, int poison);
int  trhost_set_texture_streaming_region(uint32_t region_w, uint32_t region_h);
int  trhost_get_texture_streaming_stats(uint64_t stats[5]);
int  trhost_download_min_mip(uint32_t texture, uint8_t* dst, uint64_t bytes, uint32_t* regions_x, uint32_t* regions_y);

/* The residency rule of texture streaming (csrc/host/TextureResidency.h states it; no GPU, no initialised host needed): one round
 * of one streamable texture of width x height texels and `mips` levels with regions of region_w x region_h texels.  feedback: one
 * decoded byte per region (0xFF = never sampled).  resident (bytes) and idle (words): one entry per tile, levels 0 .. S - 1 one
 * after the other, row-major; updated in place.  mapped, unmapped: one byte per tile, set for the tiles this round maps / unmaps.
 * min_mip: one byte per region, rewritten.  stats: tiles total, tiles resident, tiles mapped, tiles unmapped, bytes uploaded
 * (tiles mapped x tile_bytes).  num_tiles: the length of the per-tile arrays, which must be the texture's tile count
 * (trhost_residency_tiles). */
int  trhost_residency_tiles(uint32_t width, uint32_t height, uint32_t mips, uint32_t region_w, uint32_t region_h, uint32_t* standard_levels, uint32_t* num_tiles);
int  trhost_residency_round(uint32_t width, uint32_t height, uint32_t mips, uint32_t region_w, uint32_t region_h, uint32_t tile_bytes,
                            const uint8_t* feedback, uint32_t evict_after, uint32_t num_tiles, uint8_t* resident, uint32_t* idle,
                            uint8_t* mapped, uint8_t* unmapped, uint8_t* min_mip, uint64_t stats[5]);

#ifdef __cplusplus
}
#endif
#endif /* TRHOST_H_ */
