// trhost_capi.cpp -- a small C entry-point set over the C++ host mirror so that Python (tests,
// bench.py) can drive the SAME code path a C++ application would: Graphic::Initialize ->
// Scene::LoadFromArrays -> Graphic::Update per frame (Scene::Update -> RenderGraph -> renderers ->
// AddComputePass -> C ABI -> HIP kernels).  Declared in include/trhost.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../../include/trhost.h"
#include "CommonResources.h"
#include "Graphic.h"
#include "GraphicConstants.h"
#include "RenderGraph.h"
#include "Scene.h"
#include "TextureFeedbackManager.h"
#include "TextureResidency.h"
#include "VisibilityOutputs.h"
#include "../ShaderInterop.h"

namespace
{
thread_local std::string tl_error;
bool s_Initialized = false;

template <typename F> int guarded(F&& f)
{
    try {
        f();
        return 0;
    } catch (const std::exception& e) {
        tl_error = e.what();
        return -1;
    }
}

Matrix toMatrix(const float* m)
{
    Matrix r;
    std::memcpy(r.m, m, sizeof r.m);
    return r;
}
} // namespace

extern "C" {

const char* trhost_last_error(void) { return tl_error.c_str(); }

int trhost_initialize(int device_index, uint32_t render_width, uint32_t render_height, void* external_hip_stream)
{
    if (s_Initialized) { tl_error = "trhost_initialize: already initialized (call trhost_shutdown first)"; return -1; }
    int rc = guarded([&] { g_Graphic.Initialize(device_index, Vector2U{ render_width, render_height }, external_hip_stream); });
    s_Initialized = rc == 0;
    return rc;
}

void trhost_shutdown(void)
{
    if (!s_Initialized) return;
    (void)guarded([&] {
        ShardExchangeDestroy();
        ReleaseVisibilityPassBuffers();
        ReleaseGIProbeCullBuffers();
        ReleaseDeferredLightingOutputs();
        ReleasePostProcessOutputs();
        ReleaseBloomOutputs();
        ReleaseTAAOutputs();
        ReleaseSkyOutputs();
        ReleaseAmbientOcclusionOutputs();
        ReleaseShadowMaskOutputs();
        g_Graphic.Shutdown();
    });
    s_Initialized = false;
}

int trhost_load_scene(const void* instances, uint32_t num_instances, const void* mesh_data, uint32_t num_meshes,
                      const void* meshlets, uint64_t num_meshlets, const uint32_t* opaque_ids, uint32_t num_opaque,
                      const uint32_t* alpha_mask_ids, uint32_t num_alpha_mask)
{
    return guarded([&] {
        g_Scene->LoadFromArrays(instances, num_instances, mesh_data, num_meshes, meshlets, num_meshlets, opaque_ids, num_opaque, alpha_mask_ids, num_alpha_mask);
        g_Graphic.PostSceneLoad();
    });
}

int trhost_upload_meshlets(uint64_t first_meshlet, const void* meshlets, uint64_t count)
{
    return guarded([&] {
        check(g_Graphic.m_GlobalMeshletDataBuffer);
        nvrhi::throwIfFailed(trhip_buffer_upload(g_Graphic.m_GlobalMeshletDataBuffer->native(), first_meshlet * sizeof(interop::MeshletData), meshlets,
                                                 count * sizeof(interop::MeshletData)), "trhost_upload_meshlets");
    });
}

int trhost_load_scene_cached(const char* cached_data_path, const void* instances, uint32_t num_instances, const uint32_t* opaque_ids, uint32_t num_opaque,
                             const uint32_t* alpha_mask_ids, uint32_t num_alpha_mask)
{
    return guarded([&] {
        check(cached_data_path && instances);
        g_Scene->LoadCachedData(cached_data_path, instances, num_instances, opaque_ids, num_opaque, alpha_mask_ids, num_alpha_mask);
        g_Graphic.PostSceneLoad();
    });
}

int trhost_load_geometry(const void* vertices, uint64_t num_vertices, const uint32_t* meshlet_vertex_ids, uint64_t num_vertex_ids,
                         const uint32_t* meshlet_triangles, uint64_t num_triangles)
{
    return guarded([&] {
        check(g_Scene && (vertices || !num_vertices) && (meshlet_vertex_ids || !num_vertex_ids) && (meshlet_triangles || !num_triangles));
        g_Scene->LoadGeometry(vertices, num_vertices, meshlet_vertex_ids, num_vertex_ids, meshlet_triangles, num_triangles);
    });
}

int trhost_set_raster_depth(int enable)
{
    return guarded([&] {
        check(!enable || g_Graphic.m_GlobalVertexBuffer);      // trhost_load_geometry first
        g_Scene->m_bRasterDepth = enable != 0;
    });
}

int trhost_set_visibility_buffer(int enable)
{
    return guarded([&] {
        check(!enable || g_Graphic.m_GlobalVertexBuffer);      // trhost_load_geometry first
        if (enable && g_Graphic.m_MaxMeshletGroups > (1u << 18))
            throw nvrhi::Error("trhost_set_visibility_buffer: max_meshlet_groups above 2^18 (list positions must stay below 2^23)");
        g_Scene->m_bVisibilityBuffer = enable != 0;
        if (enable) g_Scene->m_bRasterDepth = true;            // implies raster depth
    });
}

int trhost_load_materials(const void* materials, uint32_t count)
{
    return guarded([&] {
        check(g_Scene && (materials || !count));
        g_Scene->LoadMaterials(materials, count);
    });
}

// nvrhi::Format of a TRHIP_FORMAT_* that a material texture may have
static nvrhi::Format MaterialTextureFormat(const char* who, uint32_t format)
{
    if (format == TRHIP_FORMAT_RGBA8_UNORM) return nvrhi::Format::RGBA8_UNORM;
    if (format == TRHIP_FORMAT_SRGBA8_UNORM) return nvrhi::Format::SRGBA8_UNORM;
    if (format >= TRHIP_FORMAT_BC1_UNORM && format <= TRHIP_FORMAT_BC5_UNORM) return (nvrhi::Format)((uint32_t)nvrhi::Format::BC1_UNORM + (format - TRHIP_FORMAT_BC1_UNORM));
    throw nvrhi::Error(std::string(who) + ": format " + std::to_string(format) + ": a material texture is TRHIP_FORMAT_RGBA8_UNORM, TRHIP_FORMAT_SRGBA8_UNORM or one of TRHIP_FORMAT_BC1_UNORM .. TRHIP_FORMAT_BC5_UNORM");
}

int trhost_create_material_texture(uint32_t width, uint32_t height, uint32_t mips, uint32_t format, const void* data, uint64_t bytes)
{
    int index = -1;
    int rc = guarded([&] {
        check(g_Scene);
        index = (int)g_Graphic.CreateMaterialTexture(width, height, mips, MaterialTextureFormat("trhost_create_material_texture", format), data, bytes);
    });
    return rc == 0 ? index : -1;
}

int trhost_create_material_texture_dds(const void* file, uint64_t bytes, int srgb)
{
    int index = -1;
    int rc = guarded([&] {
        check(g_Scene && file);
        trhip_dds_info info;
        nvrhi::throwIfFailed(trhip_dds_parse(file, bytes, &info), "trhost_create_material_texture_dds");
        // the material slot decides between a format and its _SRGB twin, whatever the file says (the pairs are adjacent values)
        uint32_t format = info.format;
        const bool pair = format == TRHIP_FORMAT_RGBA8_UNORM || format == TRHIP_FORMAT_SRGBA8_UNORM || (format >= TRHIP_FORMAT_BC1_UNORM && format <= TRHIP_FORMAT_BC3_UNORM_SRGB);
        if (pair) format = ((format - TRHIP_FORMAT_RGBA8_UNORM) & ~1u) + TRHIP_FORMAT_RGBA8_UNORM + (srgb ? 1u : 0u);
        uint64_t total = 0;
        for (uint32_t k = 0; k < info.mipLevels; ++k) total += info.levelBytes[k];                  // the levels are contiguous in the file
        index = (int)g_Graphic.CreateMaterialTexture(info.width, info.height, info.mipLevels, MaterialTextureFormat("trhost_create_material_texture_dds", format),
                                                     (const uint8_t*)file + info.levelOffset[0], total);
    });
    return rc == 0 ? index : -1;
}

int trhost_set_gbuffer(int enable)
{
    return guarded([&] {
        check(!enable || g_Graphic.m_GlobalVertexBuffer);      // trhost_load_geometry first
        if (enable && !g_Graphic.m_GlobalMaterialDataBuffer) throw nvrhi::Error("trhost_set_gbuffer: no materials (trhost_load_materials first)");
        if (enable && g_Graphic.m_MaxMeshletGroups > (1u << 18))
            throw nvrhi::Error("trhost_set_gbuffer: max_meshlet_groups above 2^18 (list positions must stay below 2^23)");
        g_Scene->m_bGBuffer = enable != 0;
        if (enable) { g_Scene->m_bVisibilityBuffer = true; g_Scene->m_bRasterDepth = true; }   // implies the visibility buffer
    });
}

int trhost_set_alpha_test(int enabled)
{
    return guarded([&] {
        check(g_Scene);
        if (enabled && !g_Scene->m_bRasterDepth)
            throw nvrhi::Error("trhost_set_alpha_test: the rasters are off (trhost_set_raster_depth, trhost_set_visibility_buffer or trhost_set_gbuffer first): the test runs in them");
        if (enabled && !g_Graphic.m_GlobalMaterialDataBuffer) throw nvrhi::Error("trhost_set_alpha_test: no materials (trhost_load_materials first)");
        if (enabled && g_TextureFeedbackManager.m_bEnabled)
            throw nvrhi::Error("trhost_set_alpha_test: texture streaming is on, and the alpha-tested rasters and the sun rays do not honour the min-mip map yet");
        g_Scene->m_bAlphaTest = enabled != 0;
    });
}

int trhost_set_texture_streaming(int enable, uint32_t textures_per_frame, uint32_t evict_after, int poison)
{
    return guarded([&] {
        check(g_Scene);
        TextureFeedbackManager& m = g_TextureFeedbackManager;
        if (enable && g_Scene->m_bAlphaTest)
            throw nvrhi::Error("trhost_set_texture_streaming: alpha_test is on, and the alpha-tested rasters and the sun rays do not honour the min-mip map yet");
        if (enable && (!textures_per_frame || !evict_after)) throw nvrhi::Error("trhost_set_texture_streaming: textures_per_frame and evict_after are at least 1");
        if ((enable != 0) != m.m_bEnabled && !g_Graphic.m_Textures.empty() && (enable || !m.m_Textures.empty()))
            throw nvrhi::Error("trhost_set_texture_streaming: material textures exist already; streaming is switched before the first trhost_create_material_texture");
        m.m_bEnabled = enable != 0;
        if (enable) { m.m_TexturesPerFrame = textures_per_frame; m.m_EvictAfter = evict_after; m.m_bPoison = poison != 0; }
    });
}

int trhost_set_texture_streaming_region(uint32_t region_w, uint32_t region_h)
{
    return guarded([&] {
        check(g_Scene);
        auto pow2 = [](uint32_t v) { return v >= 4u && (v & (v - 1u)) == 0u; };
        if ((region_w || region_h) && (!pow2(region_w) || !pow2(region_h))) throw nvrhi::Error("trhost_set_texture_streaming_region: the sides of a region are powers of two, at least 4 (0 x 0: the format's default)");
        g_TextureFeedbackManager.m_RegionW = region_w; g_TextureFeedbackManager.m_RegionH = region_h;
    });
}

int trhost_get_texture_streaming_stats(uint64_t stats[5])
{
    return guarded([&] {
        check(g_Scene && stats);
        const TextureFeedbackManager::Stats& s = g_TextureFeedbackManager.m_Stats;
        stats[0] = s.tilesTotal; stats[1] = s.tilesResident; stats[2] = s.tilesUploaded; stats[3] = s.bytesUploaded; stats[4] = s.texturesProcessed;
    });
}

int trhost_download_min_mip(uint32_t texture, uint8_t* dst, uint64_t bytes, uint32_t* regions_x, uint32_t* regions_y)
{
    return guarded([&] {
        check(g_Scene);
        const TextureFeedbackManager::Streamed* s = g_TextureFeedbackManager.Find(texture);
        if (!s) throw nvrhi::Error("trhost_download_min_mip: texture " + std::to_string(texture) + " is not streamed");
        if (regions_x) *regions_x = s->m_Tiled.regionsX();
        if (regions_y) *regions_y = s->m_Tiled.regionsY();
        if (!dst) return;
        if (bytes != s->m_MinMipBytes.size()) throw nvrhi::Error("trhost_download_min_mip: the map is " + std::to_string(s->m_MinMipBytes.size()) + " bytes, got " + std::to_string(bytes));
        nvrhi::throwIfFailed(trhip_texture_download(s->m_MinMip->native(), 0, dst, bytes), "trhost_download_min_mip");
    });
}

int trhost_set_debug_view_mode(uint32_t mode)
{
    return guarded([&] {
        check(g_Scene);
        if (mode == interop::kDeferredLightingDebugMode_Ambient && g_Scene->m_bDeferredLighting && !g_Scene->m_RTDDGIVolume.IsValid())
            throw nvrhi::Error("trhost_set_debug_view_mode: mode 10 (Ambient) needs the DDGI volume, which deferredlighting_PS_Main_Debug does not have (trhost_upload_ddgi_volume first)");
        g_Scene->m_DebugViewMode = mode;
    });
}

int trhost_set_deferred_lighting(int enable)
{
    return guarded([&] {
        check(!enable || g_Graphic.m_GlobalVertexBuffer);      // trhost_load_geometry first
        if (enable && !g_Graphic.m_GlobalMaterialDataBuffer) throw nvrhi::Error("trhost_set_deferred_lighting: no materials (trhost_load_materials first)");
        if (enable && g_Graphic.m_MaxMeshletGroups > (1u << 18))
            throw nvrhi::Error("trhost_set_deferred_lighting: max_meshlet_groups above 2^18 (list positions must stay below 2^23)");
        if (enable && g_Scene->m_DebugViewMode == interop::kDeferredLightingDebugMode_Ambient && !g_Scene->m_RTDDGIVolume.IsValid())
            throw nvrhi::Error("trhost_set_deferred_lighting: debug view mode 10 (Ambient) needs the DDGI volume, which deferredlighting_PS_Main_Debug does not have");
        g_Scene->m_bDeferredLighting = enable != 0;
        if (enable) { g_Scene->m_bGBuffer = true; g_Scene->m_bVisibilityBuffer = true; g_Scene->m_bRasterDepth = true; }   // implies the G-buffer
    });
}

int trhost_set_directional_light(const float vec[3], float strength)
{
    return guarded([&] {
        check(g_Scene && vec);
        memcpy(g_Scene->m_DirLightVec, vec, sizeof g_Scene->m_DirLightVec);
        g_Scene->m_DirLightStrength = strength;
    });
}

int trhost_upload_shadow_mask(const uint8_t* texels, uint64_t bytes)
{
    return guarded([&] {
        check(g_Scene);
        if (!texels) { g_Scene->m_ShadowMaskTexture = nullptr; return; }      // white
        if (!g_Scene->m_ShadowMaskTexture) {
            nvrhi::TextureDesc desc;
            desc.width = g_Graphic.m_RenderResolution.x;
            desc.height = g_Graphic.m_RenderResolution.y;
            desc.format = GraphicConstants::kShadowMaskFormat;
            desc.debugName = "Shadow Mask";
            g_Scene->m_ShadowMaskTexture = g_Graphic.m_NVRHIDevice->createTexture(desc);
        }
        nvrhi::throwIfFailed(trhip_texture_upload(g_Scene->m_ShadowMaskTexture->native(), 0, texels, bytes), "trhost_upload_shadow_mask");
    });
}

int trhost_upload_ddgi_volume(const void* desc64, const uint32_t* irradiance, uint64_t irradiance_bytes, const uint16_t* distance, uint64_t distance_bytes,
                              const uint16_t* data, uint64_t data_bytes)
{
    return guarded([&] {
        check(g_Scene);
        if (!desc64) {                                                        // drop the volume
            if (g_Scene->m_DebugViewMode == interop::kDeferredLightingDebugMode_Ambient && g_Scene->m_bDeferredLighting)
                throw nvrhi::Error("trhost_upload_ddgi_volume: debug view mode 10 (Ambient) is showing the DDGI volume");
            g_Scene->m_RTDDGIVolume = Scene::RTDDGIVolume{};
            g_Scene->m_bEnableDDGI = g_Scene->m_bDDGIUpdate = g_Scene->m_bDDGIProbeRelocation = g_Scene->m_bDDGIProbeClassification = false;
            return;
        }
        check(irradiance && distance && data);
        interop::DDGIVolumeDesc d;
        memcpy(&d, desc64, sizeof d);
        d.flags &= ~interop::kDDGIFlag_Variability;                           // trhost_set_ddgi_probe_variability's to set, with the buffers the bit needs
        for (int a = 0; a < 3; ++a) {
            if (d.probeCounts[a] < 1 || d.probeCounts[a] > (int)interop::kDDGIMaxProbeCount) throw nvrhi::Error("trhost_upload_ddgi_volume: a DDGI probe count is not in 1..1024");
            if (!(d.probeSpacing[a] > 0.0f && d.probeSpacing[a] <= 3.402823466e38f)) throw nvrhi::Error("trhost_upload_ddgi_volume: a DDGI probe spacing is not positive and finite");
        }
        if (d.numIrradianceInteriorTexels != interop::kDDGIIrradianceInteriorTexels || d.numDistanceInteriorTexels != interop::kDDGIDistanceInteriorTexels)
            throw nvrhi::Error("trhost_upload_ddgi_volume: the DDGI probe tiles have 6 (irradiance) and 14 (distance) interior texels");
        const uint32_t cx = (uint32_t)d.probeCounts[0], cy = (uint32_t)d.probeCounts[1], cz = (uint32_t)d.probeCounts[2];
        const uint64_t irrSlice = (uint64_t)cx * 8 * cz * 8 * 4, distSlice = (uint64_t)cx * 16 * cz * 16 * 4, dataSlice = (uint64_t)cx * cz * 8;
        if (irradiance_bytes != irrSlice * cy || distance_bytes != distSlice * cy || data_bytes != dataSlice * cy)
            throw nvrhi::Error("trhost_upload_ddgi_volume: the DDGI texture sizes do not match the probe counts (irradiance 8 x 8 x 4, distance 16 x 16 x 4, data 8 bytes per probe)");
        Scene::RTDDGIVolume v;                                                // GIRenderer.cpp:129-133 CreateProbeTexture, kProbeTextureFormats
        v.m_Desc = d;
        auto make = [&](uint32_t perProbe, nvrhi::Format format, const char* name) {
            nvrhi::TextureDesc desc;
            desc.width = cx * perProbe; desc.height = cz * perProbe; desc.arraySize = cy;
            desc.dimension = nvrhi::kTexture2DArray;
            desc.format = format;
            desc.debugName = name;
            desc.isUAV = true;                                                // the blends write irradiance and distance, relocation and classification the data
            return g_Graphic.m_NVRHIDevice->createTexture(desc);
        };
        v.m_ProbeData = make(1, nvrhi::Format::RGBA16_FLOAT, "DDGI Probe Data");
        v.m_ProbeIrradiance = make(8, nvrhi::Format::R10G10B10A2_UNORM, "DDGI Probe Irradiance");
        v.m_ProbeDistance = make(16, nvrhi::Format::RG16_FLOAT, "DDGI Probe Distance");
        nvrhi::BufferDesc bd;
        bd.byteSize = sizeof d; bd.structStride = sizeof d; bd.debugName = "DDGI Volume Desc";
        v.m_DescBuffer = g_Graphic.m_NVRHIDevice->createBuffer(bd);
        nvrhi::throwIfFailed(trhip_buffer_upload(v.m_DescBuffer->native(), 0, &d, sizeof d), "trhost_upload_ddgi_volume");
        for (uint32_t s = 0; s < cy; ++s) {
            nvrhi::throwIfFailed(trhip_texture_upload_slice(v.m_ProbeData->native(), s, (const char*)data + s * dataSlice, dataSlice), "trhost_upload_ddgi_volume");
            nvrhi::throwIfFailed(trhip_texture_upload_slice(v.m_ProbeIrradiance->native(), s, (const char*)irradiance + s * irrSlice, irrSlice), "trhost_upload_ddgi_volume");
            nvrhi::throwIfFailed(trhip_texture_upload_slice(v.m_ProbeDistance->native(), s, (const char*)distance + s * distSlice, distSlice), "trhost_upload_ddgi_volume");
        }
        {                                                                     // the ray data of GIRenderer::Setup, as float4 records; zero-filled
            const uint64_t rayBytes = (uint64_t)cx * cy * cz * interop::kDDGIRaysPerProbe * 16;
            nvrhi::BufferDesc rd;
            rd.byteSize = rayBytes; rd.structStride = 16; rd.canHaveUAVs = true; rd.debugName = "DDGI Ray Data";
            v.m_RayData = g_Graphic.m_NVRHIDevice->createBuffer(rd);
            const std::vector<uint8_t> zeros(rayBytes, 0);
            nvrhi::throwIfFailed(trhip_buffer_upload(v.m_RayData->native(), 0, zeros.data(), rayBytes), "trhost_upload_ddgi_volume");
        }
        {                                                                     // the distances of every probe's 32 fixed rays; zero-filled
            const uint64_t bytes = (uint64_t)cx * cy * cz * interop::kDDGIFixedRays * 4;
            nvrhi::BufferDesc fd;
            fd.byteSize = bytes; fd.structStride = 4; fd.canHaveUAVs = true; fd.debugName = "DDGI Fixed Ray Distances";
            v.m_FixedRayData = g_Graphic.m_NVRHIDevice->createBuffer(fd);
            const std::vector<uint8_t> zeros(bytes, 0);
            nvrhi::throwIfFailed(trhip_buffer_upload(v.m_FixedRayData->native(), 0, zeros.data(), bytes), "trhost_upload_ddgi_volume");
        }
        if ((g_Scene->m_bDDGIProbeRelocation && !(d.flags & interop::kDDGIFlag_Relocation)) || (g_Scene->m_bDDGIProbeClassification && !(d.flags & interop::kDDGIFlag_Classification)))
            g_Scene->m_bDDGIProbeRelocation = g_Scene->m_bDDGIProbeClassification = false;     // the new volume's flags do not allow what was set
        g_Scene->m_RTDDGIVolume = v;                                          // a fresh tracker with it: probe variability is off on a new volume
        g_Scene->m_DDGIUpdateCount = 0;
    });
}

// The variability buffer zeroed, the read-back's pending slots dropped, the whole tracker re-initialised (the reference resets
// only the count); the switch and the threshold stay.  The caller has drained the device.
static void ResetDDGIVariability(Scene::RTDDGIVolume& v)
{
    v.m_Variability.Reset();
    v.m_NumUpdateCalls = v.m_NumUpdatesSkipped = 0;
    if (!v.m_ProbeVariability) return;
    const std::vector<uint8_t> zeros(v.m_ProbeVariability->getDesc().byteSize, 0);
    nvrhi::throwIfFailed(trhip_buffer_upload(v.m_ProbeVariability->native(), 0, zeros.data(), zeros.size()), "the probe variability");
    if (v.m_ProbeVariabilityReadback) g_Graphic.m_NVRHIDevice->resetStagingBuffer(v.m_ProbeVariabilityReadback);     // the frame's list may still name it
    else v.m_ProbeVariabilityReadback = g_Graphic.m_NVRHIDevice->createStagingBuffer(sizeof(float), 2);
}

int trhost_set_ddgi_probe_variability(int enable, float stddev_threshold)
{
    return guarded([&] {
        check(g_Scene);
        Scene::RTDDGIVolume& v = g_Scene->m_RTDDGIVolume;
        if (enable && !(g_Scene->m_bDDGIUpdate && v.IsValid()))
            throw nvrhi::Error("trhost_set_ddgi_probe_variability: the probe update is off (trhost_set_ddgi_update first): ReductionCS_DDGIReductionCS has no blend whose variability it could average");
        if (enable && !(stddev_threshold >= 0.0f && stddev_threshold <= 3.402823466e38f))
            throw nvrhi::Error("trhost_set_ddgi_probe_variability: stddev_threshold must be finite and >= 0");
        if (!v.IsValid()) return;                                             // nothing to switch off
        g_Graphic.m_NVRHIDevice->waitForIdle();
        if (enable && !v.m_ProbeVariability) {
            const uint64_t cx = (uint64_t)v.m_Desc.probeCounts[0], cy = (uint64_t)v.m_Desc.probeCounts[1], cz = (uint64_t)v.m_Desc.probeCounts[2];
            const uint64_t texels = cx * cy * cz * 36;
            if (texels > (1ull << 24)) throw nvrhi::Error("trhost_set_ddgi_probe_variability: the volume has more than 2^24 interior irradiance texels; the reduction counts them in a float");
            nvrhi::BufferDesc bd;
            bd.byteSize = texels * sizeof(float); bd.structStride = sizeof(float); bd.canHaveUAVs = true; bd.debugName = "DDGI Probe Variability";
            v.m_ProbeVariability = g_Graphic.m_NVRHIDevice->createBuffer(bd);
            nvrhi::BufferDesc ad;                                             // the first pass's outputs; every later pass has fewer
            ad.byteSize = ((cx * 6 + 15) / 16) * ((cz * 6 + 15) / 16) * ((cy + 3) / 4) * 2 * sizeof(float); ad.structStride = 2 * sizeof(float); ad.canHaveUAVs = true;
            ad.debugName = "DDGI Probe Variability Average 0";
            v.m_ProbeVariabilityAverage[0] = g_Graphic.m_NVRHIDevice->createBuffer(ad);
            ad.debugName = "DDGI Probe Variability Average 1";
            v.m_ProbeVariabilityAverage[1] = g_Graphic.m_NVRHIDevice->createBuffer(ad);
        }
        v.m_Variability.m_bProbeVariabilityEnabled = enable != 0;
        if (enable) v.m_Variability.m_VariabilityStdDevThreshold = stddev_threshold;
        // the descriptor's bit 2, on the host and on the device alike
        v.m_Desc.flags = enable ? (v.m_Desc.flags | interop::kDDGIFlag_Variability) : (v.m_Desc.flags & ~interop::kDDGIFlag_Variability);
        nvrhi::throwIfFailed(trhip_buffer_upload(v.m_DescBuffer->native(), 0, &v.m_Desc, sizeof v.m_Desc), "trhost_set_ddgi_probe_variability");
        ResetDDGIVariability(v);
    });
}

int trhost_get_ddgi_variability(float* average, float* stddev, int* converged, uint32_t* samples, uint32_t* skipped)
{
    return guarded([&] {
        check(g_Scene);
        const Scene::RTDDGIVolume& v = g_Scene->m_RTDDGIVolume;
        if (average) *average = v.m_Variability.m_AverageVariability;
        if (stddev) *stddev = v.m_Variability.m_VariabilityStdDev;
        if (converged) *converged = v.m_Variability.bIsConverged ? 1 : 0;
        if (samples) *samples = v.m_Variability.m_NumVolumeVariabilitySamples;
        if (skipped) *skipped = v.m_NumUpdatesSkipped;
    });
}

int trhost_reset_ddgi_variability(void)
{
    return guarded([&] {
        check(g_Scene);
        Scene::RTDDGIVolume& v = g_Scene->m_RTDDGIVolume;
        if (!v.IsValid()) throw nvrhi::Error("trhost_reset_ddgi_variability: no DDGI volume (trhost_upload_ddgi_volume first)");
        g_Graphic.m_NVRHIDevice->waitForIdle();
        ResetDDGIVariability(v);
    });
}

int trhost_ddgi_variability_run(const float* averages, uint32_t n, float threshold, uint8_t* converged, float* stddev)
{
    return guarded([&] {
        check((averages && converged && stddev) || n == 0);
        DDGIVariability t;
        t.m_bProbeVariabilityEnabled = true;
        t.m_VariabilityStdDevThreshold = threshold;
        for (uint32_t i = 0; i < n; ++i) {
            t.Update();
            converged[i] = t.bIsConverged ? 1 : 0;
            stddev[i] = t.m_VariabilityStdDev;
            if (!t.bIsConverged) t.SetVariabilityForCurrentFrame(averages[i]);
        }
    });
}

int trhost_download_ddgi_variability(float* variability, uint64_t variability_bytes)
{
    return guarded([&] {
        check(g_Scene);
        const Scene::RTDDGIVolume& v = g_Scene->m_RTDDGIVolume;
        if (!v.m_ProbeVariability) throw nvrhi::Error("trhost_download_ddgi_variability: probe variability was never switched on (trhost_set_ddgi_probe_variability)");
        if (!variability || variability_bytes != v.m_ProbeVariability->getDesc().byteSize)
            throw nvrhi::Error("trhost_download_ddgi_variability: needs counts.y x 6 counts.z x 6 counts.x floats");
        g_Graphic.m_NVRHIDevice->waitForIdle();
        nvrhi::throwIfFailed(trhip_buffer_download(v.m_ProbeVariability->native(), 0, variability, variability_bytes), "trhost_download_ddgi_variability");
    });
}

int trhost_set_ddgi_update(int enabled, uint32_t seed)
{
    return guarded([&] {
        check(g_Scene);
        if (enabled && !g_Scene->m_RTDDGIVolume.IsValid())
            throw nvrhi::Error("trhost_set_ddgi_update: no DDGI volume (trhost_upload_ddgi_volume first): giprobetrace_CS_ProbeTrace and the probe blends have nothing to fill");
        if (enabled && !g_Scene->m_TLAS)
            throw nvrhi::Error("trhost_set_ddgi_update: no acceleration structure (trhost_load_raytracing first): giprobetrace_CS_ProbeTrace has nothing to trace");
        g_Scene->m_bDDGIUpdate = enabled != 0;
        g_Scene->m_DDGIUpdateSeed = seed;
        g_Scene->m_DDGIUpdateCount = 0;
    });
}

int trhost_set_ddgi_probe_placement(int relocation, int classification, float min_frontface_distance, float fixed_ray_backface_threshold)
{
    return guarded([&] {
        check(g_Scene);
        const Scene::RTDDGIVolume& v = g_Scene->m_RTDDGIVolume;
        if ((relocation || classification) && !v.IsValid())
            throw nvrhi::Error("trhost_set_ddgi_probe_placement: no DDGI volume (trhost_upload_ddgi_volume first): ProbeRelocationCS_DDGIProbeRelocationCS and "
                               "ProbeClassificationCS_DDGIProbeClassificationCS have no probes to place");
        if (relocation && !(v.m_Desc.flags & interop::kDDGIFlag_Relocation))
            throw nvrhi::Error("trhost_set_ddgi_probe_placement: the volume's flags have relocation (bit 0) off: nothing would read what ProbeRelocationCS_DDGIProbeRelocationCS writes");
        if (classification && !(v.m_Desc.flags & interop::kDDGIFlag_Classification))
            throw nvrhi::Error("trhost_set_ddgi_probe_placement: the volume's flags have classification (bit 1) off: nothing would read what ProbeClassificationCS_DDGIProbeClassificationCS writes");
        if (!(min_frontface_distance >= 0.0f && min_frontface_distance <= 3.402823466e38f) || !(fixed_ray_backface_threshold >= 0.0f && fixed_ray_backface_threshold <= 1.0f))
            throw nvrhi::Error("trhost_set_ddgi_probe_placement: min_frontface_distance must be finite and >= 0, fixed_ray_backface_threshold in [0, 1]");
        g_Scene->m_bDDGIProbeRelocation = relocation != 0;
        g_Scene->m_bDDGIProbeClassification = classification != 0;
        g_Scene->m_DDGIMinFrontfaceDistance = min_frontface_distance;
        g_Scene->m_DDGIFixedRayBackfaceThreshold = fixed_ray_backface_threshold;
    });
}

int trhost_set_ddgi_probe_visualization(int enable, float probe_radius, int hide_inactive)
{
    return guarded([&] {
        check(g_Scene);
        if (enable && !(probe_radius > 0.0f && probe_radius <= 3.402823466e38f))
            throw nvrhi::Error("trhost_set_ddgi_probe_visualization: probe_radius must be positive and finite");
        g_Scene->m_bDDGIProbeVisualization = enable != 0;                     // what it needs is checked when a frame is asked for
        g_Scene->m_DDGIProbeVisualizationRadius = probe_radius;
        g_Scene->m_bDDGIProbeVisualizationHideInactive = hide_inactive != 0;
    });
}

int trhost_get_ddgi_probe_visualization_consts(void* out96)
{
    return guarded([&] {
        check(g_Scene && out96);
        if (!GetLastDDGIProbeVisualizationConsts(out96))
            throw nvrhi::Error("trhost_get_ddgi_probe_visualization_consts: the last frame drew no probes (trhost_set_ddgi_probe_visualization)");
    });
}

int trhost_unit_sphere(void* vertices, uint64_t vertices_bytes, uint32_t* indices, uint64_t indices_bytes)
{
    return guarded([&] {
        std::vector<interop::UncompressedRawVertexFormat> v;
        std::vector<uint32_t> i;
        CommonResources::BuildUnitSphere(v, i);
        if (!vertices || !indices || vertices_bytes != v.size() * sizeof v[0] || indices_bytes != i.size() * sizeof i[0])
            throw nvrhi::Error("trhost_unit_sphere: needs 91 vertices of 32 bytes and 468 uint32 indices");
        memcpy(vertices, v.data(), vertices_bytes);
        memcpy(indices, i.data(), indices_bytes);
    });
}

// A frame with the probe visualisation on and nothing to draw from or into says which is missing.
static void CheckDDGIProbeVisualization()
{
    if (!g_Scene || !g_Scene->m_bDDGIProbeVisualization) return;
    if (!g_Scene->m_RTDDGIVolume.IsValid())
        throw nvrhi::Error("the probe visualisation is on (trhost_set_ddgi_probe_visualization) and there is no DDGI volume (trhost_upload_ddgi_volume): "
                           "giprobevisualization_CS_LoadGIProbes has no probes to load");
    if (!g_Scene->m_bPostProcess)
        throw nvrhi::Error("the probe visualisation is on (trhost_set_ddgi_probe_visualization) and post-processing is off (trhost_set_post_process): "
                           "giprobevisualization_PS_VisualizeGIProbes has no back buffer to draw into");
}

int trhost_reset_ddgi_volume(void)
{
    return guarded([&] {
        check(g_Scene);
        Scene::RTDDGIVolume& v = g_Scene->m_RTDDGIVolume;
        if (!v.IsValid()) throw nvrhi::Error("trhost_reset_ddgi_volume: no DDGI volume (trhost_upload_ddgi_volume first)");
        g_Graphic.m_NVRHIDevice->waitForIdle();
        ResetDDGIVariability(v);
        const uint32_t cx = (uint32_t)v.m_Desc.probeCounts[0], cy = (uint32_t)v.m_Desc.probeCounts[1], cz = (uint32_t)v.m_Desc.probeCounts[2];
        const uint64_t irrSlice = (uint64_t)cx * 8 * cz * 8 * 4, distSlice = (uint64_t)cx * 16 * cz * 16 * 4;
        const std::vector<uint8_t> zeros(distSlice, 0);                       // GIRenderer.cpp:457-458: both cleared
        for (uint32_t s = 0; s < cy; ++s) {
            nvrhi::throwIfFailed(trhip_texture_upload_slice(v.m_ProbeIrradiance->native(), s, zeros.data(), irrSlice), "trhost_reset_ddgi_volume");
            nvrhi::throwIfFailed(trhip_texture_upload_slice(v.m_ProbeDistance->native(), s, zeros.data(), distSlice), "trhost_reset_ddgi_volume");
        }
    });
}

int trhost_download_ddgi_volume(uint32_t* irradiance, uint64_t irradiance_bytes, uint16_t* distance, uint64_t distance_bytes, uint16_t* data, uint64_t data_bytes)
{
    return guarded([&] {
        check(g_Scene);
        const Scene::RTDDGIVolume& v = g_Scene->m_RTDDGIVolume;
        if (!v.IsValid()) throw nvrhi::Error("trhost_download_ddgi_volume: no DDGI volume (trhost_upload_ddgi_volume first)");
        check(irradiance && distance && data);
        const uint32_t cx = (uint32_t)v.m_Desc.probeCounts[0], cy = (uint32_t)v.m_Desc.probeCounts[1], cz = (uint32_t)v.m_Desc.probeCounts[2];
        const uint64_t irrSlice = (uint64_t)cx * 8 * cz * 8 * 4, distSlice = (uint64_t)cx * 16 * cz * 16 * 4, dataSlice = (uint64_t)cx * cz * 8;
        if (irradiance_bytes != irrSlice * cy || distance_bytes != distSlice * cy || data_bytes != dataSlice * cy)
            throw nvrhi::Error("trhost_download_ddgi_volume: the sizes do not match the probe counts (irradiance 8 x 8 x 4, distance 16 x 16 x 4, data 8 bytes per probe)");
        g_Graphic.m_NVRHIDevice->waitForIdle();
        for (uint32_t s = 0; s < cy; ++s) {
            nvrhi::throwIfFailed(trhip_texture_download_slice(v.m_ProbeData->native(), s, (char*)data + s * dataSlice, dataSlice), "trhost_download_ddgi_volume");
            nvrhi::throwIfFailed(trhip_texture_download_slice(v.m_ProbeIrradiance->native(), s, (char*)irradiance + s * irrSlice, irrSlice), "trhost_download_ddgi_volume");
            nvrhi::throwIfFailed(trhip_texture_download_slice(v.m_ProbeDistance->native(), s, (char*)distance + s * distSlice, distSlice), "trhost_download_ddgi_volume");
        }
    });
}

int trhost_get_ddgi_update_consts(void* out96)
{
    return guarded([&] {
        check(g_Scene && out96);
        if (!GetLastDDGIUpdateConsts(out96)) throw nvrhi::Error("trhost_get_ddgi_update_consts: the last frame ran no probe update (trhost_set_ddgi_update, deferred lighting on)");
    });
}

int trhost_set_ddgi(int enable)
{
    return guarded([&] {
        check(g_Scene);
        if (enable && !g_Scene->m_RTDDGIVolume.IsValid())
            throw nvrhi::Error("trhost_set_ddgi: no DDGI volume (trhost_upload_ddgi_volume first): the Ambient term needs its probes");
        g_Scene->m_bEnableDDGI = enable != 0;
    });
}

int trhost_download_lighting_output(uint32_t* words, uint64_t bytes)
{
    return guarded([&] {
        nvrhi::TextureHandle t = GetLightingOutput();
        if (!t) throw nvrhi::Error("trhost_download_lighting_output: no frame ran with deferred lighting on");
        check(words);
        nvrhi::throwIfFailed(trhip_texture_download(t->native(), 0, words, bytes), "trhost_download_lighting_output");
    });
}

int trhost_get_deferred_lighting_consts(void* out112)
{
    return guarded([&] {
        check(out112);
        if (!GetLastDeferredLightingConsts(out112)) throw nvrhi::Error("trhost_get_deferred_lighting_consts: no frame ran with deferred lighting on");
    });
}

int trhost_set_post_process(int enable)
{
    return guarded([&] {
        check(!enable || g_Graphic.m_GlobalVertexBuffer);      // trhost_load_geometry first
        if (enable && !g_Graphic.m_GlobalMaterialDataBuffer) throw nvrhi::Error("trhost_set_post_process: no materials (trhost_load_materials first)");
        if (enable && g_Graphic.m_MaxMeshletGroups > (1u << 18))
            throw nvrhi::Error("trhost_set_post_process: max_meshlet_groups above 2^18 (list positions must stay below 2^23)");
        if (enable && g_Scene->m_DebugViewMode == interop::kDeferredLightingDebugMode_Ambient && !g_Scene->m_RTDDGIVolume.IsValid())
            throw nvrhi::Error("trhost_set_post_process: debug view mode 10 (Ambient) needs the DDGI volume, which deferredlighting_PS_Main_Debug does not have");
        g_Scene->m_bPostProcess = enable != 0;
        if (enable) { g_Scene->m_bDeferredLighting = true; g_Scene->m_bGBuffer = true; g_Scene->m_bVisibilityBuffer = true; g_Scene->m_bRasterDepth = true; }   // implies deferred lighting
    });
}

int trhost_set_exposure(float manual, float middle_gray)
{
    return guarded([&] { check(g_Scene); g_Scene->m_ManualExposureOverride = manual; g_Scene->m_MiddleGray = middle_gray; });
}

int trhost_set_auto_exposure(float min_lum, float max_lum, float speed_per_ms)
{
    return guarded([&] {
        check(g_Scene);
        g_Scene->m_MinimumLuminance = min_lum; g_Scene->m_MaximumLuminance = max_lum; g_Scene->m_AutoExposureSpeed = speed_per_ms;
    });
}

int trhost_set_frame_time_ms(float ms)
{
    return guarded([&] { check(g_Scene); g_Scene->m_CPUCappedFrameTimeMs = ms; });
}

int trhost_upload_bloom(const uint32_t* words, uint64_t bytes, float strength)
{
    return guarded([&] {
        check(g_Scene);
        if (g_Scene->m_bEnableBloom) {
            if (words) throw nvrhi::Error("trhost_upload_bloom: bloom generation is on (trhost_set_bloom): the renderer makes the texture itself");
            return;                                                           // nothing uploaded to switch off
        }
        g_Scene->m_BloomStrength = strength;
        if (!words) { g_Scene->m_BloomTexture = nullptr; return; }            // bloom off: black, strength 0
        if (!g_Scene->m_BloomTexture) {
            nvrhi::TextureDesc desc;
            desc.width = g_Graphic.m_RenderResolution.x;
            desc.height = g_Graphic.m_RenderResolution.y;
            desc.format = GraphicConstants::kLightingOutputFormat;
            desc.debugName = "Bloom";
            g_Scene->m_BloomTexture = g_Graphic.m_NVRHIDevice->createTexture(desc);
        }
        nvrhi::throwIfFailed(trhip_texture_upload(g_Scene->m_BloomTexture->native(), 0, words, bytes), "trhost_upload_bloom");
    });
}

int trhost_set_bloom(int enable, uint32_t nb_mips, float filter_radius, float strength)
{
    return guarded([&] {
        check(g_Scene);
        if (!enable) { g_Scene->m_bEnableBloom = false; return; }             // the post pass reads black again, or a texture uploaded later
        if (!g_Scene->m_bPostProcess) throw nvrhi::Error("trhost_set_bloom: post-processing is off (trhost_set_post_process first): nothing would read the texture");
        if (g_Scene->m_BloomTexture) throw nvrhi::Error("trhost_set_bloom: an uploaded bloom texture is set (trhost_upload_bloom(NULL, 0, 0) first)");
        const uint32_t smaller = std::min(g_Graphic.m_RenderResolution.x, g_Graphic.m_RenderResolution.y);
        uint32_t most = 0;
        while (smaller >> most) ++most;                                       // floor(log2(min(W, H))) + 1: every mip has a texel in both axes
        if (nb_mips < 2 || nb_mips > most)
            throw nvrhi::Error("trhost_set_bloom: " + std::to_string(nb_mips) + " mips: the chain needs at least 2 and a " + std::to_string(g_Graphic.m_RenderResolution.x) +
                               "x" + std::to_string(g_Graphic.m_RenderResolution.y) + " image has at most " + std::to_string(most));
        if (!(std::isfinite(filter_radius) && filter_radius >= 0.0f)) throw nvrhi::Error("trhost_set_bloom: the filter radius must be finite and >= 0");
        g_Scene->m_bEnableBloom = true;
        g_Scene->m_NbBloomMips = nb_mips;
        g_Scene->m_BloomFilterRadius = filter_radius;
        g_Scene->m_BloomStrength = strength;
    });
}

int trhost_download_bloom(uint32_t mip, uint32_t* words, uint64_t bytes)
{
    return guarded([&] {
        nvrhi::TextureHandle t = GetGeneratedBloomTexture();
        if (!t) throw nvrhi::Error("trhost_download_bloom: no frame ran with bloom generation on");
        check(words);
        nvrhi::throwIfFailed(trhip_texture_download(t->native(), mip, words, bytes), "trhost_download_bloom");
    });
}

int trhost_get_bloom_consts(uint32_t pass, void* out16)
{
    return guarded([&] {
        check(out16);
        if (!GetLastBloomConsts(pass, out16)) throw nvrhi::Error("trhost_get_bloom_consts: pass " + std::to_string(pass) + " did not run in the last frame with bloom generation on");
    });
}

int trhost_set_taa(int enable, float min_blend, float max_sample_count)
{
    return guarded([&] {
        check(g_Scene);
        if (!enable) { g_Scene->m_bEnableTAA = false; return; }               // the projection is the camera's again and the post pass reads LightingOutput
        if (!g_Scene->m_bPostProcess) throw nvrhi::Error("trhost_set_taa: post-processing is off (trhost_set_post_process first): nothing would read the anti-aliased output");
        if (!(min_blend >= 0.0f && min_blend <= 1.0f)) throw nvrhi::Error("trhost_set_taa: min_blend must be in [0, 1]");
        if (!(max_sample_count >= 1.0f && max_sample_count <= 65504.0f)) throw nvrhi::Error("trhost_set_taa: max_sample_count must be in [1, 65504]: the count is stored as a binary16");
        g_Scene->m_bEnableTAA = true;
        g_Scene->m_TAAMinBlend = min_blend;
        g_Scene->m_TAAMaxSampleCount = max_sample_count;
    });
}

int trhost_reset_taa_history(void)
{
    return guarded([&] {
        check(g_Scene);
        if (!g_Scene->IsTAAEnabled()) throw nvrhi::Error("trhost_reset_taa_history: temporal anti-aliasing is off (trhost_set_taa first)");
        g_Scene->m_bResetTAAHistory = true;
    });
}

int trhost_download_anti_aliased_output(uint32_t* words, uint64_t bytes)
{
    return guarded([&] {
        nvrhi::TextureHandle t = GetAntiAliasedLightingOutput();
        if (!t) throw nvrhi::Error("trhost_download_anti_aliased_output: the last frame ran without temporal anti-aliasing");
        check(words);
        nvrhi::throwIfFailed(trhip_texture_download(t->native(), 0, words, bytes), "trhost_download_anti_aliased_output");
    });
}

int trhost_download_taa_history(void* halves, uint64_t bytes)
{
    return guarded([&] {
        nvrhi::TextureHandle t = GetTAAHistory();
        if (!t) throw nvrhi::Error("trhost_download_taa_history: the last frame ran without temporal anti-aliasing");
        check(halves);
        nvrhi::throwIfFailed(trhip_texture_download(t->native(), 0, halves, bytes), "trhost_download_taa_history");
    });
}

int trhost_get_taa_consts(void* out32, float* current_jitter, float* prev_jitter)
{
    return guarded([&] {
        if (!GetLastTAAConsts(out32, current_jitter, prev_jitter)) throw nvrhi::Error("trhost_get_taa_consts: the last frame ran without temporal anti-aliasing");
    });
}

int trhost_load_sky_dataset(const double* rgb, const double* rad)
{
    return guarded([&] {
        check(g_Scene);
        if (!rgb || !rad) { g_Scene->m_SkyDataset.clear(); g_Scene->m_bEnableSky = false; return; }   // unloads, and with it the pass
        for (uint32_t i = 0; i < 3 * 1080; ++i) if (!std::isfinite(rgb[i])) throw nvrhi::Error("trhost_load_sky_dataset: an RGB coefficient is not finite");
        for (uint32_t i = 0; i < 3 * 120; ++i) if (!std::isfinite(rad[i])) throw nvrhi::Error("trhost_load_sky_dataset: a radiance coefficient is not finite");
        g_Scene->m_SkyDataset.assign(rgb, rgb + 3 * 1080);
        g_Scene->m_SkyDataset.insert(g_Scene->m_SkyDataset.end(), rad, rad + 3 * 120);
    });
}

int trhost_set_sky(int enable, float turbidity, const float ground_albedo[3])
{
    return guarded([&] {
        check(g_Scene);
        if (!enable) { g_Scene->m_bEnableSky = false; return; }
        if (g_Scene->m_SkyDataset.empty()) throw nvrhi::Error("trhost_set_sky: no dataset is loaded (trhost_load_sky_dataset first)");
        if (!g_Scene->m_bDeferredLighting) throw nvrhi::Error("trhost_set_sky: deferred lighting is off (trhost_set_deferred_lighting first): there is no LightingOutput to fill");
        if (!(std::isfinite(turbidity) && turbidity >= 1.0f && turbidity <= 10.0f)) throw nvrhi::Error("trhost_set_sky: the turbidity must be a finite number in [1, 10]");
        check(ground_albedo);
        for (int i = 0; i < 3; ++i)
            if (!(ground_albedo[i] >= 0.0f && ground_albedo[i] <= 1.0f)) throw nvrhi::Error("trhost_set_sky: the ground albedo must lie in [0, 1]");
        g_Scene->m_bEnableSky = true;
        g_Scene->m_SkyTurbidity = turbidity;
        memcpy(g_Scene->m_GroundAlbedo, ground_albedo, sizeof g_Scene->m_GroundAlbedo);
    });
}

int trhost_get_sky_consts(void* out256)
{
    return guarded([&] {
        check(out256);
        if (!GetLastSkyConsts(out256)) throw nvrhi::Error("trhost_get_sky_consts: the sky pass did not run in the last frame");
    });
}

int trhost_set_ambient_occlusion(int enable, uint32_t quality, uint32_t denoise_passes, float radius, float falloff_range, float final_value_power,
                                 float depth_mip_sampling_offset)
{
    return guarded([&] {
        check(g_Scene);
        if (!enable) { g_Scene->m_bEnableAO = false; return; }
        if (!g_Scene->m_bGBuffer) throw nvrhi::Error("trhost_set_ambient_occlusion: the G-buffer is off (trhost_set_gbuffer or trhost_set_deferred_lighting first): the main pass reads GBufferA");
        if (quality > 3) throw nvrhi::Error("trhost_set_ambient_occlusion: the quality level must be 0..3");
        if (denoise_passes > 3) throw nvrhi::Error("trhost_set_ambient_occlusion: the denoise passes must be 0..3");
        if (!(std::isfinite(radius) && radius >= 0.0f)) throw nvrhi::Error("trhost_set_ambient_occlusion: the radius must be finite and >= 0");
        if (!std::isfinite(falloff_range) || !std::isfinite(final_value_power) || !std::isfinite(depth_mip_sampling_offset))
            throw nvrhi::Error("trhost_set_ambient_occlusion: falloff range, final value power and depth mip sampling offset must be finite");
        g_Scene->m_bEnableAO = true;
        g_Scene->m_AOQuality = quality;
        g_Scene->m_AODenoisePasses = denoise_passes;
        g_Scene->m_AORadius = radius;
        g_Scene->m_AOFalloffRange = falloff_range;
        g_Scene->m_AOFinalValuePower = final_value_power;
        g_Scene->m_AODepthMIPSamplingOffset = depth_mip_sampling_offset;
    });
}

int trhost_download_ssao(uint8_t* bytes, uint64_t size)
{
    return guarded([&] {
        nvrhi::TextureHandle t = GetSSAOTexture();
        if (!t) throw nvrhi::Error("trhost_download_ssao: the ambient occlusion pass did not run in the last frame");
        check(bytes);
        nvrhi::throwIfFailed(trhip_texture_download(t->native(), 0, bytes, size), "trhost_download_ssao");
    });
}

int trhost_get_gtao_consts(void* out96)
{
    return guarded([&] {
        check(out96);
        if (!GetLastGTAOConsts(out96)) throw nvrhi::Error("trhost_get_gtao_consts: the ambient occlusion pass did not run in the last frame");
    });
}

int trhost_load_raytracing(const uint32_t* indices, uint64_t num_indices, const uint32_t* index_counts, uint32_t num_meshes)
{
    return guarded([&] {
        check(g_Scene);
        check((indices || !num_indices) && (index_counts || !num_meshes));
        g_Scene->LoadRaytracing(indices, num_indices, index_counts, num_meshes);
    });
}

int trhost_upload_blue_noise(const uint8_t* rgba, uint64_t bytes)
{
    return guarded([&] {
        check(g_Scene);
        if (!rgba || bytes != 128u * 128u * 4u) throw nvrhi::Error("trhost_upload_blue_noise: needs the 128 x 128 RGBA8 image (65536 bytes)");
        if (!g_Scene->m_BlueNoise) {
            nvrhi::TextureDesc desc;
            desc.width = desc.height = 128;
            desc.format = nvrhi::Format::RGBA8_UNORM;
            desc.debugName = "Blue Noise";
            g_Scene->m_BlueNoise = g_Graphic.m_NVRHIDevice->createTexture(desc);
        }
        nvrhi::throwIfFailed(trhip_texture_upload(g_Scene->m_BlueNoise->native(), 0, rgba, bytes), "trhost_upload_blue_noise");
    });
}

int trhost_set_shadow_mask(int enable, int soft, float sun_angular_diameter, float ray_start_offset)
{
    return guarded([&] {
        check(g_Scene);
        if (!enable) { g_Scene->m_bEnableShadows = g_Scene->m_bEnableShadowDenoising = false; return; }   // the denoiser has nothing to denoise
        if (!g_Scene->m_bGBuffer) throw nvrhi::Error("trhost_set_shadow_mask: the G-buffer is off (trhost_set_gbuffer or trhost_set_deferred_lighting first): the rays start at its positions and normals");
        if (!g_Scene->m_TLAS) throw nvrhi::Error("trhost_set_shadow_mask: no acceleration structure (trhost_load_raytracing first)");
        if (!g_Scene->m_BlueNoise) throw nvrhi::Error("trhost_set_shadow_mask: no blue noise (trhost_upload_blue_noise first)");
        if (g_Scene->m_ShadowMaskTexture) throw nvrhi::Error("trhost_set_shadow_mask: a shadow mask was uploaded (trhost_upload_shadow_mask(NULL, 0) removes it): the pass generates the texture itself");
        if (!(std::isfinite(sun_angular_diameter) && sun_angular_diameter >= 0.0f && sun_angular_diameter < 180.0f)) throw nvrhi::Error("trhost_set_shadow_mask: the sun's angular diameter must be degrees in [0, 180)");
        if (!(std::isfinite(ray_start_offset) && ray_start_offset >= 0.0f)) throw nvrhi::Error("trhost_set_shadow_mask: the ray start offset must be finite and >= 0");
        g_Scene->m_bEnableShadows = true;
        g_Scene->m_bEnableSoftShadows = soft != 0;
        g_Scene->m_SunAngularDiameter = sun_angular_diameter;
        g_Scene->m_ShadowRayStartOffset = ray_start_offset;
    });
}

int trhost_download_shadow_mask(uint8_t* bytes, uint64_t size)
{
    return guarded([&] {
        nvrhi::TextureHandle t = GetShadowMaskTexture();
        if (!t) throw nvrhi::Error("trhost_download_shadow_mask: the shadow mask pass did not run in the last frame");
        check(bytes);
        nvrhi::throwIfFailed(trhip_texture_download(t->native(), 0, bytes, size), "trhost_download_shadow_mask");
    });
}

int trhost_get_shadow_mask_consts(void* out112)
{
    return guarded([&] {
        check(out112);
        if (!GetLastShadowMaskConsts(out112)) throw nvrhi::Error("trhost_get_shadow_mask_consts: the shadow mask pass did not run in the last frame");
    });
}

int trhost_set_shadow_denoising(int enable, float plane_distance_sensitivity, float stabilization_strength, float sigma_scale)
{
    return guarded([&] {
        check(g_Scene);
        if (!enable) { g_Scene->m_bEnableShadowDenoising = false; return; }
        if (!g_Scene->m_bEnableShadows) throw nvrhi::Error("trhost_set_shadow_denoising: the shadow mask is off (trhost_set_shadow_mask first): there is nothing to denoise");
        if (!(std::isfinite(plane_distance_sensitivity) && plane_distance_sensitivity > 0.0f)) throw nvrhi::Error("trhost_set_shadow_denoising: the plane distance sensitivity must be finite and > 0");
        if (!(stabilization_strength >= 0.0f && stabilization_strength <= 1.0f)) throw nvrhi::Error("trhost_set_shadow_denoising: the stabilization strength must be in [0, 1]");
        if (!(std::isfinite(sigma_scale) && sigma_scale >= 0.0f)) throw nvrhi::Error("trhost_set_shadow_denoising: the sigma scale must be finite and >= 0");
        if (!g_Scene->m_bEnableShadowDenoising) g_Scene->m_bResetShadowHistory = true;   // switched on: whatever the histories hold is from another time
        g_Scene->m_bEnableShadowDenoising = true;
        g_Scene->m_ShadowPlaneDistanceSensitivity = plane_distance_sensitivity;
        g_Scene->m_ShadowStabilizationStrength = stabilization_strength;
        g_Scene->m_ShadowSigmaScale = sigma_scale;
    });
}

int trhost_reset_shadow_history(void)
{
    return guarded([&] {
        check(g_Scene);
        if (!g_Scene->m_bEnableShadows || !g_Scene->m_bEnableShadowDenoising) throw nvrhi::Error("trhost_reset_shadow_history: shadow denoising is off (trhost_set_shadow_denoising first)");
        g_Scene->m_bResetShadowHistory = true;
    });
}

static void downloadDenoiserTexture(int which, void* out, uint64_t bytes, const char* who)
{
    nvrhi::TextureHandle t = GetShadowDenoiserTexture(which);
    if (!t) throw nvrhi::Error(std::string(who) + ": the shadow denoiser did not run in the last frame");
    check(out);
    nvrhi::throwIfFailed(trhip_texture_download(t->native(), 0, out, bytes), who);
}

int trhost_download_shadow_penumbra(void* halves, uint64_t bytes) { return guarded([&] { downloadDenoiserTexture(0, halves, bytes, "trhost_download_shadow_penumbra"); }); }
int trhost_download_shadow_tiles(uint8_t* tiles, uint64_t bytes) { return guarded([&] { downloadDenoiserTexture(1, tiles, bytes, "trhost_download_shadow_tiles"); }); }
int trhost_download_shadow_history(void* halves, uint64_t bytes) { return guarded([&] { downloadDenoiserTexture(2, halves, bytes, "trhost_download_shadow_history"); }); }

int trhost_get_sigma_consts(void* out112)
{
    return guarded([&] {
        check(out112);
        if (!GetLastSigmaConsts(out112)) throw nvrhi::Error("trhost_get_sigma_consts: the shadow denoiser did not run in the last frame");
    });
}

int trhost_download_back_buffer(uint32_t* words, uint64_t bytes)
{
    return guarded([&] {
        nvrhi::TextureHandle t = GetBackBuffer();
        if (!t) throw nvrhi::Error("trhost_download_back_buffer: no frame ran with post-processing on");
        check(words);
        nvrhi::throwIfFailed(trhip_texture_download(t->native(), 0, words, bytes), "trhost_download_back_buffer");
    });
}

int trhost_get_scene_luminance(float* luminance, float* exposure)
{
    return guarded([&] {
        if (!g_Scene->m_LuminanceBuffer) throw nvrhi::Error("trhost_get_scene_luminance: no frame ran with post-processing on");
        g_Graphic.m_NVRHIDevice->waitForIdle();
        if (luminance) nvrhi::throwIfFailed(trhip_buffer_download(g_Scene->m_LuminanceBuffer->native(), 0, luminance, sizeof(float)), "trhost_get_scene_luminance");
        if (exposure) nvrhi::throwIfFailed(trhip_texture_download(g_Scene->m_ExposureTexture->native(), 0, exposure, sizeof(float)), "trhost_get_scene_luminance");
    });
}

int trhost_reset_exposure(void)
{
    return guarded([&] { check(g_Scene); ResetExposure(); });
}

int trhost_get_post_process_consts(void* histogram16, void* adapt20, void* post24, int* adapt_ran)
{
    return guarded([&] {
        if (!GetLastPostProcessConsts(histogram16, adapt20, post24, adapt_ran)) throw nvrhi::Error("trhost_get_post_process_consts: no frame ran with post-processing on");
    });
}

int trhost_download_gbuffer_a(uint32_t* words, uint64_t bytes)
{
    return guarded([&] {
        nvrhi::TextureHandle t = GetGBufferA();
        check(t && words);
        nvrhi::throwIfFailed(trhip_texture_download(t->native(), 0, words, bytes), "trhost_download_gbuffer_a");
    });
}

int trhost_download_visibility(uint64_t* texels, uint64_t bytes)
{
    return guarded([&] {
        nvrhi::TextureHandle t = GetVisibilityBuffer();
        check(t && texels);
        nvrhi::throwIfFailed(trhip_texture_download(t->native(), 0, texels, bytes), "trhost_download_visibility");
    });
}

int trhost_download_motion(uint16_t* halves, uint64_t bytes)
{
    return guarded([&] {
        nvrhi::TextureHandle t = GetMotionBuffer();
        check(t && halves);
        nvrhi::throwIfFailed(trhip_texture_download(t->native(), 0, halves, bytes), "trhost_download_motion");
    });
}

int trhost_download_depth(float* depth, uint64_t bytes)
{
    return guarded([&] {
        nvrhi::TextureHandle t = GetLastDepthBuffer();
        check(t);
        nvrhi::throwIfFailed(trhip_texture_download(t->native(), 0, depth, bytes), "trhost_download_depth");
    });
}

int trhost_load_nodes(const void* node_local_transforms, uint32_t num_nodes, const uint32_t* primitive_to_node)
{
    return guarded([&] { g_Scene->LoadNodes(node_local_transforms, num_nodes, primitive_to_node); });
}

int trhost_set_node_transforms(const void* node_local_transforms, uint32_t num_nodes)
{
    return guarded([&] {
        check(num_nodes == g_Scene->m_NumNodes);
        std::memcpy(g_Scene->m_NodeLocalTransforms.data(), node_local_transforms, (size_t)num_nodes * sizeof(interop::NodeLocalTransform));
        g_Scene->m_bNodeLocalTransformsDirty = true;
    });
}

int trhost_set_instance_update_range(uint32_t first, uint32_t count)
{
    return guarded([&] { g_Scene->m_InstanceUpdateFirst = first; g_Scene->m_InstanceUpdateCount = count; });
}

int trhost_set_camera(const float* world_to_view, const float* prev_world_to_view, const float* view_to_clip, float near_plane)
{
    return guarded([&] {
        View& v = g_Scene->m_View;
        if (prev_world_to_view) v.SetPrevCamera(toMatrix(prev_world_to_view));
        v.SetCamera(toMatrix(world_to_view));
        if (view_to_clip) { v.m_ViewToClip = v.m_ExplicitViewToClip = toMatrix(view_to_clip); v.m_bUseExplicitProjection = true; }
        v.m_ZNearP = near_plane;
    });
}

int trhost_set_culling(int frustum, int occlusion, int cone, int freeze_culling_camera, int force_mesh_lod)
{
    return guarded([&] {
        g_Scene->m_bEnableFrustumCulling = frustum != 0;
        g_Scene->m_bEnableOcclusionCulling = occlusion != 0;
        g_Scene->m_bEnableMeshletConeCulling = cone != 0;
        g_Scene->m_bFreezeCullingCamera = freeze_culling_camera != 0;
        g_Scene->m_ForceMeshLOD = force_mesh_lod;
    });
}

int trhost_set_pipeline_statistics(int enable)
{
    return guarded([&] { g_Graphic.m_bPipelineStatistics = enable != 0; });
}

int trhost_pipeline_statistics(trhip_pipeline_statistics* last_shown, trhip_pipeline_statistics* latest)
{
    return guarded([&] {
        nvrhi::PipelineStatistics a, b;
        GetBasePassPipelineStatistics(last_shown ? &a : nullptr, latest ? &b : nullptr);
        if (last_shown) memcpy(last_shown, &a, sizeof *last_shown);
        if (latest) memcpy(latest, &b, sizeof *latest);
    });
}

int trhost_set_gpu_timers(int enable)
{
    return guarded([&] { g_Graphic.m_bEnableGPUTimers = enable != 0; });
}

int trhost_set_limits(uint32_t max_meshlet_groups, uint64_t max_transient_resource_bytes)
{
    return guarded([&] {
        if (max_meshlet_groups && g_Scene && g_Scene->m_bVisibilityBuffer && max_meshlet_groups > (1u << 18))
            throw nvrhi::Error("trhost_set_limits: max_meshlet_groups above 2^18 with the visibility buffer on");
        if (max_meshlet_groups) g_Graphic.m_MaxMeshletGroups = max_meshlet_groups;
        if (max_transient_resource_bytes) RenderGraph::ms_MaxHeapBlockSize = max_transient_resource_bytes;
    });
}

int trhost_upload_depth(const float* depth, uint32_t width, uint32_t height)
{
    return guarded([&] {
        check(g_Scene->m_SyntheticDepth);
        nvrhi::throwIfFailed(trhip_texture_upload(g_Scene->m_SyntheticDepth->native(), 0, depth, (uint64_t)width * height * 4), "trhost_upload_depth");
    });
}

int trhost_upload_hzb_mip(uint32_t mip, const uint16_t* texels, uint64_t bytes)
{
    return guarded([&] { nvrhi::throwIfFailed(trhip_texture_upload(g_Scene->m_HZB->native(), mip, texels, bytes), "trhost_upload_hzb_mip"); });
}

int trhost_download_hzb_mip(uint32_t mip, uint16_t* texels, uint64_t bytes)
{
    return guarded([&] { nvrhi::throwIfFailed(trhip_texture_download(g_Scene->m_HZB->native(), mip, texels, bytes), "trhost_download_hzb_mip"); });
}

int trhost_hzb_info(uint32_t* width, uint32_t* height, uint32_t* mips)
{
    return guarded([&] {
        const nvrhi::TextureDesc& d = g_Scene->m_HZB->getDesc();
        if (width) *width = d.width;
        if (height) *height = d.height;
        if (mips) *mips = d.mipLevels;
    });
}

int trhost_frame(void) { return guarded([&] { CheckDDGIProbeVisualization(); g_Graphic.Update(); }); }

int trhost_wait_idle(void) { return guarded([&] { g_Graphic.m_NVRHIDevice->waitForIdle(); }); }

void* trhost_device(void) { return s_Initialized ? (void*)g_Graphic.m_NVRHIDevice->native() : nullptr; }

int trhost_pass_buffers(uint32_t slot, trhost_pass_buffers_t* out)
{
    return guarded([&] {
        VisibilityPassBuffers b;
        check(GetVisibilityPassBuffers(slot, &b));
        std::memset(out, 0, sizeof *out);
        out->ran = b.m_bRan ? 1 : 0;
        auto h = [](const nvrhi::BufferHandle& x) { return x ? (void*)x->native() : nullptr; };
        out->records = h(b.m_MeshletAmplificationDataBuffer);
        out->dispatch_args = h(b.m_MeshletDispatchArgumentsBuffer);
        out->vis_mask = h(b.m_MeshletVisibilityMaskBuffer);
        out->visible_list = h(b.m_VisibleMeshletListBuffer);
        out->draw_args = h(b.m_VisibleMeshletDrawArgsBuffer);
        out->late_count = h(b.m_LateCullInstanceCountBuffer);
        out->late_args = h(b.m_LateCullDispatchIndirectArgsBuffer);
    });
}

int trhost_instance_buffer(void** buffer)
{
    return guarded([&] { *buffer = g_Scene->m_InstanceConstsBuffer ? (void*)g_Scene->m_InstanceConstsBuffer->native() : nullptr; });
}

int trhost_load_gi_probes(const float* positions, const float* states, uint32_t num_probes, float probe_radius, int hide_inactive)
{
    return guarded([&] {
        check(num_probes == 0 || (positions && states));
        g_Scene->LoadGIProbes(positions, states, num_probes, probe_radius, hide_inactive != 0);
    });
}

int trhost_gi_probe_buffers(void** positions, void** draw_args, void** instance_to_probe)
{
    return guarded([&] {
        check(positions && draw_args && instance_to_probe);
        nvrhi::BufferHandle p, a, i;
        if (!GetGIProbeCullBuffers(&p, &a, &i)) throw nvrhi::Error("no GI probe culling dispatch has been recorded");
        *positions = p->native(); *draw_args = a->native(); *instance_to_probe = i->native();
    });
}

int trhost_scene_list_sizes(uint32_t* num_opaque, uint32_t* num_alpha_mask)
{
    return guarded([&] {
        check(num_opaque && num_alpha_mask);
        *num_opaque = (uint32_t)g_Scene->m_OpaquePrimitiveIDs.size();
        *num_alpha_mask = (uint32_t)g_Scene->m_AlphaMaskPrimitiveIDs.size();
    });
}

int trhost_set_shard_late_exchange(trhost_shard_late_fn fn, void* user)
{
    return guarded([&] { SetShardLateExchange(fn, user); });
}

int trhost_exchange_create(const trhost_exchange_desc* desc)
{
    return guarded([&] {
        check(desc);
        if (g_Scene && g_Scene->m_bVisibilityBuffer) throw nvrhi::Error("trhost_exchange_create: the visibility buffer is on (list positions are per rank)");
        ShardExchangeCreate(*desc);
    });
}
int trhost_exchange_run(void) { return guarded([&] { ShardExchangeRun(); }); }
int trhost_exchange_wait(void) { return guarded([&] { ShardExchangeWait(); }); }
int trhost_exchange_outputs(uint32_t pass_slot, void** records, void** masks, void** list, void** args)
{
    return guarded([&] { check(records && masks && list && args); ShardExchangeOutputs(pass_slot, records, masks, list, args); });
}
int trhost_exchange_destroy(void) { return guarded([&] { ShardExchangeDestroy(); }); }

int trhost_set_renderer_queue(const char* renderer_name, int queue)
{
    return guarded([&] {
        check(renderer_name && (queue == 0 || queue == 1));
        for (IRenderer* r : IRenderer::ms_AllRenderers)
            if (r->m_Name == renderer_name) { r->m_Queue = queue ? nvrhi::CommandQueue::Compute : nvrhi::CommandQueue::Graphics; return; }
        throw nvrhi::Error(std::string("no renderer named ") + renderer_name);
    });
}

int trhost_render_graph_frame_stats(uint32_t* compute_queue_passes, uint32_t* cross_queue_waits, uint64_t* transient_bytes, uint64_t* aliased_bytes)
{
    return guarded([&] {
        const RenderGraph::FrameStats& f = g_Scene->m_RenderGraph->GetFrameStats();
        if (compute_queue_passes) *compute_queue_passes = f.m_NumComputeQueuePasses;
        if (cross_queue_waits) *cross_queue_waits = f.m_NumCrossQueueWaits;
        if (transient_bytes) *transient_bytes = f.m_TransientBytes;
        if (aliased_bytes) *aliased_bytes = f.m_AliasedBytes;
    });
}

int trhost_render_graph_stats(uint32_t* num_heaps, uint64_t* bytes_reserved, uint64_t* bytes_used, uint32_t* num_passes)
{
    return guarded([&] {
        const RenderGraph& rg = *g_Scene->m_RenderGraph;
        uint64_t reserved = 0, used = 0;
        for (const RenderGraph::Heap& h : rg.GetHeaps()) { reserved += h.m_Heap->getDesc().capacity; used += h.m_Used; }
        if (num_heaps) *num_heaps = (uint32_t)rg.GetHeaps().size();
        if (bytes_reserved) *bytes_reserved = reserved;
        if (bytes_used) *bytes_used = used;
        if (num_passes) *num_passes = (uint32_t)rg.GetNumPasses();
    });
}

int trhost_renderer_times(const char* renderer_name, float* cpu_ms, float* gpu_ms)
{
    return guarded([&] {
        if (std::string(renderer_name) == "<frame>") {       // host time of the last frame: recording / submission
            if (cpu_ms) *cpu_ms = g_Graphic.m_LastRecordMs;
            if (gpu_ms) *gpu_ms = g_Graphic.m_LastSubmitMs;
            return;
        }
        for (IRenderer* r : IRenderer::ms_AllRenderers)
            if (r->m_Name == renderer_name) {
                if (cpu_ms) *cpu_ms = r->m_CPUFrameTime;
                if (gpu_ms) *gpu_ms = r->m_GPUFrameTime;
                return;
            }
        throw nvrhi::Error(std::string("unknown renderer ") + renderer_name);
    });
}

static residency::Tiled tiledOf(uint32_t width, uint32_t height, uint32_t mips, uint32_t region_w, uint32_t region_h, uint32_t tile_bytes)
{
    auto pow2 = [](uint32_t v) { return v >= 4u && (v & (v - 1u)) == 0u; };
    if (!width || !height || !mips || mips > 16u) throw nvrhi::Error("residency: a texture has a size and 1 .. 16 mips");
    if (!pow2(region_w) || !pow2(region_h)) throw nvrhi::Error("residency: the sides of a region are powers of two, at least 4");
    if (width % region_w || height % region_h) throw nvrhi::Error("residency: the texture's size is not a multiple of the region: the texture is not tiled");
    residency::Tiled t;
    t.width = width; t.height = height; t.mips = mips; t.regionW = region_w; t.regionH = region_h; t.tileBytes = tile_bytes;
    return t;
}

int trhost_residency_tiles(uint32_t width, uint32_t height, uint32_t mips, uint32_t region_w, uint32_t region_h, uint32_t* standard_levels, uint32_t* num_tiles)
{
    return guarded([&] {
        const residency::Tiled t = tiledOf(width, height, mips, region_w, region_h, 0);
        if (standard_levels) *standard_levels = t.standardLevels();
        if (num_tiles) *num_tiles = t.tileOffset(t.standardLevels());
    });
}

int trhost_residency_round(uint32_t width, uint32_t height, uint32_t mips, uint32_t region_w, uint32_t region_h, uint32_t tile_bytes,
                           const uint8_t* feedback, uint32_t evict_after, uint32_t num_tiles, uint8_t* resident, uint32_t* idle,
                           uint8_t* mapped, uint8_t* unmapped, uint8_t* min_mip, uint64_t stats[5])
{
    return guarded([&] {
        const residency::Tiled t = tiledOf(width, height, mips, region_w, region_h, tile_bytes);
        const uint32_t total = t.tileOffset(t.standardLevels());
        if (num_tiles != total) throw nvrhi::Error("residency: the per-tile arrays hold " + std::to_string(num_tiles) + " tiles, the texture has " + std::to_string(total));
        if (!feedback || !min_mip || !stats || (total && (!resident || !idle))) throw nvrhi::Error("residency: null argument");
        if (!evict_after) throw nvrhi::Error("residency: evict_after is at least 1");
        residency::State state;
        state.resident.assign(resident, resident + total);
        state.idle.assign(idle, idle + total);
        std::vector<uint32_t> in, out;
        const residency::Stats s = residency::round(t, feedback, evict_after, state, in, out);
        std::copy(state.resident.begin(), state.resident.end(), resident);
        std::copy(state.idle.begin(), state.idle.end(), idle);
        if (mapped) { std::fill(mapped, mapped + total, 0); for (uint32_t i : in) mapped[i] = 1; }
        if (unmapped) { std::fill(unmapped, unmapped + total, 0); for (uint32_t i : out) unmapped[i] = 1; }
        residency::minMip(t, state, min_mip);
        stats[0] = s.tilesTotal; stats[1] = s.tilesResident; stats[2] = s.tilesMapped; stats[3] = s.tilesUnmapped; stats[4] = s.bytesUploaded;
    });
}

int trhost_heap_sim(uint64_t heap_size, const int64_t* ops, uint32_t num_ops, uint64_t* results, uint64_t* used, uint64_t* peak, uint32_t* num_blocks)
{
    return guarded([&] {
        RenderGraph::Heap heap;                       // no device heap attached: the free-list logic only
        heap.m_Blocks.push_back({ heap_size, false });
        for (uint32_t i = 0; i < num_ops; ++i) {
            if (ops[i] > 0) {
                results[i] = heap.Allocate((uint64_t)ops[i]);
            } else {
                const uint32_t ref = (uint32_t)(-ops[i]) - 1;
                check(ref < i);
                heap.Free(results[ref]);
                results[i] = results[ref];
            }
        }
        if (used) *used = heap.m_Used;
        if (peak) *peak = heap.m_Peak;
        if (num_blocks) *num_blocks = (uint32_t)heap.m_Blocks.size();
    });
}

} // extern "C"
