"""Python driver of one visibility frame over the C ABI (include/trhip.h).

Mirrors, call for call, the C++ host side (toyrenderer_amd/csrc/host/BasePassRenderers.cpp, itself
the re-authoring of the reference's source/BasePassRenderers.cpp:223-588): same buffers, same
clears, same constants, same dispatch order.  It exists so that tests and bench.py can drive the
kernels without the C++ RenderGraph layer in between (kernel-level parity tests, profiling); the
drop-in path for a C++ application is the host library.
"""
from __future__ import annotations

import numpy as np

from . import accel as accelmod
from . import ddgi as ddgimod
from . import gtao as gtaomod
from . import interop as I
from . import rhi
from . import sky as skymod
from . import taa as taamod
from .rhi import CB, PUSH, SAMPLER, SRV, TEX_SRV, TEX_TABLE, TEX_UAV, UAV

SLOT_NAMES = ("early_opaque", "late_opaque", "early_alphamask", "late_alphamask")


def culling_frustum(view_to_clip: np.ndarray) -> np.ndarray:
    """BasePassRenderers.cpp:557-563 (host-side, float32; XMVector4Normalize = v / sqrt(dot4))."""
    P = np.asarray(view_to_clip, np.float32)
    fx = (P[:, 3] + P[:, 0]).astype(np.float32)
    fy = (P[:, 3] + P[:, 1]).astype(np.float32)

    def length4(v):
        acc = np.float32(v[0] * v[0])
        for i in (1, 2, 3):
            acc = I.fmaf(v[i], v[i], acc)
        return np.sqrt(acc, dtype=np.float32)
    lx, ly = length4(fx), length4(fy)
    return np.array([fx[0] / lx, fx[2] / lx, fy[1] / ly, fy[2] / ly], np.float32)


class GpuScene:
    """Scene buffers resident in HBM (Scene.h:152-162, Graphic.h:137-143)."""

    def __init__(self, dev: rhi.Device, instances, meshData, meshlets, opaqueIds, alphaMaskIds, num_meshlets: int | None = None):
        self.dev = dev
        self.numInstances = len(instances)
        self.instances = dev.buffer_from(instances, "Instance Consts Buffer")
        self.meshData = dev.buffer_from(meshData, "GlobalMeshDataBuffer", uav=False)
        if meshlets is None:
            self.meshlets = dev.create_buffer(num_meshlets * 32, "GlobalMeshletDataBuffer", stride=32, uav=False)
        else:
            self.meshlets = dev.buffer_from(meshlets, "GlobalMeshletDataBuffer", uav=False, min_bytes=32)
        self.opaqueIds = dev.buffer_from(np.asarray(opaqueIds, np.uint32), "OpaqueInstanceIDsBuffer", uav=False)
        self.alphaMaskIds = dev.buffer_from(np.asarray(alphaMaskIds, np.uint32), "AlphaMaskInstanceIDsBuffer", uav=False)
        self.numOpaque, self.numAlphaMask = len(opaqueIds), len(alphaMaskIds)
        self.vertices = self.meshletVertexIds = self.meshletTriangles = None
        self.materials = None
        self.textures, self.texture_table, self.textured = [], None, False
        self.indices = self.rt = None

    def set_geometry(self, vertices, meshletVertexIds, meshletTriangles):
        """The buffers the mesh shader reads (basepass.hlsl t1, t5, t6): lets the frame rasterise its own depth
        (FrameDriver(raster_depth=True)) instead of taking a synthetic depth image."""
        self.vertices = self.dev.buffer_from(np.ascontiguousarray(vertices, I.RawVertexFormat), "GlobalVertexBuffer", uav=False, min_bytes=20)
        self.meshletVertexIds = self.dev.buffer_from(np.ascontiguousarray(meshletVertexIds, np.uint32), "GlobalMeshletVertexIdxOffsetsBuffer", uav=False)
        self.meshletTriangles = self.dev.buffer_from(np.ascontiguousarray(meshletTriangles, np.uint32), "GlobalMeshletIndicesBuffer", uav=False)

    def set_textures(self, textures):
        """The material textures and their table (the stand-in of ResourceDescriptorHeap[...], include/trhip.h): `textures` is a
        list of (mips, format), mips a list of uint8 [h_k, w_k, 4] arrays (level k of max(w >> k, 1) x max(h >> k, 1); interop.make_mips
        makes them from an image), format rhi.FORMAT_RGBA8_UNORM or rhi.FORMAT_SRGBA8_UNORM.  Returns their descriptor indices, which
        m_DescriptorIndex of a flagged TextureData names.  Replaces an earlier set; call it before set_materials()."""
        self.release_textures()
        if len(textures) == 0:
            return []
        self.texture_table = self.dev.create_texture_table(len(textures))
        for i, (mips, fmt) in enumerate(textures):
            self.textures.append(self.dev.create_sampled_texture(mips, fmt, f"Material Texture {i}"))
            self.texture_table.set(i, self.textures[-1])
        return list(range(len(textures)))

    def release_textures(self):
        if self.texture_table is not None:
            self.texture_table.release()
        for t in self.textures:
            t.release()
        self.textures, self.texture_table = [], None

    def set_materials(self, materials):
        """The MaterialData buffer (basepass.hlsl t3, Graphic::m_GlobalMaterialDataBuffer) that FrameDriver(gbuffer=True)
        resolves GBufferA from.  A material may use textures (m_MaterialFlags) when every flagged slot's m_DescriptorIndex names a
        texture of set_textures() and its feedback and min-mip indices are 0xFFFFFFFF (no texture streaming); FrameDriver then binds
        the texture table and the resolve samples them."""
        materials = np.ascontiguousarray(materials, I.MaterialData)
        for bit, slot in enumerate(("m_AlbedoTexture", "m_NormalTexture", "m_MetallicRoughnessTexture", "m_EmissiveTexture")):
            flagged = (materials["m_MaterialFlags"] >> bit) & 1 != 0
            t = materials[slot][flagged]
            if np.any(t["m_DescriptorIndex"] >= len(self.textures)):
                raise ValueError(f"set_materials: a material uses a texture ({slot}.m_DescriptorIndex {int(t['m_DescriptorIndex'][t['m_DescriptorIndex'] >= len(self.textures)][0]):#x}) "
                                 f"that set_textures() has not loaded ({len(self.textures)} textures)")
            if np.any(t["m_FeedbackTextureDescriptorIndex"] != 0xFFFFFFFF) or np.any(t["m_MinMapTextureDescriptorIndex"] != 0xFFFFFFFF):
                raise ValueError(f"set_materials: a material's texture ({slot}) names a sampler-feedback or min-mip texture: texture streaming is not supported")
        if self.materials is not None:
            self.materials.release()
        self.materials = self.dev.buffer_from(materials, "GlobalMaterialDataBuffer", uav=False, min_bytes=124)
        self.numMaterials = len(materials)
        self.textured = bool(np.any(materials["m_MaterialFlags"] & I.kMaterialFlagAnyTexture))

    def set_raytracing(self, indices, meshSpecific):
        """The acceleration structure FrameDriver(shadows=...) traces (include/trhip.h, "acceleration structure"): `indices` is the
        global index buffer (Graphic::m_GlobalIndexBuffer; each mesh's LOD-0 list at m_GlobalIndexBufferIdx, relative to its first
        vertex), `meshSpecific` the MeshSpecificData table (cached_scene) or one index count per mesh.  Needs set_geometry() and
        set_materials().  The BLAS of every mesh is built here, once, by the back end's builder; the TLAS topology comes from the
        instance buffer's current m_WorldMatrix (the rest transforms) and the two instance lists (opaque: ForceOpaque, alpha mask:
        ForceNonOpaque); its boxes and matrices are refit on the GPU by every recorded frame.  self.rt holds the buffers and the
        host copies ("blas", "tlas", "flags")."""
        if self.vertices is None or self.materials is None:
            raise ValueError("set_raytracing needs GpuScene.set_geometry() and set_materials()")
        dev = self.dev
        vertices = self.vertices.download(I.RawVertexFormat, self.vertices.size // I.RawVertexFormat.itemsize)
        mesh_data = self.meshData.download(I.MeshData, self.meshData.size // I.MeshData.itemsize)
        instances = self.instances.download(I.BasePassInstanceConstants, self.numInstances)
        indices = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        blas = accelmod.build_scene_blas(vertices, indices, mesh_data, meshSpecific)
        flags = accelmod.instance_flags(self.numInstances, self.opaqueIds.download(np.uint32, self.numOpaque), self.alphaMaskIds.download(np.uint32, self.numAlphaMask))
        tlas = accelmod.build_tlas(instances, flags, blas)
        self.release_raytracing()
        self.indices = dev.buffer_from(indices, "GlobalIndexBuffer", uav=False)
        self.rt = dict(blas=blas, tlas=tlas, flags=flags,
                       headers=dev.buffer_from(blas["headers"], "BLAS Headers", uav=False, min_bytes=16),
                       blas_nodes=dev.buffer_from(blas["nodes"], "BLAS Nodes", uav=False, min_bytes=32),
                       tri_order=dev.buffer_from(blas["tri_order"], "BLAS Triangle Order", uav=False),
                       tlas_nodes=dev.buffer_from(tlas["nodes"], "TLAS Nodes", min_bytes=32),
                       tlas_instances=dev.buffer_from(tlas["records"], "TLAS Instances", min_bytes=64),
                       level_nodes=dev.buffer_from(tlas["level_nodes"], "TLAS Level Nodes", uav=False),
                       level_offsets=dev.buffer_from(tlas["level_offsets"], "TLAS Level Offsets", uav=False))

    def release_raytracing(self):
        if self.rt is not None:
            for b in self.rt.values():
                if isinstance(b, rhi.Buffer):
                    b.release()
            self.indices.release()
        self.indices = self.rt = None

    def release(self):
        self.release_raytracing()
        self.release_textures()
        for b in (self.instances, self.meshData, self.meshlets, self.opaqueIds, self.alphaMaskIds, self.vertices, self.meshletVertexIds, self.meshletTriangles,
                  self.materials):
            if b is not None:
                b.release()


class FrameDriver:
    """BasePassRenderer (Setup + RenderBasePass) over rhi.  One command list per frame."""

    def __init__(self, dev: rhi.Device, scene: GpuScene, view, *, record_capacity: int, list_capacity: int | None = None,
                 culling_flags: int = 7, force_mesh_lod: int = -1, freeze_culling_camera: bool = False, alloc=None,
                 shard_late=None, raster_depth: bool = False, visibility: bool = False, gbuffer: bool = False,
                 debug_mode: int = 0, lighting: bool = False, dir_light=((0.0, -1.0, 0.0), 1.0), camera_origin=(0.0, 0.0, 0.0),
                 shadow_mask=None, ssao=None, post: bool = False, exposure=(0.0, 0.18), auto_exposure=(0.004, 12.0, 0.04),
                 bloom=(None, 0.0), bloom_mips: int = 0, bloom_filter_radius: float = 0.005, bloom_strength: float = 0.1, sky=None, ao=None,
                 shadows=None, alpha_test: bool = False, ddgi=None, ddgi_update=None, probes=None, taa=None, shadow_denoise=None):
        """alloc(nbytes, name, stride, indirect) -> rhi.Buffer or None: lets the caller own the memory of the
        output buffers (e.g. torch tensors handed to RCCL, gather.py); None -> device allocation.
        shard_late(hip_stream, late_count_ptr, shard_info_ptr, bucket, phase): multi-GPU hook, called while the
        frame is submitted: phase 0 after each early instance cull, phase 1 before each late one (include/trhost.h).
        visibility: rasterise through "basepass_MS_Main_visibility" (implies raster_depth) into self.visibility (RG32_UINT)
        and resolve self.motion (RG16_FLOAT, "basepass_PS_Main_motion") after the last slot; m_PrevWorldToClip is set.
        gbuffer: implies visibility; one "basepass_PS_Main_GBuffer" dispatch in the place of the motion resolve writes
        self.gbufferA (RGBA32_UINT) and self.motion.  Needs GpuScene.set_materials().  debug_mode: m_DebugMode (2, 3 and 12
        fill GBufferA's debug byte).
        lighting: implies gbuffer; one "deferredlighting_PS_Main" dispatch ("deferredlighting_PS_Main_Debug" when debug_mode != 0)
        after the G-buffer resolve writes self.lighting_output (R11G11B10_FLOAT), cleared to 0 with the other targets.
        dir_light = ((x, y, z), strength): m_DirectionalLightVector as given and m_DirectionalLightStrength; camera_origin:
        m_CameraOrigin (the eye of view.worldToView; a View does not carry it); shadow_mask / ssao: rhi.Texture (R8_UNORM /
        R8_UINT, render resolution) or None = unbound (1.0 / 255).  self.lighting_consts holds the 112 bytes of the last record().
        post: implies lighting (and carries its refusals); after the lighting dispatch the frame runs AdaptLuminanceRenderer and
        PostProcessRenderer: with a manual exposure of 0, a clear of the 256-word histogram, "adaptluminance_CS_GenerateLuminanceHistogram"
        and "adaptluminance_CS_AdaptExposure"; with a manual exposure > 0, one write of it into self.luminance instead
        (AdaptLuminanceRenderer.cpp:149-153); then always "postprocess_PS_PostProcess" into self.back_buffer (RGBA8_UNORM).
        exposure = (manual, middle_gray): m_ManualExposureOverride and m_MiddleGray; auto_exposure = (min_luminance, max_luminance,
        adaptation_speed): the speed is the already clamped m_AdaptationSpeed of one frame (the reference's 0.0025 per ms times the
        frame time; the driver has no clock); bloom = (rhi.Texture or None, strength): an R11G11B10_FLOAT texture at render
        resolution, None = unbound = black.  self.luminance (one float, 1.0 at construction and after reset_exposure()) and
        self.exposure_texture (1 x 1 R32_FLOAT) survive across record() and frames.  self.post_consts holds the three parameter
        structs of the last record() (histogram, adapt, post; the first two None with a manual exposure).
        bloom_mips: 0 (the default) changes nothing.  >= 2 (needs post=True, and no external bloom texture): BloomRenderer
        (BloomRenderer.cpp; the reference's defaults are 6 mips, radius 0.005, strength 0.1).  The driver owns self.bloom_texture,
        an R11G11B10_FLOAT render target with that many mips; after the lighting dispatch and before the histogram clear it
        records bloom_mips - 1 "bloom_PS_Downsample" dispatches (pass i reads mip i, LightingOutput for i = 0, and writes mip
        i + 1) and bloom_mips - 1 "bloom_PS_Upsample" dispatches (each overwrites the next finer mip) and binds the texture,
        read at mip 0, as the post pass's t2 with bloom_strength.  bloom_filter_radius: m_FilterRadius, in UV.  The count may
        not exceed floor(log2(min(W, H))) + 1: every mip has at least one texel in both axes (the reference's slider allows
        W >> k = 0; this project does not).  self.bloom_consts holds the BloomConsts of the last record(), downsamples first;
        download_bloom(mip) reads a mip back.
        sky: None (the default) changes nothing.  (dataset,) or (dataset, turbidity, ground_albedo) with a sky.HosekDataset
        (needs lighting=True; the reference's defaults are turbidity 2.0 and ground albedo (0.1, 0.1, 0.1)): SkyRenderer
        (SkyRenderer.cpp).  One "sky_PS_HosekWilkieSky" dispatch directly behind the lighting dispatch, in front of bloom and the
        histogram clear, whatever debug_mode is, fills every texel of LightingOutput whose depth is <= 0.  The sun direction is
        dir_light[0] as given, the camera position camera_origin, the matrix the lighting pass's m_ClipToWorld.
        self.sky_consts holds the 256-byte SkyPassParameters of the last record().
        ao: None (the default) changes nothing.  A dict of settings, any of quality (0..3: Low, Medium, High, Ultra), denoise_passes
        (0..3), radius, falloff_range, final_value_power, depth_mip_sampling_offset (the reference's defaults: 3, 3, 0.5, 0.615, 2.2,
        3.3; needs gbuffer=True, which lighting implies; not together with an external ssao=): AmbientOcclusionRenderer
        (AmbientOcclusionRenderer.cpp, XeGTAO).  The driver owns the working depth chain (R16_FLOAT, 5 mips), the working AO term
        (R8_UINT), the edges (R8_UNORM) and self.ssao_texture (R8_UINT); after the G-buffer resolve and in front of the lighting
        dispatch it records "ambientocclusion_CS_XeGTAO_PrefilterDepths", "ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0"
        and max(1, denoise_passes) "ambientocclusion_CS_XeGTAO_Denoise" dispatches ping-ponging between the working term and
        self.ssao_texture, the last with m_FinalApply = 1; as in the reference, with 2 passes the finally-applied image lands in
        the working term and self.ssao_texture holds the first pass's output.  With lighting the texture is the lighting pass's
        t3 and m_SSAOEnabled is 1; debug view 9 shows it, and the non-debug pass multiplies the DDGI ambient term by it: with
        ddgi= the texture changes LightingOutput, without it (no ambient term) it does not.  self.frame_counter (0; the caller may set it
        before record()) feeds NoiseIndex as g_Graphic.m_FrameCounter % 256 does; self.gtao_consts holds the 96-byte GTAOConstants
        of the last record(); download_ssao() reads self.ssao_texture back.
        shadows: None (the default) changes nothing.  A dict of settings: soft (True), sun_angular_diameter (0.533 degrees),
        ray_start_offset (0.1; the reference picks 0.01 when the scene's bounding radius is below 3, else 0.1: the caller knows the
        scene) and noise, the 128 x 128 x 4 uint8 blue noise image (required; an input as the Hosek dataset is).  Needs gbuffer=True
        (which lighting implies) and GpuScene.set_raytracing(); not together with an external shadow_mask=: ShadowMaskRenderer::
        TraceShadows without denoising (ShadowMaskRenderer.cpp:253-305).  The driver owns self.shadow_mask_texture (R8_UNORM) and
        self.linear_view_depth (R16_FLOAT); behind the G-buffer resolve (and the AO passes), in front of the lighting dispatch, it
        records "raytracing_CS_RefitTLAS" (the stand-in of the TLAS build behind updateinstanceconsts: the instance buffer's current
        matrices) and "shadowmask_CS_ShadowMask", and binds the mask as the lighting pass's t4.  The light direction is dir_light[0]
        as given, the camera position camera_origin, m_NoisePhase (self.frame_counter & 0xff) * 1.61803398875f, m_TanSunAngularRadius
        tan(radians(d / 2)) evaluated in double and rounded once (0 without soft).  self.shadow_consts holds the 112-byte
        ShadowMaskConsts of the last record(); download_shadow_mask() reads the mask back.
        alpha_test: False (the default) changes nothing: alpha-mask instances are drawn as solid triangles.  True (needs
        raster_depth, which visibility and everything above imply, and GpuScene.set_materials()): ALPHA_MASK_MODE's discard
        (basepass.hlsl:210-215).  Pass slots 2 and 3 dispatch "basepass_MS_Main_depth ALPHA_MASK_MODE=1" or
        "basepass_MS_Main_visibility ALPHA_MASK_MODE=1" with the materials at t3 and, when a loaded material uses a texture, the
        texture table at t19: a sample whose m_ConstAlbedo.w times the albedo texture's alpha is below m_AlphaCutoff is not drawn,
        so depth, the HZB, the visibility buffer and everything resolved from it see through the cut-outs.  With shadows the
        trace binds the table too and a textured cut-out casts the shadow of its kept texels (mip 0).
        ddgi: None (the default) changes nothing: no ambient term, and debug_mode 10 (Ambient) is refused.  A ddgi.Volume (needs
        lighting=True): the DDGI ambient term from a SUPPLIED probe volume (deferredlighting.hlsl:49-76; the caller
        fills the volume, e.g. ddgi.Volume.uniform, or ddgi_update= below lets it fill itself).  The driver uploads the descriptor and
        the three array textures at construction (self.ddgi_desc, self.ddgi_data, self.ddgi_irradiance, self.ddgi_distance),
        binds them as the lighting pass's t5..t8 with the linear wrap sampler, sets m_bRTDDGIEnabled = 1 and appends the
        descriptor's host copy to the constant block; debug_mode 10 then shows the irradiance.
        ddgi_update: None (the default) changes nothing: the volume stays as supplied.  A dict of settings (needs lighting=True, ddgi=
        and GpuScene.set_raytracing()): GIRenderer::RenderDDGI, the volume fills itself.  Every record() records, behind the TLAS
        refit (which then runs with or without shadows=) and in front of the lighting pass, "giprobetrace_CS_ProbeTrace" and the two
        "ProbeBlendingCS_DDGIProbeBlendingCS" passes with a new ray rotation: ddgi.random_rotation(default_rng([seed, n])) for the
        n-th record() (self.ddgi_updates counts them); the block they ran with is self.ddgi_update_consts.  Settings: seed (0),
        hysteresis (0.5), distance_exponent (50), irradiance_threshold (0.2), brightness_threshold (0.1), max_ray_distance (1e10;
        the reference passes the scene's bounding radius).  The probe textures are then created with the UAV bit, the volume's host
        arrays are the INITIAL state (ddgi.Volume.reset() clears them as the reference does), and download_ddgi() reads the
        current one back.  relocate (False) and classify (False) add GIRenderer.cpp:513-527's probe placement behind the blends:
        "giprobetrace_CS_ProbeTraceFixedRays" (32 unrotated rays from EVERY probe into self.ddgi_fixed_rays; recorded when either is
        on), then "ProbeRelocationCS_DDGIProbeRelocationCS" (rewrites data.xyz: probes leave the geometry) and
        "ProbeClassificationCS_DDGIProbeClassificationCS" (rewrites data.w: probes that see mostly back faces, or nothing within a
        cell, are switched off and wake up when that changes), with min_frontface_distance (0.3; the reference takes 0.1 for a
        scene radius below 3) and fixed_ray_backface_threshold (0.25).  Each needs its flag on the volume (ddgi.Volume(relocation=,
        classification=), on by default) and gives the data texture the UAV bit; the lighting pass of the same frame sees the new
        data; download_ddgi_fixed_rays() reads the distances back.  With both off the supplied data texture is honoured as it is
        and the update records what it recorded before (csrc/k_giprobeplacement.hip).  variability (False) with
        variability_threshold (0.001) adds the reference's convergence early-out (GIRenderer.cpp:158-190, :466-470, :529-576): the
        driver sets flags bit 2 on a COPY of the volume (self.ddgi; host and device copy of the descriptor alike; the caller's Volume is
        not touched, and one that already carries the bit is refused without the option), the radiance
        blend also writes a coefficient of variation per interior texel (u4 = self.ddgi_variability_buffer), "ReductionCS_
        DDGIReductionCS REDUCTION=1" and "ReductionCS_DDGIExtraReductionCS" average it over the active probes, and element 0 goes
        into slot n % 2 of a two-slot read-back.  Update call n first runs ddgi.VariabilityTracker.update() and, converged, records
        NOTHING of the update (no refit unless shadows= needs it, no trace, blend, placement, reduction or copy; self.
        ddgi_updates_skipped counts them, self.ddgi_updates does not); else it stores what call n - 2 copied (0 before that:
        read without waiting for the device) into the ring.  It needs record() per frame, as the rotation does.  self.
        ddgi_variability shows average, stddev, converged and samples; download_ddgi_variability() reads the buffer;
        reset_ddgi_variability() re-arms a converged volume (nothing else does: waking on a light or transform change is not built).
        probes: None (the default) changes nothing.  A dict (needs ddgi= and post=True) draws the volume's probes into the back buffer
        behind the post pass, GIDebugRenderer's three dispatches (csrc/k_giprobedraw.hip, csrc/k_giprobe.hip): "giprobevisualization_
        CS_LoadGIProbes" writes every probe's position and state from the LIVE volume into self.probe_positions and
        self.probe_states, "giprobevisualization_CS_VisualizeGIProbesCulling" culls them against the frame's HZB into
        self.probe_culled_positions, self.probe_draw_args and self.probe_instance_to_probe, and "giprobevisualization_PS_
        VisualizeGIProbes" draws the survivors as spheres shaded with their own irradiance, depth-tested against self.depth, which it
        also writes.  Settings: radius (0.1, GIRenderer.cpp's m_ProbeRadius) and hide_inactive (False).  The block the draw ran with
        is self.probe_draw_consts; download_probes() and download_probe_winners() read the results back.
        taa: None (the default) changes nothing.  A dict of settings (needs post=True): min_blend (0.1), max_sample_count (64) and
        jitter (True): temporal anti-aliasing, the place of the reference's TAARenderer (csrc/k_taa.hip, taa.py).  Every record() is
        then one frame of a sequence: the jitter is Graphic::ComputeCurrentJitterOffset's Halton offset of self.frame_counter
        ((0, 0) with jitter=False), the frame's projection is view.viewToClip times the pixel offset matrix (Scene.cpp:127-131), and
        that jittered projection is what the cull, the rasters, the resolve, AO, the shadows, lighting, the sky and the probe draw
        see; m_PrevWorldToClip is the previous record()'s jittered world-to-clip (this frame's on the first record), as
        View::Update keeps it.  One "taa_CS_TemporalResolve" dispatch behind the exposure passes and in front of
        "postprocess_PS_PostProcess" reads LightingOutput, self.depth, self.motion and the history written by the previous
        record(), and writes the other of the two self.taa_history textures (RGBA16_FLOAT) and self.anti_aliased_output
        (R11G11B10_FLOAT), which the post pass then reads in the place of LightingOutput; bloom and the histogram keep reading
        LightingOutput.  The first record() and the one after reset_taa() run with m_bResetHistory = 1.  self.taa_consts holds
        the TAAConsts of the last record(), self.taa_written the index of the history texture it wrote, self.taa_jitter its (current, previous) offsets in pixels, self.taa_view the jittered
        View it rendered with and self.taa_prev_world_to_clip its m_PrevWorldToClip; download_anti_aliased_output() and
        download_taa_history() (the texture written last) read the results back.

        shadow_denoise: None (the default) changes nothing.  A dict of settings (needs shadows=...): plane_distance_sensitivity (0.02),
        stabilization_strength (5 / 6), sigma_scale (2) and scene_radius (0: m_DenoisingRange = max(100, 2 * scene_radius)):
        ShadowMaskRenderer::DenoiseShadows (ShadowMaskRenderer.cpp:337-500), whose NRD calls are this project's own passes
        (csrc/k_sigma.hip; accel.py).  The trace then runs with m_bDoDenoising = 1 and writes self.shadow_penumbra (R16_FLOAT) in
        place of the mask, and five more dispatches follow it in front of the lighting pass: "shadowmask_CS_PackNormalAndRoughness"
        into self.normal_roughness, "SIGMA_Shadow_ClassifyTiles.cs" into self.shadow_tiles (R8_UINT) and self.shadow_data[0],
        "SIGMA_Shadow_Blur.cs" into self.shadow_data[1], "SIGMA_Shadow_PostBlur.cs" back into self.shadow_data[0] and
        "SIGMA_Shadow_TemporalStabilization.cs", which reads the motion target and the shadow history the previous record() wrote and
        writes the other of the two self.shadow_history textures (R16_FLOAT) and the shadow mask the lighting pass binds.
        m_FrameIndex is self.frame_counter, m_JitterDelta the value TAAConsts carries ((0, 0) without taa=).  The first record() and
        the one after reset_shadow_history() run with m_bResetHistory = 1.  self.sigma_consts holds the SigmaConsts of the last
        record() (m_Pass 0), self.shadow_history_written the index of the history texture it wrote; download_shadow_penumbra(),
        download_shadow_tiles() and download_shadow_history() (the texture written last) read the results back."""
        lighting = bool(lighting) or bool(post)
        gbuffer = bool(gbuffer) or bool(lighting)
        visibility = bool(visibility) or bool(gbuffer)
        if visibility and shard_late is not None:
            raise ValueError(("post-processing" if post else "deferred lighting" if lighting else "G-buffer" if gbuffer else "visibility buffer") + " with a shard exchange: list positions are per rank, not global")
        if gbuffer and scene.materials is None:
            raise ValueError(("post=True" if post else "lighting=True" if lighting else "gbuffer=True") + " needs GpuScene.set_materials()")
        if lighting and int(debug_mode) == I.kDeferredLightingDebugMode_Ambient and ddgi is None:
            raise ValueError("debug_mode 10 (Ambient) needs the DDGI volume: pass ddgi=ddgi.Volume(...)")
        if ddgi is not None and not lighting:
            raise ValueError("ddgi=... needs lighting=True: the lighting pass is what reads the probe volume")
        if ddgi is not None and not isinstance(ddgi, ddgimod.Volume):
            raise ValueError("ddgi: needs a ddgi.Volume")
        self.ddgi = ddgi
        self.ddgi_update = self.ddgi_update_consts = None
        self.ddgi_updates = 0
        if ddgi_update is not None:
            if not lighting or ddgi is None:
                raise ValueError("ddgi_update=... needs lighting=True and ddgi=ddgi.Volume(...): the volume the update fills and the pass that reads it")
            if scene.rt is None:
                raise ValueError("ddgi_update=... needs GpuScene.set_raytracing(): the acceleration structure the probe rays walk")
            self.ddgi_update = ddgimod.check_update_settings(ddgi_update)
            if self.ddgi_update["variability"]:
                if int(np.prod(ddgi.counts)) * 36 > 1 << 24:
                    raise ValueError("ddgi_update: variability=True with more than 2^24 interior irradiance texels; the reduction counts them in a float")
                ddgi = self.ddgi = ddgi.copy()       # the caller's Volume stays as it is: the bit is the driver's, on its own copy
                ddgi.variability = True              # the descriptor's bit 2, before the volume is uploaded
            elif ddgi.variability:
                raise ValueError("ddgi_update: the ddgi.Volume has variability=True (flags bit 2) and ddgi_update has variability=False: the radiance blend would "
                                 "need the variability buffer at u4; clear the flag or pass variability=True")
            for option, flag, word in (("relocate", ddgi.relocation, "relocation"), ("classify", ddgi.classification, "classification")):
                if self.ddgi_update[option] and not flag:
                    raise ValueError(f"ddgi_update: {option}=True needs ddgi.Volume({word}=True): with the flag off nothing reads what the pass writes")
        self.probes = None
        if probes is not None:
            if ddgi is None or not post:
                raise ValueError("probes=... needs " + ("ddgi=ddgi.Volume(...): the volume whose probes are drawn" if ddgi is None else "post=True: the spheres are drawn into the back buffer"))
            unknown = set(probes) - {"radius", "hide_inactive"}
            if unknown:
                raise ValueError(f"probes: unknown settings {sorted(unknown)}; known: ['hide_inactive', 'radius']")
            self.probes = dict(radius=float(probes.get("radius", 0.1)), hide_inactive=bool(probes.get("hide_inactive", False)))
            if not (np.isfinite(self.probes["radius"]) and self.probes["radius"] > 0.0):
                raise ValueError(f"probes: radius = {self.probes['radius']} is not positive and finite")
        self.taa = self.taa_consts = self.taa_jitter = self.taa_view = self.taa_prev_world_to_clip = None
        if taa is not None:
            if not post:
                raise ValueError("taa=... needs post=True: the post pass is what reads the anti-aliased output")
            self.taa = taamod.check_settings(taa)
        self.alpha_test = bool(alpha_test)
        if self.alpha_test and not (raster_depth or visibility):
            raise ValueError("alpha_test=True needs raster_depth=True (or visibility, gbuffer, lighting, post): the test runs in the rasters, and a frame without them draws nothing")
        if self.alpha_test and scene.materials is None:
            raise ValueError("alpha_test=True needs GpuScene.set_materials(): the test reads m_ConstAlbedo.w, m_AlphaCutoff and the albedo texture of each instance's material")
        self.gbuffer_on = bool(gbuffer)
        self.lighting_on = bool(lighting)
        self.post_on = bool(post)
        self.manual_exposure, self.middle_gray = np.float32(exposure[0]), np.float32(exposure[1])
        self.min_luminance, self.max_luminance, self.adaptation_speed = (np.float32(x) for x in auto_exposure)
        self.bloom, self.bloom_strength = bloom[0], np.float32(bloom[1])
        self.bloom_mips = int(bloom_mips)
        self.bloom_texture = self.bloom_consts = None
        if self.bloom_mips != 0:
            most = int(min(view.renderW, view.renderH)).bit_length()                     # floor(log2(min(W, H))) + 1
            if self.bloom_mips < 2:
                raise ValueError(f"bloom_mips = {self.bloom_mips}: the chain needs at least 2 mips (0 turns bloom generation off)")
            if self.bloom_mips > most:
                raise ValueError(f"bloom_mips = {self.bloom_mips}: a {view.renderW}x{view.renderH} image has at most {most} mips with a texel in both axes")
            if not post:
                raise ValueError("bloom_mips > 0 needs post=True: the post pass is what reads the bloom texture")
            if bloom[0] is not None:
                raise ValueError("bloom_mips > 0 together with an external bloom=(texture, strength): the driver generates the texture itself")
            if not (np.isfinite(bloom_filter_radius) and bloom_filter_radius >= 0.0):
                raise ValueError(f"bloom_filter_radius = {bloom_filter_radius}: needs a finite radius >= 0")
            self.bloom_strength = np.float32(bloom_strength)
        self.bloom_filter_radius = np.float32(bloom_filter_radius)
        self.post_consts = None
        self.sky, self.sky_consts = None, None
        if sky is not None:
            if not lighting:
                raise ValueError("sky=... needs lighting=True: the pass fills the texels of LightingOutput the lighting pass leaves")
            sky = tuple(sky)
            if not (1 <= len(sky) <= 3) or not isinstance(sky[0], skymod.HosekDataset):
                raise ValueError("sky: needs (dataset, turbidity, ground_albedo) with a sky.HosekDataset first")
            turbidity = sky[1] if len(sky) > 1 else skymod.DEFAULT_TURBIDITY
            albedo = sky[2] if len(sky) > 2 else skymod.DEFAULT_GROUND_ALBEDO
            skymod.check_settings(turbidity, albedo)
            self.sky = (sky[0], np.float32(turbidity), tuple(np.float32(x) for x in albedo))
        self.ao = self.gtao_consts = None
        self.frame_counter = 0
        if ao is not None:
            if not gbuffer:
                raise ValueError("ao=... needs gbuffer=True (or lighting=True): the main pass reads the normals of GBufferA")
            if ssao is not None:
                raise ValueError("ao=... together with an external ssao= texture: the driver generates the texture itself")
            self.ao = gtaomod.check_settings(ao)
        self.shadows = self.shadow_consts = None
        if shadows is not None:
            if not gbuffer:
                raise ValueError("shadows=... needs gbuffer=True (or lighting=True): the rays start at the G-buffer's positions and normals")
            if shadow_mask is not None:
                raise ValueError("shadows=... together with an external shadow_mask= texture: the driver generates the texture itself")
            if scene.rt is None:
                raise ValueError("shadows=... needs GpuScene.set_raytracing(): the acceleration structure the rays walk")
            self.shadows = accelmod.check_settings(shadows)
        self.shadow_denoise = self.sigma_consts = None
        if shadow_denoise is not None:
            if self.shadows is None:
                raise ValueError("shadow_denoise=... needs shadows=...: it denoises the mask those settings trace")
            self.shadow_denoise = accelmod.check_denoise_settings(shadow_denoise)
        self.dir_light = (tuple(float(x) for x in dir_light[0]), float(dir_light[1]))
        self.camera_origin = tuple(float(x) for x in camera_origin)
        self.shadow_mask, self.ssao = shadow_mask, ssao
        self.lighting_consts = None
        self.debug_mode = int(debug_mode)
        self.visibility_on = bool(visibility)
        self.raster_depth = bool(raster_depth) or self.visibility_on       # depth = the visible meshlets rasterised ("basepass_MS_Main_depth"), cleared per frame
        assert not self.raster_depth or scene.vertices is not None, "raster_depth needs GpuScene.set_geometry()"
        self.shard_late = shard_late
        self.shardInfo = [dev.create_buffer(8, f"ShardLateInfo{b}") for b in (0, 1)] if shard_late is not None else None
        self.dev, self.scene, self.view = dev, scene, view
        self.flags = culling_flags & 7
        self.force_mesh_lod = force_mesh_lod
        self.freeze = freeze_culling_camera
        self.record_capacity = int(record_capacity)
        self.list_capacity = int(list_capacity if list_capacity is not None else record_capacity * 32)
        hw, hh = I.hzb_dims(view.renderW, view.renderH)
        self.hzb_w, self.hzb_h = hw, hh
        self.hzb_mips = I.compute_nb_mips(hw, hh)
        # GBufferRenderer::Initialize (BasePassRenderers.cpp:596-616): HZB cleared to far = 0
        self.hzb = dev.create_texture(hw, hh, self.hzb_mips, rhi.FORMAT_R16_FLOAT, "HZB")
        self.depth = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_R32_FLOAT, "Depth Buffer")
        init = dev.create_command_list()
        init.open(); init.clear_texture_f32(self.hzb, 0.0); init.clear_texture_f32(self.depth, 0.0); init.close()
        dev.execute(init); dev.wait_idle(); init.release()
        self.visibility = self.motion = self.gbufferA = self.lighting_output = None
        self.back_buffer = self.exposure_texture = self.luminance = self.histogram = None
        if self.post_on:                             # AdaptLuminanceRenderer::Initialize (AdaptLuminanceRenderer.cpp:54-76) + the swap chain's format
            self.back_buffer = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_RGBA8_UNORM, "Back Buffer")
            self.exposure_texture = dev.create_texture(1, 1, 1, rhi.FORMAT_R32_FLOAT, "Exposure Texture")
            self.luminance = dev.create_buffer(4, "Exposure Buffer")
            self.histogram = dev.create_buffer(4 * 256, "Luminance Histogram")
            self.reset_exposure()
        if self.bloom_mips:                          # BloomRenderer::Setup (BloomRenderer.cpp:41-50)
            self.bloom_texture = dev.create_texture(view.renderW, view.renderH, self.bloom_mips, rhi.FORMAT_R11G11B10_FLOAT, "Bloom Texture",
                                                    render_target=True)
        self.taa_history = self.anti_aliased_output = None
        self._taa_reset, self.taa_written, self._taa_last = True, 1, None
        if self.taa is not None:                     # TAARenderer::Initialize (TAARenderer.cpp:263-271) + the two histories of the resolve
            self.taa_history = [dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_RGBA16_FLOAT, f"TAA History {i}") for i in (0, 1)]
            self.anti_aliased_output = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_R11G11B10_FLOAT, "Anti-Aliased Lighting Output")
        self.ao_depth = self.ao_working = self.ao_edges = self.ssao_texture = None
        if self.ao is not None:                      # AmbientOcclusionRenderer::Setup (AmbientOcclusionRenderer.cpp:85-127)
            self.ao_depth = dev.create_texture(view.renderW, view.renderH, gtaomod.DEPTH_MIP_LEVELS, rhi.FORMAT_R16_FLOAT, "XeGTAO Working Depth Buffer")
            self.ssao_texture = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_R8_UINT, "SSAO Buffer")
            self.ao_working = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_R8_UINT, "Working SSAO Texture")
            self.ao_edges = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_R8_UNORM, "Working Edges Texture")
            self.ssao = self.ssao_texture            # what the lighting pass binds as t3
        self.shadow_mask_texture = self.linear_view_depth = self.blue_noise = None
        if self.shadows is not None:                 # ShadowMaskRenderer::Setup (ShadowMaskRenderer.cpp:187-251) + CommonResources::BlueNoise
            self.shadow_mask_texture = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_R8_UNORM, "Shadow Mask Texture")
            self.linear_view_depth = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_R16_FLOAT, "Linear View Depth")
            self.blue_noise = dev.create_texture(I.kBlueNoiseSize, I.kBlueNoiseSize, 1, rhi.FORMAT_RGBA8_UNORM, "Blue Noise", uav=False)
            self.blue_noise.upload_mip(0, accelmod.noise_words(self.shadows["noise"]))
            self.shadow_mask = self.shadow_mask_texture      # what the lighting pass binds as t4
        self.shadow_penumbra = self.normal_roughness = self.shadow_tiles = self.shadow_data = self.shadow_history = None
        self._shadow_history_reset, self.shadow_history_written = True, 1
        if self.shadow_denoise is not None:          # ShadowMaskRenderer::Setup's textures for the denoiser (ShadowMaskRenderer.cpp:205-233) and the two histories
            W, H = view.renderW, view.renderH
            self.shadow_penumbra = dev.create_texture(W, H, 1, rhi.FORMAT_R16_FLOAT, "Shadow Penumbra Texture")
            self.normal_roughness = dev.create_texture(W, H, 1, rhi.FORMAT_R10G10B10A2_UNORM, "Normal Roughness Texture")
            self.shadow_tiles = dev.create_texture(*accelmod.sigma_tiles(W, H), 1, rhi.FORMAT_R8_UINT, "Shadow Tiles")
            self.shadow_data = [dev.create_texture(W, H, 1, rhi.FORMAT_RG16_FLOAT, f"Shadow Data {i}") for i in (0, 1)]
            self.shadow_history = [dev.create_texture(W, H, 1, rhi.FORMAT_R16_FLOAT, f"Shadow History {i}") for i in (0, 1)]
        if self.lighting_on:                         # DeferredLightingRenderer::Setup (DeferredLightingRenderer.cpp:23-34)
            self.lighting_output = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_R11G11B10_FLOAT, "Lighting Output")
        self.ddgi_desc = self.ddgi_data = self.ddgi_irradiance = self.ddgi_distance = None
        placement = self.ddgi_update is not None and (self.ddgi_update["relocate"] or self.ddgi_update["classify"])
        if self.ddgi is not None:                    # GIRenderer::Setup's textures (GIRenderer.cpp:129-133), filled by the caller
            self.ddgi_desc, self.ddgi_data, self.ddgi_irradiance, self.ddgi_distance = self.ddgi.upload(dev, uav=self.ddgi_update is not None, data_uav=placement)
        self.ddgi_rays = self.ddgi_fixed_rays = None
        self.ddgi_variability_buffer = self.ddgi_variability_readback = self._ddgi_tracker = None
        self.ddgi_variability_average = None
        self.ddgi_updates_skipped = self._ddgi_update_calls = 0
        if self.ddgi_update is not None and self.ddgi_update["variability"]:
            cx, cy, cz = self.ddgi.counts
            self.ddgi_variability_buffer = dev.create_buffer(cx * cy * cz * 36 * 4, "DDGI Probe Variability", stride=4)
            self.ddgi_variability_buffer.upload(np.zeros(cx * cy * cz * 36, np.float32))
            groups = -(-6 * cx // 16) * -(-6 * cz // 16) * -(-cy // 4)       # the first pass's outputs; every later pass has fewer
            self.ddgi_variability_average = [dev.create_buffer(groups * 8, f"DDGI Probe Variability Average {i}", stride=8) for i in range(2)]
            self.ddgi_variability_readback = dev.create_readback(4, 2)
            self._ddgi_tracker = ddgimod.VariabilityTracker(self.ddgi_update["variability_threshold"])
        if self.ddgi_update is not None:             # the ray data of GIRenderer::Setup, as a structured buffer of float4 records
            self.ddgi_rays = dev.create_buffer(int(np.prod(self.ddgi.counts)) * I.kDDGIRaysPerProbe * 16, "DDGI Ray Data", stride=16)
            self.ddgi_rays.upload(np.zeros(self.ddgi_rays.size // 4, np.float32))     # an inactive probe's records keep what they hold
            if placement:                            # the distances of the 32 fixed rays of every probe
                self.ddgi_fixed_rays = dev.create_buffer(int(np.prod(self.ddgi.counts)) * I.kDDGIFixedRays * 4, "DDGI Fixed Ray Distances", stride=4)
                self.ddgi_fixed_rays.upload(np.zeros(self.ddgi_fixed_rays.size // 4, np.float32))
        self.probe_positions = self.probe_states = self.probe_culled_positions = self.probe_draw_args = self.probe_instance_to_probe = None
        self.probe_sphere_vertices = self.probe_sphere_indices = self.probe_winners = self.probe_draw_consts = self.probe_cull_consts = None
        if self.probes is not None:                  # GIDebugRenderer::Setup (GIRenderer.cpp:612-657) + CommonResources' UnitSphere
            n_probes = int(np.prod(self.ddgi.counts))
            self.probe_positions = dev.create_buffer(12 * n_probes, "GI Probe Positions", stride=12)
            self.probe_states = dev.create_buffer(4 * n_probes, "GI Probe States")
            self.probe_culled_positions = dev.create_buffer(12 * n_probes, "Probe Positions", stride=12)
            self.probe_draw_args = dev.create_buffer(20, "Probe Draw Indirect Args", stride=20, indirect=True)
            self.probe_instance_to_probe = dev.create_buffer(4 * n_probes, "Instance ID to Probe Index")
            sphere_v, sphere_i = ddgimod.unit_sphere()
            self.probe_sphere_vertices = dev.buffer_from(sphere_v, "Unit Sphere Vertex Buffer", uav=False)
            self.probe_sphere_indices = dev.buffer_from(sphere_i, "Unit Sphere Index Buffer", uav=False)
            self.probe_winners = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_RG32_UINT, "Probe Draw Winners")
        if self.gbuffer_on:                          # GBufferA (GraphicConstants.h:24), created in GBufferRenderer::Setup (:622-632)
            self.gbufferA = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_RGBA32_UINT, "GBufferA")
        if self.visibility_on:                       # GBufferRenderer's visibility buffer + GBufferMotion, render resolution
            self.visibility = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_RG32_UINT, "VisibilityBuffer")
            self.motion = dev.create_texture(view.renderW, view.renderH, 1, rhi.FORMAT_RG16_FLOAT, "GBufferMotion")
        # BasePassRenderer::Setup (:223-296); one set of outputs per pass slot (DESIGN.md "Outputs")
        n = max(scene.numInstances, 1)

        def mk(nbytes, name, stride=4, indirect=False):
            b = alloc(nbytes, name, stride, indirect) if alloc is not None else None
            return b if b is not None else dev.create_buffer(nbytes, name, stride=stride, indirect=indirect)
        # slots 2,3 (alpha-mask lists) are only materialised when the scene has alpha-mask primitives
        slots = 4 if scene.numAlphaMask else 2
        self.records = [mk(12 * self.record_capacity, f"MeshletAmplificationDataBuffer{s}", 12) for s in range(slots)]
        self.dispatchArgs = [mk(16, f"MeshletDispatchArgumentsBuffer{s}", 16, True) for s in range(slots)]
        self.visMask = [mk(4 * self.record_capacity, f"MeshletVisibilityMaskBuffer{s}") for s in range(slots)]
        self.visibleList = [mk(4 * max(self.list_capacity, 1), f"VisibleMeshletListBuffer{s}") for s in range(slots)]
        self.drawArgs = [mk(12, f"VisibleMeshletDrawArgsBuffer{s}", 12, True) for s in range(slots)]
        self.num_slots = slots
        self.lateArgs = dev.create_buffer(12, "LateCullDispatchIndirectArgs", stride=12, indirect=True)
        self.lateCount = dev.create_buffer(4, "LateCullInstanceCountBuffer")
        self.lateIds = dev.create_buffer(4 * n, "LateCullInstanceIDsBuffer")
        self.spdAtomic = dev.create_buffer(24, "SPD Global Atomic Buffer", stride=24)
        self.dummy = dev.create_buffer(16, "DummyUIntStructuredBuffer")
        self.cl = dev.create_command_list()
        self.ran = [False] * 4

    # ---- per-frame constants (BasePassRenderers.cpp:334-347, 445-458, 551-563) ------------------
    def _cull_consts(self, nb: int) -> np.ndarray:
        v = self.view
        k = np.zeros(1, I.GPUCullingPassConstants)
        occ = bool(self.flags & 2)
        k["m_NbInstances"] = nb
        k["m_CullingFlags"] = self.flags
        k["m_HZBDimensions"] = (self.hzb_w, self.hzb_h) if occ else (1, 1)
        k["m_Frustum"] = culling_frustum(v.viewToClip)
        k["m_WorldToView"] = v.worldToView
        k["m_PrevWorldToView"] = v.prevWorldToView
        k["m_NearPlane"] = v.nearPlane
        k["m_P00"] = v.viewToClip[0, 0]
        k["m_P11"] = v.viewToClip[1, 1]
        k["m_ForcedMeshLOD"] = self.force_mesh_lod if self.force_mesh_lod >= 0 else I.kInvalidMeshLOD
        k["m_MeshLODTarget"] = np.float32(np.float32(2.0) / v.viewToClip[1, 1]) * np.float32(np.float32(1.0) / np.float32(v.renderH))
        return k

    def _basepass_consts(self, alpha_mask: bool) -> np.ndarray:
        v = self.view
        k = np.zeros(1, I.BasePassConstants)
        occ = bool(self.flags & 2)
        k["m_WorldToView"] = v.worldToView
        k["m_WorldToClip"] = I.world_to_clip(v.worldToView, v.viewToClip)
        k["m_Frustum"] = culling_frustum(v.viewToClip)
        k["m_CullingFlags"] = (self.flags & ~4) if alpha_mask else self.flags   # :436-442 (Q8)
        k["m_HZBDimensions"] = (self.hzb_w, self.hzb_h) if occ else (1, 1)
        k["m_P00"] = v.viewToClip[0, 0]
        k["m_P11"] = v.viewToClip[1, 1]
        k["m_NearPlane"] = v.nearPlane
        k["m_OutputResolution"] = (v.renderW, v.renderH)
        if self.visibility_on:                                                           # Scene.cpp:116-118 on this build's raster camera
            k["m_PrevWorldToClip"] = I.world_to_clip(v.prevWorldToView, v.viewToClip) if self.taa is None else self.taa_prev_world_to_clip   # TAA: Scene.cpp:119
        if self.gbuffer_on:
            k["m_DebugMode"] = self.debug_mode                                           # BasePassRenderers.cpp:455
        return k

    # ---- BasePassRenderer::GPUCulling (:298-404) ------------------------------------------------
    def _gpu_culling(self, cl, slot: int, late: bool, alpha_mask: bool):
        sc = self.scene
        nb = sc.numAlphaMask if alpha_mask else sc.numOpaque
        if nb == 0:
            return False
        occ = bool(self.flags & 2)
        late_args = self.lateArgs if occ else self.dummy
        late_count = self.lateCount if occ else self.dummy
        late_ids = self.lateIds if occ else self.dummy
        cl.clear_buffer_u32(self.dispatchArgs[slot], 0)                                   # :325
        if not late and occ:                                                              # :327-331
            cl.clear_buffer_u32(late_count, 0)
            cl.clear_buffer_u32(late_ids, 0)
        cb = cl.constant_buffer(self._cull_consts(nb), "GPUCullingPassConstants")         # :336-349
        bindings = [CB(0, cb), SRV(0, sc.instances), SRV(1, sc.alphaMaskIds if alpha_mask else sc.opaqueIds),
                    SRV(2, sc.meshData), UAV(0, self.records[slot]), UAV(1, self.dispatchArgs[slot]),
                    UAV(2, late_count), UAV(3, late_ids), SAMPLER(0)]
        if occ:
            bindings.append(TEX_SRV(3, self.hzb))
        name = f"gpuculling_CS_GPUCulling LATE_CULL={int(late)}"
        if not late:
            cl.dispatch(name, bindings, ((nb + 31) // 32, 1, 1))                          # :367-375
            if occ:                                                                       # :377-389
                cl.dispatch("gpuculling_CS_BuildLateCullIndirectArgs", [SRV(0, late_count), UAV(0, late_args)], (1, 1, 1))
                if self.shard_late is not None:                                           # multi-GPU only (trhost.h)
                    b = int(alpha_mask)
                    cl.host_callback(lambda stream, c=late_count.ptr, i=self.shardInfo[b].ptr, b=b: self.shard_late(stream, c, i, b, 0))
        elif occ:
            if self.shard_late is not None:                                               # multi-GPU only (trhost.h)
                bucket = int(alpha_mask)
                info = self.shardInfo[bucket]
                cl.host_callback(lambda stream, c=late_count.ptr, i=info.ptr, b=bucket: self.shard_late(stream, c, i, b, 1))
                bindings.append(SRV(4, info))
            cl.dispatch_indirect(name, bindings, late_args)                               # :392-402
        else:
            return False
        return True

    def _mesh_stage_bindings(self, cb):
        """What the raster and the resolve both read (csrc/mesh_stage.hip.h): b0 and the geometry at t0, t1, t2, t4, t5, t6."""
        sc = self.scene
        return [CB(0, cb), SRV(0, sc.instances), SRV(1, sc.vertices), SRV(2, sc.meshData), SRV(4, sc.meshlets), SRV(5, sc.meshletVertexIds),
                SRV(6, sc.meshletTriangles)]

    # ---- BasePassRenderer::RenderInstances (:406-503), cull half --------------------------------
    def _render_instances(self, cl, slot: int, late: bool, alpha_mask: bool):
        sc = self.scene
        nb = sc.numAlphaMask if alpha_mask else sc.numOpaque
        if nb == 0:
            return
        occ = bool(self.flags & 2)
        cb = cl.constant_buffer(self._basepass_consts(alpha_mask), "BasePassConstants")
        bindings = [CB(0, cb), SRV(0, sc.instances), SRV(2, sc.meshData), SRV(4, sc.meshlets), SRV(7, self.records[slot]),
                    UAV(0, self.visMask[slot]), UAV(1, self.visibleList[slot]), UAV(2, self.drawArgs[slot]), SAMPLER(4)]
        if occ:
            bindings.append(TEX_SRV(8, self.hzb))
        cl.dispatch_indirect(f"basepass_AS_Main LATE_CULL={int(late)}", bindings, self.dispatchArgs[slot])   # :497-502
        if self.raster_depth:                                                            # the mesh + pixel stage of the same draw: depth only
            b = self._mesh_stage_bindings(cb) + [SRV(7, self.records[slot]), SRV(9, self.visibleList[slot]), TEX_UAV(0, self.depth, 0)]
            permutation = ""
            if alpha_mask and self.alpha_test:                                           # BasePassRenderers.cpp:489: + t3 materials, t19 the table
                permutation = " ALPHA_MASK_MODE=1"
                b.append(SRV(3, sc.materials))
                if sc.textured:
                    b.append(TEX_TABLE(sc.texture_table))
            if self.visibility_on:                                                       # + u1 = visibility buffer, push = pass slot
                cl.dispatch_indirect("basepass_MS_Main_visibility" + permutation, b + [TEX_UAV(1, self.visibility, 0), PUSH(1)], self.drawArgs[slot],
                                     push=np.array([slot], np.uint32))
            else:
                cl.dispatch_indirect("basepass_MS_Main_depth" + permutation, b, self.drawArgs[slot])

    def _resolve_motion(self, cl):
        """GBufferMotion of every pixel the base pass drew (basepass.hlsl:226-237), once after the last slot."""
        sc, v = self.scene, self.view
        cb = cl.constant_buffer(self._basepass_consts(False), "BasePassConstants")
        b = self._mesh_stage_bindings(cb) + [TEX_SRV(18, self.visibility)]
        for s in range(4):                                                               # slots without buffers: an empty stand-in
            b += [SRV(10 + s, self.records[s] if s < self.num_slots else self.dummy),
                  SRV(14 + s, self.visibleList[s] if s < self.num_slots else self.dummy)]
        if self.gbuffer_on:                                                              # PS_Main_GBuffer: SV_Target0 + SV_Target1 in one dispatch
            b += [SRV(3, sc.materials), TEX_UAV(0, self.gbufferA, 0), TEX_UAV(1, self.motion, 0)]
            if sc.textured:                                                              # any loaded material has a texture flag: the TEXTURED kernel
                b.append(TEX_TABLE(sc.texture_table))
            cl.dispatch("basepass_PS_Main_GBuffer", b, ((v.renderW + 7) // 8, (v.renderH + 7) // 8, 1))
            return
        cl.dispatch("basepass_PS_Main_motion", b + [TEX_UAV(0, self.motion, 0)], ((v.renderW + 7) // 8, (v.renderH + 7) // 8, 1))

    # ---- DeferredLightingRenderer::Render (DeferredLightingRenderer.cpp:59-120) ---------------------
    def _lighting_consts(self) -> np.ndarray:
        v = self.view
        k = np.zeros(1, I.DeferredLightingConsts)
        k["m_ClipToWorld"] = I.clip_to_world(v.worldToView, v.viewToClip)
        k["m_CameraOrigin"] = self.camera_origin
        k["m_SSAOEnabled"] = int(self.ssao is not None)
        k["m_DebugMode"] = self.debug_mode
        k["m_DirectionalLightVector"] = self.dir_light[0]
        k["m_DirectionalLightStrength"] = self.dir_light[1]
        k["m_LightingOutputResolution"] = (v.renderW, v.renderH)
        k["m_bRTDDGIEnabled"] = int(self.ddgi is not None)                               # IsDDGIEnabled() (DeferredLightingRenderer.cpp:72)
        return k

    def _deferred_lighting(self, cl):
        v = self.view
        self.lighting_consts = self._lighting_consts()
        block = self.lighting_consts
        if self.ddgi is not None:                    # the descriptor's host copy: the constant block's second member (include/trhip.h)
            block = np.frombuffer(self.lighting_consts.tobytes() + self.ddgi.desc().tobytes(), np.uint8)
        cb = cl.constant_buffer(block, "DeferredLightingConsts")
        b = [CB(0, cb), TEX_SRV(0, self.gbufferA), TEX_SRV(1, self.motion), TEX_SRV(2, self.depth), TEX_UAV(0, self.lighting_output, 0), SAMPLER(0), SAMPLER(1)]
        if self.ddgi is not None:
            b += [SRV(5, self.ddgi_desc), TEX_SRV(6, self.ddgi_data), TEX_SRV(7, self.ddgi_irradiance), TEX_SRV(8, self.ddgi_distance)]
        if self.ssao is not None:
            b.append(TEX_SRV(3, self.ssao))
        if self.shadow_mask is not None:
            b.append(TEX_SRV(4, self.shadow_mask))
        cl.dispatch("deferredlighting_PS_Main_Debug" if self.debug_mode != 0 else "deferredlighting_PS_Main", b, ((v.renderW + 7) // 8, (v.renderH + 7) // 8, 1))

    # ---- AmbientOcclusionRenderer::Render (AmbientOcclusionRenderer.cpp:129-248) ------------------------------------------
    def _ambient_occlusion(self, cl):
        v, W, H = self.view, self.view.renderW, self.view.renderH
        self.gtao_consts = gtaomod.update_constants(W, H, self.ao, v.viewToClip, int(self.frame_counter) % 256)
        cb = cl.constant_buffer(self.gtao_consts, "GTAOConstants")
        cl.dispatch("ambientocclusion_CS_XeGTAO_PrefilterDepths",
                    [CB(0, cb), TEX_SRV(0, self.depth), *[TEX_UAV(m, self.ao_depth, m) for m in range(gtaomod.DEPTH_MIP_LEVELS)], SAMPLER(0)],
                    ((W + 15) // 16, (H + 15) // 16, 1))
        cl.dispatch("ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0",
                    [CB(0, cb), PUSH(1), TEX_SRV(0, self.ao_depth), TEX_SRV(2, self.gbufferA), TEX_UAV(0, self.ao_working, 0), TEX_UAV(1, self.ao_edges, 0), SAMPLER(0)],
                    ((W + 7) // 8, (H + 7) // 8, 1), push=gtaomod.main_pass_constants(v.worldToView, self.ao["quality"]))
        ping_pong = [self.ao_working, self.ssao_texture]
        passes = max(1, self.ao["denoise_passes"])   # without denoising one last pass still writes the term into the output texture
        for i in range(passes):
            cl.dispatch("ambientocclusion_CS_XeGTAO_Denoise",
                        [CB(0, cb), PUSH(1), TEX_SRV(0, ping_pong[0]), TEX_SRV(1, self.ao_edges), TEX_UAV(0, ping_pong[1], 0), SAMPLER(0)],
                        ((W + 15) // 16, (H + 7) // 8, 1), push=gtaomod.denoise_constants(i == passes - 1))
            ping_pong.reverse()

    def download_ssao(self) -> np.ndarray:
        """The bytes of the generated SSAO texture, (H, W) uint8."""
        if self.ssao_texture is None:
            raise ValueError("download_ssao: AO generation is off (ao=None)")
        self.dev.wait_idle()
        return self.ssao_texture.download_mip(0)

    # ---- the TLAS refit (BasePassRenderers.cpp:159-160) + ShadowMaskRenderer::TraceShadows (ShadowMaskRenderer.cpp:253-305) ---------
    def _refit_tlas(self, cl):
        sc = self.scene
        rt = sc.rt
        k = np.zeros(1, I.RefitTLASConstants)
        k["m_NumInstances"], k["m_NumNodes"], k["m_NumLevels"] = sc.numInstances, len(rt["tlas"]["nodes"]), rt["tlas"]["num_levels"]
        cl.dispatch("raytracing_CS_RefitTLAS",
                    [PUSH(0), SRV(0, sc.instances), SRV(1, rt["headers"]), SRV(2, rt["blas_nodes"]), SRV(3, rt["level_offsets"]), SRV(4, rt["level_nodes"]),
                     UAV(0, rt["tlas_nodes"]), UAV(1, rt["tlas_instances"])], (max((sc.numInstances + 63) // 64, 1), 1, 1), push=k)

    def _shadow_mask(self, cl):
        v, sc, W, H = self.view, self.scene, self.view.renderW, self.view.renderH
        rt = sc.rt
        denoise = self.shadow_denoise is not None
        self.shadow_consts = accelmod.shadow_consts(I.clip_to_world(v.worldToView, v.viewToClip), self.dir_light[0], self.camera_origin, W, H, self.shadows,
                                                    self.frame_counter, denoise)
        cb = cl.constant_buffer(self.shadow_consts, "ShadowMaskConsts")
        cl.dispatch("shadowmask_CS_ShadowMask",
                    [CB(0, cb), TEX_SRV(0, self.depth), SRV(1, rt["tlas_nodes"]), TEX_SRV(2, self.gbufferA), SRV(3, sc.instances), SRV(4, sc.vertices),
                     SRV(5, sc.materials), SRV(6, sc.indices), SRV(7, sc.meshData), TEX_SRV(8, self.blue_noise),
                     TEX_UAV(0, self.shadow_penumbra if denoise else self.shadow_mask_texture, 0),
                     TEX_UAV(1, self.linear_view_depth, 0), SRV(9, rt["tlas_instances"]), SRV(10, rt["headers"]), SRV(11, rt["blas_nodes"]),
                     SRV(12, rt["tri_order"]), SAMPLER(0), SAMPLER(1)] + ([TEX_TABLE(sc.texture_table)] if self.alpha_test and sc.textured else []),
                    ((W + 7) // 8, (H + 7) // 8, 1))

    # ---- ShadowMaskRenderer::DenoiseShadows (ShadowMaskRenderer.cpp:337-500): PackNormalRoughness and the denoiser's four dispatches ----
    def _denoise_shadows(self, cl):
        v, W, H = self.view, self.view.renderW, self.view.renderH
        groups = ((W + 7) // 8, (H + 7) // 8, 1)
        pk = np.zeros(1, I.PackNormalAndRoughnessConsts)
        pk["m_OutputResolution"] = (W, H)
        cl.dispatch("shadowmask_CS_PackNormalAndRoughness", [PUSH(0), TEX_SRV(2, self.gbufferA), TEX_UAV(0, self.normal_roughness, 0)], groups, push=pk)
        delta = taamod.jitter_delta(*self.taa_jitter) if self.taa is not None else (0.0, 0.0)
        k = [accelmod.sigma_consts(I.clip_to_world(v.worldToView, v.viewToClip), v.viewToClip, W, H, self.shadow_denoise, self.frame_counter, p,
                                   self._shadow_history_reset, delta) for p in (0, 1)]
        self.sigma_consts = k[0]
        cb = [cl.constant_buffer(x, "SigmaConsts") for x in k]
        lvd, tiles, data = self.linear_view_depth, self.shadow_tiles, self.shadow_data
        tw, th = accelmod.sigma_tiles(W, H)
        cl.dispatch("SIGMA_Shadow_ClassifyTiles.cs", [CB(0, cb[0]), TEX_SRV(0, self.shadow_penumbra), TEX_SRV(1, lvd), TEX_UAV(0, tiles, 0), TEX_UAV(1, data[0], 0)], (tw, th, 1))
        for p, name in enumerate(("SIGMA_Shadow_Blur.cs", "SIGMA_Shadow_PostBlur.cs")):
            cl.dispatch(name, [CB(0, cb[p]), TEX_SRV(0, data[p]), TEX_SRV(1, lvd), TEX_SRV(2, self.depth), TEX_SRV(3, self.normal_roughness), TEX_SRV(4, tiles),
                               TEX_UAV(0, data[1 - p], 0)], groups)
        read, write = self.shadow_history[self.shadow_history_written], self.shadow_history[1 - self.shadow_history_written]
        cl.dispatch("SIGMA_Shadow_TemporalStabilization.cs",
                    [CB(0, cb[0]), TEX_SRV(0, data[0]), TEX_SRV(1, lvd), TEX_SRV(2, self.motion), TEX_SRV(3, read), TEX_SRV(4, tiles), TEX_UAV(0, write, 0),
                     TEX_UAV(1, self.shadow_mask_texture, 0)], groups)
        self.shadow_history_written, self._shadow_history_reset = 1 - self.shadow_history_written, False

    def reset_shadow_history(self):
        """The next record() runs the stabilisation with m_bResetHistory = 1: no texel's shadow history is valid."""
        if self.shadow_denoise is None:
            raise ValueError("reset_shadow_history: shadow denoising is off (shadow_denoise=None)")
        self._shadow_history_reset = True

    def _denoise_download(self, what, tex):
        if self.shadow_denoise is None:
            raise ValueError(f"{what}: shadow denoising is off (shadow_denoise=None)")
        self.dev.wait_idle()
        return tex().download_mip(0)

    def download_shadow_penumbra(self) -> np.ndarray:
        """The binary16 words of the penumbra texture the trace wrote, (H, W) uint16."""
        return self._denoise_download("download_shadow_penumbra", lambda: self.shadow_penumbra)

    def download_shadow_tiles(self) -> np.ndarray:
        """The tile bytes of the last record(), (ceil(H / 16), ceil(W / 16)) uint8."""
        return self._denoise_download("download_shadow_tiles", lambda: self.shadow_tiles)

    def download_shadow_history(self) -> np.ndarray:
        """The binary16 words of the shadow history the last record() wrote, (H, W) uint16."""
        return self._denoise_download("download_shadow_history", lambda: self.shadow_history[self.shadow_history_written])

    # ---- GIRenderer::RenderDDGI (GIRenderer.cpp): the probe trace and the two blends ---------------------------------------------
    def _ddgi_begin_update(self):
        """RenderDDGI's opening (GIRenderer.cpp:464-470), once per record(): True when this call records nothing of the update."""
        if self._ddgi_tracker is None:
            return False
        self._ddgi_call = self._ddgi_update_calls        # this call's number since the last reset: its read-back slot is this % 2
        self._ddgi_update_calls += 1
        skip = self._ddgi_tracker.update()
        self.ddgi_updates_skipped += int(skip)
        return skip

    def _ddgi_variability(self, cl, cb):
        """GIRenderer.cpp:529-576: the sample of two calls ago into the ring, this call's reductions, the copy of their result."""
        cx, cy, cz = self.ddgi.counts
        slot = self._ddgi_call % 2
        got, _ = self.ddgi_variability_readback.read(slot, np.float32, 1)   # waits for that slot's copy only; 0 for a slot never written
        self._ddgi_tracker.set(got[0])
        size, n = (6 * cx, 6 * cz, cy), 0
        while n == 0 or max(size) > 1:
            out = tuple(-(-s // g) for s, g in zip(size, I.kDDGIReductionGroup))
            push = np.zeros(1, I.DDGIRootConstants)
            push["reductionInputSizeX"], push["reductionInputSizeY"], push["reductionInputSizeZ"] = size
            src, dst = self.ddgi_variability_average[(n + 1) % 2], self.ddgi_variability_average[n % 2]   # ping-pong: a pass never reads what it writes
            if n == 0:
                cl.dispatch("ReductionCS_DDGIReductionCS REDUCTION=1", [CB(0, cb), PUSH(1), TEX_SRV(3, self.ddgi_data), SRV(4, self.ddgi_variability_buffer), UAV(5, dst)], out, push=push)
            else:
                cl.dispatch("ReductionCS_DDGIExtraReductionCS", [PUSH(1), SRV(4, src), UAV(5, dst)], out, push=push)
            size, n = out, n + 1
        cl.copy_to_readback(self.ddgi_variability_readback, slot, self.ddgi_variability_average[(n + 1) % 2], 0, 4)

    @property
    def ddgi_variability(self):
        """dict(average, stddev, converged, samples) of the convergence rule, or None with variability off."""
        t = self._ddgi_tracker
        return None if t is None else dict(average=t.average, stddev=t.stddev, converged=t.converged, samples=t.samples)

    @property
    def ddgi_variability_ring(self):
        """A copy of the rule's ring of the last 16 stored averages (float32 [16], in index order), or None with variability off."""
        return None if self._ddgi_tracker is None else self._ddgi_tracker.ring.copy()

    def download_ddgi_variability(self) -> np.ndarray:
        """The variability buffer, float32 [counts.y, 6 counts.z, 6 counts.x]."""
        if self.ddgi_variability_buffer is None:
            raise ValueError("download_ddgi_variability: probe variability is off (ddgi_update without variability=True)")
        self.dev.wait_idle()
        cx, cy, cz = self.ddgi.counts
        return self.ddgi_variability_buffer.download(np.float32).reshape(cy, 6 * cz, 6 * cx)

    def reset_ddgi_variability(self):
        """Re-arms the update: the whole tracker starts again, the pending read-back slots are dropped and the variability buffer is zeroed."""
        if self._ddgi_tracker is None:
            raise ValueError("reset_ddgi_variability: probe variability is off (ddgi_update without variability=True)")
        self.dev.wait_idle()
        self._ddgi_tracker.reset()
        self._ddgi_update_calls = self.ddgi_updates_skipped = 0
        self.ddgi_variability_buffer.upload(np.zeros(self.ddgi_variability_buffer.size // 4, np.float32))
        self.ddgi_variability_readback.reset()       # kept: the list recorded last still names it

    def _ddgi_update(self, cl):
        sc, vol, u = self.scene, self.ddgi, self.ddgi_update
        rt = sc.rt
        k = np.zeros(1, I.DDGIUpdateConsts)
        k["m_DirectionalLightVector"], k["m_DirectionalLightStrength"] = self.dir_light
        k["rayRotation"][0, :, :3] = ddgimod.random_rotation(np.random.default_rng([u["seed"], self.ddgi_updates]))
        k["probeMaxRayDistance"], k["probeHysteresis"], k["probeDistanceExponent"] = u["max_ray_distance"], u["hysteresis"], u["distance_exponent"]
        k["probeIrradianceThreshold"], k["probeBrightnessThreshold"] = u["irradiance_threshold"], u["brightness_threshold"]
        if u["relocate"] or u["classify"]:
            k["probeMinFrontfaceDistance"], k["probeFixedRayBackfaceThreshold"] = u["min_frontface_distance"], u["fixed_ray_backface_threshold"]
        self.ddgi_update_consts = k
        self.ddgi_updates += 1
        cb = cl.constant_buffer(np.frombuffer(k.tobytes() + vol.desc().tobytes(), np.uint8), "DDGIUpdateConsts")
        cx, cy, cz = vol.counts
        cl.dispatch("giprobetrace_CS_ProbeTrace",
                    [CB(0, cb), SRV(0, self.ddgi_desc), TEX_SRV(1, self.ddgi_data), TEX_SRV(2, self.ddgi_irradiance), TEX_SRV(3, self.ddgi_distance), SRV(4, rt["tlas_nodes"]),
                     SRV(5, sc.instances), SRV(6, sc.vertices), SRV(7, sc.materials), SRV(8, sc.indices), SRV(9, sc.meshData), SRV(10, rt["tlas_instances"]),
                     SRV(11, rt["headers"]), SRV(12, rt["blas_nodes"]), SRV(13, rt["tri_order"]), UAV(0, self.ddgi_rays), SAMPLER(0), SAMPLER(1), SAMPLER(2)],
                    (I.kDDGIRaysPerProbe // 64, cx * cz, cy))
        cl.dispatch("ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=1",
                    [CB(0, cb), SRV(1, self.ddgi_rays), TEX_SRV(3, self.ddgi_data), TEX_UAV(1, self.ddgi_irradiance, 0)] +
                    ([UAV(4, self.ddgi_variability_buffer)] if u["variability"] else []), (cx, cz, cy))
        cl.dispatch("ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=0",
                    [CB(0, cb), SRV(1, self.ddgi_rays), TEX_SRV(3, self.ddgi_data), TEX_UAV(2, self.ddgi_distance, 0)], (cx, cz, cy))
        if u["relocate"] or u["classify"]:
            self._ddgi_placement(cl, cb)
        if u["variability"]:
            self._ddgi_variability(cl, cb)

    def _ddgi_placement(self, cl, cb):
        sc, u = self.scene, self.ddgi_update
        rt = sc.rt
        cx, cy, cz = self.ddgi.counts
        n = cx * cy * cz                             # GIRenderer.cpp:513-527: relocation and classification behind the blends
        cl.dispatch("giprobetrace_CS_ProbeTraceFixedRays",
                    [CB(0, cb), SRV(0, self.ddgi_desc), TEX_SRV(1, self.ddgi_data), SRV(4, rt["tlas_nodes"]), SRV(5, sc.instances), SRV(6, sc.vertices), SRV(8, sc.indices),
                     SRV(9, sc.meshData), SRV(10, rt["tlas_instances"]), SRV(11, rt["headers"]), SRV(12, rt["blas_nodes"]), SRV(13, rt["tri_order"]),
                     UAV(0, self.ddgi_fixed_rays)], ((n * I.kDDGIFixedRays + 63) // 64, 1, 1))
        for on, name in ((u["relocate"], "ProbeRelocationCS_DDGIProbeRelocationCS"), (u["classify"], "ProbeClassificationCS_DDGIProbeClassificationCS")):
            if on:
                cl.dispatch(name, [CB(0, cb), UAV(0, self.ddgi_fixed_rays), TEX_UAV(3, self.ddgi_data, 0)], ((n + 31) // 32, 1, 1))

    def download_ddgi(self):
        """A copy of the driver's ddgi.Volume with the probe textures as they are on the device now."""
        if self.ddgi is None:
            raise ValueError("download_ddgi: there is no volume (ddgi=None)")
        self.dev.wait_idle()
        vol = self.ddgi.copy()
        for s in range(vol.counts[1]):
            vol.irradiance[s] = self.ddgi_irradiance.download_slice(s)
            vol.distance[s] = self.ddgi_distance.download_slice(s).reshape(vol.distance[s].shape)
            vol.data[s] = self.ddgi_data.download_slice(s).reshape(vol.data[s].shape)
        return vol

    def download_ddgi_rays(self) -> np.ndarray:
        """The ray records of the last update, float32 [numProbes, 256, 4]."""
        if self.ddgi_rays is None:
            raise ValueError("download_ddgi_rays: the probe update is off (ddgi_update=None)")
        self.dev.wait_idle()
        return self.ddgi_rays.download(np.float32).reshape(-1, I.kDDGIRaysPerProbe, 4)

    def download_ddgi_fixed_rays(self) -> np.ndarray:
        """The fixed-ray distances of the last update, float32 [numProbes, 32]: t for a front face, -0.2 t for a back face, 1e27 for a miss."""
        if self.ddgi_fixed_rays is None:
            raise ValueError("download_ddgi_fixed_rays: probe placement is off (ddgi_update without relocate=True or classify=True)")
        self.dev.wait_idle()
        return self.ddgi_fixed_rays.download(np.float32).reshape(-1, I.kDDGIFixedRays)

    def download_shadow_mask(self) -> np.ndarray:
        """The bytes of the generated shadow mask, (H, W) uint8."""
        if self.shadow_mask_texture is None:
            raise ValueError("download_shadow_mask: shadow generation is off (shadows=None)")
        self.dev.wait_idle()
        return self.shadow_mask_texture.download_mip(0)

    # ---- SkyRenderer::Render (SkyRenderer.cpp:163-208) -------------------------------------------------------------------
    def _sky(self, cl):
        v = self.view
        dataset, turbidity, albedo = self.sky
        sun = np.asarray(self.dir_light[0], np.float32)
        params = skymod.sky_parameters(dataset, turbidity, albedo, sun)
        self.sky_consts = skymod.pass_parameters(self.lighting_consts["m_ClipToWorld"][0], sun, self.camera_origin, params)
        cb = cl.constant_buffer(self.sky_consts, "SkyPassParameters")
        cl.dispatch("sky_PS_HosekWilkieSky", [CB(0, cb), TEX_SRV(0, self.depth), TEX_UAV(0, self.lighting_output, 0)],
                    ((v.renderW + 7) // 8, (v.renderH + 7) // 8, 1))

    # ---- BloomRenderer::Render (BloomRenderer.cpp:57-141) ---------------------------------------------------------------
    def _bloom(self, cl):
        v, tex, n = self.view, self.bloom_texture, self.bloom_mips - 1
        self.bloom_consts = np.zeros(2 * n, I.BloomConsts)

        def groups(mip):
            w, h = v.renderW >> mip, v.renderH >> mip
            return ((w + 7) // 8, (h + 7) // 8, 1)
        for i in range(n):                                                               # downsample: mip i -> mip i + 1
            k = self.bloom_consts[i:i + 1]
            k["m_bIsFirstDownsample"] = int(i == 0)
            k["m_InvSourceResolution"] = (np.float32(1.0) / np.float32(v.renderW >> i), np.float32(1.0) / np.float32(v.renderH >> i))
            src = TEX_SRV(0, self.lighting_output) if i == 0 else TEX_SRV(0, tex, i)
            cl.dispatch("bloom_PS_Downsample", [PUSH(0), src, TEX_UAV(0, tex, i + 1), SAMPLER(0)], groups(i + 1), push=k)
        for i in range(n):                                                               # upsample: mip n - i -> mip n - i - 1, overwritten
            k = self.bloom_consts[n + i:n + i + 1]
            k["m_FilterRadius"] = self.bloom_filter_radius
            cl.dispatch("bloom_PS_Upsample", [PUSH(0), TEX_SRV(0, tex, n - i), TEX_UAV(0, tex, n - i - 1), SAMPLER(0)], groups(n - i - 1), push=k)

    def download_bloom(self, mip: int = 0) -> np.ndarray:
        """The words of one mip of the generated bloom texture, (H >> mip, W >> mip) uint32."""
        if self.bloom_texture is None:
            raise ValueError("download_bloom: bloom generation is off (bloom_mips = 0)")
        self.dev.wait_idle()
        return self.bloom_texture.download_mip(mip)

    # ---- AdaptLuminanceRenderer::Render (AdaptLuminanceRenderer.cpp:119-215) + PostProcessRenderer::Render (:37-74) -----
    def reset_exposure(self):
        """The adapted luminance and the exposure texel back to kInitialExposure = 1.0."""
        self.dev.wait_idle()
        self.luminance.upload(np.array([1.0], np.float32))
        self.exposure_texture.upload_mip(0, np.array([[1.0]], np.float32))

    def _post_process(self, cl):
        v = self.view
        dims = (v.renderW, v.renderH)
        hk = ak = None
        if self.manual_exposure > 0.0:                                                   # :149-153
            cl.write_buffer(self.luminance, np.array([self.manual_exposure], np.float32))
        else:
            lo, hi = I.log_luminance_range(self.min_luminance, self.max_luminance)      # :155-156
            cl.clear_buffer_u32(self.histogram, 0)
            hk = np.zeros(1, I.GenerateLuminanceHistogramParameters)
            hk["m_SrcColorDims"] = dims
            hk["m_MinLogLuminance"] = lo
            hk["m_InverseLogLuminanceRange"] = np.float32(1.0) / np.float32(hi - lo)
            cl.dispatch("adaptluminance_CS_GenerateLuminanceHistogram", [PUSH(0), TEX_SRV(0, self.lighting_output), UAV(0, self.histogram)],
                        ((v.renderW + 15) // 16, (v.renderH + 15) // 16, 1), push=hk)
            ak = np.zeros(1, I.AdaptExposureParameters)
            ak["m_AdaptationSpeed"] = self.adaptation_speed
            ak["m_MinLogLuminance"] = lo
            ak["m_LogLuminanceRange"] = np.float32(hi - lo)
            ak["m_NbPixels"] = v.renderW * v.renderH
            ak["m_MiddleGray"] = self.middle_gray
            cl.dispatch("adaptluminance_CS_AdaptExposure", [PUSH(0), SRV(0, self.histogram), UAV(0, self.luminance), TEX_UAV(1, self.exposure_texture, 0)],
                        (1, 1, 1), push=ak)
        if self.taa is not None:                                                         # Scene.cpp:506: between adapt luminance and post
            self._taa_resolve(cl)
        pk = np.zeros(1, I.PostProcessParameters)
        pk["m_OutputDims"] = dims
        pk["m_ManualExposure"] = self.manual_exposure
        pk["m_MiddleGray"] = self.middle_gray
        bloom = self.bloom_texture if self.bloom_texture is not None else self.bloom     # generated, or the caller's
        pk["m_BloomStrength"] = self.bloom_strength if bloom is not None else 0.0       # m_bEnableBloom ? m_BloomStrength : 0
        colour = self.anti_aliased_output if self.taa is not None else self.lighting_output   # PostProcessRenderer.cpp:25-27, :52
        b = [PUSH(0), TEX_SRV(0, colour), SRV(1, self.luminance), TEX_UAV(0, self.back_buffer, 0), SAMPLER(0)]
        if bloom is not None:
            b.append(TEX_SRV(2, bloom))
        cl.dispatch("postprocess_PS_PostProcess", b, ((v.renderW + 7) // 8, (v.renderH + 7) // 8, 1), push=pk)
        self.post_consts = (hk, ak, pk)

    # ---- TAARenderer::Render's place (TAARenderer.cpp:273-275 for the inputs; the resolve is csrc/k_taa.hip) ---------------------
    def _taa_begin(self):
        """The frame's jitter, its jittered View and m_PrevWorldToClip (View::Update, Scene.cpp:113-133)."""
        self.taa_view, self.taa_jitter, self.taa_prev_world_to_clip, self._taa_last = taamod.begin_frame(self.view, self.frame_counter, self.taa, self._taa_last)
        return self.taa_view

    def _taa_resolve(self, cl):
        v = self.view
        self.taa_consts = taamod.consts(v.renderW, v.renderH, self.taa, *self.taa_jitter, self._taa_reset)
        read, write = self.taa_history[self.taa_written], self.taa_history[1 - self.taa_written]
        cl.dispatch("taa_CS_TemporalResolve",
                    [PUSH(0), TEX_SRV(0, self.lighting_output), TEX_SRV(1, self.depth), TEX_SRV(2, self.motion), TEX_SRV(3, read), TEX_UAV(0, write, 0),
                     TEX_UAV(1, self.anti_aliased_output, 0), SAMPLER(0)], ((v.renderW + 7) // 8, (v.renderH + 7) // 8, 1), push=self.taa_consts)
        self.taa_written, self._taa_reset = 1 - self.taa_written, False

    def reset_taa(self):
        """The next record() runs the resolve with m_bResetHistory = 1: every texel starts again from its current colour."""
        if self.taa is None:
            raise ValueError("reset_taa: temporal anti-aliasing is off (taa=None)")
        self._taa_reset = True

    def download_anti_aliased_output(self) -> np.ndarray:
        """The words of AntiAliasedLightingOutput, (H, W) uint32."""
        if self.taa is None:
            raise ValueError("download_anti_aliased_output: temporal anti-aliasing is off (taa=None)")
        self.dev.wait_idle()
        return self.anti_aliased_output.download_mip(0)

    def download_taa_history(self) -> np.ndarray:
        """The history texture written last, (H, W, 4) float16: xyz the colour, w the accumulated sample count."""
        if self.taa is None:
            raise ValueError("download_taa_history: temporal anti-aliasing is off (taa=None)")
        self.dev.wait_idle()
        return self.taa_history[self.taa_written].download_mip(0)

    # ---- GIDebugRenderer::RenderDDGIDebug (GIRenderer.cpp:672-808) ------------------------------
    def _probe_visualization(self, cl):
        v, vol = self.view, self.ddgi
        n = int(np.prod(vol.counts))
        desc = vol.desc()
        cl.dispatch("giprobevisualization_CS_LoadGIProbes",
                    [CB(0, cl.constant_buffer(np.frombuffer(desc.tobytes(), np.uint8), "DDGIVolumeDesc")), SRV(0, self.ddgi_desc), TEX_SRV(1, self.ddgi_data),
                     UAV(0, self.probe_positions), UAV(1, self.probe_states)], ((n + 31) // 32, 1, 1))
        args = np.zeros(1, I.DrawIndexedIndirectArguments)                               # :683-689: the sphere's indices, no instance yet
        args["m_IndexCount"] = I.kUnitSphereIndices
        cl.write_buffer(self.probe_draw_args, args)
        ck = np.zeros(1, I.GIProbeVisualizationUpdateConsts)                             # :687-708
        ck["m_NumProbes"] = n
        ck["m_CameraOrigin"] = self.camera_origin
        ck["m_Frustum"] = culling_frustum(v.viewToClip)
        ck["m_WorldToView"] = v.worldToView
        ck["m_HZBDimensions"] = (self.hzb_w, self.hzb_h)
        ck["m_P00"], ck["m_P11"] = v.viewToClip[0, 0], v.viewToClip[1, 1]
        ck["m_NearPlane"] = v.nearPlane
        ck["m_ProbeRadius"] = self.probes["radius"]
        ck["m_bHideInactiveProbes"] = int(self.probes["hide_inactive"])
        cl.dispatch("giprobevisualization_CS_VisualizeGIProbesCulling",
                    [CB(0, cl.constant_buffer(ck, "GIProbeVisualizationUpdateConsts")), TEX_SRV(0, self.hzb), SRV(10, self.probe_positions), SRV(11, self.probe_states),
                     UAV(0, self.probe_culled_positions), UAV(1, self.probe_draw_args), UAV(2, self.probe_instance_to_probe), SAMPLER(0)], ((n + 31) // 32, 1, 1))
        dk = np.zeros(1, I.GIProbeVisualizationConsts)                                   # :745-752
        dk["m_WorldToClip"] = I.world_to_clip(v.worldToView, v.viewToClip)
        dk["m_CameraDirection"] = -np.asarray(v.worldToView, np.float32)[:3, 2]          # the view looks down -Z; the draw does not read it
        dk["m_ProbeRadius"] = self.probes["radius"]
        dk["m_NearPlane"] = v.nearPlane
        block = np.frombuffer(dk.tobytes() + desc.tobytes(), np.uint8)
        cl.dispatch("giprobevisualization_PS_VisualizeGIProbes",
                    [CB(0, cl.constant_buffer(block, "GIProbeVisualizationConsts")), SRV(0, self.probe_culled_positions), TEX_SRV(1, self.ddgi_data),
                     TEX_SRV(2, self.ddgi_irradiance), TEX_SRV(3, self.ddgi_distance), SRV(4, self.ddgi_desc), SRV(5, self.probe_instance_to_probe),
                     SRV(6, self.probe_draw_args), SRV(7, self.probe_sphere_vertices), SRV(8, self.probe_sphere_indices), TEX_UAV(0, self.depth, 0),
                     TEX_UAV(1, self.back_buffer, 0), TEX_UAV(2, self.probe_winners, 0), SAMPLER(0)], (1, 1, 1))
        self.probe_cull_consts, self.probe_draw_consts = ck, dk

    def download_probes(self):
        """(count, culled positions float32 [count, 3], instance -> probe index uint32 [count]) of the last frame run."""
        if self.probes is None:
            raise ValueError("download_probes: the probe visualisation is off (probes=None)")
        self.dev.wait_idle()
        n = int(np.prod(self.ddgi.counts))
        count = min(int(self.probe_draw_args.download(np.uint32, 5)[1]), n)
        return count, self.probe_culled_positions.download(np.float32, 3 * n).reshape(n, 3)[:count], self.probe_instance_to_probe.download(np.uint32, n)[:count]

    def download_probe_winners(self) -> np.ndarray:
        """The draw's winner words of the last frame run, uint64 [H, W]: (depth bits << 32) | instance << 8 | triangle, 0 = no sphere."""
        if self.probes is None:
            raise ValueError("download_probe_winners: the probe visualisation is off (probes=None)")
        self.dev.wait_idle()
        return self.probe_winners.download_mip(0)

    # ---- BasePassRenderer::GenerateHZB (:505-542) + SPD::Execute (FFXHelpers.cpp:36-115) --------
    def _generate_hzb(self, cl):
        if self.freeze:
            return
        k = np.zeros(1, I.MinMaxDownsampleConsts)
        k["m_OutputDimensions"] = (self.hzb_w, self.hzb_h)
        k["m_bDownsampleMax"] = 0
        cl.dispatch("minmaxdownsample_CS_Main", [PUSH(0), TEX_SRV(0, self.depth), TEX_UAV(0, self.hzb, 0), SAMPLER(0)],
                    ((self.hzb_w + 7) // 8, (self.hzb_h + 7) // 8, 1), push=k)
        cl.clear_buffer_u32(self.spdAtomic, 0)
        spd = np.zeros(8, np.uint32)
        spd[0] = self.hzb_mips - 1
        spd[1] = ((self.hzb_w + 63) // 64) * ((self.hzb_h + 63) // 64)
        b = [PUSH(0), TEX_SRV(0, self.depth), UAV(0, self.spdAtomic), TEX_UAV(1, self.hzb, min(6, self.hzb_mips - 1)), TEX_UAV(2, self.hzb, 0)]
        b += [TEX_UAV(3 + i, self.hzb, i + 1) for i in range(self.hzb_mips - 1)]
        cl.dispatch("ffx_spd_downsample_pass_CS FFX_SPD_OPTION_DOWNSAMPLE_FILTER=1", b,
                    ((self.hzb_w + 63) // 64, (self.hzb_h + 63) // 64, 1), push=spd)

    # ---- BasePassRenderer::RenderBasePass (:544-588) --------------------------------------------
    def record(self, query: rhi.PipelineStatsQuery | None = None):
        """query: a pipeline statistics query bracketing the whole list (begin after open, end before close), as the
        reference brackets RenderBasePass (:546-549); None records the list without one."""
        if self.taa is None:
            return self._record_frame(query)
        view = self.view
        self.view = self._taa_begin()                                                    # every pass of the frame sees the jittered projection
        try:
            return self._record_frame(query)
        finally:
            self.view = view

    def _record_frame(self, query):
        cl = self.cl
        cl.open()
        if query is not None:
            cl.begin_pipeline_stats(query)
        occ = bool(self.flags & 2)
        self.ran = [False] * 4

        if self.raster_depth:
            cl.clear_texture_f32(self.depth, 0.0)                                        # depth cleared to far at the start of the base pass
        if self.visibility_on:
            cl.clear_texture_u32(self.visibility, 0)                                     # 0 = nothing drawn
            cl.clear_texture_f32(self.motion, 0.0)
        if self.gbuffer_on:
            cl.clear_texture_u32(self.gbufferA, 0)
        if self.lighting_on:
            cl.clear_texture_f32(self.lighting_output, 0.0)                              # the reference's per-frame clear (Scene.cpp:42-70)

        def do(slot, late, am):
            self.ran[slot] = self._gpu_culling(cl, slot, late, am)
            if self.ran[slot]:
                self._render_instances(cl, slot, late, am)
        do(0, False, False)
        if occ:
            self._generate_hzb(cl)
            do(1, True, False)
            do(2, False, True)
            do(3, True, True)
            if self.visibility_on:
                self._resolve_motion(cl)
            self._generate_hzb(cl)
        else:
            do(2, False, True)
            if self.visibility_on:
                self._resolve_motion(cl)
        if query is not None:
            cl.end_pipeline_stats(query)
        if self.ao is not None:                                                          # Scene.cpp's order: behind GBufferRenderer, in front of lighting
            self._ambient_occlusion(cl)
        ddgi_skip = self.ddgi_update is not None and self._ddgi_begin_update()           # converged: nothing of the update, its refit included
        if self.shadows is not None or (self.ddgi_update is not None and not ddgi_skip):  # the TLAS of this frame's instance buffer
            self._refit_tlas(cl)
        if self.shadows is not None:                                                     # Scene.cpp:500: behind AO, in front of lighting
            self._shadow_mask(cl)
            if self.shadow_denoise is not None:
                self._denoise_shadows(cl)
        if self.ddgi_update is not None and not ddgi_skip:                               # behind the refit, in front of lighting
            self._ddgi_update(cl)
        if self.lighting_on:
            self._deferred_lighting(cl)
        if self.sky is not None:                                                         # Scene.cpp:502: between lighting and bloom
            self._sky(cl)
        if self.bloom_mips:                                                              # Scene.cpp:503: between lighting and adapt luminance
            self._bloom(cl)
        if self.post_on:                                                                 # Scene.cpp's order: adapt luminance, then post
            self._post_process(cl)
        if self.probes is not None:                                                      # Scene.cpp:317: GIDebugRenderer, behind PostProcessRenderer
            self._probe_visualization(cl)
        cl.close()
        return cl

    def run(self):
        self.dev.execute(self.cl)

    # ---- read-back (tests) ------------------------------------------------------------------------
    def results(self):
        self.dev.wait_idle()
        out = {}
        for s in range(4):
            if s >= self.num_slots or not self.ran[s]:
                out[s] = None
                continue
            args = self.dispatchArgs[s].download(np.uint32, 4)
            G = int(min(args[0], args[3], self.record_capacity))
            draw = self.drawArgs[s].download(np.uint32, 3)
            V = int(min(draw[0], self.list_capacity))
            out[s] = dict(dispatchArgs=args[:3].copy(), validRecords=int(args[3]),
                          records=self.records[s].download(I.MeshletAmplificationData, G),
                          visMask=self.visMask[s].download(np.uint32, G),
                          visibleList=self.visibleList[s].download(np.uint32, V), drawArgs=draw)
        out["lateCount"] = int(self.lateCount.download(np.uint32, 1)[0])
        out["lateArgs"] = self.lateArgs.download(np.uint32, 3)
        return out

    def release(self):
        self.cl.release()
        for lst in (self.records, self.dispatchArgs, self.visMask, self.visibleList, self.drawArgs):
            for b in lst:
                b.release()
        for b in (self.lateArgs, self.lateCount, self.lateIds, self.spdAtomic, self.dummy, *(self.shardInfo or ())):
            b.release()
        self.hzb.release(); self.depth.release()
        for t in (self.visibility, self.motion, self.gbufferA, self.lighting_output, self.back_buffer, self.exposure_texture, self.luminance, self.histogram,
                  self.bloom_texture, self.ao_depth, self.ao_working, self.ao_edges, self.ssao_texture, self.shadow_mask_texture, self.linear_view_depth,
                  self.blue_noise, self.ddgi_desc, self.ddgi_data, self.ddgi_irradiance, self.ddgi_distance, self.ddgi_rays, self.ddgi_fixed_rays,
                  self.ddgi_variability_buffer, self.ddgi_variability_readback, *(self.ddgi_variability_average or ()),
                  self.probe_positions, self.probe_states, self.probe_culled_positions, self.probe_draw_args, self.probe_instance_to_probe, self.probe_sphere_vertices,
                  self.probe_sphere_indices, self.probe_winners, self.anti_aliased_output, *(self.taa_history or ()), self.shadow_penumbra, self.normal_roughness,
                  self.shadow_tiles, *(self.shadow_data or ()), *(self.shadow_history or ())):
            if t is not None:
                t.release()
