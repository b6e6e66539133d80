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
from . import interop as I
from . import rhi
from .accel import SunShadowPass
from .ddgi import DDGIPass, ProbeDrawPass
from .gtao import AmbientOcclusionPass
from .post import BloomPass, PostPass
from .rhi import CB, PUSH, SAMPLER, SRV, TEX_SRV, TEX_TABLE, TEX_UAV, UAV
from .sky import SkyPass
from .streaming import TextureStreamingPass, check_materials, create_streamed
from .taa import TemporalAAPass

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
        self.streams = []                      # streaming.StreamedTexture of every streamable texture (set_textures(streaming=...))
        self.indices = self.rt = None

    def set_geometry(self, vertices, meshletVertexIds, meshletTriangles):
        """The buffers the mesh shader reads (basepass.hlsl t1, t5, t6): lets the frame rasterise its own depth
        (FrameDriver(raster_depth=True)) instead of taking a synthetic depth image."""
        self.vertices = self.dev.buffer_from(np.ascontiguousarray(vertices, I.RawVertexFormat), "GlobalVertexBuffer", uav=False, min_bytes=20)
        self.meshletVertexIds = self.dev.buffer_from(np.ascontiguousarray(meshletVertexIds, np.uint32), "GlobalMeshletVertexIdxOffsetsBuffer", uav=False)
        self.meshletTriangles = self.dev.buffer_from(np.ascontiguousarray(meshletTriangles, np.uint32), "GlobalMeshletIndicesBuffer", uav=False)

    def set_textures(self, textures, streaming=None):
        """The material textures and their table (the stand-in of ResourceDescriptorHeap[...], include/trhip.h): `textures` is a
        list of (mips, format), mips a list of uint8 [h_k, w_k, 4] arrays (level k of max(w >> k, 1) x max(h >> k, 1); interop.make_mips
        makes them from an image), format rhi.FORMAT_RGBA8_UNORM or rhi.FORMAT_SRGBA8_UNORM; or mips an interop.BlockMips (the levels' raw
        block bytes, as interop.parse_dds gives them) with one of rhi.BC_FORMATS.  Returns their descriptor indices, which
        m_DescriptorIndex of a flagged TextureData names.  Replaces an earlier set; call it before set_materials().
        streaming=dict(region=(w, h) or None, poison=word or None): texture streaming (streaming.py, FrameDriver(streaming=...)).  Every
        texture whose size is a multiple of the region (None: D3D's 64 KB tile shape of its format; a size that is no multiple of a
        GIVEN region is refused, of the default one it stays fully resident) becomes streamable: its mips stay on the host, only its
        packed tail is uploaded, the rest of its storage is filled with the poison word if one is given, and a min-mip map and a
        feedback map of it follow the textures in the table (self.streams; set_materials fills their indices in)."""
        self.release_textures()
        if len(textures) == 0:
            return []
        made = [create_streamed(self.dev, i, mips, fmt, streaming, f"Material Texture {i}") if streaming is not None else None for i, (mips, fmt) in enumerate(textures)]
        self.streams = [s for s in made if s is not None]
        self.texture_table = self.dev.create_texture_table(len(textures) + 2 * len(self.streams))
        for i, (mips, fmt) in enumerate(textures):
            self.textures.append(made[i].texture if made[i] is not None else self.dev.create_sampled_texture(mips, fmt, f"Material Texture {i}"))
            self.texture_table.set(i, self.textures[-1])
        for j, s in enumerate(self.streams):
            s.min_mip_index, s.feedback_index = len(textures) + 2 * j, len(textures) + 2 * j + 1
            self.texture_table.set(s.min_mip_index, s.min_mip_map)
            self.texture_table.set(s.feedback_index, s.feedback)
        return list(range(len(textures)))

    def release_textures(self):
        if self.texture_table is not None:
            self.texture_table.release()
        streamed = {id(s.texture) for s in self.streams}
        for t in self.textures:
            if id(t) not in streamed:
                t.release()
        for s in self.streams:
            s.release()
        self.textures, self.texture_table, self.streams = [], None, []

    def set_materials(self, materials):
        """The MaterialData buffer (basepass.hlsl t3, Graphic::m_GlobalMaterialDataBuffer) that FrameDriver(gbuffer=True)
        resolves GBufferA from.  A material may use textures (m_MaterialFlags) when every flagged slot's m_DescriptorIndex names a
        texture of set_textures() and its feedback and min-mip indices are 0xFFFFFFFF; FrameDriver then binds the texture table and
        the resolve samples them.  With set_textures(streaming=...) a slot of a streamable texture gets that texture's two map indices
        filled in, and may name them itself; an index that names anything else is refused."""
        materials = np.ascontiguousarray(materials, I.MaterialData).copy()
        for bit, slot in enumerate(("m_AlbedoTexture", "m_NormalTexture", "m_MetallicRoughnessTexture", "m_EmissiveTexture")):
            flagged = (materials["m_MaterialFlags"] >> bit) & 1 != 0
            t = materials[slot][flagged]
            if np.any(t["m_DescriptorIndex"] >= len(self.textures)):
                raise ValueError(f"set_materials: a material uses a texture ({slot}.m_DescriptorIndex {int(t['m_DescriptorIndex'][t['m_DescriptorIndex'] >= len(self.textures)][0]):#x}) "
                                 f"that set_textures() has not loaded ({len(self.textures)} textures)")
            if not self.streams and (np.any(t["m_FeedbackTextureDescriptorIndex"] != 0xFFFFFFFF) or np.any(t["m_MinMapTextureDescriptorIndex"] != 0xFFFFFFFF)):
                raise ValueError(f"set_materials: a material's texture ({slot}) names a sampler-feedback or min-mip texture: texture streaming is not supported")
        if self.streams:
            check_materials(materials, self.streams, len(self.textures))
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


class FrameDriver(AmbientOcclusionPass, SunShadowPass, DDGIPass, ProbeDrawPass, SkyPass, BloomPass, TemporalAAPass, PostPass, TextureStreamingPass):
    """BasePassRenderer (Setup + RenderBasePass) over rhi.  One command list per frame.

    The cull, the rasters, the motion / G-buffer resolve, the HZB, deferred lighting and the frame's order are here.  Every optional
    pass is a class of its own in its option's module (gtao.AmbientOcclusionPass, accel.SunShadowPass, ddgi.DDGIPass and
    ddgi.ProbeDrawPass, sky.SkyPass, taa.TemporalAAPass, post.BloomPass and post.PostPass), as the C++ host gives each a renderer:
    its attributes as class-level defaults (a driver without the option answers None), _check_<option>() for the refusals and the
    settings (it touches no device), _create_<option>() for the resources, the methods _record_frame calls, its download_* and
    reset_* methods, and the option's documentation.  __init__ calls the checks in the order in which they refuse, creates the base
    resources, then calls the _create_* methods.
    What a pass class may read from the driver: dev, scene, view; depth, hzb, hzb_w / hzb_h, motion, gbufferA, lighting_output,
    lighting_consts, back_buffer; dir_light, camera_origin, frame_counter, alpha_test; another option's attributes where the
    reference's renderers share them (the sigma denoiser and the post pass read taa's, the probe draw ddgi's); and three helpers:
    _own(resource), which registers what release() releases and returns it; _download(what, on, off, read), the one shape of every
    download_*; _culling_frustum(), the frustum of the frame's projection."""

    def __init__(self, dev: rhi.Device, scene: GpuScene, view, *, record_capacity: int, list_capacity: int | None = None,
                 culling_flags: int = 7, force_mesh_lod: int = -1, freeze_culling_camera: bool = False, alloc=None,
                 shard_late=None, raster_depth: bool = False, visibility: bool = False, gbuffer: bool = False,
                 debug_mode: int = 0, lighting: bool = False, dir_light=((0.0, -1.0, 0.0), 1.0), camera_origin=(0.0, 0.0, 0.0),
                 shadow_mask=None, ssao=None, post: bool = False, exposure=(0.0, 0.18), auto_exposure=(0.004, 12.0, 0.04),
                 bloom=(None, 0.0), bloom_mips: int = 0, bloom_filter_radius: float = 0.005, bloom_strength: float = 0.1, sky=None, ao=None,
                 shadows=None, alpha_test: bool = False, ddgi=None, ddgi_update=None, probes=None, taa=None, shadow_denoise=None,
                 streaming=None):
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
        alpha_test: False (the default) changes nothing: alpha-mask instances are drawn as solid triangles.  True (needs
        raster_depth, which visibility and everything above imply, and GpuScene.set_materials()): ALPHA_MASK_MODE's discard
        (basepass.hlsl:210-215).  Pass slots 2 and 3 dispatch "basepass_MS_Main_depth ALPHA_MASK_MODE=1" or
        "basepass_MS_Main_visibility ALPHA_MASK_MODE=1" with the materials at t3 and, when a loaded material uses a texture, the
        texture table at t19: a sample whose m_ConstAlbedo.w times the albedo texture's alpha is below m_AlphaCutoff is not drawn,
        so depth, the HZB, the visibility buffer and everything resolved from it see through the cut-outs.  With shadows the
        trace binds the table too and a textured cut-out casts the shadow of its kept texels (mip 0).
        post, exposure, auto_exposure, bloom: see post.PostPass.
        bloom_mips, bloom_filter_radius, bloom_strength: see post.BloomPass.
        sky: see sky.SkyPass.
        ao: see gtao.AmbientOcclusionPass.
        shadows, shadow_denoise: see accel.SunShadowPass.
        ddgi, ddgi_update: see ddgi.DDGIPass.
        probes: see ddgi.ProbeDrawPass.
        taa: see taa.TemporalAAPass.
        streaming: see streaming.TextureStreamingPass."""
        self.dev, self.scene, self.view, self._owned = dev, scene, view, []
        lighting = bool(lighting) or bool(post)
        gbuffer = bool(gbuffer) or bool(lighting)
        visibility = bool(visibility) or bool(gbuffer)
        if visibility and shard_late is not None:
            raise ValueError(("post-processing" if post else "deferred lighting" if lighting else "G-buffer" if gbuffer else "visibility buffer") + " with a shard exchange: list positions are per rank, not global")
        if gbuffer and scene.materials is None:
            raise ValueError(("post=True" if post else "lighting=True" if lighting else "gbuffer=True") + " needs GpuScene.set_materials()")
        self._check_ddgi(ddgi, ddgi_update, lighting, debug_mode)
        self._check_probes(probes, post)
        self._check_taa(taa, post)
        self.alpha_test = bool(alpha_test)
        if self.alpha_test and not (raster_depth or visibility):
            raise ValueError("alpha_test=True needs raster_depth=True (or visibility, gbuffer, lighting, post): the test runs in the rasters, and a frame without them draws nothing")
        if self.alpha_test and scene.materials is None:
            raise ValueError("alpha_test=True needs GpuScene.set_materials(): the test reads m_ConstAlbedo.w, m_AlphaCutoff and the albedo texture of each instance's material")
        self._check_streaming(streaming, gbuffer)
        self._check_post(post, exposure, auto_exposure, bloom)
        self._check_bloom(bloom_mips, bloom_filter_radius, bloom_strength, bloom, post)
        self._check_sky(sky, lighting)
        self._check_ao(ao, gbuffer, ssao)
        self._check_shadows(shadows, shadow_denoise, gbuffer, shadow_mask)
        self.gbuffer_on, self.lighting_on, self.visibility_on = bool(gbuffer), bool(lighting), bool(visibility)
        self.frame_counter = 0
        self.dir_light = (tuple(float(x) for x in dir_light[0]), float(dir_light[1]))
        self.camera_origin = tuple(float(x) for x in camera_origin)
        self.shadow_mask, self.ssao = shadow_mask, ssao
        self.lighting_consts = None
        self.debug_mode = int(debug_mode)
        self.raster_depth = bool(raster_depth) or self.visibility_on       # depth = the visible meshlets rasterised ("basepass_MS_Main_depth"), cleared per frame
        assert not self.raster_depth or scene.vertices is not None, "raster_depth needs GpuScene.set_geometry()"
        self.shard_late = shard_late
        self.shardInfo = [self._own(dev.create_buffer(8, f"ShardLateInfo{b}")) for b in (0, 1)] if shard_late is not None else None
        self.flags = culling_flags & 7
        self.force_mesh_lod = force_mesh_lod
        self.freeze = freeze_culling_camera
        self.record_capacity = int(record_capacity)
        self.list_capacity = int(list_capacity if list_capacity is not None else record_capacity * 32)
        W, H = view.renderW, view.renderH
        hw, hh = I.hzb_dims(W, H)
        self.hzb_w, self.hzb_h = hw, hh
        self.hzb_mips = I.compute_nb_mips(hw, hh)
        # GBufferRenderer::Initialize (BasePassRenderers.cpp:596-616): HZB cleared to far = 0
        self.hzb = self._own(dev.create_texture(hw, hh, self.hzb_mips, rhi.FORMAT_R16_FLOAT, "HZB"))
        self.depth = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_R32_FLOAT, "Depth Buffer"))
        init = dev.create_command_list()
        init.open(); init.clear_texture_f32(self.hzb, 0.0); init.clear_texture_f32(self.depth, 0.0); init.close()
        dev.execute(init); dev.wait_idle(); init.release()
        self.visibility = self.motion = self.gbufferA = self.lighting_output = None
        if self.lighting_on:                         # DeferredLightingRenderer::Setup (DeferredLightingRenderer.cpp:23-34)
            self.lighting_output = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_R11G11B10_FLOAT, "Lighting Output"))
        if self.gbuffer_on:                          # GBufferA (GraphicConstants.h:24), created in GBufferRenderer::Setup (:622-632)
            self.gbufferA = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_RGBA32_UINT, "GBufferA"))
        if self.visibility_on:                       # GBufferRenderer's visibility buffer + GBufferMotion, render resolution
            self.visibility = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_RG32_UINT, "VisibilityBuffer"))
            self.motion = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_RG16_FLOAT, "GBufferMotion"))
        # BasePassRenderer::Setup (:223-296); one set of outputs per pass slot (DESIGN.md "Outputs")
        n = max(scene.numInstances, 1)

        def mk(nbytes, name, stride=4, indirect=False):
            b = alloc(nbytes, name, stride, indirect) if alloc is not None else None
            return self._own(b if b is not None else dev.create_buffer(nbytes, name, stride=stride, indirect=indirect))
        # slots 2,3 (alpha-mask lists) are only materialised when the scene has alpha-mask primitives
        slots = 4 if scene.numAlphaMask else 2
        self.records = [mk(12 * self.record_capacity, f"MeshletAmplificationDataBuffer{s}", 12) for s in range(slots)]
        self.dispatchArgs = [mk(16, f"MeshletDispatchArgumentsBuffer{s}", 16, True) for s in range(slots)]
        self.visMask = [mk(4 * self.record_capacity, f"MeshletVisibilityMaskBuffer{s}") for s in range(slots)]
        self.visibleList = [mk(4 * max(self.list_capacity, 1), f"VisibleMeshletListBuffer{s}") for s in range(slots)]
        self.drawArgs = [mk(12, f"VisibleMeshletDrawArgsBuffer{s}", 12, True) for s in range(slots)]
        self.num_slots = slots
        self.lateArgs = self._own(dev.create_buffer(12, "LateCullDispatchIndirectArgs", stride=12, indirect=True))
        self.lateCount = self._own(dev.create_buffer(4, "LateCullInstanceCountBuffer"))
        self.lateIds = self._own(dev.create_buffer(4 * n, "LateCullInstanceIDsBuffer"))
        self.spdAtomic = self._own(dev.create_buffer(24, "SPD Global Atomic Buffer", stride=24))
        self.dummy = self._own(dev.create_buffer(16, "DummyUIntStructuredBuffer"))
        self.cl = dev.create_command_list()
        self.ran = [False] * 4
        self._create_post()
        self._create_bloom()
        self._create_taa()
        self._create_ao()
        self._create_shadows()
        self._create_ddgi()
        self._create_probes()
        self._create_streaming()

    def _own(self, resource):
        """Registers a resource the driver created (or was handed by alloc) for release(); returns it."""
        self._owned.append(resource)
        return resource

    def _download(self, what: str, on, off: str, read):
        """Every download_*: refuses as "<what>: <off>" when `on` (the option's setting or resource) is None; else waits and returns read()."""
        if on is None:
            raise ValueError(f"{what}: {off}")
        self.dev.wait_idle()
        return read()

    def _culling_frustum(self) -> np.ndarray:
        """m_Frustum of the cull, the base pass and the probe draw: the frame's projection, jittered under taa=."""
        return culling_frustum(self.view.viewToClip)

    # ---- per-frame constants (BasePassRenderers.cpp:334-347, 445-458, 551-563) ------------------
    def _cull_consts(self, nb: int) -> np.ndarray:
        v = self.view
        k = np.zeros(1, I.GPUCullingPassConstants)
        occ = bool(self.flags & 2)
        k["m_NbInstances"] = nb
        k["m_CullingFlags"] = self.flags
        k["m_HZBDimensions"] = (self.hzb_w, self.hzb_h) if occ else (1, 1)
        k["m_Frustum"] = self._culling_frustum()
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
        k["m_Frustum"] = self._culling_frustum()
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
            if self.streaming is not None:                                               # BasePassRenderers.cpp:458
                k["m_bWriteSamplerFeedback"], k["m_bVisualizeMinMipTilesOnAlbedoOutput"] = 1, int(self.streaming["visualize"])
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
            cl.dispatch("basepass_PS_Main_GBuffer", b, I.groups8(v.renderW, v.renderH))
            return
        cl.dispatch("basepass_PS_Main_motion", b + [TEX_UAV(0, self.motion, 0)], I.groups8(v.renderW, v.renderH))

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
        cl.dispatch("deferredlighting_PS_Main_Debug" if self.debug_mode != 0 else "deferredlighting_PS_Main", b, I.groups8(v.renderW, v.renderH))

    # ---- BasePassRenderer::GenerateHZB (:505-542) + SPD::Execute (FFXHelpers.cpp:36-115) --------
    def _generate_hzb(self, cl):
        if self.freeze:
            return
        k = np.zeros(1, I.MinMaxDownsampleConsts)
        k["m_OutputDimensions"] = (self.hzb_w, self.hzb_h)
        k["m_bDownsampleMax"] = 0
        cl.dispatch("minmaxdownsample_CS_Main", [PUSH(0), TEX_SRV(0, self.depth), TEX_UAV(0, self.hzb, 0), SAMPLER(0)],
                    I.groups8(self.hzb_w, self.hzb_h), push=k)
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
        if self.streaming is not None:                                                   # TextureFeedbackManager::BeginFrame
            self._streaming_begin_frame(cl)

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
        if self.streaming is not None:                                                   # TextureFeedbackManager::EndFrame
            self._streaming_end_frame(cl)
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
            self._adapt_luminance(cl)
            if self.taa is not None:                                                     # Scene.cpp:506: between adapt luminance and post
                self._taa_resolve(cl)
            self._post_process(cl, self.anti_aliased_output if self.taa is not None else self.lighting_output)
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
        for r in self._owned:
            r.release()
