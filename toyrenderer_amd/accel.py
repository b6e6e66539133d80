"""Host side of the ray-traced sun shadows: the acceleration structure's arrays from the back end's one builder
(trhip_blas_build / trhip_tlas_build, csrc/accel_build.cpp; no device needed) and ShadowMaskRenderer's settings and constant block
(ShadowMaskRenderer.cpp:253-305).  The C++ host (csrc/host/ShadowMaskRenderer.cpp, Scene.cpp) calls the same two functions and
fills the same block."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import interop as I
from . import rhi
from . import taa as taamod
from .rhi import CB, PUSH, SAMPLER, SRV, TEX_SRV, TEX_TABLE, TEX_UAV, UAV

DEFAULT_SUN_ANGULAR_DIAMETER = 0.533          # ShadowMaskRenderer.cpp:89
kGoldenRatio = np.float32(1.61803398875)


def max_depth() -> int:
    return int(rhi.load().trhip_accel_max_depth())


def leaf_capacity() -> int:
    return int(rhi.load().trhip_blas_leaf_capacity())


def build_blas(vertices: np.ndarray, indices: np.ndarray):
    """One mesh: `vertices` from the mesh's first vertex on (RawVertexFormat, or float32 [n, 3]), `indices` its LOD-0 index list.
    Returns (nodes AccelNode[], tri_order uint32[], depth)."""
    L = rhi.load()
    vertices = np.ascontiguousarray(vertices)
    if vertices.dtype != I.RawVertexFormat:
        vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        stride = 12
    else:
        stride = I.RawVertexFormat.itemsize
    indices = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    tris = len(indices) // 3
    cap = int(L.trhip_accel_max_nodes(tris))
    nodes = np.zeros(max(cap, 1), I.AccelNode)
    order = np.zeros(max(tris, 1), np.uint32)
    nn, nt, depth = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rhi._check(L.trhip_blas_build(vertices.ctypes.data, stride, len(vertices), indices.ctypes.data, len(indices), nodes.ctypes.data, cap, order.ctypes.data,
                                  C.byref(nn), C.byref(nt), C.byref(depth)))
    return nodes[:nn.value].copy(), order[:nt.value].copy(), int(depth.value)


def build_scene_blas(vertices: np.ndarray, indices: np.ndarray, mesh_data: np.ndarray, index_counts) -> dict:
    """Every mesh of a scene: the global vertex and index buffers, the MeshData table (m_GlobalVertexBufferIdx, m_GlobalIndexBufferIdx)
    and the index count of each mesh (MeshSpecificData.m_NumIndices).  Returns headers (BLASHeader per mesh), nodes and tri_order
    (all meshes back to back) and depths."""
    vertices = np.ascontiguousarray(vertices, I.RawVertexFormat)
    indices = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    mesh_data = np.ascontiguousarray(mesh_data, I.MeshData)
    index_counts = np.asarray(index_counts)
    if index_counts.dtype.names:
        index_counts = index_counts["m_NumIndices"]
    index_counts = np.ascontiguousarray(index_counts, np.uint32).reshape(-1)
    if len(index_counts) != len(mesh_data):
        raise ValueError(f"set_raytracing: {len(index_counts)} index counts for {len(mesh_data)} meshes")
    headers = np.zeros(len(mesh_data), I.BLASHeader)
    nodes, orders, depths = [], [], []
    node_at = tri_at = 0
    for m, md in enumerate(mesh_data):
        first, count, vbase = int(md["m_GlobalIndexBufferIdx"]), int(index_counts[m]), int(md["m_GlobalVertexBufferIdx"])
        if count % 3 or first + count > len(indices):
            raise ValueError(f"set_raytracing: mesh {m}: indices [{first}, {first + count}) of {len(indices)} are not a list of whole triangles")
        if vbase > len(vertices):
            raise ValueError(f"set_raytracing: mesh {m}: first vertex {vbase} of {len(vertices)}")
        n, o, d = build_blas(vertices[vbase:], indices[first:first + count])
        headers[m] = (node_at, len(n), tri_at, len(o))
        nodes.append(n); orders.append(o); depths.append(d)
        node_at += len(n); tri_at += len(o)
    return dict(headers=headers, nodes=np.concatenate(nodes) if nodes else np.zeros(0, I.AccelNode),
                tri_order=np.concatenate(orders) if orders else np.zeros(0, np.uint32), depths=depths, index_counts=index_counts)


def instance_flags(num_instances: int, opaque_ids, alpha_mask_ids) -> np.ndarray:
    """Scene.cpp:454: ForceOpaque for the instances of the opaque list, ForceNonOpaque for those of the alpha-mask list; an
    instance in neither list is not in the structure."""
    flags = np.zeros(num_instances, np.uint32)
    flags[np.asarray(opaque_ids, np.int64)] = I.kTLASInstanceForceOpaque
    flags[np.asarray(alpha_mask_ids, np.int64)] = I.kTLASInstanceForceNonOpaque
    return flags


def build_tlas(instances: np.ndarray, flags: np.ndarray, blas: dict) -> dict:
    """The topology over the instances' rest transforms.  Returns nodes, records (TLASInstance per instance: flags and leaf_node
    set, the matrix left to the refit), level_nodes, level_offsets, num_levels."""
    L = rhi.load()
    instances = np.ascontiguousarray(instances, I.BasePassInstanceConstants)
    flags = np.ascontiguousarray(flags, np.uint32)
    n = len(instances)
    cap = int(L.trhip_accel_max_nodes(n))
    nodes = np.zeros(max(cap, 1), I.AccelNode)
    records = np.zeros(max(n, 1), I.TLASInstance)
    level_nodes = np.zeros(max(cap, 1), np.uint32)
    level_offsets = np.zeros(max_depth() + 2, np.uint32)
    nn, nl = C.c_uint32(), C.c_uint32()
    headers, bn = np.ascontiguousarray(blas["headers"]), np.ascontiguousarray(blas["nodes"])
    rhi._check(L.trhip_tlas_build(instances.ctypes.data, n, flags.ctypes.data, headers.ctypes.data, len(headers), bn.ctypes.data, len(bn), nodes.ctypes.data, cap,
                                  records.ctypes.data, level_nodes.ctypes.data, level_offsets.ctypes.data, C.byref(nn), C.byref(nl)))
    return dict(nodes=nodes[:nn.value].copy(), records=records[:n].copy(), level_nodes=level_nodes[:max(nn.value, 1)].copy(), level_offsets=level_offsets,
                num_levels=int(nl.value))


# ---- ShadowMaskRenderer's settings and constants ---------------------------------------------------------------------------------
DEFAULTS = dict(soft=True, sun_angular_diameter=DEFAULT_SUN_ANGULAR_DIAMETER, ray_start_offset=0.1, noise=None)


def check_settings(settings) -> dict:
    """The dict FrameDriver(shadows=...) takes, completed with the reference's defaults and checked.  noise is required: the
    128 x 128 x 4 uint8 blue noise image (CommonResources::BlueNoise), an input as the Hosek dataset is."""
    if not isinstance(settings, dict):
        raise ValueError("shadows: needs a dict of settings (soft, sun_angular_diameter, ray_start_offset, noise)")
    unknown = set(settings) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"shadows: unknown setting {sorted(unknown)[0]!r}")
    s = {**DEFAULTS, **settings}
    if s["noise"] is None:
        raise ValueError("shadows: needs noise = the 128 x 128 x 4 uint8 blue noise image")
    noise = np.asarray(s["noise"])
    if noise.dtype != np.uint8 or noise.shape != (I.kBlueNoiseSize, I.kBlueNoiseSize, 4):
        raise ValueError(f"shadows: noise is {noise.dtype} {noise.shape}, needs uint8 (128, 128, 4)")
    d, off = float(s["sun_angular_diameter"]), float(s["ray_start_offset"])
    if not (math.isfinite(d) and 0.0 <= d < 180.0):
        raise ValueError(f"shadows: sun_angular_diameter = {d}: needs degrees in [0, 180)")
    if not (math.isfinite(off) and off >= 0.0):
        raise ValueError(f"shadows: ray_start_offset = {off}: needs a finite offset >= 0")
    return dict(soft=bool(s["soft"]), sun_angular_diameter=d, ray_start_offset=off, noise=np.ascontiguousarray(noise))


def tan_sun_angular_radius(settings: dict) -> np.float32:
    """tan(radians(d / 2)) of the float32 diameter, evaluated in double and rounded once (the reference calls tanf: a stated
    deviation, so that both hosts hand the GPU the same word); 0 without soft shadows."""
    if not settings["soft"]:
        return np.float32(0.0)
    return np.float32(math.tan(math.radians(float(np.float32(settings["sun_angular_diameter"])) / 2.0)))


def noise_words(noise: np.ndarray) -> np.ndarray:
    """The RGBA8_UNORM texels of the noise image, R in the low byte: uint32 [128, 128]."""
    return np.ascontiguousarray(noise, np.uint8).reshape(I.kBlueNoiseSize, I.kBlueNoiseSize, 4).view("<u4").reshape(I.kBlueNoiseSize, I.kBlueNoiseSize)


def shadow_consts(clip_to_world, light_direction, camera_position, W: int, H: int, settings: dict, frame_counter: int, denoise: bool = False) -> np.ndarray:
    """ShadowMaskConsts of one frame (ShadowMaskRenderer.cpp:266-274).  m_bDoDenoising = 0 unless denoise: the trace then writes the
    R16_FLOAT penumbra texture in place of the mask (csrc/k_shadowmask.hip)."""
    k = np.zeros(1, I.ShadowMaskConsts)
    k["m_ClipToWorld"] = clip_to_world
    k["m_DirectionalLightDirection"] = light_direction
    k["m_NoisePhase"] = np.float32(int(frame_counter) & 0xFF) * kGoldenRatio
    k["m_CameraPosition"] = camera_position
    k["m_TanSunAngularRadius"] = tan_sun_angular_radius(settings)
    k["m_OutputResolution"] = (W, H)
    k["m_RayStartOffset"] = np.float32(settings["ray_start_offset"])
    if denoise:
        k["m_bDoDenoising"] = 1
    return k


# ---- the shadow denoiser's settings and constants (csrc/k_sigma.hip) -----------------------------------------------------------------
# plane_distance_sensitivity and stabilization_strength: NRD's published defaults.  sigma_scale: this project's choice (csrc/k_sigma.hip,
# SETTINGS).  Nobody has judged any of them on a picture from this build.
DENOISE_DEFAULTS = dict(plane_distance_sensitivity=0.02, stabilization_strength=5.0 / 6.0, sigma_scale=2.0, scene_radius=0.0)
kSigmaTile = 16
DENOISE_OFF = "shadow denoising is off (shadow_denoise=None)"


def check_denoise_settings(settings) -> dict:
    """The dict FrameDriver(shadow_denoise=...) takes, completed with DENOISE_DEFAULTS and checked: plane_distance_sensitivity > 0,
    stabilization_strength in [0, 1], sigma_scale >= 0, scene_radius >= 0 (m_DenoisingRange = max(100, 2 * scene_radius)), all finite."""
    if not isinstance(settings, dict):
        raise ValueError("shadow_denoise: needs a dict of settings (plane_distance_sensitivity, stabilization_strength, sigma_scale, scene_radius)")
    unknown = set(settings) - set(DENOISE_DEFAULTS)
    if unknown:
        raise ValueError(f"shadow_denoise: unknown setting {sorted(unknown)[0]!r}")
    s = {k: float(v) for k, v in {**DENOISE_DEFAULTS, **settings}.items()}
    if not (math.isfinite(s["plane_distance_sensitivity"]) and s["plane_distance_sensitivity"] > 0.0):
        raise ValueError(f"shadow_denoise: plane_distance_sensitivity = {s['plane_distance_sensitivity']}: needs a finite value > 0")
    if not 0.0 <= s["stabilization_strength"] <= 1.0:
        raise ValueError(f"shadow_denoise: stabilization_strength = {s['stabilization_strength']}: needs a value in [0, 1]")
    if not (math.isfinite(s["sigma_scale"]) and s["sigma_scale"] >= 0.0):
        raise ValueError(f"shadow_denoise: sigma_scale = {s['sigma_scale']}: needs a finite value >= 0")
    if not (math.isfinite(s["scene_radius"]) and s["scene_radius"] >= 0.0):
        raise ValueError(f"shadow_denoise: scene_radius = {s['scene_radius']}: needs a finite value >= 0")
    return s


def sigma_tiles(W: int, H: int):
    """(width, height) of the denoiser's R8_UINT tile texture."""
    return (W + kSigmaTile - 1) // kSigmaTile, (H + kSigmaTile - 1) // kSigmaTile


def sigma_consts(clip_to_world, view_to_clip, W: int, H: int, settings: dict, frame_index: int, pass_index: int = 0, reset_history: bool = False,
                 jitter_delta=(0.0, 0.0)) -> np.ndarray:
    """SigmaConsts of one dispatch.  m_PixelUnproject = 2 / (m_ViewToClip[1][1] * H) in binary32: the world height of one pixel at
    unit distance; m_DenoisingRange = max(100, 2 * scene_radius) (ShadowMaskRenderer.cpp:368)."""
    F = np.float32
    k = np.zeros(1, I.SigmaConsts)
    k["m_ClipToWorld"] = clip_to_world
    k["m_OutputDims"] = (W, H)
    k["m_JitterDelta"] = jitter_delta
    k["m_PixelUnproject"] = F(2.0) / (F(np.asarray(view_to_clip, F).reshape(4, 4)[1, 1]) * F(H))
    k["m_DenoisingRange"] = max(F(100.0), F(2.0) * F(settings["scene_radius"]))
    k["m_PlaneDistanceSensitivity"] = F(settings["plane_distance_sensitivity"])
    k["m_StabilizationStrength"] = F(settings["stabilization_strength"])
    k["m_SigmaScale"] = F(settings["sigma_scale"])
    k["m_FrameIndex"] = int(frame_index) & 0xFFFFFFFF
    k["m_Pass"] = pass_index
    k["m_bResetHistory"] = 1 if reset_history else 0
    return k


class SunShadowPass:
    """The TLAS refit, which the DDGI probe update shares, and the sun shadows.
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
    shadows = shadow_consts = shadow_mask_texture = linear_view_depth = blue_noise = None
    shadow_denoise = sigma_consts = shadow_penumbra = normal_roughness = shadow_tiles = shadow_data = shadow_history = None
    _shadow_history_reset, shadow_history_written = True, 1

    def _check_shadows(self, shadows, shadow_denoise, gbuffer, shadow_mask):
        if shadows is not None:
            if not gbuffer:
                raise ValueError("shadows=... needs gbuffer=True (or lighting=True): the rays start at the G-buffer's positions and normals")
            if shadow_mask is not None:
                raise ValueError("shadows=... together with an external shadow_mask= texture: the driver generates the texture itself")
            if self.scene.rt is None:
                raise ValueError("shadows=... needs GpuScene.set_raytracing(): the acceleration structure the rays walk")
            self.shadows = check_settings(shadows)
        if shadow_denoise is not None:
            if self.shadows is None:
                raise ValueError("shadow_denoise=... needs shadows=...: it denoises the mask those settings trace")
            self.shadow_denoise = check_denoise_settings(shadow_denoise)

    def _create_shadows(self):
        dev, W, H = self.dev, self.view.renderW, self.view.renderH
        if self.shadows is not None:                 # ShadowMaskRenderer::Setup (ShadowMaskRenderer.cpp:187-251) + CommonResources::BlueNoise
            self.shadow_mask_texture = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_R8_UNORM, "Shadow Mask Texture"))
            self.linear_view_depth = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_R16_FLOAT, "Linear View Depth"))
            self.blue_noise = self._own(dev.create_texture(I.kBlueNoiseSize, I.kBlueNoiseSize, 1, rhi.FORMAT_RGBA8_UNORM, "Blue Noise", uav=False))
            self.blue_noise.upload_mip(0, noise_words(self.shadows["noise"]))
            self.shadow_mask = self.shadow_mask_texture      # what the lighting pass binds as t4
        if self.shadow_denoise is not None:          # ShadowMaskRenderer::Setup's textures for the denoiser (ShadowMaskRenderer.cpp:205-233) and the two histories
            self.shadow_penumbra = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_R16_FLOAT, "Shadow Penumbra Texture"))
            self.normal_roughness = self._own(dev.create_texture(W, H, 1, rhi.FORMAT_R10G10B10A2_UNORM, "Normal Roughness Texture"))
            self.shadow_tiles = self._own(dev.create_texture(*sigma_tiles(W, H), 1, rhi.FORMAT_R8_UINT, "Shadow Tiles"))
            self.shadow_data = [self._own(dev.create_texture(W, H, 1, rhi.FORMAT_RG16_FLOAT, f"Shadow Data {i}")) for i in (0, 1)]
            self.shadow_history = [self._own(dev.create_texture(W, H, 1, rhi.FORMAT_R16_FLOAT, f"Shadow History {i}")) for i in (0, 1)]

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
        self.shadow_consts = shadow_consts(I.clip_to_world(v.worldToView, v.viewToClip), self.dir_light[0], self.camera_origin, W, H, self.shadows,
                                           self.frame_counter, denoise)
        cb = cl.constant_buffer(self.shadow_consts, "ShadowMaskConsts")
        cl.dispatch("shadowmask_CS_ShadowMask",
                    [CB(0, cb), TEX_SRV(0, self.depth), SRV(1, rt["tlas_nodes"]), TEX_SRV(2, self.gbufferA), SRV(3, sc.instances), SRV(4, sc.vertices),
                     SRV(5, sc.materials), SRV(6, sc.indices), SRV(7, sc.meshData), TEX_SRV(8, self.blue_noise),
                     TEX_UAV(0, self.shadow_penumbra if denoise else self.shadow_mask_texture, 0),
                     TEX_UAV(1, self.linear_view_depth, 0), SRV(9, rt["tlas_instances"]), SRV(10, rt["headers"]), SRV(11, rt["blas_nodes"]),
                     SRV(12, rt["tri_order"]), SAMPLER(0), SAMPLER(1)] + ([TEX_TABLE(sc.texture_table)] if self.alpha_test and sc.textured else []),
                    I.groups8(W, H))

    # ---- ShadowMaskRenderer::DenoiseShadows (ShadowMaskRenderer.cpp:337-500): PackNormalRoughness and the denoiser's four dispatches ----
    def _denoise_shadows(self, cl):
        v, W, H = self.view, self.view.renderW, self.view.renderH
        groups = I.groups8(W, H)
        pk = np.zeros(1, I.PackNormalAndRoughnessConsts)
        pk["m_OutputResolution"] = (W, H)
        cl.dispatch("shadowmask_CS_PackNormalAndRoughness", [PUSH(0), TEX_SRV(2, self.gbufferA), TEX_UAV(0, self.normal_roughness, 0)], groups, push=pk)
        delta = taamod.jitter_delta(*self.taa_jitter) if self.taa is not None else (0.0, 0.0)
        k = [sigma_consts(I.clip_to_world(v.worldToView, v.viewToClip), v.viewToClip, W, H, self.shadow_denoise, self.frame_counter, p,
                          self._shadow_history_reset, delta) for p in (0, 1)]
        self.sigma_consts = k[0]
        cb = [cl.constant_buffer(x, "SigmaConsts") for x in k]
        lvd, tiles, data = self.linear_view_depth, self.shadow_tiles, self.shadow_data
        tw, th = sigma_tiles(W, H)
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
            raise ValueError("reset_shadow_history: " + DENOISE_OFF)
        self._shadow_history_reset = True

    def download_shadow_mask(self) -> np.ndarray:
        """The bytes of the generated shadow mask, (H, W) uint8."""
        return self._download("download_shadow_mask", self.shadow_mask_texture, "shadow generation is off (shadows=None)", lambda: self.shadow_mask_texture.download_mip(0))

    def download_shadow_penumbra(self) -> np.ndarray:
        """The binary16 words of the penumbra texture the trace wrote, (H, W) uint16."""
        return self._download("download_shadow_penumbra", self.shadow_denoise, DENOISE_OFF, lambda: self.shadow_penumbra.download_mip(0))

    def download_shadow_tiles(self) -> np.ndarray:
        """The tile bytes of the last record(), (ceil(H / 16), ceil(W / 16)) uint8."""
        return self._download("download_shadow_tiles", self.shadow_denoise, DENOISE_OFF, lambda: self.shadow_tiles.download_mip(0))

    def download_shadow_history(self) -> np.ndarray:
        """The binary16 words of the shadow history the last record() wrote, (H, W) uint16."""
        return self._download("download_shadow_history", self.shadow_denoise, DENOISE_OFF, lambda: self.shadow_history[self.shadow_history_written].download_mip(0))
