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
