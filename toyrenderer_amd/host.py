"""ctypes binding of the C++ host mirror (include/trhost.h -> lib/libtoyrenderer_host.so):
Graphic / Scene / RenderGraph / BasePassRenderers driving the HIP kernels through the C ABI.
This is the drop-in path; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import interop as I
from . import rhi
from .rhi import PipelineStatistics

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtoyrenderer_host.so")

HOST_SYMBOLS = [
    "trhost_last_error", "trhost_initialize", "trhost_shutdown", "trhost_load_scene", "trhost_upload_meshlets", "trhost_load_nodes",
    "trhost_set_node_transforms", "trhost_set_instance_update_range", "trhost_set_camera", "trhost_set_culling", "trhost_set_limits", "trhost_upload_depth",
    "trhost_upload_hzb_mip", "trhost_download_hzb_mip", "trhost_hzb_info", "trhost_frame", "trhost_wait_idle",
    "trhost_pass_buffers", "trhost_instance_buffer", "trhost_device", "trhost_render_graph_stats", "trhost_renderer_times",
    "trhost_heap_sim", "trhost_residency_tiles", "trhost_residency_round",
    "trhost_set_texture_streaming", "trhost_set_texture_streaming_region", "trhost_get_texture_streaming_stats", "trhost_download_min_mip", "trhost_set_shard_late_exchange", "trhost_set_gpu_timers",
    "trhost_set_pipeline_statistics", "trhost_pipeline_statistics",
    "trhost_rccl_allgather", "trhost_exchange_create", "trhost_exchange_run", "trhost_exchange_wait", "trhost_exchange_outputs",
    "trhost_exchange_destroy", "trhost_load_geometry", "trhost_set_raster_depth", "trhost_download_depth",
    "trhost_set_visibility_buffer", "trhost_download_visibility", "trhost_download_motion",
    "trhost_load_materials", "trhost_create_material_texture", "trhost_create_material_texture_dds", "trhost_set_gbuffer", "trhost_set_alpha_test", "trhost_set_debug_view_mode", "trhost_download_gbuffer_a",
    "trhost_load_scene_cached", "trhost_scene_list_sizes", "trhost_rccl_allreduce_max_u32", "trhost_load_gi_probes", "trhost_gi_probe_buffers",
    "trhost_set_renderer_queue", "trhost_render_graph_frame_stats",
    "trhost_set_deferred_lighting", "trhost_set_directional_light", "trhost_upload_shadow_mask", "trhost_download_lighting_output",
    "trhost_get_deferred_lighting_consts", "trhost_upload_ddgi_volume", "trhost_set_ddgi",
    "trhost_set_ddgi_update", "trhost_set_ddgi_probe_placement", "trhost_reset_ddgi_volume", "trhost_download_ddgi_volume", "trhost_get_ddgi_update_consts",
    "trhost_set_ddgi_probe_variability", "trhost_get_ddgi_variability", "trhost_reset_ddgi_variability", "trhost_ddgi_variability_run", "trhost_download_ddgi_variability",
    "trhost_set_ddgi_probe_visualization", "trhost_get_ddgi_probe_visualization_consts", "trhost_unit_sphere",
    "trhost_set_post_process", "trhost_set_exposure", "trhost_set_auto_exposure", "trhost_set_frame_time_ms", "trhost_upload_bloom",
    "trhost_download_back_buffer", "trhost_get_scene_luminance", "trhost_reset_exposure", "trhost_get_post_process_consts",
    "trhost_set_bloom", "trhost_download_bloom", "trhost_get_bloom_consts",
    "trhost_set_taa", "trhost_reset_taa_history", "trhost_download_anti_aliased_output", "trhost_download_taa_history", "trhost_get_taa_consts",
    "trhost_load_sky_dataset", "trhost_set_sky", "trhost_get_sky_consts",
    "trhost_set_ambient_occlusion", "trhost_download_ssao", "trhost_get_gtao_consts",
    "trhost_load_raytracing", "trhost_upload_blue_noise", "trhost_set_shadow_mask", "trhost_download_shadow_mask", "trhost_get_shadow_mask_consts",
    "trhost_set_shadow_denoising", "trhost_reset_shadow_history", "trhost_download_shadow_penumbra", "trhost_download_shadow_tiles", "trhost_download_shadow_history",
    "trhost_get_sigma_consts",
]

ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)   # trhost_allgather_fn


class ExchangeDesc(C.Structure):
    _fields_ = [("world", C.c_uint32), ("rank", C.c_uint32), ("slot_groups", C.c_uint32), ("group_capacity", C.c_uint32),
                ("list_capacity", C.c_uint64), ("pass_slot_mask", C.c_uint32), ("overlap", C.c_int),
                ("slots_allgather", C.c_void_p), ("slots_user", C.c_void_p), ("late_allgather", C.c_void_p), ("late_user", C.c_void_p),
                ("list_presence_mask", C.c_uint32), ("depth_allreduce_max", C.c_void_p), ("depth_user", C.c_void_p),
                ("slot_runs", C.c_uint32), ("global_group_capacity", C.c_uint32)]


DEPTH_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)   # trhost_exchange_desc.depth_allreduce_max
SHARD_LATE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int)   # trhost_shard_late_fn


class PassBuffers(C.Structure):
    _fields_ = [("ran", C.c_int), ("records", C.c_void_p), ("dispatch_args", C.c_void_p), ("vis_mask", C.c_void_p),
                ("visible_list", C.c_void_p), ("draw_args", C.c_void_p), ("late_count", C.c_void_p), ("late_args", C.c_void_p)]


class HostError(RuntimeError):
    pass


_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    rhi.load()   # libtrhip.so first (RPATH $ORIGIN also finds it)
    if not os.path.exists(LIB_PATH):
        raise HostError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
    L = C.CDLL(LIB_PATH)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.trhost_last_error.restype = C.c_char_p
    L.trhost_initialize.argtypes = [C.c_int, u32, u32, vp]
    L.trhost_shutdown.restype = None
    L.trhost_load_scene.argtypes = [vp, u32, vp, u32, vp, u64, vp, u32, vp, u32]
    L.trhost_upload_meshlets.argtypes = [u64, vp, u64]
    L.trhost_load_nodes.argtypes = [vp, u32, vp]
    L.trhost_set_node_transforms.argtypes = [vp, u32]
    L.trhost_set_instance_update_range.argtypes = [u32, u32]
    L.trhost_set_camera.argtypes = [vp, vp, vp, C.c_float]
    L.trhost_set_culling.argtypes = [C.c_int] * 5
    L.trhost_set_limits.argtypes = [u32, u64]
    L.trhost_upload_depth.argtypes = [vp, u32, u32]
    L.trhost_load_geometry.argtypes = [vp, u64, vp, u64, vp, u64]
    L.trhost_load_scene_cached.argtypes = [C.c_char_p, vp, u32, vp, u32, vp, u32]
    L.trhost_set_raster_depth.argtypes = [C.c_int]
    L.trhost_download_depth.argtypes = [vp, u64]
    L.trhost_set_visibility_buffer.argtypes = [C.c_int]
    L.trhost_download_visibility.argtypes = [vp, u64]
    L.trhost_download_motion.argtypes = [vp, u64]
    L.trhost_load_materials.argtypes = [vp, u32]
    L.trhost_create_material_texture.argtypes = [u32, u32, u32, u32, vp, u64]
    L.trhost_create_material_texture_dds.argtypes = [vp, u64, C.c_int]
    L.trhost_set_gbuffer.argtypes = [C.c_int]
    L.trhost_set_alpha_test.argtypes = [C.c_int]
    L.trhost_set_debug_view_mode.argtypes = [u32]
    L.trhost_download_gbuffer_a.argtypes = [vp, u64]
    L.trhost_set_deferred_lighting.argtypes = [C.c_int]
    L.trhost_set_directional_light.argtypes = [vp, C.c_float]
    L.trhost_upload_shadow_mask.argtypes = [vp, u64]
    L.trhost_download_lighting_output.argtypes = [vp, u64]
    L.trhost_get_deferred_lighting_consts.argtypes = [vp]
    L.trhost_upload_ddgi_volume.argtypes = [vp, vp, u64, vp, u64, vp, u64]
    L.trhost_set_ddgi.argtypes = [C.c_int]
    L.trhost_set_ddgi_update.argtypes = [C.c_int, C.c_uint32]
    L.trhost_set_ddgi_probe_placement.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float]
    L.trhost_reset_ddgi_volume.argtypes = []
    L.trhost_download_ddgi_volume.argtypes = [vp, u64, vp, u64, vp, u64]
    L.trhost_get_ddgi_update_consts.argtypes = [vp]
    L.trhost_set_ddgi_probe_variability.argtypes = [C.c_int, C.c_float]
    L.trhost_get_ddgi_variability.argtypes = [vp] * 5
    L.trhost_reset_ddgi_variability.argtypes = []
    L.trhost_ddgi_variability_run.argtypes = [vp, C.c_uint32, C.c_float, vp, vp]
    L.trhost_download_ddgi_variability.argtypes = [vp, u64]
    L.trhost_set_ddgi_probe_visualization.argtypes = [C.c_int, C.c_float, C.c_int]
    L.trhost_get_ddgi_probe_visualization_consts.argtypes = [vp]
    L.trhost_unit_sphere.argtypes = [vp, u64, vp, u64]
    L.trhost_set_post_process.argtypes = [C.c_int]
    L.trhost_set_exposure.argtypes = [C.c_float, C.c_float]
    L.trhost_set_auto_exposure.argtypes = [C.c_float, C.c_float, C.c_float]
    L.trhost_set_frame_time_ms.argtypes = [C.c_float]
    L.trhost_upload_bloom.argtypes = [vp, u64, C.c_float]
    L.trhost_download_back_buffer.argtypes = [vp, u64]
    L.trhost_set_bloom.argtypes = [C.c_int, u32, C.c_float, C.c_float]
    L.trhost_download_bloom.argtypes = [u32, vp, u64]
    L.trhost_get_bloom_consts.argtypes = [u32, vp]
    L.trhost_set_taa.argtypes = [C.c_int, C.c_float, C.c_float]
    L.trhost_reset_taa_history.argtypes = []
    L.trhost_download_anti_aliased_output.argtypes = [vp, u64]
    L.trhost_download_taa_history.argtypes = [vp, u64]
    L.trhost_get_taa_consts.argtypes = [vp, vp, vp]
    L.trhost_load_sky_dataset.argtypes = [vp, vp]
    L.trhost_set_sky.argtypes = [C.c_int, C.c_float, vp]
    L.trhost_get_sky_consts.argtypes = [vp]
    L.trhost_set_ambient_occlusion.argtypes = [C.c_int, u32, u32, C.c_float, C.c_float, C.c_float, C.c_float]
    L.trhost_download_ssao.argtypes = [vp, u64]
    L.trhost_get_gtao_consts.argtypes = [vp]
    L.trhost_load_raytracing.argtypes = [vp, u64, vp, u32]
    L.trhost_upload_blue_noise.argtypes = [vp, u64]
    L.trhost_set_shadow_mask.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float]
    L.trhost_download_shadow_mask.argtypes = [vp, u64]
    L.trhost_get_shadow_mask_consts.argtypes = [vp]
    L.trhost_set_shadow_denoising.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float]
    L.trhost_reset_shadow_history.argtypes = []
    L.trhost_download_shadow_penumbra.argtypes = [vp, u64]
    L.trhost_download_shadow_tiles.argtypes = [vp, u64]
    L.trhost_download_shadow_history.argtypes = [vp, u64]
    L.trhost_get_sigma_consts.argtypes = [vp]
    L.trhost_get_scene_luminance.argtypes = [vp, vp]
    L.trhost_reset_exposure.argtypes = []
    L.trhost_get_post_process_consts.argtypes = [vp, vp, vp, vp]
    L.trhost_upload_hzb_mip.argtypes = [u32, vp, u64]
    L.trhost_download_hzb_mip.argtypes = [u32, vp, u64]
    L.trhost_hzb_info.argtypes = [C.POINTER(u32)] * 3
    L.trhost_pass_buffers.argtypes = [u32, C.POINTER(PassBuffers)]
    L.trhost_instance_buffer.argtypes = [C.POINTER(vp)]
    L.trhost_device.restype = vp
    L.trhost_render_graph_stats.argtypes = [C.POINTER(u32), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)]
    L.trhost_renderer_times.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.trhost_set_gpu_timers.argtypes = [C.c_int]
    L.trhost_set_pipeline_statistics.argtypes = [C.c_int]
    L.trhost_pipeline_statistics.argtypes = [C.POINTER(PipelineStatistics), C.POINTER(PipelineStatistics)]
    L.trhost_exchange_create.argtypes = [C.POINTER(ExchangeDesc)]
    L.trhost_scene_list_sizes.argtypes = [C.POINTER(u32), C.POINTER(u32)]
    L.trhost_load_gi_probes.argtypes = [vp, vp, u32, C.c_float, C.c_int]
    L.trhost_set_renderer_queue.argtypes = [C.c_char_p, C.c_int]
    L.trhost_render_graph_frame_stats.argtypes = [C.POINTER(u32), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64)]
    L.trhost_gi_probe_buffers.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.trhost_exchange_outputs.argtypes = [u32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.trhost_set_shard_late_exchange.argtypes = [SHARD_LATE_FN, vp]
    L.trhost_heap_sim.argtypes = [u64, vp, u32, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)]
    L.trhost_set_texture_streaming.argtypes = [C.c_int, u32, u32, C.c_int]
    L.trhost_set_texture_streaming_region.argtypes = [u32, u32]
    L.trhost_get_texture_streaming_stats.argtypes = [vp]
    L.trhost_download_min_mip.argtypes = [u32, vp, u64, C.POINTER(u32), C.POINTER(u32)]
    L.trhost_residency_tiles.argtypes = [u32, u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
    L.trhost_residency_round.argtypes = [u32, u32, u32, u32, u32, u32, vp, u32, u32, vp, vp, vp, vp, vp, vp]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise HostError(load().trhost_last_error().decode(errors="replace"))


RESIDENCY_STATS = ("tilesTotal", "tilesResident", "tilesMapped", "tilesUnmapped", "bytesUploaded")


def residency_tiles(size, region):
    """(standard levels S, tiles over levels 0 .. S - 1) of a streamable texture: size = (width, height, mips), region = (w, h)."""
    s, n = C.c_uint32(), C.c_uint32()
    _check(load().trhost_residency_tiles(int(size[0]), int(size[1]), int(size[2]), int(region[0]), int(region[1]), C.byref(s), C.byref(n)))
    return int(s.value), int(n.value)


def residency_round(size, region, tile_bytes: int, feedback, evict_after: int, resident, idle):
    """One round of THE RESIDENCY RULE (csrc/host/TextureResidency.h; no GPU): feedback = the decoded bytes, uint8 [regions y, regions
    x]; resident (uint8) and idle (uint32) per tile.  Returns dict(resident, idle, mapped, unmapped (uint8 per tile), min_mip (uint8
    [regions y, regions x]), stats {RESIDENCY_STATS})."""
    _, n = residency_tiles(size, region)
    fb = np.ascontiguousarray(feedback, np.uint8)
    if fb.shape != (size[1] // region[1], size[0] // region[0]):
        raise ValueError(f"residency_round: the feedback is {fb.shape}, the texture has {(size[1] // region[1], size[0] // region[0])} regions")
    m = max(n, 1)
    res, idl = np.zeros(m, np.uint8), np.zeros(m, np.uint32)
    res[:n], idl[:n] = np.asarray(resident, np.uint8)[:n], np.asarray(idle, np.uint32)[:n]
    mapped, unmapped, min_mip, stats = np.zeros(m, np.uint8), np.zeros(m, np.uint8), np.zeros(fb.shape, np.uint8), np.zeros(5, np.uint64)
    _check(load().trhost_residency_round(int(size[0]), int(size[1]), int(size[2]), int(region[0]), int(region[1]), int(tile_bytes), fb.ctypes.data,
                                         int(evict_after), n, res.ctypes.data, idl.ctypes.data, mapped.ctypes.data, unmapped.ctypes.data,
                                         min_mip.ctypes.data, stats.ctypes.data))
    return dict(resident=res, idle=idl, mapped=mapped, unmapped=unmapped, min_mip=min_mip, stats={k: int(v) for k, v in zip(RESIDENCY_STATS, stats)})


def heap_sim(heap_size: int, ops):
    """RenderGraph::Heap allocator without a GPU (tests)."""
    ops = np.asarray(ops, np.int64)
    res = np.zeros(len(ops), np.uint64)
    used, peak, nb = C.c_uint64(), C.c_uint64(), C.c_uint32()
    _check(load().trhost_heap_sim(heap_size, ops.ctypes.data, len(ops), res.ctypes.data, C.byref(used), C.byref(peak), C.byref(nb)))
    return res, int(used.value), int(peak.value), int(nb.value)


def _download(handle, dtype, count):
    out = np.empty(count, dtype)
    if count:
        rc = rhi.load().trhip_buffer_download(C.c_void_p(handle), 0, out.ctypes.data, out.nbytes)
        if rc != 0:
            raise HostError(rhi.load().trhip_last_error().decode())
    return out


def unit_sphere():
    """(vertices UncompressedRawVertexFormat [91], indices uint32 [468]) of the host library's CommonResources::UnitSphere, the sphere
    GIDebugRenderer draws a probe as.  Needs no device."""
    v, ix = np.zeros(I.kUnitSphereVertices, I.UncompressedRawVertexFormat), np.zeros(I.kUnitSphereIndices, np.uint32)
    _check(load().trhost_unit_sphere(v.ctypes.data, v.nbytes, ix.ctypes.data, ix.nbytes))
    return v, ix


class Renderer:
    """One process-wide renderer context (Graphic / Scene are singletons in the reference)."""

    def __init__(self, render=(3840, 2160), device_index=0, stream: int | None = None, max_groups: int | None = None,
                 max_transient_bytes: int | None = None):
        L = load()
        _check(L.trhost_initialize(device_index, render[0], render[1], C.c_void_p(stream) if stream else None))
        self.render = render
        self.max_groups = 65535
        if max_groups or max_transient_bytes:
            _check(L.trhost_set_limits(max_groups or 0, max_transient_bytes or 0))
            if max_groups:
                self.max_groups = max_groups
        w, h, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(L.trhost_hzb_info(C.byref(w), C.byref(h), C.byref(m)))
        self.hzb_w, self.hzb_h, self.hzb_mips = w.value, h.value, m.value

    def load_scene(self, instances, meshData, meshlets, opaqueIds, alphaMaskIds, num_meshlets: int | None = None):
        """meshlets=None + num_meshlets: allocate only; stream the data in with upload_meshlets()."""
        a = [np.ascontiguousarray(x) for x in (instances, meshData)]
        ml = np.ascontiguousarray(meshlets) if meshlets is not None else None
        op = np.ascontiguousarray(opaqueIds, np.uint32)
        am = np.ascontiguousarray(alphaMaskIds, np.uint32)
        _check(load().trhost_load_scene(a[0].ctypes.data, len(a[0]), a[1].ctypes.data, len(a[1]),
                                        ml.ctypes.data if ml is not None else None, len(ml) if ml is not None else int(num_meshlets),
                                        op.ctypes.data if op.size else None, op.size, am.ctypes.data if am.size else None, am.size))
        self.num_opaque, self.num_alpha = op.size, am.size

    def load_scene_cached(self, cached_data_path: str, instances, opaqueIds, alphaMaskIds):
        """Meshes, meshlets and geometry from a `<scene>_CachedData.bin` v3 (read natively), instances / id lists from the caller."""
        a = np.ascontiguousarray(instances)
        op = np.ascontiguousarray(opaqueIds, np.uint32)
        am = np.ascontiguousarray(alphaMaskIds, np.uint32)
        _check(load().trhost_load_scene_cached(os.fsencode(cached_data_path), a.ctypes.data, len(a), op.ctypes.data if op.size else None, op.size,
                                               am.ctypes.data if am.size else None, am.size))
        self.num_opaque, self.num_alpha = op.size, am.size

    def upload_meshlets(self, first: int, meshlets):
        ml = np.ascontiguousarray(meshlets)
        _check(load().trhost_upload_meshlets(int(first), ml.ctypes.data, len(ml)))

    def load_nodes(self, nodes, prim_to_node):
        n = np.ascontiguousarray(nodes); p = np.ascontiguousarray(prim_to_node, np.uint32)
        _check(load().trhost_load_nodes(n.ctypes.data, len(n), p.ctypes.data))

    def set_node_transforms(self, nodes):
        n = np.ascontiguousarray(nodes)
        _check(load().trhost_set_node_transforms(n.ctypes.data, len(n)))

    def set_instance_update_range(self, first: int, count: int):
        """Multi-GPU: the per-frame transform update covers instances [first, first + count) only (this rank's shard)."""
        _check(load().trhost_set_instance_update_range(int(first), int(count)))

    def set_camera(self, view):
        w = np.ascontiguousarray(view.worldToView, np.float32); p = np.ascontiguousarray(view.prevWorldToView, np.float32)
        c = np.ascontiguousarray(view.viewToClip, np.float32)
        _check(load().trhost_set_camera(w.ctypes.data, p.ctypes.data, c.ctypes.data, float(view.nearPlane)))

    def set_culling(self, flags=7, freeze=False, force_mesh_lod=-1):
        _check(load().trhost_set_culling(flags & 1, (flags >> 1) & 1, (flags >> 2) & 1, int(freeze), int(force_mesh_lod)))
        self.flags = flags

    def upload_depth(self, depth):
        d = np.ascontiguousarray(depth, np.float32)
        _check(load().trhost_upload_depth(d.ctypes.data, d.shape[1], d.shape[0]))

    def load_geometry(self, vertices, meshlet_vertex_ids, meshlet_triangles):
        """The buffers the mesh shader reads (RawVertexFormat vertices, meshlet vertex ids, packed meshlet triangles)."""
        from . import interop as I
        v = np.ascontiguousarray(vertices, I.RawVertexFormat)
        vid, tri = np.ascontiguousarray(meshlet_vertex_ids, np.uint32), np.ascontiguousarray(meshlet_triangles, np.uint32)
        _check(load().trhost_load_geometry(v.ctypes.data, len(v), vid.ctypes.data, len(vid), tri.ctypes.data, len(tri)))

    def load_gi_probes(self, positions, states, radius: float, hide_inactive: bool = False):
        """GI debug view: probe world positions [n,3] and states [n] (1 = inactive); GIDebugRenderer culls them every frame."""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); st = np.ascontiguousarray(states, np.float32)
        assert len(p) == len(st)
        _check(load().trhost_load_gi_probes(p.ctypes.data if len(p) else None, st.ctypes.data if len(st) else None, len(p), float(radius), int(hide_inactive)))

    def gi_probe_results(self):
        """(positions[k,3], DrawIndexedIndirectArguments (5 words), instance -> probe index [k]) of the last frame."""
        self.wait_idle()
        h = [C.c_void_p() for _ in range(3)]
        _check(load().trhost_gi_probe_buffers(*[C.byref(x) for x in h]))
        args = _download(h[1].value, np.uint32, 5)
        k = int(args[1])
        return _download(h[0].value, np.float32, 3 * k).reshape(-1, 3), args, _download(h[2].value, np.uint32, k)

    def set_raster_depth(self, on: bool = True):
        """The frame rasterises the depth of its own visible meshlets instead of taking the uploaded depth image."""
        _check(load().trhost_set_raster_depth(int(on)))

    def set_visibility_buffer(self, on: bool = True):
        """Per-pixel visibility buffer + motion target (implies raster depth; include/trhost.h)."""
        _check(load().trhost_set_visibility_buffer(int(on)))

    def download_visibility(self) -> np.ndarray:
        """The last frame's visibility buffer: uint64 [H, W]."""
        self.wait_idle()
        v = np.empty((self.render[1], self.render[0]), np.uint64)
        _check(load().trhost_download_visibility(v.ctypes.data, v.nbytes))
        return v

    def download_motion(self) -> np.ndarray:
        """The last frame's motion target: float16 [H, W, 2] (pixels)."""
        self.wait_idle()
        m = np.empty((self.render[1], self.render[0], 2), np.float16)
        _check(load().trhost_download_motion(m.ctypes.data, m.nbytes))
        return m

    def create_material_texture(self, mips, fmt: int) -> int:
        """One material texture from its mips (uint8 [h_k, w_k, 4] arrays), fmt rhi.FORMAT_RGBA8_UNORM or FORMAT_SRGBA8_UNORM; returns
        the descriptor index a flagged TextureData.m_DescriptorIndex names (include/trhost.h).  For one of rhi.BC_FORMATS mips is an
        interop.BlockMips: the levels' raw block bytes, uploaded as they are (there is no encoder)."""
        if hasattr(mips, "width"):
            data = np.concatenate([np.frombuffer(bytes(m), np.uint8) if isinstance(m, (bytes, bytearray, memoryview)) else np.ascontiguousarray(m).reshape(-1).view(np.uint8)
                                   for m in mips])
            index = load().trhost_create_material_texture(mips.width, mips.height, len(mips), int(fmt), data.ctypes.data, data.nbytes)
            if index < 0:
                _check(-1)
            return index
        mips = [np.ascontiguousarray(m, np.uint8) for m in mips]
        if not mips or any(m.ndim != 3 or m.shape[2] != 4 for m in mips):
            raise ValueError("mips: a non-empty list of uint8 [h, w, 4] arrays")
        data = np.concatenate([m.reshape(-1) for m in mips])
        index = load().trhost_create_material_texture(mips[0].shape[1], mips[0].shape[0], len(mips), int(fmt), data.ctypes.data, data.nbytes)
        if index < 0:
            _check(-1)
        return index

    def create_material_texture_dds(self, data, srgb: bool) -> int:
        """One material texture from the bytes of a .dds file (trhost_create_material_texture_dds): srgb is the material slot's choice
        between a format and its _SRGB twin.  Returns the descriptor index."""
        buf = np.frombuffer(bytes(data), np.uint8)
        index = load().trhost_create_material_texture_dds(buf.ctypes.data if len(buf) else None, len(buf), int(bool(srgb)))
        if index < 0:
            _check(-1)
        return index

    def set_texture_streaming(self, enable=True, textures_per_frame=1, evict_after=4, poison=False, region=None):
        """trhost_set_texture_streaming (+ _region): before the first create_material_texture / load_textures.  region=(w, h) or None =
        the format's default tile shape; poison: the non-resident storage and unmapped tiles are filled with 0xFF00FFFF."""
        if region is not None:
            _check(load().trhost_set_texture_streaming_region(int(region[0]), int(region[1])))
        _check(load().trhost_set_texture_streaming(int(bool(enable)), int(textures_per_frame), int(evict_after), int(bool(poison))))

    @property
    def streaming_stats(self) -> dict:
        s = np.zeros(5, np.uint64)
        _check(load().trhost_get_texture_streaming_stats(s.ctypes.data))
        return dict(zip(("tilesTotal", "tilesResident", "tilesUploaded", "bytesUploaded", "texturesProcessed"), (int(x) for x in s)))

    def download_min_mip(self, texture: int) -> np.ndarray:
        """uint8 [regions y, regions x]: the min-mip map of a streamed texture on the device."""
        self.wait_idle()
        rx, ry = C.c_uint32(), C.c_uint32()
        _check(load().trhost_download_min_mip(int(texture), None, 0, C.byref(rx), C.byref(ry)))
        out = np.empty((ry.value, rx.value), np.uint8)
        _check(load().trhost_download_min_mip(int(texture), out.ctypes.data, out.nbytes, None, None))
        return out

    def load_textures(self, textures):
        """[(mips, format)] -> descriptor indices, as GpuScene.set_textures; before load_materials."""
        return [self.create_material_texture(m, f) for m, f in textures]

    def load_materials(self, materials):
        """MaterialData[] for the G-buffer resolve; a textured material names textures created before (include/trhost.h)."""
        m = np.ascontiguousarray(materials, I.MaterialData)
        _check(load().trhost_load_materials(m.ctypes.data, len(m)))

    def set_gbuffer(self, on: bool = True):
        """GBufferA + motion through one "basepass_PS_Main_GBuffer" dispatch (implies the visibility buffer)."""
        _check(load().trhost_set_gbuffer(int(on)))

    def set_alpha_test(self, on: bool = True):
        """ALPHA_MASK_MODE's discard in the alpha-mask pass slots' rasters and textured alpha in the sun rays (needs the rasters and
        load_materials); off by default: alpha-mask instances are drawn as solid triangles."""
        _check(load().trhost_set_alpha_test(int(on)))

    def set_debug_view_mode(self, mode: int):
        _check(load().trhost_set_debug_view_mode(int(mode)))

    def download_gbuffer_a(self) -> np.ndarray:
        """The last frame's GBufferA: uint32 [H, W, 4]."""
        self.wait_idle()
        g = np.empty((self.render[1], self.render[0], 4), np.uint32)
        _check(load().trhost_download_gbuffer_a(g.ctypes.data, g.nbytes))
        return g

    def set_deferred_lighting(self, on: bool = True):
        """DeferredLightingRenderer after GBufferRenderer (implies the G-buffer; include/trhost.h)."""
        _check(load().trhost_set_deferred_lighting(int(on)))

    def set_directional_light(self, vec, strength: float):
        v = np.ascontiguousarray(vec, np.float32).reshape(3)
        _check(load().trhost_set_directional_light(v.ctypes.data, float(strength)))

    def upload_shadow_mask(self, mask):
        """uint8 [H, W] R8_UNORM shadow mask at render resolution; None = white."""
        if mask is None:
            _check(load().trhost_upload_shadow_mask(None, 0))
            return
        m = np.ascontiguousarray(mask, np.uint8)
        _check(load().trhost_upload_shadow_mask(m.ctypes.data, m.nbytes))

    def download_lighting_output(self) -> np.ndarray:
        """The last frame's LightingOutput: uint32 [H, W] R11G11B10_FLOAT words."""
        self.wait_idle()
        w = np.empty((self.render[1], self.render[0]), np.uint32)
        _check(load().trhost_download_lighting_output(w.ctypes.data, w.nbytes))
        return w

    def deferred_lighting_consts(self) -> np.ndarray:
        """The DeferredLightingConsts (1 element) the last frame uploaded."""
        k = np.zeros(1, I.DeferredLightingConsts)
        _check(load().trhost_get_deferred_lighting_consts(k.ctypes.data))
        return k

    def upload_ddgi_volume(self, volume):
        """A ddgi.Volume (descriptor and the three probe textures) as the lighting pass's t5..t8; None drops it (include/trhost.h)."""
        if volume is None:
            _check(load().trhost_upload_ddgi_volume(None, None, 0, None, 0, None, 0))
            return
        d = np.ascontiguousarray(volume.desc())
        irr, dist, data = (np.ascontiguousarray(a) for a in (volume.irradiance, volume.distance, volume.data))
        _check(load().trhost_upload_ddgi_volume(d.ctypes.data, irr.ctypes.data, irr.nbytes, dist.ctypes.data, dist.nbytes, data.ctypes.data, data.nbytes))

    def set_ddgi(self, on: bool = True):
        """Scene::IsDDGIEnabled(): the ambient term from the uploaded volume (needs upload_ddgi_volume)."""
        _check(load().trhost_set_ddgi(int(on)))

    def set_ddgi_update(self, on: bool = True, seed: int = 0):
        """GIRenderer::RenderDDGI: the probe trace and the two blends fill the uploaded volume every frame (needs upload_ddgi_volume,
        load_raytracing and deferred lighting; include/trhost.h)."""
        _check(load().trhost_set_ddgi_update(int(on), int(seed)))

    def set_ddgi_probe_placement(self, relocate: bool = True, classify: bool = True, min_frontface_distance: float = 0.3, fixed_ray_backface_threshold: float = 0.25):
        """Probe relocation and classification behind the blends of every update (needs the volume and, per pass, its flag in the
        volume's descriptor; include/trhost.h)."""
        _check(load().trhost_set_ddgi_probe_placement(int(relocate), int(classify), float(min_frontface_distance), float(fixed_ray_backface_threshold)))

    def reset_ddgi_volume(self):
        """Irradiance and distance cleared to zero words, the reference's start."""
        _check(load().trhost_reset_ddgi_volume())

    def download_ddgi_volume(self, volume):
        """A copy of `volume` (the ddgi.Volume that was uploaded: its descriptor gives the shapes) with the three textures as the
        device holds them now."""
        v = volume.copy()
        _check(load().trhost_download_ddgi_volume(v.irradiance.ctypes.data, v.irradiance.nbytes, v.distance.ctypes.data, v.distance.nbytes, v.data.ctypes.data, v.data.nbytes))
        return v

    def set_ddgi_probe_variability(self, enable: bool = True, stddev_threshold: float = 0.001):
        """The reference's probe variability: the update stops recording once the volume's average variability has settled
        (needs set_ddgi_update; include/trhost.h)."""
        _check(load().trhost_set_ddgi_probe_variability(int(enable), float(stddev_threshold)))

    def ddgi_variability(self) -> dict:
        """average (the last one read back), stddev (of the ring), converged, samples, skipped (updates that recorded nothing)."""
        a, s, c, n, k = C.c_float(), C.c_float(), C.c_int(), C.c_uint32(), C.c_uint32()
        _check(load().trhost_get_ddgi_variability(C.byref(a), C.byref(s), C.byref(c), C.byref(n), C.byref(k)))
        return dict(average=np.float32(a.value), stddev=np.float32(s.value), converged=bool(c.value), samples=int(n.value), skipped=int(k.value))

    def reset_ddgi_variability(self):
        """Re-arms a converged volume: the whole tracker and the variability buffer start again."""
        _check(load().trhost_reset_ddgi_variability())

    def download_ddgi_variability(self, volume) -> np.ndarray:
        """The variability buffer, float32 [counts.y, 6 counts.z, 6 counts.x] of `volume` (the ddgi.Volume that was uploaded)."""
        cx, cy, cz = volume.counts
        out = np.zeros((cy, 6 * cz, 6 * cx), np.float32)
        _check(load().trhost_download_ddgi_variability(out.ctypes.data, out.nbytes))
        return out

    def ddgi_update_consts(self) -> np.ndarray:
        """The DDGIUpdateConsts of the last frame's probe update, the ray rotation among them; raises if none ran in it."""
        k = np.zeros(1, I.DDGIUpdateConsts)
        _check(load().trhost_get_ddgi_update_consts(k.ctypes.data))
        return k

    def set_ddgi_probe_visualization(self, enable: bool = True, probe_radius: float = 0.1, hide_inactive: bool = False):
        """GIDebugRenderer on the live volume: LoadGIProbes, the cull, and the draw of the surviving probes as spheres into the back
        buffer behind the post pass (needs the volume and set_post_process: the next frame() raises and says which is missing;
        include/trhost.h).  gi_probe_results() reads the cull's outputs."""
        _check(load().trhost_set_ddgi_probe_visualization(int(enable), float(probe_radius), int(hide_inactive)))

    def ddgi_probe_visualization_consts(self) -> np.ndarray:
        """The GIProbeVisualizationConsts of the last frame's probe draw; raises if it drew none."""
        k = np.zeros(1, I.GIProbeVisualizationConsts)
        _check(load().trhost_get_ddgi_probe_visualization_consts(k.ctypes.data))
        return k

    def set_post_process(self, on: bool = True):
        """AdaptLuminanceRenderer and PostProcessRenderer after DeferredLightingRenderer (implies deferred lighting; include/trhost.h)."""
        _check(load().trhost_set_post_process(int(on)))

    def set_exposure(self, manual: float = 0.0, middle_gray: float = 0.18):
        _check(load().trhost_set_exposure(float(manual), float(middle_gray)))

    def set_auto_exposure(self, min_luminance: float = 0.004, max_luminance: float = 12.0, speed_per_ms: float = 0.0025):
        _check(load().trhost_set_auto_exposure(float(min_luminance), float(max_luminance), float(speed_per_ms)))

    def set_frame_time_ms(self, ms: float):
        _check(load().trhost_set_frame_time_ms(float(ms)))

    def upload_bloom(self, words, strength: float = 0.0):
        """uint32 [H, W] R11G11B10_FLOAT bloom texture at render resolution and its strength; None switches bloom off."""
        if words is None:
            _check(load().trhost_upload_bloom(None, 0, float(strength)))
            return
        w = np.ascontiguousarray(words, np.uint32)
        _check(load().trhost_upload_bloom(w.ctypes.data, w.nbytes, float(strength)))

    def set_bloom(self, enable: bool, mips: int = 6, filter_radius: float = 0.005, strength: float = 0.1):
        """BloomRenderer on or off (needs set_post_process(True); excludes an uploaded bloom texture)."""
        _check(load().trhost_set_bloom(int(bool(enable)), int(mips), float(filter_radius), float(strength)))

    def download_bloom(self, mip: int = 0) -> np.ndarray:
        """One mip of the generated bloom texture: uint32 [H >> mip, W >> mip] R11G11B10_FLOAT words."""
        self.wait_idle()
        w = np.empty((self.render[1] >> mip, self.render[0] >> mip), np.uint32)
        _check(load().trhost_download_bloom(int(mip), w.ctypes.data, w.nbytes))
        return w

    def set_taa(self, enable: bool, min_blend: float = 0.1, max_sample_count: float = 64.0):
        """TAARenderer and the jittered projection on or off (needs set_post_process(True))."""
        _check(load().trhost_set_taa(int(bool(enable)), float(min_blend), float(max_sample_count)))

    def reset_taa_history(self):
        """The next frame's resolve starts every texel again from its current colour."""
        _check(load().trhost_reset_taa_history())

    def download_anti_aliased_output(self) -> np.ndarray:
        """The last frame's AntiAliasedLightingOutput: uint32 [H, W] R11G11B10_FLOAT words."""
        self.wait_idle()
        w = np.empty((self.render[1], self.render[0]), np.uint32)
        _check(load().trhost_download_anti_aliased_output(w.ctypes.data, w.nbytes))
        return w

    def download_taa_history(self) -> np.ndarray:
        """The history texture the last frame wrote: float16 [H, W, 4], xyz the colour, w the accumulated sample count."""
        self.wait_idle()
        h = np.empty((self.render[1], self.render[0], 4), np.float16)
        _check(load().trhost_download_taa_history(h.ctypes.data, h.nbytes))
        return h

    def taa_consts(self):
        """(TAAConsts of the last frame, its current jitter offset, its previous one), the offsets float32 [2] in pixels."""
        k, current, previous = np.zeros(1, I.TAAConsts), np.zeros(2, np.float32), np.zeros(2, np.float32)
        _check(load().trhost_get_taa_consts(k.ctypes.data, current.ctypes.data, previous.ctypes.data))
        return k, current, previous

    def load_sky_dataset(self, dataset):
        """A sky.HosekDataset (the Hosek-Wilkie RGB tables, an input of the integrator); None unloads it and switches the pass off."""
        if dataset is None:
            _check(load().trhost_load_sky_dataset(None, None))
            return
        rgb, rad = np.ascontiguousarray(dataset.rgb, np.float64), np.ascontiguousarray(dataset.rad, np.float64)
        assert rgb.shape == (3, 1080) and rad.shape == (3, 120)
        _check(load().trhost_load_sky_dataset(rgb.ctypes.data, rad.ctypes.data))

    def set_sky(self, enable: bool, turbidity: float = 2.0, ground_albedo=(0.1, 0.1, 0.1)):
        """SkyRenderer on or off (needs load_sky_dataset() and set_deferred_lighting(True))."""
        a = np.ascontiguousarray(ground_albedo, np.float32).reshape(3)
        _check(load().trhost_set_sky(int(bool(enable)), float(turbidity), a.ctypes.data))

    def sky_consts(self) -> np.ndarray:
        """The SkyPassParameters of the last frame; raises if the pass did not run in it."""
        k = np.zeros(1, I.SkyPassParameters)
        _check(load().trhost_get_sky_consts(k.ctypes.data))
        return k

    def set_ambient_occlusion(self, enable: bool, quality: int = 3, denoise_passes: int = 3, radius: float = 0.5, falloff_range: float = 0.615,
                              final_value_power: float = 2.2, depth_mip_sampling_offset: float = 3.3):
        """AmbientOcclusionRenderer on or off (needs set_gbuffer(True) or set_deferred_lighting(True)); the defaults are the reference's."""
        _check(load().trhost_set_ambient_occlusion(int(bool(enable)), int(quality), int(denoise_passes), float(radius), float(falloff_range),
                                                   float(final_value_power), float(depth_mip_sampling_offset)))

    def download_ssao(self) -> np.ndarray:
        """The last frame's SSAO texture: uint8 [H, W]; raises if the pass did not run in it."""
        self.wait_idle()
        b = np.empty((self.render[1], self.render[0]), np.uint8)
        _check(load().trhost_download_ssao(b.ctypes.data, b.nbytes))
        return b

    def gtao_consts(self) -> np.ndarray:
        """The GTAOConstants of the last frame; raises if the pass did not run in it."""
        k = np.zeros(1, I.GTAOConstants)
        _check(load().trhost_get_gtao_consts(k.ctypes.data))
        return k

    def load_raytracing(self, indices, mesh_specific):
        """The acceleration structure of the ray-traced shadows: the global index buffer and the MeshSpecificData table (or one
        index count per mesh).  After load_scene, load_geometry and load_materials."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        counts = np.asarray(mesh_specific)
        counts = np.ascontiguousarray(counts["m_NumIndices"] if counts.dtype.names else counts, np.uint32)
        _check(load().trhost_load_raytracing(idx.ctypes.data, len(idx), counts.ctypes.data, len(counts)))

    def upload_blue_noise(self, noise):
        n = np.ascontiguousarray(noise, np.uint8)
        _check(load().trhost_upload_blue_noise(n.ctypes.data, n.nbytes))

    def set_shadow_mask(self, enable: bool, soft: bool = True, sun_angular_diameter: float = 0.533, ray_start_offset: float = 0.1):
        """ShadowMaskRenderer on or off (needs the G-buffer, load_raytracing and upload_blue_noise; not with an uploaded shadow mask)."""
        _check(load().trhost_set_shadow_mask(int(bool(enable)), int(bool(soft)), float(sun_angular_diameter), float(ray_start_offset)))

    def download_shadow_mask(self) -> np.ndarray:
        """The last frame's shadow mask: uint8 [H, W]; raises if the pass did not run in it."""
        self.wait_idle()
        b = np.empty((self.render[1], self.render[0]), np.uint8)
        _check(load().trhost_download_shadow_mask(b.ctypes.data, b.nbytes))
        return b

    def shadow_mask_consts(self) -> np.ndarray:
        """The ShadowMaskConsts of the last frame; raises if the pass did not run in it."""
        k = np.zeros(1, I.ShadowMaskConsts)
        _check(load().trhost_get_shadow_mask_consts(k.ctypes.data))
        return k


    def set_shadow_denoising(self, enable: bool, plane_distance_sensitivity: float = 0.02, stabilization_strength: float = 5.0 / 6.0, sigma_scale: float = 2.0):
        """ShadowMaskRenderer's DenoiseShadows on or off (needs set_shadow_mask(True)): the pack pass and the four dispatches of
        csrc/k_sigma.hip behind the trace."""
        _check(load().trhost_set_shadow_denoising(int(bool(enable)), float(plane_distance_sensitivity), float(stabilization_strength), float(sigma_scale)))

    def reset_shadow_history(self):
        """The next frame's stabilisation reads no history."""
        _check(load().trhost_reset_shadow_history())

    def _download_denoiser(self, fn, shape, dtype) -> np.ndarray:
        self.wait_idle()
        out = np.empty(shape, dtype)
        _check(fn(out.ctypes.data, out.nbytes))
        return out

    def download_shadow_penumbra(self) -> np.ndarray:
        """The last frame's penumbra texture: binary16 words uint16 [H, W]; raises if the denoiser did not run in it."""
        return self._download_denoiser(load().trhost_download_shadow_penumbra, (self.render[1], self.render[0]), np.uint16)

    def download_shadow_tiles(self) -> np.ndarray:
        """The last frame's tile bytes: uint8 [ceil(H / 16), ceil(W / 16)]."""
        return self._download_denoiser(load().trhost_download_shadow_tiles, ((self.render[1] + 15) // 16, (self.render[0] + 15) // 16), np.uint8)

    def download_shadow_history(self) -> np.ndarray:
        """The shadow history the last frame wrote: binary16 words uint16 [H, W]."""
        return self._download_denoiser(load().trhost_download_shadow_history, (self.render[1], self.render[0]), np.uint16)

    def sigma_consts(self) -> np.ndarray:
        """The SigmaConsts (m_Pass 0) of the last frame; raises if the denoiser did not run in it."""
        k = np.zeros(1, I.SigmaConsts)
        _check(load().trhost_get_sigma_consts(k.ctypes.data))
        return k

    def bloom_consts(self, passes: int) -> np.ndarray:
        """The BloomConsts of the first `passes` bloom dispatches of the last frame, downsamples first."""
        k = np.zeros(passes, I.BloomConsts)
        for i in range(passes):
            _check(load().trhost_get_bloom_consts(i, k[i:i + 1].ctypes.data))
        return k

    def download_back_buffer(self) -> np.ndarray:
        """The last frame's back buffer: uint32 [H, W] RGBA8_UNORM words, R in the low byte."""
        self.wait_idle()
        w = np.empty((self.render[1], self.render[0]), np.uint32)
        _check(load().trhost_download_back_buffer(w.ctypes.data, w.nbytes))
        return w

    def scene_luminance(self):
        """(adapted luminance, exposure) as they are now, float32 scalars."""
        lum, exp = np.zeros(1, np.float32), np.zeros(1, np.float32)
        _check(load().trhost_get_scene_luminance(lum.ctypes.data, exp.ctypes.data))
        return lum[0], exp[0]

    def reset_exposure(self):
        _check(load().trhost_reset_exposure())

    def post_process_consts(self):
        """(GenerateLuminanceHistogramParameters, AdaptExposureParameters, PostProcessParameters) of the last frame, 1 element
        each; the first two are None when the last frame had a manual exposure."""
        hk, ak, pk = np.zeros(1, I.GenerateLuminanceHistogramParameters), np.zeros(1, I.AdaptExposureParameters), np.zeros(1, I.PostProcessParameters)
        ran = C.c_int(0)
        _check(load().trhost_get_post_process_consts(hk.ctypes.data, ak.ctypes.data, pk.ctypes.data, C.addressof(ran)))
        return (hk, ak, pk) if ran.value else (None, None, pk)

    def download_depth(self) -> np.ndarray:
        self.wait_idle()
        d = np.empty((self.render[1], self.render[0]), np.float32)
        _check(load().trhost_download_depth(d.ctypes.data, d.nbytes))
        return d

    def upload_hzb(self, texels, offsets):
        for k in range(self.hzb_mips):
            mw, mh = max(self.hzb_w >> k, 1), max(self.hzb_h >> k, 1)
            t = np.ascontiguousarray(texels[offsets[k]:offsets[k] + mw * mh], np.uint16)
            _check(load().trhost_upload_hzb_mip(k, t.ctypes.data, t.nbytes))

    def download_hzb(self) -> np.ndarray:
        parts = []
        for k in range(self.hzb_mips):
            t = np.empty(max(self.hzb_w >> k, 1) * max(self.hzb_h >> k, 1), np.uint16)
            _check(load().trhost_download_hzb_mip(k, t.ctypes.data, t.nbytes))
            parts.append(t)
        return np.concatenate(parts)

    def frame(self):
        _check(load().trhost_frame())

    def wait_idle(self):
        _check(load().trhost_wait_idle())

    def set_pipeline_statistics(self, enable: bool = True):
        """The base pass brackets every frame with a pipeline statistics query (include/trhost.h); off by default."""
        _check(load().trhost_set_pipeline_statistics(int(bool(enable))))

    def pipeline_statistics(self):
        """(last_shown, latest) as {field: int} dicts: the value the last frame showed (its query of two frames earlier)
        and the last executed frame's own query (waits for it)."""
        a, b = PipelineStatistics(), PipelineStatistics()
        _check(load().trhost_pipeline_statistics(C.byref(a), C.byref(b)))
        return a.as_dict(), b.as_dict()

    def set_gpu_timers(self, enable: bool):
        _check(load().trhost_set_gpu_timers(int(bool(enable))))

    def set_shard_late_exchange(self, fn):
        """Multi-GPU hook (include/trhost.h): fn(hip_stream, late_count_ptr, shard_info_ptr, bucket, phase) runs inside
        frame(): phase 0 after each early instance cull, phase 1 before each late one; None removes it."""
        if fn is None:
            self._shard_late_cb = C.cast(None, SHARD_LATE_FN)
        else:
            self._shard_late_cb = SHARD_LATE_FN(lambda _u, s, c, i, b, ph: fn(int(s or 0), int(c), int(i), int(b), int(ph)))
        _check(load().trhost_set_shard_late_exchange(self._shard_late_cb, None))

    def pass_buffers(self, slot: int) -> PassBuffers:
        pb = PassBuffers()
        _check(load().trhost_pass_buffers(slot, C.byref(pb)))
        return pb

    def results(self):
        """Read back every pass slot of the last frame (tests)."""
        self.wait_idle()
        out = {}
        late = None
        for s in range(4):
            pb = self.pass_buffers(s)
            if not pb.ran:
                out[s] = None
                continue
            args = _download(pb.dispatch_args, np.uint32, 4)
            G = int(min(args[0], args[3], self.max_groups))
            draw = _download(pb.draw_args, np.uint32, 3)
            V = int(min(draw[0], self.max_groups * 32))
            out[s] = dict(dispatchArgs=args[:3].copy(), validRecords=int(args[3]),
                          records=_download(pb.records, I.MeshletAmplificationData, G),
                          visMask=_download(pb.vis_mask, np.uint32, G),
                          visibleList=_download(pb.visible_list, np.uint32, V), drawArgs=draw)
            late = pb
        if late is not None and (self.flags & 2):
            out["lateCount"] = int(_download(late.late_count, np.uint32, 1)[0])
            out["lateArgs"] = _download(late.late_args, np.uint32, 3)
        return out

    def instances(self, count) -> np.ndarray:
        h = C.c_void_p()
        _check(load().trhost_instance_buffer(C.byref(h)))
        self.wait_idle()
        return _download(h.value, I.BasePassInstanceConstants, count)

    def render_graph_stats(self):
        nh, res, used, npass = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        _check(load().trhost_render_graph_stats(C.byref(nh), C.byref(res), C.byref(used), C.byref(npass)))
        return dict(heaps=nh.value, reserved=res.value, used=used.value, passes=npass.value)

    def set_renderer_queue(self, name: str, compute: bool):
        """Async compute: the renderer records for the compute queue (a second stream) instead of the graphics queue."""
        _check(load().trhost_set_renderer_queue(name.encode(), int(bool(compute))))

    def render_graph_frame_stats(self):
        a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(load().trhost_render_graph_frame_stats(C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(compute_queue_passes=a.value, cross_queue_waits=b.value, transient_bytes=c.value, aliased_bytes=d.value)

    def renderer_times(self, name: str):
        c, g = C.c_float(), C.c_float()
        _check(load().trhost_renderer_times(name.encode(), C.byref(c), C.byref(g)))
        return float(c.value), float(g.value)

    def device(self) -> int:
        return load().trhost_device()

    def shutdown(self):
        load().trhost_shutdown()


def ddgi_variability_run(averages, threshold: float = 0.001):
    """csrc/host/DDGIVariability.h's rule over a sequence of averages, no device: (converged bool [n], stddev float32 [n]) after
    each Update (trhost_ddgi_variability_run, include/trhost.h)."""
    a = np.ascontiguousarray(averages, np.float32)
    conv, dev = np.zeros(len(a), np.uint8), np.zeros(len(a), np.float32)
    _check(load().trhost_ddgi_variability_run(a.ctypes.data, len(a), float(threshold), conv.ctypes.data, dev.ctypes.data))
    return conv.astype(bool), dev
