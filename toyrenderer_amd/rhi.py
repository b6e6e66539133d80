"""ctypes binding of the C-ABI compute back end (include/trhip.h -> lib/libtrhip.so).

Thin and literal: one Python method per C entry point, numpy arrays in and out.  There is NO CPU
fallback: if the HIP library is missing or no GPU is visible this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TRHIP_LIB") or os.path.join(_HERE, "lib", "libtrhip.so")   # TRHIP_LIB: experiment builds only

FORMAT_R16_FLOAT = 1
FORMAT_R32_FLOAT = 2
FORMAT_RG32_UINT = 3      # visibility buffer: one u64 per texel
FORMAT_RG16_FLOAT = 4     # motion target: two fp16 per texel
FORMAT_RGBA32_UINT = 5    # GBufferA: four u32 per texel (x, y, z, w)
FORMAT_R11G11B10_FLOAT = 6  # LightingOutput: one u32 per texel, R bits 0-10, G 11-21, B 22-31
FORMAT_R8_UNORM = 7       # shadow mask: one byte per texel
FORMAT_R8_UINT = 8        # SSAO texture: one byte per texel
SAMPLER_FEEDBACK_FORMAT = 9  # a feedback map: one u32 per region; made by Device.create_sampler_feedback only (create_texture refuses it)
FORMAT_RGBA8_UNORM = 10   # back buffer: one u32 per texel, R in the low byte
FORMAT_SRGBA8_UNORM = 11  # RGBA8_UNORM's layout; R, G, B decoded through the sRGB transfer function when sampled
FORMAT_R10G10B10A2_UNORM = 12  # DDGI probe irradiance: one u32 per texel, R bits 0-9, G 10-19, B 20-29, A 30-31
FORMAT_RGBA16_FLOAT = 13  # DDGI probe data: four fp16 per texel
# Block-compressed material textures (include/trhip.h): 4 x 4 texel blocks of 8 (BC1, BC4) or 16 bytes, sampled through the texture
# table only, decoded one texel per fetch.  There is no encoder: the blocks come from files (interop.parse_dds) or other tools.
FORMAT_BC1_UNORM = 14
FORMAT_BC1_UNORM_SRGB = 15
FORMAT_BC2_UNORM = 16
FORMAT_BC2_UNORM_SRGB = 17
FORMAT_BC3_UNORM = 18
FORMAT_BC3_UNORM_SRGB = 19
FORMAT_BC4_UNORM = 20     # decodes to (R, 0, 0, 255)
FORMAT_BC5_UNORM = 21     # decodes to (R, G, 0, 255)
BC_FORMATS = tuple(range(FORMAT_BC1_UNORM, FORMAT_BC5_UNORM + 1))

TEXTURE_RENDER_TARGET = 2   # or'ed into trhip_texture_desc.isUAV

BIND_CONSTANT_BUFFER, BIND_PUSH_CONSTANTS, BIND_STRUCTURED_SRV, BIND_STRUCTURED_UAV, BIND_TEXTURE_SRV, BIND_TEXTURE_UAV, BIND_SAMPLER, BIND_TEXTURE_TABLE = range(8)
TEXTURE_TABLE_SLOT = 19   # t19 of "basepass_PS_Main_GBuffer": the first slot after the visibility buffer's t18

# every symbol include/trhip.h declares (checked by tests/test_abi_symbols.py)
ABI_SYMBOLS = [
    "trhip_last_error", "trhip_abi_version", "trhip_shader_count", "trhip_shader_name", "trhip_shader_exists",
    "trhip_device_create", "trhip_device_create_on_stream", "trhip_device_destroy", "trhip_device_wait_idle",
    "trhip_device_info", "trhip_device_stream", "trhip_device_join_side_stream",
    "trhip_heap_create", "trhip_heap_release",
    "trhip_buffer_create", "trhip_buffer_wrap", "trhip_buffer_memory_requirements", "trhip_buffer_bind_memory",
    "trhip_buffer_retain", "trhip_buffer_release", "trhip_buffer_device_ptr", "trhip_buffer_size",
    "trhip_texture_create", "trhip_texture_memory_requirements", "trhip_texture_bind_memory", "trhip_texture_retain",
    "trhip_texture_release", "trhip_texture_device_ptr", "trhip_texture_mip_info", "trhip_texture_size",
    "trhip_buffer_upload", "trhip_buffer_download", "trhip_texture_upload", "trhip_texture_download",
    "trhip_texture_create_array", "trhip_texture_array_size", "trhip_texture_slice_pitch", "trhip_texture_upload_slice", "trhip_texture_download_slice",
    "trhip_buffer_mark_written", "trhip_texture_mark_written",
    "trhip_texture_table_create", "trhip_texture_table_retain", "trhip_texture_table_release", "trhip_texture_table_capacity",
    "trhip_texture_table_set", "trhip_texture_table_clear", "trhip_srgb_table", "trhip_format_block_bytes", "trhip_dds_parse",
    "trhip_texture_set_streaming_region", "trhip_texture_streaming_region", "trhip_sampler_feedback_create",
    "trhip_cmd_clear_sampler_feedback", "trhip_cmd_decode_sampler_feedback", "trhip_cmd_write_texture_region",
    "trhip_cmd_create", "trhip_cmd_release", "trhip_cmd_open", "trhip_cmd_close", "trhip_cmd_write_buffer",
    "trhip_cmd_clear_buffer_u32", "trhip_cmd_clear_texture_f32", "trhip_cmd_clear_texture_u32", "trhip_cmd_copy_buffer", "trhip_cmd_copy_texture", "trhip_cmd_host_callback", "trhip_cmd_dispatch", "trhip_cmd_dispatch_indirect",
    "trhip_cmd_begin_timer", "trhip_cmd_end_timer", "trhip_cmd_begin_marker", "trhip_cmd_end_marker",
    "trhip_queue_execute",
    "trhip_timer_create", "trhip_timer_release", "trhip_timer_get_ms",
    "trhip_pipeline_stats_create", "trhip_pipeline_stats_release", "trhip_cmd_begin_pipeline_stats",
    "trhip_cmd_end_pipeline_stats", "trhip_pipeline_stats_get",
    "trhip_readback_create", "trhip_readback_release", "trhip_readback_reset", "trhip_cmd_copy_to_readback", "trhip_readback_read", "trhip_readback_poll",
    "trhip_profile_enable", "trhip_profile_filter", "trhip_profile_reset", "trhip_profile_count", "trhip_profile_entry",
    "trhip_launch_shard_late_info",
    "trhip_accel_max_depth", "trhip_blas_leaf_capacity", "trhip_accel_max_nodes", "trhip_blas_build", "trhip_tlas_build",
    "trhip_stream_create", "trhip_stream_create_priority", "trhip_stream_destroy", "trhip_stream_synchronize", "trhip_event_create", "trhip_event_destroy",
    "trhip_event_record", "trhip_stream_wait_event",
]

HOST_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)       # trhip_host_fn(user, hip_stream)


class BufferDesc(C.Structure):
    _fields_ = [("byteSize", C.c_uint64), ("structStride", C.c_uint32), ("canHaveUAVs", C.c_uint32),
                ("isDrawIndirectArgs", C.c_uint32), ("isVirtual", C.c_uint32), ("isVolatileConstant", C.c_uint32),
                ("debugName", C.c_char_p)]


class TextureDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("mipLevels", C.c_uint32), ("format", C.c_uint32),
                ("isUAV", C.c_uint32), ("isVirtual", C.c_uint32), ("debugName", C.c_char_p)]


class DdsInfo(C.Structure):
    """trhip_dds_info (include/trhip.h)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("mipLevels", C.c_uint32), ("format", C.c_uint32),
                ("levelOffset", C.c_uint64 * 16), ("levelBytes", C.c_uint64 * 16)]


class Binding(C.Structure):
    _fields_ = [("type", C.c_uint32), ("slot", C.c_uint32), ("resource", C.c_void_p), ("baseMip", C.c_uint32),
                ("reserved", C.c_uint32)]


# trhip_pipeline_statistics: D3D12_QUERY_DATA_PIPELINE_STATISTICS1's fields, in its order (include/trhip.h)
PIPELINE_STATISTICS_FIELDS = ("IAVertices", "IAPrimitives", "VSInvocations", "GSInvocations", "GSPrimitives", "CInvocations",
                              "CPrimitives", "PSInvocations", "HSInvocations", "DSInvocations", "CSInvocations", "ASInvocations",
                              "MSInvocations", "MSPrimitives")


class PipelineStatistics(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in PIPELINE_STATISTICS_FIELDS]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f in PIPELINE_STATISTICS_FIELDS}


class TrhipError(RuntimeError):
    pass


_lib = None


def load() -> C.CDLL:
    """Load lib/libtrhip.so; raises (never falls back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TrhipError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(there is no CPU fallback for the HIP back end)")
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.trhip_last_error.restype = C.c_char_p
    L.trhip_abi_version.restype = u32
    L.trhip_shader_count.restype = u32
    L.trhip_shader_name.restype = C.c_char_p
    L.trhip_shader_name.argtypes = [u32]
    L.trhip_shader_exists.argtypes = [C.c_char_p]
    L.trhip_device_create.argtypes = [i32, C.POINTER(vp)]
    L.trhip_device_create_on_stream.argtypes = [i32, vp, C.POINTER(vp)]
    L.trhip_device_destroy.argtypes = [vp]
    L.trhip_device_destroy.restype = None
    L.trhip_device_wait_idle.argtypes = [vp]
    L.trhip_device_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64)]
    L.trhip_device_stream.argtypes = [vp]
    L.trhip_device_stream.restype = vp
    L.trhip_heap_create.argtypes = [vp, u64, C.POINTER(vp)]
    L.trhip_heap_release.argtypes = [vp]
    L.trhip_heap_release.restype = None
    L.trhip_buffer_create.argtypes = [vp, C.POINTER(BufferDesc), C.POINTER(vp)]
    L.trhip_buffer_wrap.argtypes = [vp, vp, C.POINTER(BufferDesc), C.POINTER(vp)]
    L.trhip_buffer_memory_requirements.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.trhip_buffer_bind_memory.argtypes = [vp, vp, u64]
    # An older build named by TRHIP_LIB (tools/material_texture_cost.py --baseline-lib) has no texture table: its texture-free
    # frames still run, TextureTable and srgb_table raise.  lib/libtrhip.so itself exports them (tests/test_abi_symbols.py).
    has_tables = hasattr(L, "trhip_texture_table_create")
    if has_tables:
        L.trhip_texture_table_create.argtypes = [vp, u32, C.POINTER(vp)]
        L.trhip_texture_table_capacity.argtypes = [vp]
        L.trhip_texture_table_capacity.restype = u32
        L.trhip_texture_table_set.argtypes = [vp, u32, vp]
        L.trhip_texture_table_clear.argtypes = [vp, u32]
        L.trhip_srgb_table.argtypes = [vp]
    for n in ("trhip_buffer_retain", "trhip_buffer_release", "trhip_texture_retain", "trhip_texture_release",
              "trhip_cmd_release", "trhip_timer_release") + (("trhip_texture_table_retain", "trhip_texture_table_release") if has_tables else ()):
        getattr(L, n).argtypes = [vp]
        getattr(L, n).restype = None
    L.trhip_buffer_device_ptr.argtypes = [vp]
    L.trhip_buffer_device_ptr.restype = vp
    L.trhip_buffer_size.argtypes = [vp]
    L.trhip_buffer_size.restype = u64
    L.trhip_texture_create.argtypes = [vp, C.POINTER(TextureDesc), C.POINTER(vp)]
    L.trhip_texture_memory_requirements.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.trhip_texture_bind_memory.argtypes = [vp, vp, u64]
    L.trhip_texture_device_ptr.argtypes = [vp]
    L.trhip_texture_device_ptr.restype = vp
    L.trhip_texture_mip_info.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64)]
    L.trhip_texture_size.argtypes = [vp]
    L.trhip_texture_size.restype = u64
    L.trhip_buffer_upload.argtypes = [vp, u64, vp, u64]
    L.trhip_buffer_download.argtypes = [vp, u64, vp, u64]
    L.trhip_texture_upload.argtypes = [vp, u32, vp, u64]
    L.trhip_texture_download.argtypes = [vp, u32, vp, u64]
    if hasattr(L, "trhip_texture_create_array"):             # absent from an older build named by TRHIP_LIB (see above)
        L.trhip_texture_create_array.argtypes = [vp, C.POINTER(TextureDesc), u32, C.POINTER(vp)]
        L.trhip_texture_array_size.argtypes = [vp]
        L.trhip_texture_array_size.restype = u32
        L.trhip_texture_slice_pitch.argtypes = [vp]
        L.trhip_texture_slice_pitch.restype = u64
        L.trhip_texture_upload_slice.argtypes = [vp, u32, vp, u64]
        L.trhip_texture_download_slice.argtypes = [vp, u32, vp, u64]
    if hasattr(L, "trhip_dds_parse"):                       # absent from an older build named by TRHIP_LIB (see above)
        L.trhip_format_block_bytes.argtypes = [u32]
        L.trhip_format_block_bytes.restype = u32
        L.trhip_dds_parse.argtypes = [vp, u64, C.POINTER(DdsInfo)]
    if hasattr(L, "trhip_sampler_feedback_create"):         # absent from an older build named by TRHIP_LIB (see above)
        L.trhip_texture_set_streaming_region.argtypes = [vp, u32, u32]
        L.trhip_texture_streaming_region.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
        L.trhip_sampler_feedback_create.argtypes = [vp, vp, C.c_char_p, C.POINTER(vp)]
        L.trhip_cmd_clear_sampler_feedback.argtypes = [vp, vp]
        L.trhip_cmd_decode_sampler_feedback.argtypes = [vp, vp, u64, vp]
        L.trhip_cmd_write_texture_region.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp, u64]
    L.trhip_cmd_create.argtypes = [vp, C.POINTER(vp)]
    L.trhip_cmd_open.argtypes = [vp]
    L.trhip_cmd_close.argtypes = [vp]
    L.trhip_cmd_write_buffer.argtypes = [vp, vp, u64, vp, u64]
    L.trhip_cmd_clear_buffer_u32.argtypes = [vp, vp, u32]
    L.trhip_cmd_clear_texture_f32.argtypes = [vp, vp, C.c_float]
    L.trhip_cmd_clear_texture_u32.argtypes = [vp, vp, u32]
    L.trhip_cmd_copy_buffer.argtypes = [vp, vp, u64, vp, u64, u64]
    L.trhip_cmd_copy_texture.argtypes = [vp, vp, vp]
    L.trhip_cmd_host_callback.argtypes = [vp, HOST_FN, vp]
    L.trhip_launch_shard_late_info.argtypes = [vp, vp, u32, u32, vp]
    L.trhip_stream_create.argtypes = [i32, C.POINTER(vp)]
    L.trhip_stream_create_priority.argtypes = [i32, i32, C.POINTER(vp)]
    L.trhip_stream_destroy.argtypes = [vp]
    L.trhip_stream_destroy.restype = None
    L.trhip_stream_synchronize.argtypes = [vp]
    L.trhip_event_create.argtypes = [i32, C.POINTER(vp)]
    L.trhip_event_destroy.argtypes = [vp]
    L.trhip_event_destroy.restype = None
    L.trhip_event_record.argtypes = [vp, vp]
    L.trhip_stream_wait_event.argtypes = [vp, vp]
    L.trhip_cmd_dispatch.argtypes = [vp, C.c_char_p, C.POINTER(Binding), u32, vp, u32, u32, u32, u32]
    L.trhip_cmd_dispatch_indirect.argtypes = [vp, C.c_char_p, C.POINTER(Binding), u32, vp, u32, vp, u32]
    L.trhip_cmd_begin_timer.argtypes = [vp, vp]
    L.trhip_cmd_end_timer.argtypes = [vp, vp]
    L.trhip_cmd_begin_marker.argtypes = [vp, C.c_char_p]
    L.trhip_cmd_end_marker.argtypes = [vp]
    L.trhip_queue_execute.argtypes = [vp, C.POINTER(vp), u32]
    L.trhip_timer_create.argtypes = [vp, C.POINTER(vp)]
    L.trhip_timer_get_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.trhip_pipeline_stats_create.argtypes = [vp, C.POINTER(vp)]
    L.trhip_pipeline_stats_release.argtypes = [vp]
    L.trhip_pipeline_stats_release.restype = None
    L.trhip_cmd_begin_pipeline_stats.argtypes = [vp, vp]
    L.trhip_cmd_end_pipeline_stats.argtypes = [vp, vp]
    L.trhip_pipeline_stats_get.argtypes = [vp, C.POINTER(PipelineStatistics)]
    if hasattr(L, "trhip_readback_create"):              # an experiment build (TRHIP_LIB) from before the read-back has none
        L.trhip_readback_create.argtypes = [vp, C.c_uint64, u32, C.POINTER(vp)]
        L.trhip_readback_release.argtypes = [vp]
        L.trhip_readback_release.restype = None
        L.trhip_readback_reset.argtypes = [vp]
        L.trhip_cmd_copy_to_readback.argtypes = [vp, vp, u32, vp, C.c_uint64, C.c_uint64]
        L.trhip_readback_read.argtypes = [vp, u32, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        if hasattr(L, "trhip_readback_poll"):
            L.trhip_readback_poll.argtypes = [vp, u32, C.POINTER(C.c_int)]
    L.trhip_profile_enable.argtypes = [vp, i32]
    L.trhip_profile_filter.argtypes = [vp, C.c_char_p]
    L.trhip_profile_reset.argtypes = [vp]
    L.trhip_buffer_mark_written.argtypes = [vp]
    L.trhip_texture_mark_written.argtypes = [vp]
    L.trhip_profile_count.argtypes = [vp, C.POINTER(u32)]
    L.trhip_profile_entry.argtypes = [vp, u32, C.POINTER(C.c_char_p), C.POINTER(u64), C.POINTER(C.c_double)]
    for n in ("trhip_accel_max_depth", "trhip_blas_leaf_capacity", "trhip_accel_max_nodes"):
        getattr(L, n).restype = u32
    L.trhip_accel_max_nodes.argtypes = [u32]
    pu32 = C.POINTER(u32)
    L.trhip_blas_build.argtypes = [vp, u32, u32, vp, u32, vp, u32, vp, pu32, pu32, pu32]
    L.trhip_tlas_build.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, vp, vp, pu32, pu32]
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise TrhipError(f"trhip error {rc}: {load().trhip_last_error().decode(errors='replace')}")


def srgb_table() -> np.ndarray:
    """trhip_srgb_table: the 256 floats SRGBA8_UNORM texels decode to (no device needed)."""
    out = np.empty(256, np.float32)
    if not hasattr(load(), "trhip_srgb_table"):
        raise TrhipError(f"{LIB_PATH} has no trhip_srgb_table: a build from before textured materials")
    _check(load().trhip_srgb_table(out.ctypes.data))
    return out


def format_block_bytes(fmt: int) -> int:
    """trhip_format_block_bytes: 8 or 16 for one of BC_FORMATS, 0 for every other format (no device needed)."""
    if not hasattr(load(), "trhip_format_block_bytes"):
        raise TrhipError(f"{LIB_PATH} has no trhip_format_block_bytes: a build from before block-compressed textures")
    return int(load().trhip_format_block_bytes(int(fmt)))


def dds_parse(data) -> DdsInfo:
    """trhip_dds_parse on the bytes of a .dds file: what the file says (no device needed); raises TrhipError with the parser's message."""
    if not hasattr(load(), "trhip_dds_parse"):
        raise TrhipError(f"{LIB_PATH} has no trhip_dds_parse: a build from before block-compressed textures")
    buf = np.frombuffer(bytes(data), np.uint8)
    info = DdsInfo()
    _check(load().trhip_dds_parse(buf.ctypes.data if len(buf) else None, len(buf), C.byref(info)))
    return info


def shader_names():
    L = load()
    return [L.trhip_shader_name(i).decode() for i in range(L.trhip_shader_count())]


class Buffer:
    def __init__(self, dev: "Device", handle, size: int, name: str):
        self.dev, self.h, self.size, self.name = dev, handle, size, name

    def upload(self, arr: np.ndarray, offset: int = 0):
        arr = np.ascontiguousarray(arr)
        _check(load().trhip_buffer_upload(self.h, offset, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype=np.uint32, count: int | None = None, offset: int = 0) -> np.ndarray:
        dtype = np.dtype(dtype)
        n = (self.size - offset) // dtype.itemsize if count is None else count
        out = np.empty(n, dtype)
        if n:
            _check(load().trhip_buffer_download(self.h, offset, out.ctypes.data, out.nbytes))
        return out

    @property
    def ptr(self) -> int:
        return load().trhip_buffer_device_ptr(self.h) or 0

    def mark_written(self):
        """The memory was written behind the back end's back (raw pointer, another wrap, an aliased resource): derived data
        (instance cull cache, meshlet cull stream) must be rebuilt.  include/trhip.h: trhip_buffer_mark_written."""
        _check(load().trhip_buffer_mark_written(self.h))

    def release(self):
        if self.h:
            load().trhip_buffer_release(self.h)
            self.h = None


class Texture:
    def __init__(self, dev: "Device", handle, w: int, h: int, mips: int, fmt: int, name: str, array_size: int = 0):
        self.dev, self.h, self.w, self.hgt, self.mips, self.format, self.name = dev, handle, w, h, mips, fmt, name
        self.array_size = array_size            # 0: not an array texture (trhip_texture_create_array)

    def mip_dims(self, k: int):
        return max(self.w >> k, 1), max(self.hgt >> k, 1)

    def mip_info(self, k: int):
        """(width, height, byte offset) of level k (trhip_texture_mip_info)."""
        w, h, off = C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(load().trhip_texture_mip_info(self.h, k, C.byref(w), C.byref(h), C.byref(off)))
        return int(w.value), int(h.value), int(off.value)

    def _dtype(self):
        return {FORMAT_R16_FLOAT: np.uint16, FORMAT_RG32_UINT: np.uint64, FORMAT_RG16_FLOAT: np.float16, FORMAT_RGBA32_UINT: np.uint32,
                FORMAT_R11G11B10_FLOAT: np.uint32, FORMAT_R8_UNORM: np.uint8, FORMAT_R8_UINT: np.uint8, FORMAT_RGBA8_UNORM: np.uint32,
                FORMAT_SRGBA8_UNORM: np.uint32, FORMAT_R10G10B10A2_UNORM: np.uint32, FORMAT_RGBA16_FLOAT: np.float16,
                SAMPLER_FEEDBACK_FORMAT: np.uint32}.get(self.format, np.float32)

    def _shape(self, mw: int, mh: int):
        return (mh, mw, 2) if self.format == FORMAT_RG16_FLOAT else (mh, mw, 4) if self.format in (FORMAT_RGBA32_UINT, FORMAT_RGBA16_FLOAT) else (mh, mw)

    def set_streaming_region(self, region_w: int = 0, region_h: int = 0):
        """trhip_texture_set_streaming_region: makes a material texture streamable with regions of region_w x region_h texels
        (0, 0: D3D's 64 KB tile shape of the format); refused when the size of mip 0 is no multiple of it.  Before TextureTable.set."""
        _check(load().trhip_texture_set_streaming_region(self.h, int(region_w), int(region_h)))
        return self.streaming_region()

    def streaming_region(self):
        """(region_w, region_h) in texels, (0, 0) for a texture that is not streamable; a feedback map answers its texture's."""
        w, h = C.c_uint32(), C.c_uint32()
        _check(load().trhip_texture_streaming_region(self.h, C.byref(w), C.byref(h)))
        return int(w.value), int(h.value)

    def upload_slice(self, k: int, arr: np.ndarray):
        """Slice k of an array texture (trhip_texture_upload_slice)."""
        arr = np.ascontiguousarray(arr, self._dtype())
        _check(load().trhip_texture_upload_slice(self.h, k, arr.ctypes.data, arr.nbytes))

    def download_slice(self, k: int) -> np.ndarray:
        out = np.empty(self._shape(self.w, self.hgt), self._dtype())
        _check(load().trhip_texture_download_slice(self.h, k, out.ctypes.data, out.nbytes))
        return out

    @property
    def slice_pitch(self) -> int:
        return int(load().trhip_texture_slice_pitch(self.h))

    def upload_mip(self, k: int, arr):
        """Level k.  A block-compressed texture takes the level's raw block bytes (bytes, or an array of any shape): ceil(w_k / 4) x
        ceil(h_k / 4) blocks of format_block_bytes(format) bytes, row-major; a wrong byte count is refused."""
        if self.format in BC_FORMATS:
            arr = np.frombuffer(arr, np.uint8) if isinstance(arr, (bytes, bytearray, memoryview)) else np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
            _check(load().trhip_texture_upload(self.h, k, arr.ctypes.data, arr.nbytes))
            return
        if self.format in (FORMAT_RGBA8_UNORM, FORMAT_SRGBA8_UNORM) and np.asarray(arr).dtype == np.uint8:   # [h, w, 4] bytes R, G, B, A
            arr = np.ascontiguousarray(arr).reshape(-1).view(np.uint32)
        arr = np.ascontiguousarray(arr, self._dtype())
        _check(load().trhip_texture_upload(self.h, k, arr.ctypes.data, arr.nbytes))

    def download_mip(self, k: int) -> np.ndarray:
        """Level k; of a block-compressed texture its raw block bytes, uint8 [ceil(h_k / 4), ceil(w_k / 4), block bytes]."""
        mw, mh = self.mip_dims(k)
        if self.format in BC_FORMATS:
            out = np.empty(((mh + 3) // 4, (mw + 3) // 4, format_block_bytes(self.format)), np.uint8)
            _check(load().trhip_texture_download(self.h, k, out.ctypes.data, out.nbytes))
            return out
        out = np.empty(self._shape(mw, mh), self._dtype())
        _check(load().trhip_texture_download(self.h, k, out.ctypes.data, out.nbytes))
        return out

    def upload_chain(self, texels: np.ndarray, offsets):
        """texels: packed mip chain (oracle / interop.hzb_layout order)."""
        for k in range(self.mips):
            mw, mh = self.mip_dims(k)
            self.upload_mip(k, texels[offsets[k]:offsets[k] + mw * mh])

    def download_chain(self) -> np.ndarray:
        return np.concatenate([self.download_mip(k).ravel() for k in range(self.mips)])

    def mark_written(self):
        """See Buffer.mark_written: the footprint-min table of an HZB written through its raw pointer is stale."""
        _check(load().trhip_texture_mark_written(self.h))

    def release(self):
        if self.h:
            load().trhip_texture_release(self.h)
            self.h = None


def bind(kind: int, slot: int, res=None, base_mip: int = 0) -> Binding:
    b = Binding()
    b.type, b.slot, b.baseMip = kind, slot, base_mip
    b.resource = res.h if res is not None else None
    return b


def CB(slot, buf): return bind(BIND_CONSTANT_BUFFER, slot, buf)
def PUSH(slot): return bind(BIND_PUSH_CONSTANTS, slot)
def SRV(slot, buf): return bind(BIND_STRUCTURED_SRV, slot, buf)
def UAV(slot, buf): return bind(BIND_STRUCTURED_UAV, slot, buf)
def TEX_SRV(slot, tex, mip=0): return bind(BIND_TEXTURE_SRV, slot, tex, mip)   # mip: read by bloom_PS_* only
def TEX_UAV(slot, tex, mip=0): return bind(BIND_TEXTURE_UAV, slot, tex, mip)
def SAMPLER(slot): return bind(BIND_SAMPLER, slot)
def TEX_TABLE(table, slot=TEXTURE_TABLE_SLOT): return bind(BIND_TEXTURE_TABLE, slot, table)


class TextureTable:
    """trhip_texture_table: descriptor index -> texture, the stand-in of ResourceDescriptorHeap[...] (include/trhip.h)."""
    def __init__(self, dev, handle, capacity: int):
        self.dev, self.h, self.capacity = dev, handle, capacity

    def set(self, index: int, tex: "Texture"):
        _check(load().trhip_texture_table_set(self.h, index, tex.h))

    def clear(self, index: int):
        _check(load().trhip_texture_table_clear(self.h, index))

    def release(self):
        if self.h:
            load().trhip_texture_table_release(self.h)
            self.h = None


class Timer:
    def __init__(self, dev, handle):
        self.dev, self.h = dev, handle

    def ms(self) -> float:
        v = C.c_float(0)
        _check(load().trhip_timer_get_ms(self.h, C.byref(v)))
        return float(v.value)

    def release(self):
        if self.h:
            load().trhip_timer_release(self.h)
            self.h = None


class PipelineStatsQuery:
    """nvrhi::IPipelineStatisticsQuery: trhip_pipeline_stats (include/trhip.h)."""
    def __init__(self, dev, handle):
        self.dev, self.h = dev, handle

    def get(self) -> dict:
        """Waits for the last executed end; {field: int} in trhip_pipeline_statistics order."""
        v = PipelineStatistics()
        _check(load().trhip_pipeline_stats_get(self.h, C.byref(v)))
        return v.as_dict()

    def release(self):
        if self.h:
            load().trhip_pipeline_stats_release(self.h)
            self.h = None


class Readback:
    """nvrhi's staging resource: trhip_readback (include/trhip.h), `slots` slots of pinned host memory with one event each."""
    def __init__(self, dev, handle, bytes_per_slot: int, slots: int):
        self.dev, self.h, self.bytes_per_slot, self.slots = dev, handle, int(bytes_per_slot), int(slots)

    def read(self, slot: int, dtype=np.uint8, count: int | None = None):
        """(array, bytes written): waits for that slot's copy only.  A slot never written gives zeros and 0."""
        dt = np.dtype(dtype)
        out = np.zeros(self.bytes_per_slot // dt.itemsize if count is None else int(count), dt)
        written = C.c_uint64()
        _check(load().trhip_readback_read(self.h, int(slot), out.ctypes.data, out.nbytes, C.byref(written)))
        return out, int(written.value)

    def ready(self, slot: int) -> bool:
        """trhip_readback_poll: never waits; True when read(slot) would return at once."""
        r = C.c_int(0)
        _check(load().trhip_readback_poll(self.h, int(slot), C.byref(r)))
        return bool(r.value)

    def reset(self):
        """Waits for the device and marks every slot as never written; recorded lists that name the resource stay valid."""
        _check(load().trhip_readback_reset(self.h))

    def release(self):
        """Every list that names the resource must have been re-opened or released first (include/trhip.h)."""
        if self.h:
            load().trhip_readback_release(self.h)
            self.h = None


class CommandList:
    def __init__(self, dev: "Device", handle):
        self.dev, self.h = dev, handle
        self._keep = []
        self._keep_cb = []

    def open(self):
        self._keep.clear()
        self._keep_cb = []
        _check(load().trhip_cmd_open(self.h))
        return self

    def close(self):
        _check(load().trhip_cmd_close(self.h))
        return self

    def write_buffer(self, buf: Buffer, arr: np.ndarray, offset: int = 0):
        arr = np.ascontiguousarray(arr)
        _check(load().trhip_cmd_write_buffer(self.h, buf.h, offset, arr.ctypes.data, arr.nbytes))

    def clear_buffer_u32(self, buf: Buffer, value: int = 0):
        _check(load().trhip_cmd_clear_buffer_u32(self.h, buf.h, value))

    def clear_texture_f32(self, tex: Texture, value: float):
        _check(load().trhip_cmd_clear_texture_f32(self.h, tex.h, value))

    def clear_texture_u32(self, tex: Texture, value: int):
        _check(load().trhip_cmd_clear_texture_u32(self.h, tex.h, value))

    def copy_buffer(self, dst: Buffer, src: Buffer, nbytes: int, dst_offset: int = 0, src_offset: int = 0):
        _check(load().trhip_cmd_copy_buffer(self.h, dst.h, dst_offset, src.h, src_offset, nbytes))

    def copy_texture(self, dst: Texture, src: Texture):
        _check(load().trhip_cmd_copy_texture(self.h, dst.h, src.h))

    def constant_buffer(self, data: np.ndarray, name="cb") -> Buffer:
        """Graphic::CreateConstantBuffer (Graphic.h:66-72): volatile CB + writeBuffer."""
        data = np.ascontiguousarray(data)
        cb = self.dev.create_buffer(data.nbytes, name=name, volatile_constant=True)
        self.write_buffer(cb, data)
        self._keep.append(cb)
        return cb

    def dispatch(self, shader: str, bindings, groups, push: np.ndarray | None = None):
        arr = (Binding * len(bindings))(*bindings)
        p, pb = (None, 0) if push is None else (np.ascontiguousarray(push).ctypes.data, np.ascontiguousarray(push).nbytes)
        gx, gy, gz = groups
        _check(load().trhip_cmd_dispatch(self.h, shader.encode(), arr, len(bindings), p, pb, gx, gy, gz))

    def dispatch_indirect(self, shader: str, bindings, args: Buffer, offset: int = 0, push: np.ndarray | None = None):
        arr = (Binding * len(bindings))(*bindings)
        p, pb = (None, 0) if push is None else (np.ascontiguousarray(push).ctypes.data, np.ascontiguousarray(push).nbytes)
        _check(load().trhip_cmd_dispatch_indirect(self.h, shader.encode(), arr, len(bindings), p, pb, args.h, offset))

    def host_callback(self, fn):
        """fn(hip_stream: int) is called while the list is executed, in order (include/trhip.h)."""
        cb = HOST_FN(lambda _user, stream: fn(int(stream or 0)))
        self._keep_cb.append(cb)
        _check(load().trhip_cmd_host_callback(self.h, cb, None))

    def begin_timer(self, t: Timer): _check(load().trhip_cmd_begin_timer(self.h, t.h))
    def end_timer(self, t: Timer): _check(load().trhip_cmd_end_timer(self.h, t.h))
    def begin_pipeline_stats(self, q: PipelineStatsQuery): _check(load().trhip_cmd_begin_pipeline_stats(self.h, q.h))
    def end_pipeline_stats(self, q: PipelineStatsQuery): _check(load().trhip_cmd_end_pipeline_stats(self.h, q.h))
    def copy_to_readback(self, rb: Readback, slot: int, src: Buffer, offset: int, nbytes: int):
        _check(load().trhip_cmd_copy_to_readback(self.h, rb.h, int(slot), src.h, int(offset), int(nbytes)))
    def clear_sampler_feedback(self, feedback: Texture): _check(load().trhip_cmd_clear_sampler_feedback(self.h, feedback.h))
    def decode_sampler_feedback(self, dst: Buffer, feedback: Texture, offset: int = 0):
        """One byte per region of the feedback map into dst at `offset` (row-major; the level asked for, 0xFF = never sampled)."""
        _check(load().trhip_cmd_decode_sampler_feedback(self.h, dst.h, int(offset), feedback.h))

    def write_texture_region(self, tex: Texture, mip: int, x: int, y: int, w: int, h: int, data):
        """trhip_cmd_write_texture_region: a w x h texel rectangle of one mip of a material texture at (x, y); data: uint8 [h, w, 4], or
        the rectangle's blocks (bytes or any array) for a block-compressed texture.  Copied when recorded."""
        arr = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        _check(load().trhip_cmd_write_texture_region(self.h, tex.h, int(mip), int(x), int(y), int(w), int(h), arr.ctypes.data, arr.nbytes))

    def begin_marker(self, name: str): _check(load().trhip_cmd_begin_marker(self.h, name.encode()))
    def end_marker(self): _check(load().trhip_cmd_end_marker(self.h))

    def release(self):
        if self.h:
            load().trhip_cmd_release(self.h)
            self.h = None
        for b in self._keep:
            b.release()
        self._keep.clear()


class Device:
    def __init__(self, index: int = 0, stream: int | None = None, handle: int | None = None):
        """handle: wrap an existing trhip_device (e.g. the host library's, trhost_device()); not owned."""
        L = load()
        h = C.c_void_p()
        self.owned = handle is None
        if handle is not None:
            h = C.c_void_p(handle)
        elif stream is None:
            _check(L.trhip_device_create(index, C.byref(h)))
        else:
            _check(L.trhip_device_create_on_stream(index, C.c_void_p(stream), C.byref(h)))
        self.h = h
        cu, wave, mem = C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(L.trhip_device_info(self.h, C.byref(cu), C.byref(wave), C.byref(mem)))
        self.compute_units, self.wave_size, self.total_mem = cu.value, wave.value, mem.value

    def wait_idle(self):
        _check(load().trhip_device_wait_idle(self.h))

    def create_buffer(self, nbytes: int, name="", stride=4, uav=True, indirect=False, virtual=False, volatile_constant=False) -> Buffer:
        d = BufferDesc(int(nbytes), stride, int(uav), int(indirect), int(virtual), int(volatile_constant), name.encode())
        h = C.c_void_p()
        _check(load().trhip_buffer_create(self.h, C.byref(d), C.byref(h)))
        return Buffer(self, h, int(nbytes), name)

    def wrap_buffer(self, ptr: int, nbytes: int, name="", stride=4, uav=True) -> Buffer:
        d = BufferDesc(int(nbytes), stride, int(uav), 0, 0, 0, name.encode())
        h = C.c_void_p()
        _check(load().trhip_buffer_wrap(self.h, C.c_void_p(ptr), C.byref(d), C.byref(h)))
        return Buffer(self, h, int(nbytes), name)

    def buffer_from(self, arr: np.ndarray, name="", uav=True, min_bytes: int = 4) -> Buffer:
        arr = np.ascontiguousarray(arr)
        b = self.create_buffer(max(arr.nbytes, min_bytes), name=name, stride=max(arr.dtype.itemsize, 1), uav=uav)
        if arr.nbytes:
            b.upload(arr)
        return b

    def create_texture(self, w: int, h: int, mips: int, fmt: int, name="", uav=True, render_target=False) -> Texture:
        """render_target: TRHIP_TEXTURE_RENDER_TARGET; only such an R11G11B10_FLOAT texture (the bloom chain) may have mips."""
        d = TextureDesc(w, h, mips, fmt, int(bool(uav)) | (TEXTURE_RENDER_TARGET if render_target else 0), 0, name.encode())
        hd = C.c_void_p()
        _check(load().trhip_texture_create(self.h, C.byref(d), C.byref(hd)))
        return Texture(self, hd, w, h, mips, fmt, name)

    def create_texture_array(self, w: int, h: int, slices: int, fmt: int, name="", uav=False) -> Texture:
        """trhip_texture_create_array: `slices` slices of w x h, one mip; R10G10B10A2_UNORM, RG16_FLOAT or RGBA16_FLOAT."""
        d = TextureDesc(w, h, 1, fmt, int(bool(uav)), 0, name.encode())
        hd = C.c_void_p()
        _check(load().trhip_texture_create_array(self.h, C.byref(d), slices, C.byref(hd)))
        return Texture(self, hd, w, h, 1, fmt, name, array_size=slices)

    def create_texture_table(self, capacity: int) -> TextureTable:
        h = C.c_void_p()
        if not hasattr(load(), "trhip_texture_table_create"):
            raise TrhipError(f"{LIB_PATH} has no texture table: a build from before textured materials")
        _check(load().trhip_texture_table_create(self.h, capacity, C.byref(h)))
        return TextureTable(self, h, capacity)

    def create_sampled_texture(self, mips, fmt: int, name="") -> Texture:
        """A material texture from its mip chain: mips = uint8 arrays [h_k, w_k, 4] (R, G, B, A), level k of
        max(w >> k, 1) x max(h >> k, 1); fmt = FORMAT_RGBA8_UNORM or FORMAT_SRGBA8_UNORM.  Created without the UAV bit.
        For one of BC_FORMATS mips is an interop.BlockMips: the raw block bytes of every level with the size of level 0 in texels
        (any size >= 1); the blocks are uploaded as they are -- there is no encoder."""
        if fmt in BC_FORMATS:
            if not hasattr(mips, "width") or len(mips) == 0:
                raise ValueError("a block-compressed texture takes an interop.BlockMips (the levels' block bytes and the size in texels)")
            t = self.create_texture(int(mips.width), int(mips.height), len(mips), fmt, name, uav=False)
            try:
                for k, m in enumerate(mips):
                    t.upload_mip(k, m)
            except Exception:
                t.release()
                raise
            return t
        if fmt not in (FORMAT_RGBA8_UNORM, FORMAT_SRGBA8_UNORM):
            raise ValueError(f"a sampled texture is RGBA8_UNORM, SRGBA8_UNORM or one of BC_FORMATS, not format {fmt}")
        mips = [np.ascontiguousarray(m, np.uint8) for m in mips]
        if not mips or any(m.ndim != 3 or m.shape[2] != 4 for m in mips):
            raise ValueError("mips: a non-empty list of uint8 [h, w, 4] arrays")
        h0, w0 = mips[0].shape[:2]
        for k, m in enumerate(mips):
            if m.shape[:2] != (max(h0 >> k, 1), max(w0 >> k, 1)):
                raise ValueError(f"mip {k} is {m.shape[1]} x {m.shape[0]}, expected {max(w0 >> k, 1)} x {max(h0 >> k, 1)}")
        t = self.create_texture(w0, h0, len(mips), fmt, name, uav=False)
        for k, m in enumerate(mips):
            t.upload_mip(k, m)
        return t

    def create_sampler_feedback(self, paired: Texture, name="") -> Texture:
        """trhip_sampler_feedback_create: the feedback map of a streamable material texture, one 32-bit word per region, created
        as never sampled (0xFFFFFFFF).  download_mip(0) gives the raw words, CommandList.decode_sampler_feedback the bytes."""
        if not hasattr(load(), "trhip_sampler_feedback_create"):
            raise TrhipError(f"{LIB_PATH} has no sampler feedback: a build from before texture streaming")
        h = C.c_void_p()
        _check(load().trhip_sampler_feedback_create(self.h, paired.h, name.encode(), C.byref(h)))
        rw, rh = paired.streaming_region()
        return Texture(self, h, paired.w // rw, paired.hgt // rh, 1, SAMPLER_FEEDBACK_FORMAT, name)

    def create_command_list(self) -> CommandList:
        h = C.c_void_p()
        _check(load().trhip_cmd_create(self.h, C.byref(h)))
        return CommandList(self, h)

    def create_timer(self) -> Timer:
        h = C.c_void_p()
        _check(load().trhip_timer_create(self.h, C.byref(h)))
        return Timer(self, h)

    def create_pipeline_stats(self) -> PipelineStatsQuery:
        h = C.c_void_p()
        _check(load().trhip_pipeline_stats_create(self.h, C.byref(h)))
        return PipelineStatsQuery(self, h)

    def create_readback(self, bytes_per_slot: int, slots: int) -> Readback:
        h = C.c_void_p()
        if not hasattr(load(), "trhip_readback_create"):
            raise TrhipError(f"{LIB_PATH} has no read-back: a build from before probe variability")
        _check(load().trhip_readback_create(self.h, int(bytes_per_slot), int(slots), C.byref(h)))
        return Readback(self, h, bytes_per_slot, slots)

    def execute(self, *lists: CommandList):
        arr = (C.c_void_p * len(lists))(*[cl.h for cl in lists])
        _check(load().trhip_queue_execute(self.h, arr, len(lists)))

    def profile_enable(self, on: bool = True): _check(load().trhip_profile_enable(self.h, int(on)))
    def profile_reset(self): _check(load().trhip_profile_reset(self.h))
    def profile_filter(self, name: str | None): _check(load().trhip_profile_filter(self.h, name.encode() if name else None))

    def profile(self) -> dict:
        n = C.c_uint32()
        _check(load().trhip_profile_count(self.h, C.byref(n)))
        out = {}
        for i in range(n.value):
            name, cnt, ms = C.c_char_p(), C.c_uint64(), C.c_double()
            _check(load().trhip_profile_entry(self.h, i, C.byref(name), C.byref(cnt), C.byref(ms)))
            out[name.value.decode()] = (int(cnt.value), float(ms.value))
        return out

    def destroy(self):
        if self.h and self.owned:
            load().trhip_device_destroy(self.h)
        self.h = None
