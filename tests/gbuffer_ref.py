"""ctypes wrapper of tests/gbuffer_ref.c, the test reference of GBufferA and the fused motion target
("basepass_PS_Main_GBuffer"), and numpy decoders of GBufferA's words.

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C

import numpy as np

from ref_build import compile_ref
from toyrenderer_amd import interop as I


def _declare(lib):
    lib.gr_gbuffer.argtypes = [C.c_void_p] * 14
    lib.gr_gbuffer.restype = None
    for n in ("gr_pack_rgba8_n", "gr_pack_oct_n", "gr_pack_r9g9b9e5_n", "gr_quick_random_float_n", "gr_mesh_lod_value_n", "gr_unpack_normal_n"):
        getattr(lib, n).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        getattr(lib, n).restype = None
    lib.gr_vertex_normal.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    lib.gr_vertex_normal.restype = None


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "gbuffer_ref", _declare, include_oracle=True)


def _p(a):
    return a.ctypes.data if a is not None else None


def _map(fn, arr, in_dtype, width, out_dtype, out_width=1):
    a = np.ascontiguousarray(arr, in_dtype).reshape(-1, width) if width > 1 else np.ascontiguousarray(arr, in_dtype).reshape(-1)
    out = np.empty((len(a), out_width) if out_width > 1 else len(a), out_dtype)
    fn(_p(a), len(a), _p(out))
    return out


def pack_rgba8(lib, rgba):
    return _map(lib.gr_pack_rgba8_n, rgba, np.float32, 4, np.uint32)


def pack_oct(lib, xyz):
    return _map(lib.gr_pack_oct_n, xyz, np.float32, 3, np.uint32)


def pack_r9g9b9e5(lib, rgb):
    return _map(lib.gr_pack_r9g9b9e5_n, rgb, np.float32, 3, np.uint32)


def quick_random_float(lib, seeds):
    return _map(lib.gr_quick_random_float_n, seeds, np.uint32, 1, np.float32)


def mesh_lod_value(lib, lods):
    return _map(lib.gr_mesh_lod_value_n, lods, np.uint32, 1, np.float32)


def unpack_normal(lib, words):
    return _map(lib.gr_unpack_normal_n, words, np.uint32, 1, np.float32, 3)


def vertex_normal(lib, word, world):
    w = np.ascontiguousarray(world, np.float32).reshape(4, 4)
    out = np.zeros(3, np.float32)
    lib.gr_vertex_normal(int(word), _p(w), _p(out))
    return out


def gbuffer(lib, consts, geo, records4, lists4, vis, materials, debug_mode=0, gbuffer_init=None, motion_init=None):
    """(uint32 [H, W, 4] GBufferA, float32 [H, W, 2] motion) of every texel of vis; geo: visibility_ref.Geometry;
    records4 / lists4: the four slots' arrays (None: an empty slot).  Texels that are 0, or whose chain of indices leaves
    a buffer, keep gbuffer_init / motion_init (default 0)."""
    k = np.ascontiguousarray(consts).copy()
    k["m_DebugMode"] = debug_mode
    H, W = vis.shape
    g = np.zeros((H, W, 4), np.uint32) if gbuffer_init is None else np.ascontiguousarray(gbuffer_init, np.uint32).copy()
    m = np.zeros((H, W, 2), np.float32) if motion_init is None else np.ascontiguousarray(motion_init, np.float32).copy()
    present = [r is not None and len(r) > 0 for r in records4]
    recs = [np.ascontiguousarray(r) if ok else np.zeros(1, I.MeshletAmplificationData) for r, ok in zip(records4, present)]
    lsts = [np.ascontiguousarray(x, np.uint32) if x is not None and len(x) else np.zeros(1, np.uint32) for x in lists4]
    mats = np.ascontiguousarray(materials, I.MaterialData)
    limits = np.array([len(geo.instances), len(geo.meshData), len(geo.meshlets), len(geo.vertices), len(geo.vertexIds), len(geo.triangles), len(mats)]
                      + [len(r) if ok else 0 for r, ok in zip(recs, present)]
                      + [len(x) if x_in is not None and len(x_in) else 0 for x, x_in in zip(lsts, lists4)], np.uint64)
    rp = (C.c_void_p * 4)(*[_p(r) for r in recs])
    lp = (C.c_void_p * 4)(*[_p(x) for x in lsts])
    lib.gr_gbuffer(_p(k), *geo.args(), C.addressof(rp), C.addressof(lp), _p(np.ascontiguousarray(vis, np.uint64)), _p(mats), _p(limits), _p(g), _p(m))
    return g, m


def frame_gbuffer(lib, consts, geo, ref, vis, materials, debug_mode=0):
    """GBufferA and motion of a pyoracle.frame(raster=...) result, as visibility_ref.frame_motion."""
    recs = [ref.records[s] if ref.passRan[s] else None for s in range(4)]
    lsts = [ref.visibleList[s] if ref.passRan[s] else None for s in range(4)]
    return gbuffer(lib, consts, geo, recs, lsts, vis, materials, debug_mode)


# ---- decoders (float64) -------------------------------------------------------------------------------------------
def decode_oct(word):
    """Unit normal (float64 [..., 3]) of GBufferA.y: unorm 2x16 -> octahedral -> normalised."""
    w = np.asarray(word, np.uint32)
    fx = (w & 0xFFFF).astype(np.float64) / 65535.0 * 2.0 - 1.0
    fy = (w >> 16).astype(np.float64) / 65535.0 * 2.0 - 1.0
    z = 1.0 - np.abs(fx) - np.abs(fy)
    t = np.clip(-z, 0.0, 1.0)
    x = fx + np.where(fx >= 0, -t, t)
    y = fy + np.where(fy >= 0, -t, t)
    n = np.stack([x, y, z], -1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def decode_r9g9b9e5(word):
    """float64 [..., 3] of GBufferA.z: mantissa * 2^(E - 24), E = bits 27-31."""
    w = np.asarray(word, np.uint32)
    e = (w >> 27).astype(np.int64)
    m = np.stack([w & 0x1FF, (w >> 9) & 0x1FF, (w >> 18) & 0x1FF], -1).astype(np.float64)
    return m * np.exp2((e - 24).astype(np.float64))[..., None]


def albedo_bytes(word):
    w = np.asarray(word, np.uint32)
    return np.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF], -1)
