"""ctypes wrapper of tests/material_textures_ref.c, the test reference of the textured G-buffer resolve
("basepass_PS_Main_GBuffer" with a texture table at t19): the software sampler alone (sample) and whole frames (gbuffer).

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C

import numpy as np

from ref_build import compile_ref
from toyrenderer_amd import interop as I

MAX_MIPS = 16
FORMAT_RGBA8, FORMAT_SRGBA8 = 10, 11


class MtTexture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("mipCount", C.c_uint32), ("format", C.c_uint32),
                ("mips", C.c_void_p * MAX_MIPS)]


def _declare(lib):
    lib.mt_gbuffer.argtypes = [C.c_void_p] * 16
    lib.mt_gbuffer.restype = None
    lib.mt_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mt_sample.restype = C.c_uint32
    lib.mt_srgb_table.argtypes = [C.c_void_p]
    lib.mt_srgb_table.restype = None
    lib.mt_log2.argtypes = [C.c_float]
    lib.mt_log2.restype = C.c_float
    lib.mt_half_to_float.argtypes = [C.c_uint16]
    lib.mt_half_to_float.restype = C.c_float


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "material_textures_ref", _declare, include_oracle=True)


def _p(a):
    return a.ctypes.data if a is not None else None


class Texture:
    """(mips, format): mips = uint8 [h_k, w_k, 4] arrays; None for an empty table entry."""
    def __init__(self, mips, fmt):
        self.mips = [np.ascontiguousarray(m, np.uint8) for m in mips]
        self.format = fmt
        self.c = MtTexture()
        self.c.height, self.c.width = self.mips[0].shape[:2]
        self.c.mipCount, self.c.format = len(self.mips), fmt
        for k, m in enumerate(self.mips):
            assert m.shape == (max(self.c.height >> k, 1), max(self.c.width >> k, 1), 4), (k, m.shape)
            self.c.mips[k] = m.ctypes.data


def srgb_table(lib) -> np.ndarray:
    out = np.empty(256, np.float32)
    lib.mt_srgb_table(_p(out))
    return out


def sample(lib, tex: Texture, wrap, uv, ddx, ddy):
    """(float32 [4] value, N, lod) of one SampleMaterialValue."""
    srgb = srgb_table(lib)
    uv, ddx, ddy = (np.ascontiguousarray(a, np.float32) for a in (uv, ddx, ddy))
    out, lod = np.zeros(4, np.float32), C.c_float(0)
    n = lib.mt_sample(C.addressof(tex.c), _p(srgb), int(bool(wrap)), _p(uv), _p(ddx), _p(ddy), _p(out), C.addressof(lod))
    return out, int(n), float(lod.value)


def gbuffer(lib, consts, geo, records4, lists4, vis, materials, textures, debug_mode=0, gbuffer_init=None, motion_init=None):
    """(uint32 [H, W, 4] GBufferA, float32 [H, W, 2] motion, uint8 [H, W, 4] taps) of every texel of vis, as gbuffer_ref.gbuffer;
    textures: the table, a list of Texture or None (an empty entry); taps: the N of the albedo, normal, metallic-roughness and
    emissive sample of each written pixel (0: not sampled)."""
    k = np.ascontiguousarray(consts).copy()
    k["m_DebugMode"] = debug_mode
    H, W = vis.shape
    g = np.zeros((H, W, 4), np.uint32) if gbuffer_init is None else np.ascontiguousarray(gbuffer_init, np.uint32).copy()
    m = np.zeros((H, W, 2), np.float32) if motion_init is None else np.ascontiguousarray(motion_init, np.float32).copy()
    taps = np.zeros((H, W, 4), np.uint8)
    present = [r is not None and len(r) > 0 for r in records4]
    recs = [np.ascontiguousarray(r) if ok else np.zeros(1, I.MeshletAmplificationData) for r, ok in zip(records4, present)]
    lsts = [np.ascontiguousarray(x, np.uint32) if x is not None and len(x) else np.zeros(1, np.uint32) for x in lists4]
    mats = np.ascontiguousarray(materials, I.MaterialData)
    table = (MtTexture * max(len(textures), 1))()
    for i, t in enumerate(textures):
        if t is not None:
            table[i] = t.c
    limits = np.array([len(geo.instances), len(geo.meshData), len(geo.meshlets), len(geo.vertices), len(geo.vertexIds), len(geo.triangles), len(mats)]
                      + [len(r) if ok else 0 for r, ok in zip(recs, present)]
                      + [len(x) if x_in is not None and len(x_in) else 0 for x, x_in in zip(lsts, lists4)] + [len(textures)], np.uint64)
    rp = (C.c_void_p * 4)(*[_p(r) for r in recs])
    lp = (C.c_void_p * 4)(*[_p(x) for x in lsts])
    lib.mt_gbuffer(_p(k), *geo.args(), C.addressof(rp), C.addressof(lp), _p(np.ascontiguousarray(vis, np.uint64)), _p(mats),
                   C.addressof(table), _p(limits), _p(g), _p(m), _p(taps))
    return g, m, taps
