"""ctypes wrapper of tests/texture_streaming_ref.c, the test reference of texture streaming: the streamed G-buffer resolve (the
min-mip clamp, the feedback marks, the min-mip colours), the decode of a feedback map and the residency rule.

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C

import numpy as np

import material_textures_ref as MT
from ref_build import compile_ref
from toyrenderer_amd import interop as I

FORMAT_MINMIP, FORMAT_FEEDBACK = 8, 9
NEVER = 0xFF


class TsTiled(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "mips", "regionW", "regionH", "tileBytes")]


class TsStats(C.Structure):
    _fields_ = [("tilesTotal", C.c_uint32), ("tilesResident", C.c_uint32), ("tilesMapped", C.c_uint32), ("tilesUnmapped", C.c_uint32),
                ("bytesUploaded", C.c_uint64)]


def _declare(lib):
    MT._declare(lib)
    lib.ts_gbuffer.argtypes = [C.c_void_p] * 17
    lib.ts_gbuffer.restype = None
    lib.ts_decode.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.ts_decode.restype = None
    lib.ts_standard_levels.argtypes = [C.c_void_p]
    lib.ts_standard_levels.restype = C.c_uint32
    lib.ts_tile_offset.argtypes = [C.c_void_p, C.c_uint32]
    lib.ts_tile_offset.restype = C.c_uint32
    lib.ts_residency_round.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
    lib.ts_residency_round.restype = None


def load(tmpdir, defines=()) -> C.CDLL:
    """defines: the reference's negative-control switches (TS_REF_MUTATE_*, TS_REF_LANE_DROP); none for the reference itself."""
    return compile_ref(tmpdir, "texture_streaming_ref", _declare, include_oracle=True, defines=tuple(defines))


def _p(a):
    return a.ctypes.data if a is not None else None


class Streamable(MT.Texture):
    """A material texture (decoded mips, format) with its region (rw, rh) in texels."""
    def __init__(self, mips, fmt, region):
        super().__init__(mips, fmt)
        self.region = (int(region[0]), int(region[1]))
        assert self.c.width % self.region[0] == 0 and self.c.height % self.region[1] == 0

    @property
    def regions(self):
        return self.c.width // self.region[0], self.c.height // self.region[1]


class MinMip:
    """A min-mip map: uint8 [regions y, regions x]."""
    def __init__(self, texels):
        self.texels = np.ascontiguousarray(texels, np.uint8)
        self.region = (0, 0)
        self.c = MT.MtTexture()
        self.c.height, self.c.width = self.texels.shape
        self.c.mipCount, self.c.format = 1, FORMAT_MINMIP
        self.c.mips[0] = self.texels.ctypes.data


class Feedback:
    """A feedback map of `texture` (a Streamable): uint32 [regions y, regions x] words, all 0xFFFFFFFF at first."""
    def __init__(self, texture):
        rx, ry = texture.regions
        self.words = np.full((ry, rx), 0xFFFFFFFF, np.uint32)
        self.region = texture.region
        self.c = MT.MtTexture()
        self.c.height, self.c.width = ry, rx
        self.c.mipCount, self.c.format = 1, FORMAT_FEEDBACK
        self.c.mips[0] = self.words.ctypes.data

    def clear(self):
        self.words[...] = 0xFFFFFFFF


def decode(lib, words) -> np.ndarray:
    words = np.ascontiguousarray(words, np.uint32)
    out = np.empty(words.shape, np.uint8)
    lib.ts_decode(_p(words), words.size, _p(out))
    return out


def gbuffer(lib, consts, geo, records4, lists4, vis, materials, table, debug_mode=0, gbuffer_init=None, motion_init=None, feedback=False, visualize=False):
    """As material_textures_ref.gbuffer; table: a list of MT.Texture (not streamable), Streamable, MinMip, Feedback or None.  feedback:
    m_bWriteSamplerFeedback (the Feedback entries' words are lowered in place); visualize: m_bVisualizeMinMipTilesOnAlbedoOutput."""
    k = np.ascontiguousarray(consts).copy()
    k["m_DebugMode"] = debug_mode
    k["m_bWriteSamplerFeedback"] = int(bool(feedback))
    k["m_bVisualizeMinMipTilesOnAlbedoOutput"] = int(bool(visualize))
    H, W = vis.shape
    g = np.zeros((H, W, 4), np.uint32) if gbuffer_init is None else np.ascontiguousarray(gbuffer_init, np.uint32).copy()
    m = np.zeros((H, W, 2), np.float32) if motion_init is None else np.ascontiguousarray(motion_init, np.float32).copy()
    taps = np.zeros((H, W, 4), np.uint8)
    present = [r is not None and len(r) > 0 for r in records4]
    recs = [np.ascontiguousarray(r) if ok else np.zeros(1, I.MeshletAmplificationData) for r, ok in zip(records4, present)]
    lsts = [np.ascontiguousarray(x, np.uint32) if x is not None and len(x) else np.zeros(1, np.uint32) for x in lists4]
    mats = np.ascontiguousarray(materials, I.MaterialData)
    entries = (MT.MtTexture * max(len(table), 1))()
    regions = np.zeros((max(len(table), 1), 2), np.uint32)
    for i, t in enumerate(table):
        if t is not None:
            entries[i] = t.c
            regions[i] = getattr(t, "region", (0, 0))
    limits = np.array([len(geo.instances), len(geo.meshData), len(geo.meshlets), len(geo.vertices), len(geo.vertexIds), len(geo.triangles), len(mats)]
                      + [len(r) if ok else 0 for r, ok in zip(recs, present)]
                      + [len(x) if x_in is not None and len(x_in) else 0 for x, x_in in zip(lsts, lists4)] + [len(table)], np.uint64)
    rp = (C.c_void_p * 4)(*[_p(r) for r in recs])
    lp = (C.c_void_p * 4)(*[_p(x) for x in lsts])
    lib.ts_gbuffer(_p(k), *geo.args(), C.addressof(rp), C.addressof(lp), _p(np.ascontiguousarray(vis, np.uint64)), _p(mats),
                   C.addressof(entries), _p(limits), _p(g), _p(m), _p(taps), _p(regions))
    return g, m, taps


class Residency:
    """The residency state of one streamable texture under the rule of tests/texture_streaming_ref.c: `resident` and `idle` per tile
    (levels 0 .. S - 1 one after the other, row-major), `min_mip` per region.  Starts with the packed tail alone."""
    def __init__(self, lib, width, height, mips, region, tile_bytes):
        self.lib = lib
        self.t = TsTiled(width, height, mips, region[0], region[1], tile_bytes)
        self.S = int(lib.ts_standard_levels(C.byref(self.t)))
        self.offsets = [int(lib.ts_tile_offset(C.byref(self.t), k)) for k in range(self.S + 1)]
        self.total = self.offsets[-1]
        self.resident = np.zeros(max(self.total, 1), np.uint8)
        self.idle = np.zeros(max(self.total, 1), np.uint32)
        self.regions = (width // region[0], height // region[1])
        self.min_mip = np.full((self.regions[1], self.regions[0]), self.S, np.uint8)

    def tiles(self, k):
        """(tiles x, tiles y) of standard level k."""
        return (self.t.width >> k) // self.t.regionW, (self.t.height >> k) // self.t.regionH

    def round(self, feedback, evict_after):
        """One processed feedback (uint8 [regions y, regions x]): (mapped, unmapped) bytes per tile and the statistics; min_mip is rewritten."""
        fb = np.ascontiguousarray(feedback, np.uint8)
        assert fb.shape == self.min_mip.shape, (fb.shape, self.min_mip.shape)
        mapped, unmapped, stats = np.zeros_like(self.resident), np.zeros_like(self.resident), TsStats()
        self.lib.ts_residency_round(C.byref(self.t), _p(fb), int(evict_after), _p(self.resident), _p(self.idle), _p(mapped), _p(unmapped),
                                    _p(self.min_mip), C.byref(stats))
        return mapped, unmapped, {n: int(getattr(stats, n)) for n, _ in TsStats._fields_}
