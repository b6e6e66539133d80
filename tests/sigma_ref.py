"""ctypes wrapper of tests/sigma_ref.c, the definition of the sun shadow denoiser and of what feeds it: the penumbra trace and the
normal / roughness pack (csrc/k_shadowmask.hip), the tile classification, the two blur passes and the temporal stabilisation
(csrc/k_sigma.hip); and denoise(), the chain of one frame in the order the driver records it.

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C

import numpy as np

import alpha_test_ref as AT
from ref_build import compile_ref
import shadowmask_ref as SR
from toyrenderer_amd import accel
from toyrenderer_amd import interop as I

F = np.float32
BRUTE, WALK = SR.BRUTE, SR.WALK
SENTINEL16 = SR.SENTINEL16                         # pre-fill of a binary16 target: a NaN word no pass stores
SENTINEL32 = 0xFE5AFE5B                            # pre-fill of an RG16_FLOAT or R10G10B10A2_UNORM target
SENTINEL8 = SR.SENTINEL8
NO_OCCLUDER = 0x7BFF
PATH_FILTERED, PATH_CAPPED, PATH_HISTORY, PATH_CLAMPED = 1, 2, 4, 8


def _declare(lib):
    SR._declare(lib); AT._declare(lib)              # the two references the C file includes: the library serves as theirs too
    vp, u32, i64 = C.c_void_p, C.c_uint32, C.c_int64
    lib.sg_consts_size.restype = u32
    lib.sg_pack_penumbra.argtypes = [C.c_int, C.c_float, C.c_float]
    lib.sg_pack_penumbra.restype = C.c_uint16
    lib.sg_trace_penumbra.argtypes = [vp, C.POINTER(SR._Scene), vp, i64, vp, vp, vp, C.c_int, vp, vp, vp]
    lib.sg_trace_penumbra.restype = None
    lib.sg_pack_normal_roughness.argtypes = [u32, u32, vp, vp]
    lib.sg_pack_normal_roughness.restype = None
    lib.sg_decode_normal.argtypes = [u32, vp]
    lib.sg_decode_normal.restype = None
    lib.sg_classify.argtypes = [vp] * 5
    lib.sg_classify.restype = None
    lib.sg_blur.argtypes = [vp] * 8
    lib.sg_blur.restype = None
    lib.sg_stabilize.argtypes = [vp] * 10
    lib.sg_stabilize.restype = None
    assert lib.sg_consts_size() == I.SigmaConsts.itemsize


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "sigma_ref", _declare, include_oracle=True)


def trace_penumbra(lib, k, acc: SR.Accel, depth, gbuffer, noise, mode, textures=None, instances=None, nodes=None, records=None, penumbra=None, lvd=None):
    """The trace with m_bDoDenoising != 0 over one image: (penumbra words uint16 [H, W], linear view depth words uint16 [H, W], t
    float32 [H, W], 1e10 where nothing commits).  mode BRUTE is the definition; WALK walks `nodes` / `records` (default: the refit
    of `instances`).  textures: the table of tests/alpha_test_ref.py, None = no table."""
    sc = acc.scene
    k = np.ascontiguousarray(k, I.ShadowMaskConsts)
    W, H = (int(x) for x in k["m_OutputResolution"][0])
    inst = np.ascontiguousarray(sc["instances"] if instances is None else instances, I.BasePassInstanceConstants)
    if mode == WALK and nodes is None:
        nodes, records = SR.refit(lib, acc, inst)
    if nodes is None:
        nodes, records = acc.tlas["nodes"], acc.tlas["records"]
    s, keep = SR._scene(acc, inst, nodes, records)
    depth = np.ascontiguousarray(depth, F).reshape(H, W)
    g = np.ascontiguousarray(gbuffer, np.uint32).reshape(H, W, 4)
    nz = np.ascontiguousarray(accel.noise_words(noise))
    penumbra = np.full((H, W), SENTINEL16, np.uint16) if penumbra is None else np.ascontiguousarray(penumbra, np.uint16).copy()
    lvd = np.full((H, W), SENTINEL16, np.uint16) if lvd is None else np.ascontiguousarray(lvd, np.uint16).copy()
    t = np.zeros((H, W), F)
    table, made = AT.table_of(textures if textures is not None else [])
    lib.sg_trace_penumbra(k.ctypes.data, C.byref(s), C.addressof(table) if textures is not None else None, len(textures) if textures is not None else -1,
                          depth.ctypes.data, g.ctypes.data, nz.ctypes.data, mode, penumbra.ctypes.data, lvd.ctypes.data, t.ctypes.data)
    del made, keep
    return penumbra, lvd, t


def pack_normal_roughness(lib, gbuffer) -> np.ndarray:
    g = np.ascontiguousarray(gbuffer, np.uint32)
    H, W = g.shape[:2]
    out = np.zeros((H, W), np.uint32)
    lib.sg_pack_normal_roughness(W, H, g.ctypes.data, out.ctypes.data)
    return out


def decode_normal(lib, word) -> np.ndarray:
    """The normal the blur reads from one normal roughness word: float32 [3]."""
    out = np.zeros(3, F)
    lib.sg_decode_normal(int(word), out.ctypes.data)
    return out


def pack_penumbra(lib, occluded, t, tan_sun_angular_radius) -> int:
    return int(lib.sg_pack_penumbra(int(bool(occluded)), C.c_float(float(t)), C.c_float(float(tan_sun_angular_radius))))


def _dims(k):
    k = np.ascontiguousarray(k, I.SigmaConsts)
    W, H = (int(x) for x in k["m_OutputDims"][0])
    return k, W, H


def with_pass(k, pass_index):
    k = np.ascontiguousarray(k, I.SigmaConsts).copy()
    k["m_Pass"] = pass_index
    return k


def classify(lib, k, penumbra, lvd):
    """(tiles uint8 [ceil(H / 16), ceil(W / 16)], shadow data uint32 [H, W]: x in the low half)."""
    k, W, H = _dims(k)
    p, z = np.ascontiguousarray(penumbra, np.uint16).reshape(H, W), np.ascontiguousarray(lvd, np.uint16).reshape(H, W)
    tw, th = accel.sigma_tiles(W, H)
    tiles, data = np.full((th, tw), SENTINEL8, np.uint8), np.full((H, W), SENTINEL32, np.uint32)
    lib.sg_classify(k.ctypes.data, p.ctypes.data, z.ctypes.data, tiles.ctypes.data, data.ctypes.data)
    return tiles, data


def blur(lib, k, data, lvd, depth, normal_roughness, tiles, path=None):
    """One blur pass (k's m_Pass): shadow data out uint32 [H, W].  path: uint8 [H, W], OR-ed into."""
    k, W, H = _dims(k)
    d, z = np.ascontiguousarray(data, np.uint32).reshape(H, W), np.ascontiguousarray(lvd, np.uint16).reshape(H, W)
    dp, nr = np.ascontiguousarray(depth, F).reshape(H, W), np.ascontiguousarray(normal_roughness, np.uint32).reshape(H, W)
    t = np.ascontiguousarray(tiles, np.uint8)
    assert t.shape == accel.sigma_tiles(W, H)[::-1], t.shape
    out = np.full((H, W), SENTINEL32, np.uint32)
    assert path is None or (path.dtype == np.uint8 and path.shape == (H, W) and path.flags.c_contiguous)
    lib.sg_blur(k.ctypes.data, d.ctypes.data, z.ctypes.data, dp.ctypes.data, nr.ctypes.data, t.ctypes.data, out.ctypes.data, None if path is None else path.ctypes.data)
    return out


def stabilize(lib, k, data, lvd, motion, history, tiles, path=None):
    """(new history words uint16 [H, W], mask uint8 [H, W], texels of `history` read)."""
    k, W, H = _dims(k)
    d, z = np.ascontiguousarray(data, np.uint32).reshape(H, W), np.ascontiguousarray(lvd, np.uint16).reshape(H, W)
    mv, h = np.ascontiguousarray(motion, np.uint32).reshape(H, W), np.ascontiguousarray(history, np.uint16).reshape(H, W)
    t = np.ascontiguousarray(tiles, np.uint8)
    assert t.shape == accel.sigma_tiles(W, H)[::-1], t.shape
    new, mask = np.full((H, W), SENTINEL16, np.uint16), np.full((H, W), SENTINEL8, np.uint8)
    reads = np.zeros(1, np.uint64)
    assert path is None or (path.dtype == np.uint8 and path.shape == (H, W) and path.flags.c_contiguous)
    lib.sg_stabilize(k.ctypes.data, d.ctypes.data, z.ctypes.data, mv.ctypes.data, h.ctypes.data, t.ctypes.data, new.ctypes.data, mask.ctypes.data,
                     None if path is None else path.ctypes.data, reads.ctypes.data)
    return new, mask, int(reads[0])


def denoise(lib, k, penumbra, lvd, depth, gbuffer, motion, history):
    """The chain of one frame: pack, classify, blur, post-blur, stabilisation.  A dict of every intermediate and output: normal_roughness,
    tiles, data0 (after classify), data1 (after blur), data2 (after post-blur, in shadow data 0 again), history, mask, path, reads."""
    nr = pack_normal_roughness(lib, gbuffer)
    tiles, data0 = classify(lib, k, penumbra, lvd)
    path = np.zeros(data0.shape, np.uint8)
    data1 = blur(lib, with_pass(k, 0), data0, lvd, depth, nr, tiles, path)
    data2 = blur(lib, with_pass(k, 1), data1, lvd, depth, nr, tiles, path)
    new, mask, reads = stabilize(lib, k, data2, lvd, motion, history, tiles, path)
    return dict(normal_roughness=nr, tiles=tiles, data0=data0, data1=data1, data2=data2, history=new, mask=mask, path=path, reads=reads)
