"""ctypes wrapper of tests/lighting_ref.c, the test reference of "deferredlighting_PS_Main" and
"deferredlighting_PS_Main_Debug" (csrc/k_deferredlighting.hip).

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C

import numpy as np

from ref_build import compile_ref
from toyrenderer_amd import interop as I


def _declare(lib):
    lib.lr_lighting.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    lib.lr_lighting.restype = None
    lib.lr_pack_ufloat_n.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    lib.lr_pack_ufloat_n.restype = None
    for n in ("lr_exp2_n", "lr_unpack_unorm8_n", "lr_unpack_unorm16_n", "lr_unpack_oct_n", "lr_unpack_r9g9b9e5_n"):
        getattr(lib, n).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        getattr(lib, n).restype = None


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "lighting_ref", _declare)


def _p(a):
    return a.ctypes.data if a is not None else None


def exp2_bound(lib) -> float:
    """LR_EXP2_BOUND of the source's error analysis: absolute error of lr_exp2(x) over 2^ceil(x)."""
    return float(C.c_double.in_dll(lib, "LR_EXP2_BOUND").value)


def pack_ufloat(lib, values, mbits: int) -> np.ndarray:
    v = np.ascontiguousarray(values, np.float32).reshape(-1)
    out = np.empty(len(v), np.uint32)
    lib.lr_pack_ufloat_n(_p(v), len(v), mbits, _p(out))
    return out


def pack_r11g11b10(lib, rgb) -> np.ndarray:
    rgb = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    return pack_ufloat(lib, rgb[:, 0], 6) | pack_ufloat(lib, rgb[:, 1], 6) << np.uint32(11) | pack_ufloat(lib, rgb[:, 2], 5) << np.uint32(22)


def _map(fn, arr, in_dtype, out_dtype, out_width=1):
    a = np.ascontiguousarray(arr, in_dtype).reshape(-1)
    out = np.empty((len(a), out_width) if out_width > 1 else len(a), out_dtype)
    fn(_p(a), len(a), _p(out))
    return out


def exp2(lib, x): return _map(lib.lr_exp2_n, x, np.float32, np.float32)
def unpack_unorm8(lib, v): return _map(lib.lr_unpack_unorm8_n, v, np.uint32, np.float32)
def unpack_unorm16(lib, v): return _map(lib.lr_unpack_unorm16_n, v, np.uint32, np.float32)
def unpack_oct(lib, v): return _map(lib.lr_unpack_oct_n, v, np.uint32, np.float32, 3)
def unpack_r9g9b9e5(lib, v): return _map(lib.lr_unpack_r9g9b9e5_n, v, np.uint32, np.float32, 3)


def consts(clip_to_world, origin, light, strength, resolution, debug_mode=0, ssao_enabled=0) -> np.ndarray:
    k = np.zeros(1, I.DeferredLightingConsts)
    k["m_ClipToWorld"] = np.asarray(clip_to_world, np.float32).reshape(4, 4)
    k["m_CameraOrigin"] = origin
    k["m_SSAOEnabled"] = ssao_enabled
    k["m_DebugMode"] = debug_mode
    k["m_DirectionalLightVector"] = light
    k["m_DirectionalLightStrength"] = strength
    k["m_LightingOutputResolution"] = resolution
    return k


def lighting(lib, k, gbuffer, depth, *, debug=None, motion=None, ssao=None, shadow=None, out_init=None, want_rgb=False):
    """The pass over one image.  k: DeferredLightingConsts (1 element or 112 bytes); gbuffer uint32 [H, W, 4]; depth float32
    [H, W]; motion: the RG16_FLOAT texels as float16 [H, W, 2] or uint32 [H, W]; ssao / shadow uint8 [H, W] or None (unbound).
    debug: None = by m_DebugMode != 0.  Returns uint32 [H, W] words (texels with depth not > 0 keep out_init, default 0), and
    the float32 [H, W, 3] before the store when want_rgb (NaN where nothing was written)."""
    k = np.ascontiguousarray(np.frombuffer(np.ascontiguousarray(k).tobytes(), I.DeferredLightingConsts))
    W, H = (int(x) for x in k["m_LightingOutputResolution"][0])
    g = np.ascontiguousarray(gbuffer, np.uint32).reshape(H, W, 4)
    d = np.ascontiguousarray(depth, np.float32).reshape(H, W)
    if motion is not None:
        motion = np.ascontiguousarray(motion)
        motion = np.ascontiguousarray(motion.view(np.uint16).reshape(H, W, 2)).view(np.uint32).reshape(H, W) if motion.dtype != np.uint32 else motion.reshape(H, W)
    ssao = None if ssao is None else np.ascontiguousarray(ssao, np.uint8).reshape(H, W)
    shadow = None if shadow is None else np.ascontiguousarray(shadow, np.uint8).reshape(H, W)
    out = np.zeros((H, W), np.uint32) if out_init is None else np.ascontiguousarray(out_init, np.uint32).reshape(H, W).copy()
    rgb = np.full((H, W, 3), np.nan, np.float32) if want_rgb else None
    is_debug = bool(k["m_DebugMode"][0] != 0) if debug is None else bool(debug)
    lib.lr_lighting(_p(k), int(is_debug), _p(g), _p(motion), _p(d), _p(ssao), _p(shadow), _p(out), _p(rgb))
    return (out, rgb) if want_rgb else out
