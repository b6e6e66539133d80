"""ctypes wrapper of tests/bloom_ref.c, the test reference of "bloom_PS_Downsample" and "bloom_PS_Upsample"
(csrc/k_bloom.hip), the pass constants as FrameDriver and the host mirror make them, and the inputs the CPU and the GPU
tests share.

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C

import numpy as np

from ref_build import compile_ref
from toyrenderer_amd import interop as I

F = np.float32


def _declare(lib):
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    lib.bl_unpack_ufloat.argtypes = [u32, u32]
    lib.bl_unpack_ufloat.restype = f32
    lib.bl_pack_ufloat.argtypes = [f32, u32]
    lib.bl_pack_ufloat.restype = u32
    lib.bl_axis.argtypes = [f32, u32, vp]
    lib.bl_sample_n.argtypes = [vp, u32, u32, vp, u64, vp]
    lib.bl_downsample.argtypes = [vp, u32, u32, u32, u32, f32, f32, u32, vp, vp]
    lib.bl_upsample.argtypes = [vp, u32, u32, u32, u32, f32, vp, vp]
    lib.bl_chain.argtypes = [vp, u32, u32, u32, f32, vp]
    for n in ("bl_axis", "bl_sample_n", "bl_downsample", "bl_upsample", "bl_chain"):
        getattr(lib, n).restype = None


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "bloom_ref", _declare)


def _p(a):
    return a.ctypes.data if a is not None else None


def axis(lib, uv, dim: int):
    """(i0, i1, f) of one axis of the sampler."""
    out = np.zeros(3, np.uint32)
    lib.bl_axis(float(F(uv)), dim, _p(out))
    return int(out[0]), int(out[1]), out[2:3].view(F)[0]


def sample(lib, words, uv) -> np.ndarray:
    """SampleLevel(LinearClamp, uv, 0) of an (H, W) image of words at n coordinates (n, 2): float32 (n, 3)."""
    w = np.ascontiguousarray(words, np.uint32)
    uv = np.ascontiguousarray(uv, F).reshape(-1, 2)
    out = np.empty((len(uv), 3), F)
    lib.bl_sample_n(_p(w), w.shape[1], w.shape[0], _p(uv), len(uv), _p(out))
    return out


def half_dims(w: int, h: int):
    return max(w >> 1, 1), max(h >> 1, 1)


def downsample(lib, words, first: bool, *, dest=None, inv=None, want_rgb=False):
    """PS_Downsample of an (H, W) image into dest = (dW, dH) (default: (W >> 1, H >> 1), at least 1) with m_InvSourceResolution =
    inv (default: 1 / (W, H))."""
    w = np.ascontiguousarray(words, np.uint32)
    sH, sW = w.shape
    dW, dH = dest if dest is not None else half_dims(sW, sH)
    ix, iy = inv if inv is not None else (F(1.0) / F(sW), F(1.0) / F(sH))
    out = np.empty((dH, dW), np.uint32)
    rgb = np.empty((dH, dW, 3), F) if want_rgb else None
    lib.bl_downsample(_p(w), sW, sH, dW, dH, float(F(ix)), float(F(iy)), int(bool(first)), _p(out), _p(rgb))
    return (out, rgb) if want_rgb else out


def upsample(lib, words, radius, dest, want_rgb=False):
    """PS_Upsample of an (H, W) image into dest = (dW, dH)."""
    w = np.ascontiguousarray(words, np.uint32)
    sH, sW = w.shape
    dW, dH = dest
    out = np.empty((dH, dW), np.uint32)
    rgb = np.empty((dH, dW, 3), F) if want_rgb else None
    lib.bl_upsample(_p(w), sW, sH, dW, dH, float(F(radius)), _p(out), _p(rgb))
    return (out, rgb) if want_rgb else out


def chain_dims(W: int, H: int, mips: int):
    return [(W >> k, H >> k) for k in range(mips)]


def bloom_chain(lib, words, W: int, H: int, mips: int, radius) -> list:
    """Every mip of the bloom texture after BloomRenderer::Render on the colour image `words`: a list of (H >> k, W >> k) arrays."""
    c = np.ascontiguousarray(words, np.uint32).reshape(H, W)
    dims = chain_dims(W, H, mips)
    assert dims[-1][0] >= 1 and dims[-1][1] >= 1
    flat = np.zeros(sum(w * h for w, h in dims), np.uint32)
    lib.bl_chain(_p(c), W, H, mips, float(F(radius)), _p(flat))
    out, off = [], 0
    for w, h in dims:
        out.append(flat[off:off + w * h].reshape(h, w).copy())
        off += w * h
    return out


def pass_consts(W: int, H: int, mips: int, radius) -> np.ndarray:
    """The BloomConsts of the 2 * (mips - 1) passes, downsamples first, as BloomRenderer::Render fills them (fields a pass does
    not set are zero here: the reference leaves them uninitialised and its shaders do not read them)."""
    n = mips - 1
    k = np.zeros(2 * n, I.BloomConsts)
    for i in range(n):
        k[i]["m_InvSourceResolution"] = (F(1.0) / F(W >> i), F(1.0) / F(H >> i))
        k[i]["m_bIsFirstDownsample"] = int(i == 0)
        k[n + i]["m_FilterRadius"] = radius
    return k


def max_mips(W: int, H: int) -> int:
    """floor(log2(min(W, H))) + 1: the largest count whose last mip still has a texel in both axes."""
    return int(min(W, H)).bit_length()


# ---- inputs shared by the CPU and the GPU tests -------------------------------------------------------------------------------
def pack_words(lib, rgb) -> np.ndarray:
    """float32 [..., 3] -> words, through the reference's store."""
    rgb = np.ascontiguousarray(rgb, F)
    flat = rgb.reshape(-1, 3)
    out = np.empty(len(flat), np.uint32)
    for i, (r, g, b) in enumerate(flat):
        out[i] = lib.bl_pack_ufloat(float(r), 6) | lib.bl_pack_ufloat(float(g), 6) << 11 | lib.bl_pack_ufloat(float(b), 5) << 22
    return out.reshape(rgb.shape[:-1])


def seeded_words(W: int, H: int, seed: int) -> np.ndarray:
    """Words over the whole format, NaN and infinity patterns included."""
    return np.random.default_rng(seed).integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)


def seeded_finite_words(W: int, H: int, seed: int, top_exponent: int = 24) -> np.ndarray:
    """Words whose three channels are finite, exponents 0 .. top_exponent - 1 (24: values below 512, whose sums stay finite)."""
    rng = np.random.default_rng(seed)
    r, g, b = rng.integers(0, top_exponent << 6, (H, W)), rng.integers(0, top_exponent << 6, (H, W)), rng.integers(0, top_exponent << 5, (H, W))
    return (r | g << 11 | b << 22).astype(np.uint32)


INF_WORD = 0x7C0 | 0x7C0 << 11 | 0x3E0 << 22
NAN_WORD = 0x7FF | 0x7FF << 11 | 0x3FF << 22
MAX_FINITE_WORD = 0x7BF | 0x7BF << 11 | 0x3DF << 22
ONE_WORD = 0x3C0 | 0x3C0 << 11 | 0x1E0 << 22        # 1.0 in each channel


def special_images(W: int, H: int) -> dict:
    """Black; subnormal codes; the largest finite; +inf beside a finite texel; +inf beside +inf (NaN by the lerp: inf - inf); NaN
    codes.  Each an (H, W) image of words."""
    out = {"black": np.zeros((H, W), np.uint32)}
    sub = np.zeros((H, W), np.uint32)
    sub.ravel()[:] = [((i % 63) + 1) | ((i * 7 % 63) + 1) << 11 | ((i * 3 % 31) + 1) << 22 for i in range(W * H)]
    out["subnormal"] = sub
    out["largest finite"] = np.full((H, W), MAX_FINITE_WORD, np.uint32)
    one_inf = np.full((H, W), ONE_WORD, np.uint32)
    one_inf[H // 2, W // 2] = INF_WORD
    out["inf beside finite"] = one_inf
    two_inf = np.full((H, W), ONE_WORD, np.uint32)
    two_inf[H // 2, W // 2] = INF_WORD
    two_inf[H // 2, min(W // 2 + 1, W - 1)] = INF_WORD
    two_inf[min(H // 2 + 1, H - 1), W // 2] = INF_WORD
    out["inf beside inf"] = two_inf
    nan = np.full((H, W), ONE_WORD, np.uint32)
    nan[H // 2, W // 2] = NAN_WORD
    nan[0, 0] = 0x7C1                              # a NaN in red only
    out["nan"] = nan
    return out
