"""ctypes wrapper of tests/postprocess_ref.c, the test reference of "adaptluminance_CS_GenerateLuminanceHistogram",
"adaptluminance_CS_AdaptExposure" and "postprocess_PS_PostProcess" (csrc/k_postprocess.hip), and the constructed inputs the
CPU and the GPU tests share.

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C

import numpy as np

from ref_build import compile_ref
from toyrenderer_amd import interop as I

F = np.float32


def _declare(lib):
    for n in ("pr_log2_n", "pr_exp2_n", "pr_exp2_reduced_n", "pr_pow_gamma_n", "pr_luminance_n"):
        getattr(lib, n).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        getattr(lib, n).restype = None
    lib.pr_unpack_ufloat_n.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    lib.pr_bin_n.argtypes = [C.c_void_p, C.c_uint64, C.c_float, C.c_float, C.c_void_p]
    lib.pr_histogram.argtypes = [C.c_void_p, C.c_uint64, C.c_float, C.c_float, C.c_void_p]
    lib.pr_adapt_exposure.argtypes = [C.c_void_p] * 4
    lib.pr_post.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, C.c_void_p, C.c_void_p]
    lib.pr_tone_map_n.argtypes = [C.c_void_p, C.c_uint64]
    lib.pr_constants.argtypes = [C.c_void_p]
    for n in ("pr_unpack_ufloat_n", "pr_bin_n", "pr_histogram", "pr_adapt_exposure", "pr_post", "pr_tone_map_n", "pr_constants"):
        getattr(lib, n).restype = None


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "postprocess_ref", _declare)


def _p(a):
    return a.ctypes.data if a is not None else None


def bound(lib, name: str) -> float:
    """PR_LOG2_BOUND, PR_EXP2_BOUND, PR_POW_BOUND_A, PR_POW_BOUND_B of the source's error analyses."""
    return float(C.c_double.in_dll(lib, name).value)


def _map(fn, arr, in_dtype, out_dtype):
    a = np.ascontiguousarray(arr, in_dtype).reshape(-1)
    out = np.empty(len(a), out_dtype)
    fn(_p(a), len(a), _p(out))
    return out


def log2(lib, x): return _map(lib.pr_log2_n, x, F, F)
def exp2(lib, x): return _map(lib.pr_exp2_n, x, F, F)
def exp2_reduced(lib, x): return _map(lib.pr_exp2_reduced_n, x, F, F)
def pow_gamma(lib, x): return _map(lib.pr_pow_gamma_n, x, F, F)
def luminance(lib, words): return _map(lib.pr_luminance_n, words, np.uint32, F)


def unpack_ufloat(lib, codes, mbits: int) -> np.ndarray:
    c = np.ascontiguousarray(codes, np.uint32).reshape(-1)
    out = np.empty(len(c), F)
    lib.pr_unpack_ufloat_n(_p(c), len(c), mbits, _p(out))
    return out


def constants(lib) -> dict:
    out = np.zeros(8, F)
    lib.pr_constants(_p(out))
    return dict(zip(("lumR", "lumG", "lumB", "startCompression", "d", "dd", "desaturation", "invGamma"), out))


def tone_map(lib, rgb) -> np.ndarray:
    c = np.ascontiguousarray(rgb, F).reshape(-1, 3).copy()
    lib.pr_tone_map_n(_p(c), len(c))
    return c


# ---- the pass constants, as FrameDriver and the host mirror make them -------------------------------------------------------
def histogram_params(dims, min_luminance=0.004, max_luminance=12.0) -> np.ndarray:
    lo, hi = I.log_luminance_range(min_luminance, max_luminance)
    k = np.zeros(1, I.GenerateLuminanceHistogramParameters)
    k["m_SrcColorDims"] = dims
    k["m_MinLogLuminance"] = lo
    k["m_InverseLogLuminanceRange"] = F(1.0) / F(hi - lo)
    return k


def adapt_params(nb_pixels, speed, middle_gray=0.18, min_luminance=0.004, max_luminance=12.0) -> np.ndarray:
    lo, hi = I.log_luminance_range(min_luminance, max_luminance)
    k = np.zeros(1, I.AdaptExposureParameters)
    k["m_MinLogLuminance"] = lo
    k["m_LogLuminanceRange"] = F(hi - lo)
    k["m_AdaptationSpeed"] = speed
    k["m_NbPixels"] = nb_pixels
    k["m_MiddleGray"] = middle_gray
    return k


def post_params(dims, manual=0.0, middle_gray=0.18, bloom_strength=0.0) -> np.ndarray:
    k = np.zeros(1, I.PostProcessParameters)
    k["m_OutputDims"] = dims
    k["m_ManualExposure"] = manual
    k["m_MiddleGray"] = middle_gray
    k["m_BloomStrength"] = bloom_strength
    return k


# ---- the three passes -------------------------------------------------------------------------------------------------------
def bins(lib, words, k) -> np.ndarray:
    k = np.frombuffer(np.ascontiguousarray(k).tobytes(), I.GenerateLuminanceHistogramParameters)
    w = np.ascontiguousarray(words, np.uint32).reshape(-1)
    out = np.empty(len(w), np.uint32)
    lib.pr_bin_n(_p(w), len(w), float(k["m_MinLogLuminance"][0]), float(k["m_InverseLogLuminanceRange"][0]), _p(out))
    return out


def histogram(lib, words, k, init=None) -> np.ndarray:
    """u0 after the pass: init (default zeros) plus the counts of the image's bins, uint32[256]."""
    k = np.frombuffer(np.ascontiguousarray(k).tobytes(), I.GenerateLuminanceHistogramParameters)
    w = np.ascontiguousarray(words, np.uint32).reshape(-1)
    out = np.zeros(256, np.uint32) if init is None else np.ascontiguousarray(init, np.uint32)[:256].copy()
    lib.pr_histogram(_p(w), len(w), float(k["m_MinLogLuminance"][0]), float(k["m_InverseLogLuminanceRange"][0]), _p(out))
    return out


def adapt_exposure(lib, k, hist, luminance_in):
    """(luminance, exposure) after one CS_AdaptExposure, float32 scalars."""
    k = np.ascontiguousarray(np.frombuffer(np.ascontiguousarray(k).tobytes(), I.AdaptExposureParameters))
    h = np.ascontiguousarray(hist, np.uint32).reshape(-1)[:256]
    lum, exp = np.array([luminance_in], F), np.zeros(1, F)
    lib.pr_adapt_exposure(_p(k), _p(h), _p(lum), _p(exp))
    return lum[0], exp[0]


def post(lib, k, colour, *, bloom=None, luminance_in=1.0, want_srgb=False):
    """The back-buffer words (uint32, the shape of colour) and, when want_srgb, the float32 [..., 3] before the store."""
    k = np.ascontiguousarray(np.frombuffer(np.ascontiguousarray(k).tobytes(), I.PostProcessParameters))
    c = np.ascontiguousarray(colour, np.uint32)
    b = None if bloom is None else np.ascontiguousarray(bloom, np.uint32).reshape(c.shape)
    out = np.empty(c.shape, np.uint32)
    srgb = np.empty(c.shape + (3,), F) if want_srgb else None
    lib.pr_post(_p(k), _p(c), _p(b), c.size, float(F(luminance_in)), _p(out), _p(srgb))
    return (out, srgb) if want_srgb else out


# ---- constructed inputs shared by the CPU and the GPU tests -----------------------------------------------------------------
def grey(code: int) -> int:
    """The word whose three channels hold the 11-bit code's value, as far as blue's 10 bits can (code >> 1)."""
    return code | code << 11 | (code >> 1) << 22


def seeded_words(n: int, seed: int) -> np.ndarray:
    """Words over the whole format, NaN and infinity patterns included."""
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def seeded_finite_words(n: int, seed: int) -> np.ndarray:
    """Words whose three channels are finite (exponent < 31), spread over all exponents."""
    rng = np.random.default_rng(seed)
    r, g, b = rng.integers(0, 31 << 6, n), rng.integers(0, 31 << 6, n), rng.integers(0, 31 << 5, n)
    return (r | g << 11 | b << 22).astype(np.uint32)


SPECIAL_WORDS = np.array([0, 1, 1 << 11, 1 << 22, 0x3F | 0x3F << 11 | 0x1F << 22,            # zero, the smallest subnormals, the largest
                          0x7BF | 0x7BF << 11 | 0x3DF << 22,                                  # the largest finite
                          0x7C0 | 0x7C0 << 11 | 0x3E0 << 22, 0x7C0, 0x3E0 << 22,              # +inf in all, in red, in blue
                          0x7FF | 0x7FF << 11 | 0x3FF << 22, 0x7C1, 0x7FF << 11], np.uint32)  # NaN in all, in red, in green


def straddling_words(lib) -> np.ndarray:
    """Grey-ish words whose luminance lies on both sides of 0.005, the bin-0 test: green codes around the one whose value times
    0.71516 crosses it, with red and blue 0 and with a little red."""
    codes = np.arange(0, 31 << 6, dtype=np.uint32)
    lum = luminance(lib, codes << 11)
    j = int(np.searchsorted(lum, F(0.005)))
    near = codes[max(j - 8, 0):j + 8]
    return np.concatenate([near << 11, near << 11 | 1, near << 11 | 0x100])


ADAPT_HISTOGRAMS = {
    "all zero": (np.zeros(256, np.uint32), 640 * 360),
    "everything in bin 0": (np.bincount([0], minlength=256).astype(np.uint32) * np.uint32(640 * 360), 640 * 360),
    "one pixel in each bin": (np.ones(256, np.uint32), 256),
    "weighted sum wraps uint32": (np.bincount([255, 17], weights=[17_000_000, 123], minlength=256).astype(np.uint32), 17_000_123),
    "mid bins": (np.bincount([100, 101, 140], weights=[1000, 3000, 500], minlength=256).astype(np.uint32), 4500),
}
