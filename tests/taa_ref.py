"""ctypes wrapper of tests/taa_ref.c, the definition of "taa_CS_TemporalResolve" (csrc/k_taa.hip), and the inputs the CPU and the
GPU tests share.

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C

import numpy as np

from ref_build import compile_ref
from toyrenderer_amd import interop as I
from toyrenderer_amd import taa as T

F = np.float32
VALID, CLAMPED, DILATED = 1, 2, 4                   # the path byte's low bits
W00, W10, W01, W11 = 16, 32, 64, 128                # the bilinear texels (x0, y0), (x1, y0), (x0, y1), (x1, y1) with a nonzero weight
WEIGHTS = W00 | W10 | W01 | W11


def _declare(lib):
    vp = C.c_void_p
    lib.taa_resolve.argtypes = [vp] * 8
    lib.taa_resolve.restype = None
    lib.taa_repack.argtypes = [vp, C.c_uint64, vp]
    lib.taa_repack.restype = None


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "taa_ref", _declare)


def consts(W, H, jitter_delta=(0.0, 0.0), min_blend=0.1, max_sample_count=64.0, reset=False) -> np.ndarray:
    k = np.zeros(1, I.TAAConsts)
    k["m_OutputDims"], k["m_JitterDelta"], k["m_MinBlend"], k["m_MaxSampleCount"], k["m_bResetHistory"] = (W, H), jitter_delta, min_blend, max_sample_count, int(reset)
    return k


def resolve(lib, k, colour, depth, motion, history):
    """One pass.  colour (H, W) words; depth (H, W) float32; motion (H, W, 2) float16 (or (H, W) words); history (H, W, 4)
    float16 (or uint16 bits).  Returns (new history (H, W, 4) uint16 bits, colour words (H, W), path bytes (H, W))."""
    W, H = (int(x) for x in k["m_OutputDims"][0])
    colour = np.ascontiguousarray(colour, np.uint32).reshape(H, W)
    depth = np.ascontiguousarray(depth, F).reshape(H, W)
    motion = np.ascontiguousarray(motion)
    motion = motion.view(np.uint32).reshape(H, W) if motion.dtype != np.uint32 else motion.reshape(H, W)
    history = np.ascontiguousarray(history).view(np.uint16).reshape(H, W, 4)
    kk = np.ascontiguousarray(k)
    new, out, path = np.empty((H, W, 4), np.uint16), np.empty((H, W), np.uint32), np.empty((H, W), np.uint8)
    lib.taa_resolve(kk.ctypes.data, colour.ctypes.data, depth.ctypes.data, motion.ctypes.data, history.ctypes.data, new.ctypes.data, out.ctypes.data, path.ctypes.data)
    return new, out, path


def repack(lib, words) -> np.ndarray:
    """Colour words loaded and stored again: what a pass that copies a colour writes (a NaN channel becomes the one NaN code)."""
    w = np.ascontiguousarray(words, np.uint32)
    out = np.empty_like(w)
    lib.taa_repack(w.ctypes.data, w.size, out.ctypes.data)
    return out


def halves(x) -> np.ndarray:
    """float values -> binary16 bits (numpy rounds to nearest even, as the reference's store does for a number)."""
    return np.asarray(x, F).astype(np.float16).view(np.uint16)


def motion_of(mx, my, W=None, H=None) -> np.ndarray:
    """An (H, W, 2) float16 motion image from two scalars or (H, W) arrays."""
    if W is not None:
        mx, my = np.full((H, W), mx, F), np.full((H, W), my, F)
    return np.stack([np.asarray(mx, F), np.asarray(my, F)], -1).astype(np.float16)


# ---- inputs shared by the CPU and the GPU tests -------------------------------------------------------------------------------
def seeded_inputs(W, H, seed, finite_history=False):
    """(colour, depth, motion, history) over the whole of every format: colour words with the NaN and infinity codes; depths in
    [0, 1) with runs of equal values (ties) and a few NaN; motion up to +-3 pixels with fractional parts; history bits over the
    whole of binary16 (negative, infinite and NaN values included) unless finite_history, then colours in [0, 8) and counts in
    [0, 80)."""
    rng = np.random.default_rng(seed)
    colour = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    depth = (rng.integers(0, 6, (H, W)) / 8.0).astype(F)
    depth[rng.random((H, W)) < 0.02] = np.nan
    motion = (rng.integers(-3 * 64, 3 * 64 + 1, (H, W, 2)) / 64.0).astype(np.float16)
    if finite_history:
        history = np.concatenate([rng.random((H, W, 3)) * 8.0, rng.random((H, W, 1)) * 80.0], -1).astype(np.float16).view(np.uint16)
    else:
        history = rng.integers(0, 1 << 16, (H, W, 4), dtype=np.uint32).astype(np.uint16)
    return colour, depth, motion, history


def finite_colour(W, H, seed, top_exponent=20) -> np.ndarray:
    """Colour words with finite channels below 2^(top_exponent - 15)."""
    rng = np.random.default_rng(seed)
    r, g, b = rng.integers(0, top_exponent << 6, (H, W)), rng.integers(0, top_exponent << 6, (H, W)), rng.integers(0, top_exponent << 5, (H, W))
    return (r | g << 11 | b << 22).astype(np.uint32)


def history_of(words, count) -> np.ndarray:
    """The history texture that holds the colours of an (H, W) image of R11G11B10 words (every one a binary16 number) with a
    constant count: (H, W, 4) uint16 bits."""
    w = np.asarray(words, np.uint32)

    def chan(c, mbits):
        e, m = c >> mbits, c & ((1 << mbits) - 1)
        return np.where(e == 0, m * 2.0 ** (-14 - mbits), (1 + m / 2.0 ** mbits) * 2.0 ** (e.astype(np.float64) - 15))
    rgb = np.stack([chan(w & 0x7FF, 6), chan((w >> 11) & 0x7FF, 6), chan(w >> 22, 5), np.full(w.shape, float(count))], -1)
    return rgb.astype(np.float16).view(np.uint16)


ONE_WORD = 0x3C0 | 0x3C0 << 11 | 0x1E0 << 22        # 1.0 in each channel
INF_WORD = 0x7C0 | 0x7C0 << 11 | 0x3E0 << 22
NAN_WORD = 0x7FF | 0x7FF << 11 | 0x3FF << 22


def constructed_cases(W, H):
    """name -> (consts, colour, depth, motion, history): cases 3 to 7 of tests/test_taa_ref.py at one size, for the GPU to repeat.
    Needs W, H >= 4."""
    rng = np.random.default_rng(7 * W + H)
    flat = np.full((H, W), 0.25, F)
    colour = finite_colour(W, H, 3)
    out = {}
    # 3. history outside and inside the neighbourhood box
    hist = history_of(colour, 3)
    outside = hist.copy()
    outside[::2, ::2, :3] = halves(40.0)
    out["clamp"] = (consts(W, H), colour, flat, motion_of(0.0, 0.0, W, H), outside)
    # 4. whole-pixel shifts and motion equal to the jitter delta
    out["shift"] = (consts(W, H), colour, flat, motion_of(-2.0, 1.0, W, H), hist)
    out["jitter delta"] = (consts(W, H, jitter_delta=(0.375, -0.25)), colour, flat, motion_of(0.375, -0.25, W, H), hist)
    # 5. motion that leaves the image on each side, and lands exactly on 0 and on W
    mx, my = np.zeros((H, W), F), np.zeros((H, W), F)
    mx[0, :] = -(np.arange(W) + 0.5)                                                                 # hp.x = 0: valid
    mx[1, :] = W - (np.arange(W) + 0.5)                                                              # hp.x = W: invalid
    mx[2, :] = -(np.arange(W) + 1.0)                                                                 # hp.x = -0.5
    my[3, :] = H                                                                                     # below the image
    my[:, 0] = np.where(np.arange(H) > 3, -(np.arange(H) + 1.0), my[:, 0])                           # above the image
    out["leaving"] = (consts(W, H), colour, flat, motion_of(mx, my), hist)
    # 6. a one-pixel foreground with its own motion on a static background; a tie keeps the centre
    depth = flat.copy()
    depth[H // 2, W // 2] = 0.75                                                                     # everywhere else the nine depths are equal: ties
    mx, my = np.zeros((H, W), F), np.zeros((H, W), F)
    mx[H // 2, W // 2], my[H // 2, W // 2] = 1.5, -0.75
    out["dilation"] = (consts(W, H), colour, depth, motion_of(mx, my), hist)
    # 7. NaN and infinity in the history, the motion and the colour
    bad = hist.copy()
    for i, bits in enumerate((0x7C00, 0xFC00, 0x7E00, 0x7C01)):
        bad[i % H, (2 * i) % W, i % 4] = bits
    m = motion_of(0.0, 0.0, W, H)
    m[H - 1, W - 1, 0] = np.nan
    m[H - 1, 0, 1] = np.inf
    special = colour.copy()
    special[H - 2, 1], special[H - 2, W - 2] = INF_WORD, NAN_WORD
    out["not finite"] = (consts(W, H), special, flat, m, bad)
    out["fractional"] = (consts(W, H, jitter_delta=(0.125, 0.0625)), colour, (rng.integers(0, 4, (H, W)) / 4.0).astype(F),
                         (rng.integers(-96, 97, (H, W, 2)) / 64.0).astype(np.float16), hist)
    return out


def jitter_sequence(n):
    return [T.jitter_offset(i) for i in range(n)]
