"""Plain numpy reference of the HZB build and of the footprint-min table derived from it.

Written from the rules, not from any implementation of them:
  * mip 0: minmaxdownsample.hlsl:10-35 -- uv = (tid + 0.5) / outDim in fp32, Gather with a point-clamp sampler = the 2 x 2
    quad floor(uv * dim - 0.5) + {0, 1} clamped to the edge, Min4 / Max4, store to R16_FLOAT (round to nearest even);
  * mips 1..N-1: the SPD rule as DESIGN.md and oracle/tr_oracle.h state it -- a texel of mip k+1 is the min (max) of the
    2 x 2 block of mip k, source indices clamped to the edge where a dimension has run out (2 x 1 / 1 x 2 blocks);
  * table: the header comment of toyrenderer_amd/csrc/hzb_quad.hip.h -- entry (X, Y) of mip k, X in [0, w_k], Y in [0, h_k],
    is the min over {clamp(X-1), clamp(X)} x {clamp(Y-1), clamp(Y)}, and sits at
    quadOffset[k] + ((Y >> 3) * blocksPerRow + (X >> 3)) * 64 + (Y & 7) * 8 + (X & 7), blocksPerRow = (w_k >> 3) + 1.

Used by tests/test_hzb_ref.py (CPU: ties this file to the oracle) and tests/test_gpu_hzb.py (GPU: the kernels against it).

Value classes: min / max are np.fmin / np.fmax (minNum / maxNum: a quiet NaN loses against a number, NaN only from all-NaN).
-0.0 and signalling NaNs are outside the reference: minNum does not order the zeros, and what a signalling NaN becomes
depends on the IEEE mode of the wave; neither the HLSL nor the oracle defines them.
"""
from __future__ import annotations

import numpy as np


def mip_dims(w: int, h: int, k: int):
    return max(w >> k, 1), max(h >> k, 1)


def num_mips(w: int, h: int) -> int:
    return int(max(w, h)).bit_length()


def gather_index_fp32(out_dim: int, src_dim: int) -> np.ndarray:
    """floor(fma((x + 0.5) / out_dim, src_dim, -0.5)) for x = 0 .. out_dim-1, every operation in fp32 (int64 result, unclamped).
    The fma is ONE rounding of the exact value: the fp32 quotient (24 bits) times src_dim (< 2^24) minus 0.5 is exact in fp64
    (< 53 significant bits for every src_dim below 2^24 and out_dim below 2^24), and is then rounded once to fp32."""
    x = np.arange(out_dim, dtype=np.float32) + np.float32(0.5)
    u = x / np.float32(out_dim)                                         # fp32 division, correctly rounded
    exact = u.astype(np.float64) * np.float64(src_dim) - 0.5            # exact (see above)
    return np.floor(exact.astype(np.float32)).astype(np.int64)


def gather_index_exact(out_dim: int, src_dim: int) -> np.ndarray:
    """The same index in exact arithmetic: floor(((2x + 1) * src_dim - out_dim) / (2 * out_dim))."""
    x = np.arange(out_dim, dtype=np.int64)
    return ((2 * x + 1) * src_dim - out_dim) // (2 * out_dim)


def gather_indices(out_dim: int, src_dim: int):
    """(i0, i1, raw): the two clamped source indices per output texel and the unclamped floor."""
    raw = gather_index_fp32(out_dim, src_dim)
    return np.clip(raw, 0, src_dim - 1), np.clip(raw + 1, 0, src_dim - 1), raw


def _red(maximum: bool):
    return np.fmax if maximum else np.fmin


def mip0(depth: np.ndarray, ow: int, oh: int, maximum: bool = False) -> np.ndarray:
    """depth: float32 [H, W] -> float16 [oh, ow]."""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    x0, x1, _ = gather_indices(ow, W)
    y0, y1, _ = gather_indices(oh, H)
    f = _red(maximum)
    top = f(depth[np.ix_(y0, x0)], depth[np.ix_(y0, x1)])
    bot = f(depth[np.ix_(y1, x0)], depth[np.ix_(y1, x1)])
    with np.errstate(over="ignore"):
        return f(top, bot).astype(np.float16)                           # RNE; above 65519.996 -> inf


def chain(m0: np.ndarray, w: int, h: int, maximum: bool = False) -> list:
    """m0: float16 [h, w] -> list of float16 mips [h_k, w_k], k = 0 .. num_mips-1 (min / max of halves is exact)."""
    m0 = np.asarray(m0, np.float16)
    assert m0.shape == (h, w)
    f = _red(maximum)
    out = [m0]
    for k in range(1, num_mips(w, h)):
        p = out[-1]
        ph, pw = p.shape
        mw, mh = mip_dims(w, h, k)
        xa, xb = np.minimum(2 * np.arange(mw), pw - 1), np.minimum(2 * np.arange(mw) + 1, pw - 1)
        ya, yb = np.minimum(2 * np.arange(mh), ph - 1), np.minimum(2 * np.arange(mh) + 1, ph - 1)
        out.append(f(f(p[np.ix_(ya, xa)], p[np.ix_(ya, xb)]), f(p[np.ix_(yb, xa)], p[np.ix_(yb, xb)])))
    return out


def build(depth: np.ndarray, w: int, h: int, maximum: bool = False) -> list:
    return chain(mip0(depth, w, h, maximum), w, h, maximum)


def pack(mips: list) -> np.ndarray:
    """The packed chain as uint16 words (mips back to back, row-major: Texture.download_chain / HzbTexture.texels)."""
    return np.concatenate([np.ascontiguousarray(m, np.float16).view(np.uint16).ravel() for m in mips])


def unpack(words: np.ndarray, w: int, h: int) -> list:
    out, o = [], 0
    for k in range(num_mips(w, h)):
        mw, mh = mip_dims(w, h, k)
        out.append(np.asarray(words[o:o + mw * mh], np.uint16).view(np.float16).reshape(mh, mw))
        o += mw * mh
    assert o == len(words)
    return out


def same_words(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """Element-wise equality of fp16 words; a NaN equals any NaN (HLSL leaves payload and sign of a NaN result open)."""
    got, ref = np.asarray(got, np.uint16), np.asarray(ref, np.uint16)
    nan_g, nan_r = (got & 0x7FFF) > 0x7C00, (ref & 0x7FFF) > 0x7C00
    return (got == ref) | (nan_g & nan_r)


# ---- footprint-min table ---------------------------------------------------------------------------------------------------
def table(mips: list, w: int, h: int) -> list:
    """Per mip k a float16 array [h_k + 1, w_k + 1]: entry [Y, X] = min of texels {clamp(X-1), clamp(X)} x {clamp(Y-1), clamp(Y)}."""
    out = []
    for k, t in enumerate(mips):
        mw, mh = mip_dims(w, h, k)
        assert t.shape == (mh, mw)
        X, Y = np.arange(mw + 1), np.arange(mh + 1)
        xa, xb = np.clip(X - 1, 0, mw - 1), np.clip(X, 0, mw - 1)
        ya, yb = np.clip(Y - 1, 0, mh - 1), np.clip(Y, 0, mh - 1)
        out.append(np.fmin(np.fmin(t[np.ix_(ya, xa)], t[np.ix_(ya, xb)]), np.fmin(t[np.ix_(yb, xa)], t[np.ix_(yb, xb)])))
    return out


def table_layout(w: int, h: int):
    """(quadOffset per mip, total entries): mip k has ((w_k >> 3) + 1) * ((h_k >> 3) + 1) blocks of 64 entries."""
    offs, total = [], 0
    for k in range(num_mips(w, h)):
        mw, mh = mip_dims(w, h, k)
        offs.append(total)
        total += ((mw >> 3) + 1) * ((mh >> 3) + 1) * 64
    return offs, total


def table_index(X, Y, k: int, w: int, h: int):
    """Position of entry (X, Y) of mip k in the blocked layout (X, Y: ints or int arrays)."""
    mw, _ = mip_dims(w, h, k)
    bpr = (mw >> 3) + 1
    return table_layout(w, h)[0][k] + ((Y >> 3) * bpr + (X >> 3)) * 64 + (Y & 7) * 8 + (X & 7)


def table_packed(mips: list, w: int, h: int):
    """(words uint16 [total], defined bool [total]): the table as it lies in memory; padding entries are not defined."""
    offs, total = table_layout(w, h)
    words, defined = np.zeros(total, np.uint16), np.zeros(total, bool)
    for k, e in enumerate(table(mips, w, h)):
        Y, X = np.meshgrid(np.arange(e.shape[0]), np.arange(e.shape[1]), indexing="ij")
        idx = table_index(X, Y, k, w, h)
        assert not defined[idx].any() and idx.max() < (offs[k + 1] if k + 1 < len(offs) else total)
        words[idx] = np.ascontiguousarray(e).view(np.uint16)
        defined[idx] = True
    return words, defined


# ---- test images ---------------------------------------------------------------------------------------------------------------
def all_halves() -> np.ndarray:
    """The 63 488 finite halves and +-inf as uint16 words, -0.0 left out (see the module docstring): 63 489 words."""
    h = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    return h[((h & 0x7FFF) <= 0x7C00) & (h != 0x8000)]


def half_midpoints() -> np.ndarray:
    """fp32 midpoints between adjacent non-negative halves (subnormals included; the last one is 65520 = (65504 + 65536) / 2)."""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    nxt = np.append(h[1:], 65536.0)
    return ((h + nxt) / 2).astype(np.float32)                           # 12 significant bits at most: exact in fp32


def hostile_depth(W: int, H: int, seed: int) -> np.ndarray:
    """float32 [H, W]: [0, 1) noise with, scattered over it, exact half midpoints +- 1 fp32 ulp (normal and subnormal, both
    signs), 65504 / 65519.996 / 65520 / 1e30, negatives, +-inf, all-NaN 2 x 2 blocks and single quiet NaNs among numbers.
    No -0.0 (the noise's zeros are +0.0), no negative of magnitude <= 2^-25 (it would be stored as -0.0 and meet +0.0 in the next
    mip's min: the same undefined order) and no signalling NaN."""
    rng = np.random.default_rng(seed)
    d = rng.random((H, W), np.float32) ** 6
    d[rng.random(d.shape) < 0.2] = 0.0
    n = W * H
    flat = d.reshape(-1)
    mid = half_midpoints()
    mid = np.concatenate([mid[:2048], mid[rng.integers(0, len(mid), 4096)], mid[-4:]])      # every subnormal + first normals, a sample, the top
    trio = np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))])
    special = np.concatenate([trio, -trio[trio > 0],
                              np.array([65504.0, 65519.996, 65520.0, 1e30, -65504.0, -65520.0, -1e30, np.inf, -np.inf] * 8, np.float32),
                              -rng.random(256, np.float32), np.full(64, np.nan, np.float32)]).astype(np.float32)
    special = special[~(np.signbit(special) & (np.abs(special) <= np.float32(2.0 ** -25)))]   # would be STORED as -0.0 (a tie or below half the smallest subnormal)
    take = min(len(special), max(n // 3, 1))
    pos = rng.choice(n, take, replace=False)
    flat[pos] = rng.permutation(special)[:take]
    if W >= 2 and H >= 2:
        # blocks large enough for whole gather footprints (and for 2 x 2 blocks of the mips above): all NaN; +inf with one quiet
        # NaN inside (a min that must come out as inf, not NaN); 65520 (finite in fp32, inf once stored); -inf
        for _ in range(max(1, n // 8192)):
            for fill in (np.nan, np.inf, 65520.0, -np.inf):
                s = 4 * int(rng.integers(1, 4))
                y, x = int(rng.integers(0, max(H - s + 1, 1))), int(rng.integers(0, max(W - s + 1, 1)))
                d[y:y + s, x:x + s] = fill
                if fill == np.inf:
                    d[y + min(1, H - 1), x + min(2, W - 1)] = np.nan
    return d
