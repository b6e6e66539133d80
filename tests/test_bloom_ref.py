"""tests/bloom_ref.c, the reference the GPU tests compare "bloom_PS_Downsample" and "bloom_PS_Upsample" with word for word,
pinned by means other than itself: the sampler on constructed coordinates, constant images (exact), impulses in exact rationals,
a numpy float64 restatement of bloom.hlsl with a derived band, special inputs word by word, a g++ probe for the layout, the pass
constants written out, and the registry and facade refusals.  No GPU."""
import math
import os
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bloom_ref as BR  # noqa: E402
from ref_build import layout_probe  # noqa: E402
from suite_support import bl  # noqa: E402, F401
from toyrenderer_amd import interop as I  # noqa: E402

F = np.float32
U = 2.0 ** -24                                                   # binary32 unit roundoff
LUM = (float(F(0.212671)), float(F(0.715160)), float(F(0.072169)))
FLOOR = float(F(0.0001))


# ---- the format in numpy float64 and in exact rationals ---------------------------------------------------------------------
def decode64(code, m):
    code = np.asarray(code, np.int64)
    e, f = code >> m, code & ((1 << m) - 1)
    with np.errstate(over="ignore"):
        v = np.where(e == 0, f * 2.0 ** (-14 - m), (1.0 + f / float(1 << m)) * 2.0 ** (e.astype(np.float64) - 15))
    return np.where(e == 31, np.where(f == 0, np.inf, np.nan), v)


def encode64(v, m):
    """Round to nearest even into the format: NaN -> the NaN code, <= 0 -> 0, +inf -> inf, overflow -> the largest finite."""
    v = np.asarray(v, np.float64)
    safe = np.where(np.isfinite(v) & (v > 0), v, 1.0)
    E = np.frexp(safe)[1] - 1
    sub = E < -14
    q = np.rint(np.ldexp(safe, np.where(sub, 14 + m, m - E))).astype(np.int64)
    code = np.where(sub, q, ((E + 15).astype(np.int64) << m) + q - (1 << m))
    code = np.minimum(code, (31 << m) - 1)
    code = np.where(v > 0, code, 0)
    code = np.where(np.isposinf(v), 31 << m, code)
    return np.where(np.isnan(v), (32 << m) - 1, code)


def decode_words(words):
    w = np.asarray(words, np.uint32).astype(np.int64)
    return np.stack([decode64(w & 0x7FF, 6), decode64((w >> 11) & 0x7FF, 6), decode64(w >> 22, 5)], axis=-1)


def codes_of_words(words):
    w = np.asarray(words, np.uint32).astype(np.int64)
    return np.stack([w & 0x7FF, (w >> 11) & 0x7FF, w >> 22], axis=-1)


def encode_words(rgb):
    return (encode64(rgb[..., 0], 6) | encode64(rgb[..., 1], 6) << 11 | encode64(rgb[..., 2], 5) << 22).astype(np.uint32)


def boundary_distance(v, m):
    """The distance of v >= 0 to the nearest value at which the store's result changes (a midpoint of neighbouring codes); inf where
    there is none on a side (below code 0; above the largest finite, which overflow clamps to)."""
    c = encode64(v, m)
    top = (31 << m) - 1
    here = decode64(c, m)
    below = np.where(c > 0, (here + decode64(np.maximum(c - 1, 0), m)) / 2, -np.inf)
    above = np.where(c < top, (here + decode64(np.minimum(c + 1, top), m)) / 2, np.inf)
    return np.minimum(v - below, above - v)


def round_fraction(x: Fraction, m: int) -> int:
    """x >= 0 rounded once, to nearest even, into the format (exact arithmetic)."""
    if x == 0:
        return 0
    e = math.floor(math.log2(x))
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    scale = Fraction(2) ** (14 + m) if e < -14 else Fraction(2) ** (m - e)
    q = x * scale
    n = math.floor(q)
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2):
        n += 1
    code = n if e < -14 else ((e + 15) << m) + n - (1 << m)
    return min(code, (31 << m) - 1)


def test_the_numpy_store_is_the_reference_store(bl):
    """encode64 / decode64 (used below) against the C reference's load and store on every code and on seeded values."""
    for m in (6, 5):
        codes = np.arange(31 << m)
        vals = decode64(codes, m)
        assert all(bl.bl_unpack_ufloat(int(c), m) == v for c, v in zip(codes, vals))
        assert np.array_equal(encode64(vals, m), codes)
        rng = np.random.default_rng(5)
        x = np.exp(rng.normal(0, 6, 4000)).astype(F)
        assert np.array_equal(encode64(x.astype(np.float64), m), [bl.bl_pack_ufloat(float(v), m) for v in x])
        for c in (1, 5, 64, 65, 500, (31 << m) - 2):                      # ties go to the even code
            mid = (Fraction(float(decode64(c, m))) + Fraction(float(decode64(c + 1, m)))) / 2
            assert round_fraction(mid, m) == (c if c % 2 == 0 else c + 1) == bl.bl_pack_ufloat(float(mid), m) == int(encode64(float(mid), m))


# ---- the sampler ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (1, 7), (7, 1), (5, 3), (16, 16)])
def test_sampler_returns_texels_at_centres_and_clamps_at_every_edge(bl, W, H):
    img = BR.seeded_finite_words(W, H, 11)
    dec = decode_words(img).astype(F)
    pow2 = (W & (W - 1)) == 0 and (H & (H - 1)) == 0
    if pow2:                                                                 # centres are exact coordinates when the size is a power of two
        uv = [((x + 0.5) / W, (y + 0.5) / H) for y in range(H) for x in range(W)]
        assert np.array_equal(BR.sample(bl, img, uv), dec.reshape(-1, 3))
    # outside [0, 1] and on the border the nearest edge texel comes back, exactly: both columns (rows) are the same texel
    for u, x in ((-0.3, 0), (-5.0, 0), (0.0, 0), (1.0, W - 1), (1.2, W - 1), (9.0, W - 1)):
        for v, y in ((-0.3, 0), (-7.0, 0), (0.0, 0), (1.0, H - 1), (1.4, H - 1), (3.0, H - 1)):
            assert np.array_equal(BR.sample(bl, img, [(u, v)])[0], dec[y, x]), (u, v)
    for dim in (W, H):
        for uv, want in ((-2.0, (0, 0)), (0.0, (0, 0)), (1.0, (dim - 1, dim - 1)), (1.5, (dim - 1, dim - 1)), (math.nan, (0, 0))):
            assert BR.axis(bl, uv, dim)[:2] == want
    if W == 1 and H == 1:
        assert np.array_equal(BR.sample(bl, img, [(0.5, 0.5), (0.1, 0.9)]), np.stack([dec[0, 0]] * 2))
    # an infinite or NaN coordinate reads texel 0 or the last (never outside) with the weight inf - inf = NaN: a NaN sample
    assert np.all(np.isnan(BR.sample(bl, img, [(-math.inf, 0.5), (0.5, math.inf), (math.nan, 0.5)])))


@pytest.mark.parametrize("W", [2, 8, 16, 64, 1024, 4096, 6, 10, 134, 270, 540, 1080, 1920, 3840])
def test_downsample_taps_of_an_even_sized_source_sit_on_texel_corners(bl, W):
    """uv = (p + 0.5) / (W / 2), taps uv + k / W, k in -2 .. 2: tx = 2 p + 0.5 + k in exact arithmetic, so the weight is 0.5 and the
    columns are 2 p + k and 2 p + k + 1 (clamped).  In binary32 that is exact when W is a power of two (every quotient and product
    is); for another even W the quotients round, the columns stay (tx is half a texel from the next integer) and the weight is
    within the coordinate bound 4 u W of 0.5 (derived in _pass64)."""
    pow2 = W & (W - 1) == 0
    inv = F(1.0) / F(W)
    for p in sorted({0, 1, 2, W // 4, W // 2 - 2, W // 2 - 1} & set(range(W // 2))):
        u = F(F(p) + F(0.5)) / F(W // 2)
        for k, coord in ((-2, F(u - F(2) * inv)), (-1, F(u - inv)), (0, u), (1, F(u + inv)), (2, F(u + F(2) * inv))):
            i0, i1, f = BR.axis(bl, coord, W)
            assert f == F(0.5) if pow2 else abs(float(f) - 0.5) <= 4 * U * W, (W, p, k, f)
            assert (i0, i1) == (min(max(2 * p + k, 0), W - 1), min(max(2 * p + k + 1, 0), W - 1))


# ---- constant images ----------------------------------------------------------------------------------------------------------
def _grey(code):
    return code | code << 11 | (code >> 1) << 22


def test_constant_images_of_every_finite_code(bl):
    """Later downsamples and the upsample return a constant image unchanged, bit for bit: every tap is lerp(c, c, f) = c + f * 0,
    the four-tap sums c + c + c + c need two more bits than the code's seven, and the weights are powers of two that sum to 1.
    No code of the format comes near binary32's overflow (the largest is 65024), so there is no exception to make.  The first
    downsample gives max(sum of five c_g * K(c_g), 0.0001f) with c_g = c / 8 four times and c / 2 once: checked against float64
    within 10 u c: per group 3 u for the luminance dot3 and 1 u each for 1 + luma, the division and the product (6 u c_g, and the
    groups sum to c), then 4 additions of partial sums <= c."""
    for code in range(31 << 6):
        img = np.full((6, 10), _grey(code), np.uint32)
        assert np.all(BR.downsample(bl, img, False) == img[0, 0]), code
        for r in (0.001, 0.005, 0.1):
            assert np.all(BR.upsample(bl, img, r, (20, 12)) == img[0, 0]), (code, r)
        words, rgb = BR.downsample(bl, img, True, want_rgb=True)
        c = decode_words(img[0, 0])
        want = np.zeros(3)
        for g in (c / 8, c / 8, c / 8, c / 8, c / 2):
            want += g / (1.0 + 0.25 * (g[0] * LUM[0] + g[1] * LUM[1] + g[2] * LUM[2]))
        want = np.maximum(want, FLOOR)
        assert np.all(np.abs(rgb.astype(np.float64) - want) <= 10 * U * np.maximum(c, FLOOR)), code
        assert np.all(rgb == rgb[0, 0]) and np.all(words == words[0, 0])


# ---- impulses in exact rationals ----------------------------------------------------------------------------------------------
DOWN_TAPS = [(-2, 2, 1, 32), (0, 2, 1, 16), (2, 2, 1, 32), (-2, 0, 1, 16), (0, 0, 1, 8), (2, 0, 1, 16), (-2, -2, 1, 32), (0, -2, 1, 16),
             (2, -2, 1, 32), (-1, 1, 1, 8), (1, 1, 1, 8), (-1, -1, 1, 8), (1, -1, 1, 8)]            # (kx, ky, weight = n / d)
UP_TAPS = [(-1, 1, 1, 16), (0, 1, 2, 16), (1, 1, 1, 16), (-1, 0, 2, 16), (0, 0, 4, 16), (1, 0, 2, 16), (-1, -1, 1, 16), (0, -1, 2, 16), (1, -1, 1, 16)]


def _exact_weights(taps, step_x: Fraction, step_y: Fraction, sW, sH, dW, dH, ix, iy):
    """The weight, an exact rational, with which source texel (ix, iy) enters every destination texel: bloom.hlsl's taps at
    uv + k * step through the convention's bilinear sampler, all in exact arithmetic."""
    out = {}
    for py in range(dH):
        for px in range(dW):
            total = Fraction(0)
            for kx, ky, n, d in taps:
                tx = (Fraction(2 * px + 1, 2 * dW) + kx * step_x) * sW - Fraction(1, 2)
                ty = (Fraction(2 * py + 1, 2 * dH) + ky * step_y) * sH - Fraction(1, 2)
                x0, y0 = math.floor(tx), math.floor(ty)
                fx, fy = tx - x0, ty - y0
                for cx, wx in ((x0, 1 - fx), (x0 + 1, fx)):
                    for cy, wy in ((y0, 1 - fy), (y0 + 1, fy)):
                        if min(max(cx, 0), sW - 1) == ix and min(max(cy, 0), sH - 1) == iy:
                            total += Fraction(n, d) * wx * wy
            if total:
                out[(px, py)] = total
    return out


def _check_impulse(bl, kind, sW, sH, dW, dH, ix, iy, step):
    word = 0x3D5 | 0x2A7 << 11 | 0x1B3 << 22                                 # three different seven- and six-bit significands
    img = np.zeros((sH, sW), np.uint32)
    img[iy, ix] = word
    value = [Fraction(float(v)) for v in decode_words(word)]
    if kind == "down":
        got, rgb = BR.downsample(bl, img, False, dest=(dW, dH), want_rgb=True)
        weights = _exact_weights(DOWN_TAPS, Fraction(1, sW), Fraction(1, sH), sW, sH, dW, dH, ix, iy)
    else:
        got, rgb = BR.upsample(bl, img, float(step), (dW, dH), want_rgb=True)
        weights = _exact_weights(UP_TAPS, step, step, sW, sH, dW, dH, ix, iy)
    assert weights and set(zip(*np.nonzero(got)[::-1])) == set(weights)
    for (px, py), w in weights.items():
        want = round_fraction(value[0] * w, 6) | round_fraction(value[1] * w, 6) << 11 | round_fraction(value[2] * w, 5) << 22
        assert got[py, px] == want, (px, py, w)
        assert [Fraction(float(c)) for c in rgb[py, px]] == [v * w for v in value]      # the unrounded value is the exact rational
    total = sum(weights.values())
    assert [sum(Fraction(float(c)) for c in rgb[..., ch].ravel()) for ch in range(3)] == [v * total for v in value]
    return total


@pytest.mark.parametrize("ix,iy", [(7, 6), (0, 0), (15, 9), (1, 15)])
def test_downsample_of_an_impulse_equals_exact_rationals(bl, ix, iy):
    total = _check_impulse(bl, "down", 16, 16, 8, 8, ix, iy, None)
    if 4 <= ix < 12 and 4 <= iy < 12:
        assert total == Fraction(1, 4)                                       # energy: every interior texel enters with the weights' sum over 4 texels


@pytest.mark.parametrize("ix,iy,step", [(3, 4, Fraction(1, 16)), (0, 0, Fraction(1, 16)), (7, 2, Fraction(1, 8)), (4, 4, Fraction(1, 32))])
def test_upsample_of_an_impulse_equals_exact_rationals(bl, ix, iy, step):
    """8 x 8 into 16 x 16 with a radius that is a power of two: every coordinate, weight and product is exact in binary32."""
    total = _check_impulse(bl, "up", 8, 8, 16, 16, ix, iy, step)
    if 2 <= ix < 6 and 2 <= iy < 6:
        assert total == 4                                                    # four destination texels per source texel, weights summing to 1


# ---- against float64 ----------------------------------------------------------------------------------------------------------
def _window_max(a, r=2):
    p = np.pad(a, ((r, r), (r, r), (0, 0)), mode="edge")
    out = np.zeros_like(a)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = np.maximum(out, p[dy:dy + a.shape[0], dx:dx + a.shape[1]])
    return out


class Source64:
    """A source mip in float64, with what the band needs: per texel the largest value and the largest horizontal / vertical
    difference of neighbours within two texels (a bound of the bilinear surface's slope around any tap that lands there)."""
    def __init__(self, words):
        self.T = decode_words(words)
        self.H, self.W = self.T.shape[:2]
        dx = np.abs(np.diff(self.T, axis=1, append=self.T[:, -1:]))
        dy = np.abs(np.diff(self.T, axis=0, append=self.T[-1:]))
        self.SX, self.SY, self.M = _window_max(dx), _window_max(dy), _window_max(self.T, 1)

    def tap(self, u, v):
        """(value, largest nearby texel, slope in x, slope in y) at float64 coordinates u, v (arrays), each (..., 3)."""
        tx, ty = u * self.W - 0.5, v * self.H - 0.5
        x0, y0 = np.floor(tx), np.floor(ty)
        fx, fy = (tx - x0)[..., None], (ty - y0)[..., None]
        c0, c1 = np.clip(x0, 0, self.W - 1).astype(int), np.clip(x0 + 1, 0, self.W - 1).astype(int)
        r0, r1 = np.clip(y0, 0, self.H - 1).astype(int), np.clip(y0 + 1, 0, self.H - 1).astype(int)
        T = self.T
        lerp = lambda a, b, s: a + s * (b - a)
        val = lerp(lerp(T[r0, c0], T[r0, c1], fx), lerp(T[r1, c0], T[r1, c1], fx), fy)
        return val, self.M[r0, c0], self.SX[r0, c0], self.SY[r0, c0]


def _pass64(kind, words, dW, dH, inv, radius):
    """bloom.hlsl in float64 (the constants as the binary32 numbers the pass receives) and the band within which binary32 may land.

    BAND, per channel, absolute, u = 2^-24.  (1) A tap's coordinate: uv rounds once (<= u / 2 since uv < 1), the tap offset once
    (|uv +- 2 x| < 1.2: <= u), the product with W once and the - 0.5f once (each <= 1.2 u W): tx is off by dt <= 4 u W (floor and
    tx - floor are exact).  The bilinear surface is continuous and piecewise linear, so the tap moves by at most dt_x * SX +
    dt_y * SY, SX / SY the largest neighbour difference within two texels (covers the cell a floor flips into).  (2) A tap's three
    lerps: three roundings each, every intermediate <= M (the largest texel nearby), the inner errors enter with weights that sum
    to 1: <= 6 u M.  (3) The sums: the weights are powers of two (exact), each addition rounds by u times a partial sum that is
    at most S = sum of weight * M: 12 additions in a later downsample, 8 in the upsample.  (4) First downsample: a group g =
    (sum of four) * w has 3 additions; phi(g) = g / (1 + 0.25 dot(c, g)) has |d phi_i / d g_j| <= [i = j] + c_j / c_i (from
    g_i * 0.25 c_j / (1 + 0.25 c_i g_i) <= c_j / c_i), so an input error e_j moves channel i by at most e_i + sum_j (c_j / c_i) e_j;
    its own roundings (dot3 three, 1 + luma, the division, the product) are <= 6 u g_i; then 4 additions of partial sums <= S.
    float64's own rounding (2^-53) is covered by the factor 1.001."""
    src = Source64(words)
    py, px = np.mgrid[0:dH, 0:dW]
    u, v = (px + 0.5) / dW, (py + 0.5) / dH
    dtx, dty = 4 * U * src.W, 4 * U * src.H

    def tap(kx, ky, sx, sy):
        val, M, SX, SY = src.tap(u + kx * sx, v + ky * sy)
        return val, dtx * SX + dty * SY + 6 * U * M, M
    if kind == "up":
        r = float(F(radius))
        t = {(kx, ky): tap(kx, ky, r, r) for kx in (-1, 0, 1) for ky in (-1, 0, 1)}
        weights = {k: (4 if k == (0, 0) else 2 if 0 in k else 1) / 16 for k in t}
        val = sum(weights[k] * t[k][0] for k in t)
        S = sum(weights[k] * t[k][2] for k in t)
        return val, 1.001 * (sum(weights[k] * t[k][1] for k in t) + 8 * U * S)
    x, y = float(F(inv[0])), float(F(inv[1]))
    t = {(kx, ky): tap(kx, ky, x, y) for kx, ky, _, _ in DOWN_TAPS}
    if kind == "down":
        weights = {(kx, ky): n / d for kx, ky, n, d in DOWN_TAPS}
        val = sum(weights[k] * t[k][0] for k in t)
        S = sum(weights[k] * t[k][2] for k in t)
        return val, 1.001 * (sum(weights[k] * t[k][1] for k in t) + 12 * U * S)
    groups = [((-2, 2), (0, 2), (-2, 0), (0, 0), 1 / 32), ((0, 2), (2, 2), (0, 0), (2, 0), 1 / 32), ((-2, 0), (0, 0), (-2, -2), (0, -2), 1 / 32),
              ((0, 0), (2, 0), (0, -2), (2, -2), 1 / 32), ((-1, 1), (1, 1), (-1, -1), (1, -1), 1 / 8)]
    c = np.array(LUM)
    val, err, S = 0.0, 0.0, 0.0
    for *keys, w in groups:
        g = w * sum(t[k][0] for k in keys)
        m = w * sum(t[k][2] for k in keys)
        e = w * sum(t[k][1] for k in keys) + 3 * U * m
        e = e + np.stack([sum(c[j] / c[i] * e[..., j] for j in range(3)) for i in range(3)], axis=-1) + 6 * U * m
        val = val + g / (1.0 + 0.25 * (g @ c))[..., None]
        err, S = err + e, S + m
    return np.maximum(val, FLOOR), 1.001 * (err + 4 * U * S)


def _lognormal_words(W, H, scale, seed):
    rng = np.random.default_rng(seed)
    return encode_words(scale * np.exp(rng.normal(0.0, 2.0, (H, W, 3))))


FLOAT64_DIFFERING = {}


@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("W,H", [(17, 17), (67, 35), (270, 135)])
@pytest.mark.parametrize("kind,radius", [("down", None), ("first", None), ("up", 0.001), ("up", 0.005), ("up", 0.1)])
def test_passes_against_float64(bl, kind, radius, W, H, scale):
    """Seeded log-normal images (sigma 2).  Every channel that differs from float64's is one code apart and lies within the derived
    band of a rounding boundary; at most 2e-3 of the channels differ."""
    if kind == "up":                                                         # the size is the destination's; the source is the mip below
        sW, sH, dW, dH = W >> 1, H >> 1, W, H
    else:
        sW, sH, dW, dH = W, H, W >> 1, H >> 1
    img = _lognormal_words(sW, sH, scale, 1000 + W + (1000 if scale > 1 else 0))
    inv = (F(1.0) / F(sW), F(1.0) / F(sH))
    got = BR.upsample(bl, img, radius, (dW, dH)) if kind == "up" else BR.downsample(bl, img, kind == "first")
    val, band = _pass64(kind, img, dW, dH, inv, radius)
    got_codes, want_codes = codes_of_words(got), codes_of_words(encode_words(val))
    differs = got_codes != want_codes
    assert np.all(np.abs(got_codes - want_codes)[differs] == 1)
    dist = np.stack([boundary_distance(val[..., ch], 6 if ch < 2 else 5) for ch in range(3)], axis=-1)
    assert np.all(dist[differs] <= band[differs]), float(np.max(dist[differs] / band[differs]))
    share = differs.mean()
    FLOAT64_DIFFERING[(kind, radius, W, H, scale)] = (int(differs.sum()), differs.size)
    print(f"{kind} radius {radius} {W}x{H} scale {scale}: {int(differs.sum())} of {differs.size} channels differ ({share:.2e})")
    assert share <= 2e-3


def test_chain_is_the_passes_in_the_renderers_order(bl):
    W, H, mips, r = 67, 35, 5, 0.005
    img = _lognormal_words(W, H, 1.0, 3)
    chain = BR.bloom_chain(bl, img, W, H, mips, r)
    dims = BR.chain_dims(W, H, mips)
    assert [c.shape for c in chain] == [(h, w) for w, h in dims] and dims[-1] == (4, 2)
    down = [None, BR.downsample(bl, img, True)]
    for k in range(2, mips):
        down.append(BR.downsample(bl, down[-1], False))
    assert np.array_equal(chain[mips - 1], down[mips - 1])
    cur = down[mips - 1]
    for k in range(mips - 2, -1, -1):                                        # each upsample OVERWRITES the finer mip: no trace of its downsample
        cur = BR.upsample(bl, cur, r, dims[k])
        assert np.array_equal(chain[k], cur)


# ---- special inputs, word by word -----------------------------------------------------------------------------------------------
def test_special_inputs_word_by_word(bl):
    W, H = 8, 8
    sp = BR.special_images(W, H)
    floor_word = int(encode_words(np.full(3, FLOOR)))
    black = sp["black"]
    assert np.all(BR.downsample(bl, black, False) == 0) and np.all(BR.upsample(bl, black, 0.005, (16, 16)) == 0)
    assert np.all(BR.downsample(bl, black, True) == floor_word)              # max(0, 0.0001f): the floor of the first downsample
    assert floor_word == 0x069 | 0x069 << 11 | 0x034 << 22 and bl.bl_pack_ufloat(FLOOR, 6) == 0x069   # 0.0001 = 1.6384 * 2^-14: exponent field 1, mantissa rint(0.6384 * 64) = 41, blue rint(0.6384 * 32) = 20
    # subnormal codes: exact rationals (8 x 8 -> 4 x 4: every weight is a power of two and nothing is lost before the one store)
    sub = sp["subnormal"]
    got = BR.downsample(bl, sub, False)
    dec = [[[Fraction(float(c)) for c in px] for px in row] for row in decode_words(sub)]
    for py in range(4):
        for px in range(4):
            acc = [Fraction(0)] * 3
            for kx, ky, n, d in DOWN_TAPS:
                for cx in (2 * px + kx, 2 * px + kx + 1):
                    for cy in (2 * py + ky, 2 * py + ky + 1):
                        t = dec[min(max(cy, 0), H - 1)][min(max(cx, 0), W - 1)]
                        acc = [a + Fraction(n, 4 * d) * c for a, c in zip(acc, t)]
            assert got[py, px] == round_fraction(acc[0], 6) | round_fraction(acc[1], 6) << 11 | round_fraction(acc[2], 5) << 22
    # the largest finite: unchanged by the later passes; the Karis weights pull the first downsample far below it
    big = sp["largest finite"]
    assert np.all(BR.downsample(bl, big, False) == BR.MAX_FINITE_WORD) and np.all(BR.upsample(bl, big, 0.1, (16, 16)) == BR.MAX_FINITE_WORD)
    first = decode_words(BR.downsample(bl, big, True))
    assert np.all(first > 4.0) and np.all(first < 40.0)
    # +inf: lerp(1, inf, f) = 1 + f * inf = inf, but lerp(inf, 1, f) = inf + f * (1 - inf) = NaN for f > 0, and lerp(inf, inf, f) has
    # inf - inf.  8 x 8 -> 4 x 4 (all weights 0.5): every destination whose 13 taps reach texel (4, 4) has a tap with it in the
    # first column or row, so all nine are NaN; the others keep 1.0.  The Karis factor of an infinite group is 1 / inf = 0 and
    # inf * 0 is a NaN, which the first downsample's max turns into the floor.
    O, N, Inf = BR.ONE_WORD, BR.NAN_WORD, BR.INF_WORD
    nine = np.full((4, 4), O, np.uint32)
    nine[1:, 1:] = N
    for name in ("inf beside finite", "inf beside inf"):
        assert np.array_equal(BR.downsample(bl, sp[name], False), nine)
        first = BR.downsample(bl, sp[name], True)
        assert np.all(first[1:, 1:] == floor_word) and np.all(first[0] == first[0, 0]) and np.all(first[:, 0] == first[0, 0])
        assert first[0, 0] == BR.downsample(bl, np.full((8, 8), O, np.uint32), True)[0, 0]
    # the upsample 8 x 8 -> 16 x 16 at radius 0.005 (0.04 texels: every tap stays in its centre's cell): destinations 7 and 8 have
    # tx = 3.25, 3.75, the infinite column second (inf); 9 and 10 have it first (NaN)
    up = np.full((16, 16), O, np.uint32)
    up[7:11, 7:11] = N
    up[7:9, 7:9] = Inf
    assert np.array_equal(BR.upsample(bl, sp["inf beside finite"], 0.005, (16, 16)), up)
    up[7:11, 11:13] = N                                                      # the second infinity at (5, 4) and the third at (4, 5)
    up[11:13, 7:11] = N
    assert np.array_equal(BR.upsample(bl, sp["inf beside inf"], 0.005, (16, 16)), up)
    # NaN codes reach every texel whose taps touch them; a NaN in red only (texel (0, 0), green and blue 0) leaves green and blue finite
    nan = BR.downsample(bl, sp["nan"], False)
    assert np.all(nan[1:, 1:] == N) and nan[3, 0] == O and nan[0, 3] == O
    assert (nan[0, 0] & 0x7FF) == 0x7FF and nan[0, 0] != N and nan[0, 0] == (codes_of_words(nan[0, 0]) @ [1, 1 << 11, 1 << 22])
    g, b = decode_words(nan[0, 0])[1:]
    assert 0.0 < g < 1.0 and 0.0 < b < 1.0
    up = BR.upsample(bl, sp["nan"], 0.005, (16, 16))
    assert np.all(up[7:11, 7:11] == N) and up[0, 0] == 0x7FF and up[15, 15] == O and np.all(up[3:7] == O)
    first = BR.downsample(bl, sp["nan"], True)
    assert N not in first and np.all(first[1:, 1:] == floor_word) and first[0, 0] == floor_word


# ---- layout and constants -----------------------------------------------------------------------------------------------------
def test_bloom_consts_layout(tmp_path):
    """A g++-compiled probe prints sizeof / offsetof of BloomConsts of csrc/ShaderInterop.h: every field where the numpy dtype has it."""
    want = {"m_InvSourceResolution": 0, "m_FilterRadius": 8, "m_bIsFirstDownsample": 12}
    out = layout_probe(tmp_path, [("size", "sizeof(interop::BloomConsts)")] + [(f, f"offsetof(interop::BloomConsts, {f})") for f in want])
    assert int(out["size"]) == 16 == I.BloomConsts.itemsize == I.SIZES["BloomConsts"]
    assert list(I.BloomConsts.names) == list(want)
    for f, off in want.items():
        assert int(out[f]) == I.BloomConsts.fields[f][1] == off


@pytest.mark.parametrize("W,H,dims", [(1920, 1080, [(960, 540), (480, 270), (240, 135), (120, 67), (60, 33)]),
                                      (270, 135, [(135, 67), (67, 33), (33, 16), (16, 8), (8, 4)])])
def test_pass_constants_and_mip_dimensions(W, H, dims):
    assert BR.chain_dims(W, H, 6)[1:] == dims
    k = BR.pass_consts(W, H, 6, 0.005)
    assert len(k) == 10
    src = [(W, H)] + dims[:-1]
    for i in range(5):
        assert k[i]["m_InvSourceResolution"].tobytes() == np.array([F(1) / F(src[i][0]), F(1) / F(src[i][1])], F).tobytes()
        assert k[i]["m_bIsFirstDownsample"] == (1 if i == 0 else 0) and k[i]["m_FilterRadius"] == 0
        assert k[5 + i]["m_FilterRadius"].tobytes() == F(0.005).tobytes() == bytes.fromhex("0ad7a33b")
        assert k[5 + i]["m_bIsFirstDownsample"] == 0 and not k[5 + i]["m_InvSourceResolution"].any()
    if W == 1920:
        assert k[0].tobytes() == bytes.fromhex("8988083a" "d6b9723a" "00000000" "01000000")      # 1 / 1920, 1 / 1080
        assert k[4].tobytes() == bytes.fromhex("8988083c" "8d89743c" "00000000" "00000000")      # 1 / 120, 1 / 67
    else:
        assert k[0].tobytes() == bytes.fromhex("d6b9723b" "d6b9f23b" "00000000" "01000000")      # 1 / 270, 1 / 135
        assert k[4].tobytes() == bytes.fromhex("0000803d" "0000003e" "00000000" "00000000")      # 1 / 16, 1 / 8
    assert BR.max_mips(1920, 1080) == 11 and BR.max_mips(270, 135) == 8 and BR.max_mips(67, 35) == 6 and BR.max_mips(2, 2) == 2


# ---- registry and refusals ------------------------------------------------------------------------------------------------------
def test_shader_registry_has_both_entries():
    from toyrenderer_amd import rhi
    assert {"bloom_PS_Downsample", "bloom_PS_Upsample"} <= set(rhi.shader_names())


def test_host_library_exports_the_bloom_symbols():
    from toyrenderer_amd import host
    lib = host.load()
    for name in ("trhost_set_bloom", "trhost_download_bloom", "trhost_get_bloom_consts"):
        assert name in host.HOST_SYMBOLS and hasattr(lib, name), name


def test_frame_driver_refusals_need_no_device():
    """Each refusal comes before the driver touches the device."""
    from toyrenderer_amd.frame import FrameDriver
    scene = types.SimpleNamespace(materials=object(), vertices=object(), numInstances=1, numAlphaMask=0)
    view = types.SimpleNamespace(renderW=67, renderH=35)

    def make(**kw):
        kw.setdefault("post", True)
        return FrameDriver(None, scene, view, record_capacity=1, **kw)
    with pytest.raises(ValueError, match="at least 2 mips"):
        make(bloom_mips=1)
    with pytest.raises(ValueError, match="at most 6 mips"):
        make(bloom_mips=7)
    with pytest.raises(ValueError, match="needs post=True"):
        make(bloom_mips=3, post=False, lighting=True)
    with pytest.raises(ValueError, match="external bloom"):
        make(bloom_mips=3, bloom=(object(), 0.5))
    for r in (-0.001, math.inf, math.nan):
        with pytest.raises(ValueError, match="finite radius"):
            make(bloom_mips=3, bloom_filter_radius=r)
    with pytest.raises(AttributeError):                                      # an allowed count gets as far as the device (None here)
        make(bloom_mips=6)
