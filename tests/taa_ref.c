/* taa_ref.c -- the definition of "taa_CS_TemporalResolve" (csrc/k_taa.hip): the temporal anti-aliasing resolve after Karis, "High
 * Quality Temporal Supersampling" (SIGGRAPH 2014), with the closest-depth velocity dilation and the neighbourhood clamp of
 * Pedersen, "Temporal Reprojection Anti-Aliasing in INSIDE" (GDC 2016).  The reference's TAARenderer calls DLSS or FSR, neither
 * of which is in its tree, so there is no shader to restate: this file is what the GPU must equal word for word.  Compiled by the
 * tests themselves with gcc -O2 -ffp-contract=off: only the fmaf calls written here fuse.
 *
 * CONVENTION (the kernel's header states it, DESIGN.md 3 repeats it).  IEEE binary32, / correctly rounded, min / max = fminf /
 * fmaxf (a NaN operand is dropped), lerp(x, y, s) = x + s * (y - x) always evaluated, dot3 = fmaf(a.z, b.z, fmaf(a.y, b.y,
 * a.x * b.x)), binary16 loads exact and stores round to nearest even with every NaN stored as 0x7E00, R11G11B10_FLOAT as
 * ref_formats.h states it.  For the pixel (px, py) of a W x H image:
 *   window   : columns max(px - 1, 0), px, min(px + 1, W - 1) and the same rows; nine texels, row by row;
 *   YCoCg    : Y = (0.25f * R + 0.5f * G) + 0.25f * B; Co = 0.5f * R - 0.5f * B; Cg = (0.5f * G - 0.25f * R) - 0.25f * B;
 *   box      : lo = hi = the first texel's YCoCg, then per channel fminf / fmaxf over the other eight in order; c = the centre's RGB;
 *   dilation : best = the centre's depth, at the centre; over the nine in order a depth > best (a NaN never is) replaces it; mv =
 *              the motion texel at that position;
 *   history  : hp.x = (((float)px + 0.5f) + mv.x) - jitterDelta.x, the same in y; valid when reset == 0, 0 <= hp.x < W, 0 <= hp.y < H
 *              (comparisons a NaN fails) and the four channels of the fetch are finite; the fetch is bloom_ref.c's bilinear
 *              sampler at (hp.x / (float)W, hp.y / (float)H) over the four binary16 channels;
 *   clamp    : k = YCoCg(history.xyz); q = fminf(fmaxf(k, lo), hi) + 0.0f per channel; q == k in all three: h = history.xyz as
 *              fetched; else h = ((q.Y + q.Co) - q.Cg, q.Y + q.Cg, (q.Y - q.Co) - q.Cg);
 *   blend    : n = fminf(fmaxf(history.w, 0), maxCount); alpha = fmaxf(1.0f / (n + 1.0f), minBlend); L = dot3(rgb, (0x1.b38cdap-3f,
 *              0x1.6e2974p-1f, 0x1.279aaep-4f)); wc = alpha / (1.0f + L(c)); wh = (1.0f - alpha) / (1.0f + L(h)); out = (c * wc +
 *              h * wh) / (wc + wh); with invalid history out = c and n = 0.  A NaN or infinite c is not treated specially: with
 *              valid history an infinite channel makes wc 0 and out NaN, stored as the NaN codes, and the next frame finds the
 *              history not finite and starts again;
 *   store    : history = (out, fminf(n + 1.0f, maxCount)) as four binary16; colour = out packed to R11G11B10_FLOAT.
 * The path byte, for the tests only: bit 0 history valid; bit 1 the clamp changed a channel; bit 2 dilation chose another texel
 * than the centre; bits 4..7 the bilinear texels (x0, y0), (x1, y0), (x0, y1), (x1, y1) whose weight is not zero, set when the
 * fetch happens (reset == 0 and the position test passes).
 */
#include "ref_formats.h"

typedef struct { uint32_t W, H; float jitterX, jitterY, minBlend, maxCount; uint32_t reset, pad; } TAAConsts;   /* csrc/ShaderInterop.h */

typedef struct { uint32_t i0, i1; float f; } Axis;

static Axis axis_of(float uv, uint32_t dim)                                    /* bloom_ref.c's, word for word */
{
    const float t = uv * (float)dim - 0.5f, t0 = floorf(t), last = (float)(dim - 1u);
    Axis a;
    a.i0 = (uint32_t)fminf(fmaxf(t0, 0.0f), last);
    a.i1 = (uint32_t)fminf(fmaxf(t0 + 1.0f, 0.0f), last);
    a.f = t - t0;
    return a;
}

static void to_ycocg(const float c[3], float k[3])
{
    k[0] = (0.25f * c[0] + 0.5f * c[1]) + 0.25f * c[2];
    k[1] = 0.5f * c[0] - 0.5f * c[2];
    k[2] = (0.5f * c[1] - 0.25f * c[0]) - 0.25f * c[2];
}

static float luminance(const float c[3])
{
    const float w[3] = { 0x1.b38cdap-3f, 0x1.6e2974p-1f, 0x1.279aaep-4f };
    return dot3(c, w);
}

static uint32_t window(uint32_t p, int d, uint32_t dim) { return d < 0 ? (p > 0u ? p - 1u : 0u) : d > 0 ? (p + 1u < dim ? p + 1u : dim - 1u) : p; }
static int finite_(float x) { return fabsf(x) < INFINITY; }

static uint8_t resolve_pixel(const TAAConsts* k, const uint32_t* colour, const float* depth, const uint32_t* motion, const uint16_t* history,
                             uint32_t px, uint32_t py, uint16_t newHistory[4], uint32_t* out)
{
    const uint32_t W = k->W, H = k->H;
    float lo[3], hi[3], c[3], best = depth[(uint64_t)py * W + px];
    uint32_t bx = px, by = py;
    uint8_t path = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const uint32_t x = window(px, dx, W), y = window(py, dy, H);
            float rgb[3], ycc[3];
            unpack_r11g11b10(colour[(uint64_t)y * W + x], rgb);
            to_ycocg(rgb, ycc);
            for (int ch = 0; ch < 3; ++ch) {
                lo[ch] = dy == -1 && dx == -1 ? ycc[ch] : fminf(lo[ch], ycc[ch]);
                hi[ch] = dy == -1 && dx == -1 ? ycc[ch] : fmaxf(hi[ch], ycc[ch]);
            }
            if (dy == 0 && dx == 0) memcpy(c, rgb, 12);
            const float z = depth[(uint64_t)y * W + x];
            if (z > best) { best = z; bx = x; by = y; }
        }
    if (bx != px || by != py) path |= 4;
    const uint32_t mw = motion[(uint64_t)by * W + bx];
    const float hx = (((float)px + 0.5f) + half_to_float(mw & 0xFFFFu)) - k->jitterX, hy = (((float)py + 0.5f) + half_to_float(mw >> 16)) - k->jitterY;
    int valid = k->reset == 0u && hx >= 0.0f && hx < (float)W && hy >= 0.0f && hy < (float)H;
    float o[3] = { c[0], c[1], c[2] }, n = 0.0f;
    if (valid) {
        const Axis x = axis_of(hx / (float)W, W), y = axis_of(hy / (float)H, H);
        const uint16_t *t00 = history + 4 * ((uint64_t)y.i0 * W + x.i0), *t10 = history + 4 * ((uint64_t)y.i0 * W + x.i1);
        const uint16_t *t01 = history + 4 * ((uint64_t)y.i1 * W + x.i0), *t11 = history + 4 * ((uint64_t)y.i1 * W + x.i1);
        float f[4];
        for (int ch = 0; ch < 4; ++ch)
            f[ch] = lerp(lerp(half_to_float(t00[ch]), half_to_float(t10[ch]), x.f), lerp(half_to_float(t01[ch]), half_to_float(t11[ch]), x.f), y.f);
        /* a weight is a product of (1 - f) and f factors as the lerps apply them: zero where f is 0 (the second texel) or 1 (the first) */
        path |= (uint8_t)((x.f != 1.0f && y.f != 1.0f) << 4 | (x.f != 0.0f && y.f != 1.0f) << 5 | (x.f != 1.0f && y.f != 0.0f) << 6 | (x.f != 0.0f && y.f != 0.0f) << 7);
        valid = finite_(f[0]) && finite_(f[1]) && finite_(f[2]) && finite_(f[3]);
        if (valid) {
            float h[3] = { f[0], f[1], f[2] }, kk[3], q[3];
            to_ycocg(h, kk);
            for (int ch = 0; ch < 3; ++ch) q[ch] = fminf(fmaxf(kk[ch], lo[ch]), hi[ch]) + 0.0f;
            if (!(q[0] == kk[0] && q[1] == kk[1] && q[2] == kk[2])) {
                path |= 2;
                h[0] = (q[0] + q[1]) - q[2]; h[1] = q[0] + q[2]; h[2] = (q[0] - q[1]) - q[2];
            }
            n = fminf(fmaxf(f[3], 0.0f), k->maxCount);
            const float alpha = fmaxf(1.0f / (n + 1.0f), k->minBlend);
            const float wc = alpha / (1.0f + luminance(c)), wh = (1.0f - alpha) / (1.0f + luminance(h)), sum = wc + wh;
            for (int ch = 0; ch < 3; ++ch) o[ch] = (c[ch] * wc + h[ch] * wh) / sum;
            path |= 1;
        }
    }
    for (int ch = 0; ch < 3; ++ch) newHistory[ch] = float_to_half(o[ch]);
    newHistory[3] = float_to_half(fminf(n + 1.0f, k->maxCount));
    *out = pack_r11g11b10(o[0], o[1], o[2]);
    return path;
}

/* The pass over a W x H image.  colour, motion: W * H words; depth: W * H floats; history, newHistory: 4 * W * H binary16; out:
 * W * H words; path: W * H bytes or NULL. */
void taa_resolve(const TAAConsts* k, const uint32_t* colour, const float* depth, const uint32_t* motion, const uint16_t* history,
                 uint16_t* newHistory, uint32_t* out, uint8_t* path)
{
    for (uint32_t py = 0; py < k->H; ++py)
        for (uint32_t px = 0; px < k->W; ++px) {
            const uint64_t i = (uint64_t)py * k->W + px;
            const uint8_t p = resolve_pixel(k, colour, depth, motion, history, px, py, newHistory + 4 * i, out + i);
            if (path) path[i] = p;
        }
}

/* A colour word loaded and stored again: itself, except that a NaN channel comes back as the format's one NaN code. */
void taa_repack(const uint32_t* words, uint64_t n, uint32_t* out)
{
    for (uint64_t i = 0; i < n; ++i) {
        float c[3];
        unpack_r11g11b10(words[i], c);
        out[i] = pack_r11g11b10(c[0], c[1], c[2]);
    }
}
