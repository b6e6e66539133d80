/* bloom_ref.c -- test reference of "bloom_PS_Downsample" and "bloom_PS_Upsample" (csrc/k_bloom.hip; bloom.hlsl,
 * BloomRenderer.cpp).  Compiled by the tests themselves with gcc -O2 -ffp-contract=off: only the fmaf calls written here fuse.
 *
 * CONVENTION (parity unpinned; the kernel's header states it, DESIGN.md 3 repeats it).  It extends the post-process convention
 * (postprocess_ref.c): IEEE binary32, / correctly rounded, min / max = fminf / fmaxf (a NaN operand is dropped), lerp(x, y, s) =
 * x + s * (y - x) always evaluated, dot3 = fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)), the R11G11B10_FLOAT load exact, the store
 * round to nearest even with NaN -> the NaN code, negative -> 0, overflow -> the largest finite, +inf -> inf.
 *   uv       : per axis ((float)p + 0.5f) / (float)destDim;
 *   taps     : uv.x - 2 * x, uv.x - x, uv.x, uv.x + x, uv.x + 2 * x (2 * x exact) and the same in y; x, y = m_InvSourceResolution
 *              for the downsample, m_FilterRadius for the upsample;
 *   bilinear : on a W x H mip: tx = uv.x * (float)W - 0.5f; x0 = floorf(tx); fx = tx - x0; columns x0 and x0 + 1.0f, each clamped
 *              as a float to [0, W - 1] (fminf(fmaxf(., 0), W - 1): a NaN gives 0) and then converted; the same in y; per channel
 *              lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy).  The project's definition: D3D hardware filters with
 *              fixed-point weights, and parity with it is unpinned;
 *   first downsample: groups (a + b + d + e), (b + c + e + f), (d + e + g + h), (e + f + h + i) each * 0.03125f and
 *              (j + k + l + m) * 0.125f, sums left to right; group *= 1.0f / (1.0f + luminance(group) * 0.25f); the five added in
 *              order; fmaxf(., 0.0001f) per channel (a NaN becomes 0.0001f);
 *   later downsamples: e * 0.125f, += (a + c + g + i) * 0.03125f, += (b + d + f + h) * 0.0625f, += (j + k + l + m) * 0.125f;
 *   upsample : e * 4.0f, += (b + d + f + h) * 2.0f, += (a + c + g + i), *= 0.0625f; the destination is overwritten;
 *   chain    : BloomRenderer::Render: mips - 1 downsamples (pass i reads mip i -- the colour image for i = 0 -- and writes mip
 *              i + 1 of size (W >> (i + 1), H >> (i + 1)) with m_InvSourceResolution = 1.0f / (W >> i, H >> i)), then mips - 1
 *              upsamples from mip mips - 1 - i into the next finer one.  Mip 0 is written by the last upsample only.
 */
#include "ref_formats.h"

/* ---- the format of tests/ref_formats.h under this library's names --------------------------------------------------------- */
float bl_unpack_ufloat(uint32_t c, uint32_t mbits) { return unpack_ufloat(c, mbits); }
uint32_t bl_pack_ufloat(float v, uint32_t mbits) { return pack_ufloat(v, mbits); }

/* ---- the sampler -------------------------------------------------------------------------------------------------------- */
typedef struct { uint32_t i0, i1; float f; } Axis;

static Axis axis_of(float uv, uint32_t dim)
{
    const float t = uv * (float)dim - 0.5f, t0 = floorf(t), last = (float)(dim - 1u);
    Axis a;
    a.i0 = (uint32_t)fminf(fmaxf(t0, 0.0f), last);
    a.i1 = (uint32_t)fminf(fmaxf(t0 + 1.0f, 0.0f), last);
    a.f = t - t0;
    return a;
}

/* What one axis resolves to: out = { i0, i1, bits of f } */
void bl_axis(float uv, uint32_t dim, uint32_t out[3])
{
    const Axis a = axis_of(uv, dim);
    out[0] = a.i0; out[1] = a.i1; out[2] = bits_of(a.f);
}

static void sample(const uint32_t* src, uint32_t W, uint32_t H, float u, float v, float out[3])
{
    const Axis x = axis_of(u, W), y = axis_of(v, H);
    float t00[3], t10[3], t01[3], t11[3];
    unpack_r11g11b10(src[(uint64_t)y.i0 * W + x.i0], t00); unpack_r11g11b10(src[(uint64_t)y.i0 * W + x.i1], t10);
    unpack_r11g11b10(src[(uint64_t)y.i1 * W + x.i0], t01); unpack_r11g11b10(src[(uint64_t)y.i1 * W + x.i1], t11);
    for (int c = 0; c < 3; ++c) out[c] = lerp(lerp(t00[c], t10[c], x.f), lerp(t01[c], t11[c], x.f), y.f);
}

/* SampleLevel(LinearClamp, (u, v), 0) of n coordinates: out = n x 3 floats */
void bl_sample_n(const uint32_t* src, uint32_t W, uint32_t H, const float* uv, uint64_t n, float* out)
{
    for (uint64_t i = 0; i < n; ++i) sample(src, W, H, uv[2 * i], uv[2 * i + 1], out + 3 * i);
}

/* ---- the two entries ---------------------------------------------------------------------------------------------------- */
static void sum4(const float* a, const float* b, const float* c, const float* d, float s, float out[3])
{
    for (int k = 0; k < 3; ++k) out[k] = (((a[k] + b[k]) + c[k]) + d[k]) * s;
}

static void karis(float g[3])
{
    const float luma = fmaf(g[2], 0x1.279aaep-4f, fmaf(g[1], 0x1.6e2974p-1f, g[0] * 0x1.b38cdap-3f)) * 0.25f;
    const float k = 1.0f / (1.0f + luma);
    for (int c = 0; c < 3; ++c) g[c] = g[c] * k;
}

/* One destination texel of PS_Downsample before the store: rgb[3] */
static void downsample_texel(const uint32_t* src, uint32_t sW, uint32_t sH, uint32_t dW, uint32_t dH, float x, float y, uint32_t first,
                             uint32_t px, uint32_t py, float rgb[3])
{
    const float u = ((float)px + 0.5f) / (float)dW, v = ((float)py + 0.5f) / (float)dH;
    float a[3], b[3], c[3], d[3], e[3], f[3], g[3], h[3], i[3], j[3], k[3], l[3], m[3];
    sample(src, sW, sH, u - 2 * x, v + 2 * y, a); sample(src, sW, sH, u, v + 2 * y, b); sample(src, sW, sH, u + 2 * x, v + 2 * y, c);
    sample(src, sW, sH, u - 2 * x, v, d);         sample(src, sW, sH, u, v, e);         sample(src, sW, sH, u + 2 * x, v, f);
    sample(src, sW, sH, u - 2 * x, v - 2 * y, g); sample(src, sW, sH, u, v - 2 * y, h); sample(src, sW, sH, u + 2 * x, v - 2 * y, i);
    sample(src, sW, sH, u - x, v + y, j); sample(src, sW, sH, u + x, v + y, k);
    sample(src, sW, sH, u - x, v - y, l); sample(src, sW, sH, u + x, v - y, m);
    if (first) {
        float g0[3], g1[3], g2[3], g3[3], g4[3];
        sum4(a, b, d, e, 0.03125f, g0); sum4(b, c, e, f, 0.03125f, g1); sum4(d, e, g, h, 0.03125f, g2); sum4(e, f, h, i, 0.03125f, g3);
        sum4(j, k, l, m, 0.125f, g4);
        karis(g0); karis(g1); karis(g2); karis(g3); karis(g4);
        for (int ch = 0; ch < 3; ++ch) rgb[ch] = fmaxf((((g0[ch] + g1[ch]) + g2[ch]) + g3[ch]) + g4[ch], 0.0001f);
    } else {
        float s0[3], s1[3], s2[3];
        sum4(a, c, g, i, 0.03125f, s0); sum4(b, d, f, h, 0.0625f, s1); sum4(j, k, l, m, 0.125f, s2);
        for (int ch = 0; ch < 3; ++ch) rgb[ch] = ((e[ch] * 0.125f + s0[ch]) + s1[ch]) + s2[ch];
    }
}

static void upsample_texel(const uint32_t* src, uint32_t sW, uint32_t sH, uint32_t dW, uint32_t dH, float r, uint32_t px, uint32_t py, float rgb[3])
{
    const float u = ((float)px + 0.5f) / (float)dW, v = ((float)py + 0.5f) / (float)dH;
    float a[3], b[3], c[3], d[3], e[3], f[3], g[3], h[3], i[3], s1[3], s2[3];
    sample(src, sW, sH, u - r, v + r, a); sample(src, sW, sH, u, v + r, b); sample(src, sW, sH, u + r, v + r, c);
    sample(src, sW, sH, u - r, v, d);     sample(src, sW, sH, u, v, e);     sample(src, sW, sH, u + r, v, f);
    sample(src, sW, sH, u - r, v - r, g); sample(src, sW, sH, u, v - r, h); sample(src, sW, sH, u + r, v - r, i);
    sum4(b, d, f, h, 2.0f, s1); sum4(a, c, g, i, 1.0f, s2);                 /* * 1.0f is exact: (a + c + g + i) as written */
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = ((e[ch] * 4.0f + s1[ch]) + s2[ch]) * 0.0625f;
}

/* PS_Downsample over a dW x dH destination: words out (dW * dH) and, when rgb != NULL, the floats before the store */
void bl_downsample(const uint32_t* src, uint32_t sW, uint32_t sH, uint32_t dW, uint32_t dH, float invX, float invY, uint32_t first,
                   uint32_t* out, float* rgb)
{
    for (uint32_t py = 0; py < dH; ++py)
        for (uint32_t px = 0; px < dW; ++px) {
            float c[3];
            downsample_texel(src, sW, sH, dW, dH, invX, invY, first, px, py, c);
            out[(uint64_t)py * dW + px] = pack_r11g11b10(c[0], c[1], c[2]);
            if (rgb) memcpy(rgb + 3 * ((uint64_t)py * dW + px), c, 12);
        }
}

void bl_upsample(const uint32_t* src, uint32_t sW, uint32_t sH, uint32_t dW, uint32_t dH, float radius, uint32_t* out, float* rgb)
{
    for (uint32_t py = 0; py < dH; ++py)
        for (uint32_t px = 0; px < dW; ++px) {
            float c[3];
            upsample_texel(src, sW, sH, dW, dH, radius, px, py, c);
            out[(uint64_t)py * dW + px] = pack_r11g11b10(c[0], c[1], c[2]);
            if (rgb) memcpy(rgb + 3 * ((uint64_t)py * dW + px), c, 12);
        }
}

/* BloomRenderer::Render.  chain: the mips packed one after the other (mip k of (W >> k) x (H >> k) words); mip 0 is written by
 * the last upsample only, so it needs no initial value.  W >> (mips - 1) and H >> (mips - 1) must be >= 1. */
void bl_chain(const uint32_t* colour, uint32_t W, uint32_t H, uint32_t mips, float radius, uint32_t* chain)
{
    uint64_t off[17];
    off[0] = 0;
    for (uint32_t k = 0; k < mips; ++k) off[k + 1] = off[k] + (uint64_t)(W >> k) * (H >> k);
    for (uint32_t i = 0; i + 1 < mips; ++i)
        bl_downsample(i == 0 ? colour : chain + off[i], W >> i, H >> i, W >> (i + 1), H >> (i + 1), 1.0f / (float)(W >> i), 1.0f / (float)(H >> i),
                      i == 0, chain + off[i + 1], NULL);
    for (uint32_t i = 0; i + 1 < mips; ++i) {
        const uint32_t s = mips - 1 - i, d = s - 1;
        bl_upsample(chain + off[s], W >> s, H >> s, W >> d, H >> d, radius, chain + off[d], NULL);
    }
}
