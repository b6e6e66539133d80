/* gtao_ref.c -- test reference and DEFINITION of "ambientocclusion_CS_XeGTAO_PrefilterDepths", "ambientocclusion_CS_XeGTAO_MainPass
 * DEBUG_OUTPUT_MODE=0" and "ambientocclusion_CS_XeGTAO_Denoise" (csrc/k_ambientocclusion.hip, csrc/soft_math.hip.h): XeGTAO with
 * binary16 arithmetic, 16-bit working depths, no bent normals, the compiled-in default constants.  Compiled by the tests themselves
 * with gcc -O2 -ffp-contract=off: only the fmaf calls written here fuse.  The GPU matches every word: each fp16 depth texel, each
 * edge byte, each working byte and each final byte.
 *
 * CONVENTION (DESIGN.md 3 repeats it).
 *   binary16  : gcc has no _Float16 on x86, so a binary16 value ("h") is carried as the binary32 of the same value and every
 *               h operation (+ - * / sqrt) is the binary32 operation followed by r16(), round to nearest even to binary16 with
 *               subnormals kept and overflow to infinity.  As 24 >= 2 * 11 + 2 this is the IEEE binary16 operation, so the
 *               kernel uses native fp16 + - *; it divides and takes square roots in binary32 and rounds, like this file.
 *   composite : hlerp(x, y, s) = x + s * (y - x); hdot(a, b) = ((a.x b.x + a.y b.y) + a.z b.z) (+ a.w b.w); hlength = sqrt(hdot(v, v));
 *               hnormalize = v / hlength(v) (one division per component); hcross = (a.y b.z - a.z b.y, a.z b.x - a.x b.z,
 *               a.x b.y - a.y b.x); saturate = fmin(fmax(x, 0), 1) (a NaN gives 0); frac = x - floor(x); round = rint (half to even);
 *               min / max = fmin / fmax (a NaN operand is dropped); sign(x) = x > 0 ? 1 : x < 0 ? -1 : 0; every step rounded, in
 *               the order written, nothing contracted.
 *   types     : as HLSL: an unsuffixed literal takes the other operand's type (the binary16 nearest its decimal value, written
 *               below in hexadecimal); h (+) float is float; a cast rounds.  The lines where the reference mixes the two:
 *               normalizedScreenPos (float), the R2 noise (float until its cast), pixCenterPos and viewVec (float, cast after
 *               normalize), pixelDirRBViewspaceSizeAtCenterZ ((float)viewspaceZ * float, cast before the division), the mip level
 *               (h log2 minus float offset, clamped in float, cast), sampleScreenPos (float + h), the float3 sample positions and
 *               deltas, sampleDist ((h) of a float length), sampleHorizonVec ((h) of float / (float)h), the view-space normal
 *               (float until its cast).  binary32 parts follow the lighting convention: dot3 = fmaf(a.z, b.z, fmaf(a.y, b.y,
 *               a.x * b.x)), normalize = v / sqrt(dot3(v, v)), a * b + c as two operations.
 *   software  : sin / cos = gt_sin / gt_cos below on the converted argument, rounded once to h; log2(x) = x > 0 ? r16(log2Soft(x))
 *               : -inf; pow(v, p) = v > 0 ? r16(exp2Signed(p * log2Soft(v))) : 0; pow(s, 2.0) = s * s; FastSqrt and FastACos are
 *               the reference's bit trick and polynomial, literally.
 *   uint(x)   : !(x >= 0) gives 0 (NaN, negative), x >= 2^32 gives 0xFFFFFFFF, else truncation.  An R8_UINT store keeps
 *               min(word, 255).  An R8_UNORM store is uint(saturate(v) * 255.0f + 0.5f) in binary32; its load (float)byte / 255.0f
 *               rounded to h.
 *   textures  : a mip k of a W x H chain is max(W >> k, 1) x max(H >> k, 1) (the back end's rule for every chain).  GatherRed at
 *               pix * ViewportPixelSize with offset o reads texels (pix + o - 1 + {0, 1}) with every coordinate clamped to the
 *               extent: it does not look at ViewportPixelSize.  SampleLevel(point, uv, mip) reads level (int)floor(mip + 0.5f)
 *               clamped to [0, 4] at texel floor(u * (float)w), floor(v * (float)h), each clamped as a float (NaN gives 0).
 *   special   : whatever these rules give.  With the project's projection DepthUnpackConsts = (-near, +0): a depth word of +0
 *               gives -near / (0 - 0) = -inf, which the clamp turns into view depth 0; a NaN depth gives 0 likewise.
 */
#include "ref_formats.h"
#include "ref_soft_math.h"

typedef float hf;                                 /* a binary16 value, carried exactly */
typedef struct { int32_t ViewportSize[2]; float ViewportPixelSize[2]; float DepthUnpackConsts[2]; float CameraTanHalfFOV[2];
                 float NDCToViewMul[2]; float NDCToViewAdd[2]; float NDCToViewMul_x_PixelSize[2]; float EffectRadius, EffectFalloffRange;
                 float RadiusMultiplier, Padding0, FinalValuePower, DenoiseBlurBeta;
                 float SampleDistributionPower, ThinOccluderCompensation, DepthMIPSamplingOffset; int32_t NoiseIndex; } GtConsts;
typedef struct { float m[4][4]; uint32_t quality; } GtMainPush;
typedef struct { hf x, y, z; } H3;
typedef struct { hf x, y, z, w; } H4;
typedef struct { float x, y, z; } F3;

/* ---- binary32 -> binary16, round to nearest even ------------------------------------------------------------------------ */
float gt_r16(float x)
{
    const uint32_t u = bits_of(x), s = u & 0x80000000u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return x;                                         /* NaN */
    if (a >= 0x477FF000u) return float_of(s | 0x7F800000u);                /* >= 65520: infinity (65520 is the tie, to even) */
    if (a < 0x38800000u) {                                                 /* below 2^-14: a multiple of 2^-24 */
        const float m = (float_of(a) + 0.5f) - 0.5f;                       /* ulp of [0.5, 1) is 2^-24: the add rounds to even, the subtraction is exact */
        return float_of(s | bits_of(m));
    }
    return float_of(s | ((a + 0x0FFFu + ((a >> 13) & 1u)) & 0xFFFFE000u));
}
#define r16 gt_r16

/* the word of a binary16 value and back: the conversions of tests/ref_base.h (the passes hand gt_half_bits exact values only) */
uint16_t gt_half_bits(float h) { return float_to_half(h); }
float gt_half_value(uint16_t w) { return half_to_float(w); }

static hf hadd(hf a, hf b) { return r16(a + b); }
static hf hsub(hf a, hf b) { return r16(a - b); }
static hf hmul(hf a, hf b) { return r16(a * b); }
static hf hdiv(hf a, hf b) { return r16(a / b); }
static hf hsqrt(hf a) { return r16(sqrtf(a)); }
static hf hmin(hf a, hf b) { return fminf(a, b); }
static hf hmax(hf a, hf b) { return fmaxf(a, b); }
static hf hsat(hf a) { return fminf(fmaxf(a, 0.0f), 1.0f); }
static hf hlerp(hf x, hf y, hf s) { return hadd(x, hmul(s, hsub(y, x))); }
static hf hdot2(hf ax, hf ay, hf bx, hf by) { return hadd(hmul(ax, bx), hmul(ay, by)); }
static hf hdot3(H3 a, H3 b) { return hadd(hadd(hmul(a.x, b.x), hmul(a.y, b.y)), hmul(a.z, b.z)); }
static hf hdot4(H4 a, H4 b) { return hadd(hadd(hadd(hmul(a.x, b.x), hmul(a.y, b.y)), hmul(a.z, b.z)), hmul(a.w, b.w)); }
static hf hlength3(H3 a) { return hsqrt(hdot3(a, a)); }
static H3 hnormalize3(H3 a) { const hf l = hlength3(a); const H3 r = { hdiv(a.x, l), hdiv(a.y, l), hdiv(a.z, l) }; return r; }
static H3 hcross(H3 a, H3 b)
{
    const H3 r = { hsub(hmul(a.y, b.z), hmul(a.z, b.y)), hsub(hmul(a.z, b.x), hmul(a.x, b.z)), hsub(hmul(a.x, b.y), hmul(a.y, b.x)) };
    return r;
}
static hf hsign(hf x) { return x > 0.0f ? 1.0f : x < 0.0f ? -1.0f : 0.0f; }
static uint32_t to_uint(float x) { return !(x >= 0.0f) ? 0u : x >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)x; }
static float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
static float dot3f(F3 a, F3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }

/* the literals of XeGTAO.hlsli as binary16 */
#define H_PI          0x1.92p+1f       /* 3.14159..., also FastACos' 3.141593 */
#define H_PI_HALF     0x1.92p+0f       /* 1.57079..., also FastACos' 1.570796 */
#define H_GOLDEN      0x1.3c8p-1f      /* 0.6180339887498948482 */
#define H_0_9992      0x1.ff8p-1f
#define H_1_3         0x1.4ccp+0f
#define H_0_011       0x1.688p-7f
#define H_2_9         0x1.734p+1f
#define H_64_255      0x1.01p-2f
#define H_16_255      0x1.01p-4f
#define H_4_255       0x1.01p-6f
#define H_1_255       0x1.01p-8f
#define H_ACOS_C      -0x1.40cp-3f     /* -0.156583 */
#define H_DIAG        0x1.b34p-2f      /* 0.85 * 0.5 */
#define H_0_615       0x1.3bp-1f       /* (h)XE_GTAO_DEFAULT_FALLOFF_RANGE */
#define H_1_457       0x1.75p+0f       /* (h)XE_GTAO_DEFAULT_RADIUS_MULTIPLIER */
#define H_0_03        0x1.eb8p-6f
#define H_0_05        0x1.998p-5f

/* ---- software sine and cosine, |x| <= 10 ---------------------------------------------------------------------------------
 * k = rintf(x * RN(2 / pi)), |k| <= 7; r = x - k * pi / 2 by three fmaf against P1 + P2 + P3 = pi / 2 - 6.1e-17 (P1, P2 with
 * their low 11 bits zero, so k * P1 and k * P2 are exact for |k| < 2^11).  |r| <= pi / 4 + 10 * 2^-24 * 0.64 + ... < 0.7855: the
 * fits below hold on [-0.8, 0.8].
 *   sin r = r + r z S(z), cos r = 1 - z / 2 + z^2 C(z), z = r * r; S and C are the degree-2 weighted least-squares fits of
 *   (sin r / r - 1) / z and (cos r - 1 + z / 2) / z^2 at 400 Chebyshev nodes of z in [0, 0.64] (weights r^3 and z^2, so that the
 *   residual is the error of the result), coefficients rounded to binary32.  Truncation on 400 001 points, coefficients as
 *   rounded: sin 0.067 * 2^-24, cos 0.014 * 2^-24.
 *   quadrant q = k & 3: sin x = S, C, -S, -C; cos x = C, -S, -C, S.
 * ERROR, absolute, in units of u = 2^-24.  Reduction: each fmaf rounds a result of magnitude below 1 (the first: below 1 when it
 * is not exact), at most 0.5 u each, and |d sin|, |d cos| <= 1: 1.5 u; the representation of pi / 2: 7 * 6.1e-17, nothing.
 * sin: the last fmaf 0.5 u (|result| < 1); z's rounding moves r z S by 2^-24 * 0.081: 0.08 u; the product r * z by as much: 0.08 u;
 * S's two fmaf round by 2^-27 together at most, times |r z| <= 0.49: nothing; truncation 0.067 u: 0.73 u.  cos: fmaf(-0.5, z, 1)
 * 0.5 u, the outer fmaf 0.5 u, z^2's two roundings times C <= 0.0417: 0.01 u, truncation 0.014 u, z's rounding 0.32 * 2^-24 -> 0.32 u:
 * 1.35 u.  BOUND 3 u = GT_SINCOS_BOUND (1.79e-7); rounded to binary16 the result (|.| <= 1) is within 2^-12 + 3 u.  Measured
 * maxima: DESIGN.md 9.
 * !(|x| <= 10) (larger, infinite, NaN) gives NaN.  The pass forms |x| <= 3 pi only: phi in [0, pi], n +- pi / 2, 2 h - n. */
const double GT_SINCOS_BOUND = 3.0 * 0x1p-24;
static const float kTwoOverPi = 0x1.45f306p-1f, kP1 = 0x1.921p+0f, kP2 = 0x1.f6ap-13f, kP3 = 0x1.110b46p-26f;
static const float kSinC[3] = { -0x1.55553cp-3f, 0x1.1104a6p-7f, -0x1.98896ep-13f };
static const float kCosC[3] = { 0x1.55554ap-5f, -0x1.6c0b94p-10f, 0x1.99bcaap-16f };

static float sincos_soft(float x, int quarter)                            /* quarter 0: sin, 1: cos = sin(x + pi / 2) */
{
    if (!(fabsf(x) <= 10.0f)) return float_of(0x7FC00000u);
    const float k = rintf(x * kTwoOverPi);
    float r = fmaf(-k, kP1, x);
    r = fmaf(-k, kP2, r);
    r = fmaf(-k, kP3, r);
    const float z = r * r;
    const int q = ((int)k + quarter) & 3;
    float v;
    if (q & 1) {
        float p = kCosC[2];
        p = fmaf(p, z, kCosC[1]);
        p = fmaf(p, z, kCosC[0]);
        v = fmaf(z * z, p, fmaf(-0.5f, z, 1.0f));
    } else {
        float p = kSinC[2];
        p = fmaf(p, z, kSinC[1]);
        p = fmaf(p, z, kSinC[0]);
        v = fmaf(r * z, p, r);
    }
    return (q & 2) ? -v : v;
}
float gt_sin(float x) { return sincos_soft(x, 0); }
float gt_cos(float x) { return sincos_soft(x, 1); }
static hf hsin(hf x) { return r16(gt_sin(x)); }
static hf hcos(hf x) { return r16(gt_cos(x)); }
static hf hlog2(hf x) { return x > 0.0f ? r16(log2_soft(x)) : -INFINITY; }
static hf hpow(hf v, hf p) { return r16(pow_soft(v, p)); }

/* ---- XeGTAO_FastSqrt, XeGTAO_FastACos ------------------------------------------------------------------------------------ */
static hf fast_sqrt(float x) { return r16(float_of(0x1FBD1DF5u + (uint32_t)((int32_t)bits_of(x) >> 1))); }
static hf fast_acos(hf inX)
{
    const hf x = fabsf(inX);
    hf res = hadd(hmul(H_ACOS_C, x), H_PI_HALF);
    res = hmul(res, fast_sqrt(hsub(1.0f, x)));
    return inX >= 0.0f ? res : hsub(H_PI, res);
}

/* ---- the Hilbert index of (x, y) mod 64, branch-free -------------------------------------------------------------------- */
uint32_t gt_hilbert(uint32_t x, uint32_t y)
{
    uint32_t index = 0u;
    x &= 63u; y &= 63u;
    for (uint32_t level = 32u; level > 0u; level >>= 1) {
        const uint32_t rx = (x & level) != 0u, ry = (y & level) != 0u;
        index += level * level * ((3u * rx) ^ ry);
        const uint32_t flip = 63u * (rx & (ry ^ 1u));                      /* regionY == 0 and regionX == 1: mirror both */
        const uint32_t fx = x ^ flip, fy = y ^ flip;                       /* 63 - v == v ^ 63 for v in [0, 63] */
        const uint32_t swap = (fx ^ fy) & (0u - (ry ^ 1u));                /* regionY == 0: exchange */
        x = fx ^ swap; y = fy ^ swap;
    }
    return index;
}

/* ---- texture access ----------------------------------------------------------------------------------------------------- */
static uint32_t mip_dim(uint32_t d, uint32_t k) { return (d >> k) ? (d >> k) : 1u; }
static uint32_t clampi(int32_t v, uint32_t dim) { return v < 0 ? 0u : (uint32_t)v >= dim ? dim - 1u : (uint32_t)v; }
uint64_t gt_chain_offset(uint32_t W, uint32_t H, uint32_t k)
{
    uint64_t off = 0;
    for (uint32_t j = 0; j < k; ++j) off += (uint64_t)mip_dim(W, j) * mip_dim(H, j);
    return off;
}

/* ---- pass 1: depths ----------------------------------------------------------------------------------------------------- */
static hf clamp_depth(float d) { return r16(clampf(d, 0.0f, 65504.0f)); }
static hf view_depth(float d, const GtConsts* k) { return clamp_depth(k->DepthUnpackConsts[0] / (k->DepthUnpackConsts[1] - d)); }

static void falloff_terms(const GtConsts* k, hf effectRadius, hf* mul, hf* add)
{
    const hf falloffRange = hmul(H_0_615, effectRadius);
    const hf falloffFrom = hmul(effectRadius, hsub(1.0f, r16(k->EffectFalloffRange)));
    *mul = hdiv(-1.0f, falloffRange);
    *add = hadd(hdiv(falloffFrom, falloffRange), 1.0f);
}

static hf mip_filter(hf d0, hf d1, hf d2, hf d3, const GtConsts* k)
{
    const hf maxDepth = hmax(hmax(d0, d1), hmax(d2, d3));
    const hf effectRadius = hmul(hmul(0.75f, r16(k->EffectRadius)), H_1_457);
    hf mul, add;
    falloff_terms(k, effectRadius, &mul, &add);
    const hf w0 = hsat(hadd(hmul(hsub(maxDepth, d0), mul), add));
    const hf w1 = hsat(hadd(hmul(hsub(maxDepth, d1), mul), add));
    const hf w2 = hsat(hadd(hmul(hsub(maxDepth, d2), mul), add));
    const hf w3 = hsat(hadd(hmul(hsub(maxDepth, d3), mul), add));
    const hf weightSum = hadd(hadd(hadd(w0, w1), w2), w3);
    return hdiv(hadd(hadd(hadd(hmul(w0, d0), hmul(w1, d1)), hmul(w2, d2)), hmul(w3, d3)), weightSum);
}

/* chain: the five mips packed back to back (gt_chain_offset), binary16 words; texels outside a mip's extent are not stored */
void gt_prefilter(const GtConsts* k, uint32_t W, uint32_t H, const float* depth, uint16_t* chain)
{
    uint16_t* mip[5]; uint32_t mw[5], mh[5];
    for (uint32_t j = 0; j < 5; ++j) { mip[j] = chain + gt_chain_offset(W, H, j); mw[j] = mip_dim(W, j); mh[j] = mip_dim(H, j); }
    for (uint32_t gy = 0; gy < (H + 15u) / 16u; ++gy)
        for (uint32_t gx = 0; gx < (W + 15u) / 16u; ++gx) {
            hf scratch[8][8];
            for (uint32_t ty = 0; ty < 8; ++ty)
                for (uint32_t tx = 0; tx < 8; ++tx) {
                    const uint32_t bx = gx * 8u + tx, by = gy * 8u + ty, px = bx * 2u, py = by * 2u;
                    const uint32_t x0 = clampi((int32_t)px, W), x1 = clampi((int32_t)px + 1, W), y0 = clampi((int32_t)py, H), y1 = clampi((int32_t)py + 1, H);
                    const hf d0 = view_depth(depth[(uint64_t)y0 * W + x0], k), d1 = view_depth(depth[(uint64_t)y0 * W + x1], k);
                    const hf d2 = view_depth(depth[(uint64_t)y1 * W + x0], k), d3 = view_depth(depth[(uint64_t)y1 * W + x1], k);
                    if (px < W && py < H) mip[0][(uint64_t)py * W + px] = gt_half_bits(d0);
                    if (px + 1u < W && py < H) mip[0][(uint64_t)py * W + px + 1u] = gt_half_bits(d1);
                    if (px < W && py + 1u < H) mip[0][(uint64_t)(py + 1u) * W + px] = gt_half_bits(d2);
                    if (px + 1u < W && py + 1u < H) mip[0][(uint64_t)(py + 1u) * W + px + 1u] = gt_half_bits(d3);
                    const hf dm1 = mip_filter(d0, d1, d2, d3, k);
                    if (bx < mw[1] && by < mh[1]) mip[1][(uint64_t)by * mw[1] + bx] = gt_half_bits(dm1);
                    scratch[tx][ty] = dm1;
                }
            for (uint32_t level = 2; level <= 4; ++level) {
                const uint32_t step = 1u << (level - 1u), half = step >> 1;
                for (uint32_t ty = 0; ty < 8; ty += step)
                    for (uint32_t tx = 0; tx < 8; tx += step) {
                        const hf v = mip_filter(scratch[tx][ty], scratch[tx + half][ty], scratch[tx][ty + half], scratch[tx + half][ty + half], k);
                        const uint32_t ox = (gx * 8u + tx) >> (level - 1u), oy = (gy * 8u + ty) >> (level - 1u);
                        if (ox < mw[level] && oy < mh[level]) mip[level][(uint64_t)oy * mw[level] + ox] = gt_half_bits(v);
                        scratch[tx][ty] = v;
                    }
            }
        }
}

/* ---- pass 2: the main pass ---------------------------------------------------------------------------------------------- */
static H4 calculate_edges(hf c, hf l, hf r, hf t, hf b)
{
    H4 e = { hsub(l, c), hsub(r, c), hsub(t, c), hsub(b, c) };
    const hf slopeLR = hmul(hsub(e.y, e.x), 0.5f), slopeTB = hmul(hsub(e.w, e.z), 0.5f);
    const H4 adj = { hadd(e.x, slopeLR), hadd(e.y, -slopeLR), hadd(e.z, slopeTB), hadd(e.w, -slopeTB) };
    e.x = hmin(fabsf(e.x), fabsf(adj.x)); e.y = hmin(fabsf(e.y), fabsf(adj.y)); e.z = hmin(fabsf(e.z), fabsf(adj.z)); e.w = hmin(fabsf(e.w), fabsf(adj.w));
    const hf den = hmul(c, H_0_011);
    const H4 out = { hsat(hsub(1.25f, hdiv(e.x, den))), hsat(hsub(1.25f, hdiv(e.y, den))), hsat(hsub(1.25f, hdiv(e.z, den))), hsat(hsub(1.25f, hdiv(e.w, den))) };
    return out;
}
static hf pack_edges(H4 e)
{
    const H4 q = { rintf(hmul(hsat(e.x), H_2_9)), rintf(hmul(hsat(e.y), H_2_9)), rintf(hmul(hsat(e.z), H_2_9)), rintf(hmul(hsat(e.w), H_2_9)) };
    const H4 c = { H_64_255, H_16_255, H_4_255, H_1_255 };
    return hdot4(q, c);
}
static uint8_t unorm8_store(hf v) { return (uint8_t)to_uint(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f); }
static hf unorm8_load(uint8_t b) { return r16((float)b / 255.0f); }
static uint8_t uint8_store(uint32_t w) { return (uint8_t)(w < 255u ? w : 255u); }

static F3 view_position(float sx, float sy, float depth, const GtConsts* k)
{
    const F3 p = { (k->NDCToViewMul[0] * sx + k->NDCToViewAdd[0]) * depth, (k->NDCToViewMul[1] * sy + k->NDCToViewAdd[1]) * depth, depth };
    return p;
}
static float sample_level(const uint16_t* chain, uint32_t W, uint32_t H, float u, float v, hf mip)
{
    const int level = (int)clampf(floorf(mip + 0.5f), 0.0f, 4.0f);
    const uint32_t w = mip_dim(W, (uint32_t)level), h = mip_dim(H, (uint32_t)level);
    const uint32_t x = (uint32_t)clampf(floorf(u * (float)w), 0.0f, (float)(w - 1u)), y = (uint32_t)clampf(floorf(v * (float)h), 0.0f, (float)(h - 1u));
    return gt_half_value(chain[gt_chain_offset(W, H, (uint32_t)level) + (uint64_t)y * w + x]);
}

/* the view-space normal of a GBufferA texel: UnpackOctadehron of .y (tests/ref_formats.h unpack_oct), the row vector (n, 1) times
 * the matrix, z negated, all in binary32 */
static F3 view_normal(const uint32_t g[4], const GtMainPush* p)
{
    float n[3], o[3];
    unpack_oct(g[1], n);
    for (int j = 0; j < 3; ++j) o[j] = fmaf(n[2], p->m[2][j], fmaf(n[1], p->m[1][j], n[0] * p->m[0][j])) + p->m[3][j];
    const F3 r = { o[0], o[1], o[2] * -1.0f };
    return r;
}

static const float kSlices[4] = { 1.0f, 2.0f, 3.0f, 9.0f }, kSteps[4] = { 2.0f, 2.0f, 3.0f, 2.0f };

static void main_pixel(const GtConsts* k, const GtMainPush* push, uint32_t W, uint32_t H, const uint16_t* chain, const uint32_t* gbufferA,
                       uint32_t px, uint32_t py, uint8_t* outAO, uint8_t* outEdges)
{
    const uint32_t quality = push->quality < 4u ? push->quality : 0u;     /* the switch's default: the initial values, which are Low's */
    const hf sliceCount = kSlices[quality], stepsPerSlice = kSteps[quality];
    uint32_t noiseIndex = gt_hilbert(px % 64u, py % 64u);
    noiseIndex += (uint32_t)(288 * (k->NoiseIndex % 64));
    const float n0 = 0.5f + (float)noiseIndex * 0.75487766624669276005f, n1 = 0.5f + (float)noiseIndex * 0.5698402909980532659114f;
    const hf noiseSlice = r16(n0 - floorf(n0)), noiseSample = r16(n1 - floorf(n1));
    const F3 nf = view_normal(gbufferA + 4u * ((uint64_t)py * W + px), push);
    const H3 viewspaceNormal = { r16(nf.x), r16(nf.y), r16(nf.z) };

    const float nspx = ((float)px + 0.5f) * k->ViewportPixelSize[0], nspy = ((float)py + 0.5f) * k->ViewportPixelSize[1];
    const uint32_t xl = clampi((int32_t)px - 1, W), xr = clampi((int32_t)px + 1, W), yt = clampi((int32_t)py - 1, H), yb = clampi((int32_t)py + 1, H);
    hf viewspaceZ = gt_half_value(chain[(uint64_t)py * W + px]);
    const hf pixLZ = gt_half_value(chain[(uint64_t)py * W + xl]), pixRZ = gt_half_value(chain[(uint64_t)py * W + xr]);
    const hf pixTZ = gt_half_value(chain[(uint64_t)yt * W + px]), pixBZ = gt_half_value(chain[(uint64_t)yb * W + px]);
    outEdges[(uint64_t)py * W + px] = unorm8_store(pack_edges(calculate_edges(viewspaceZ, pixLZ, pixRZ, pixTZ, pixBZ)));

    viewspaceZ = hmul(viewspaceZ, H_0_9992);
    const F3 pixCenterPos = view_position(nspx, nspy, viewspaceZ, k);
    const F3 neg = { -pixCenterPos.x, -pixCenterPos.y, -pixCenterPos.z };
    const float negLen = sqrtf(dot3f(neg, neg));
    const H3 viewVec = { r16(neg.x / negLen), r16(neg.y / negLen), r16(neg.z / negLen) };

    const hf effectRadius = hmul(r16(k->EffectRadius), H_1_457);
    hf falloffMul, falloffAdd;
    falloff_terms(k, effectRadius, &falloffMul, &falloffAdd);

    hf visibility = 0.0f;
    const float pixelDirX = viewspaceZ * k->NDCToViewMul_x_PixelSize[0];
    const hf screenspaceRadius = hdiv(effectRadius, r16(pixelDirX));
    visibility = hadd(visibility, hmul(hsat(hdiv(hsub(10.0f, screenspaceRadius), 100.0f)), 0.5f));
    const hf minS = hdiv(H_1_3, screenspaceRadius);
    const hf pixelSizeX = r16(k->ViewportPixelSize[0]), pixelSizeY = r16(k->ViewportPixelSize[1]);

    for (hf slice = 0.0f; slice < sliceCount; slice += 1.0f) {
        const hf sliceK = hdiv(hadd(slice, noiseSlice), sliceCount);
        const hf phi = hmul(sliceK, H_PI);
        const hf cosPhi = hcos(phi), sinPhi = hsin(phi);
        const hf omegaX = hmul(cosPhi, screenspaceRadius), omegaY = hmul(-sinPhi, screenspaceRadius);
        const H3 directionVec = { cosPhi, sinPhi, 0.0f };
        const hf dv = hdot3(directionVec, viewVec);
        const H3 orthoDirectionVec = { hsub(directionVec.x, hmul(dv, viewVec.x)), hsub(directionVec.y, hmul(dv, viewVec.y)), hsub(directionVec.z, hmul(dv, viewVec.z)) };
        const H3 axisVec = hnormalize3(hcross(orthoDirectionVec, viewVec));
        const hf na = hdot3(viewspaceNormal, axisVec);
        const H3 projectedNormalVec = { hsub(viewspaceNormal.x, hmul(axisVec.x, na)), hsub(viewspaceNormal.y, hmul(axisVec.y, na)), hsub(viewspaceNormal.z, hmul(axisVec.z, na)) };
        const hf signNorm = hsign(hdot3(orthoDirectionVec, projectedNormalVec));
        hf projectedNormalVecLength = hlength3(projectedNormalVec);
        const hf cosNorm = hsat(hdiv(hdot3(projectedNormalVec, viewVec), projectedNormalVecLength));
        const hf n = hmul(signNorm, fast_acos(cosNorm));
        const hf lowHorizonCos0 = hcos(hadd(n, H_PI_HALF)), lowHorizonCos1 = hcos(hsub(n, H_PI_HALF));
        hf horizonCos0 = lowHorizonCos0, horizonCos1 = lowHorizonCos1;

        for (hf step = 0.0f; step < stepsPerSlice; step += 1.0f) {
            const hf stepBaseNoise = hmul(hadd(slice, hmul(step, stepsPerSlice)), H_GOLDEN);
            const hf sn = hadd(noiseSample, stepBaseNoise);
            const hf stepNoise = hsub(sn, floorf(sn));
            hf s = hdiv(hadd(step, stepNoise), stepsPerSlice);
            s = hmul(s, s);
            s = hadd(s, minS);
            hf offX = hmul(s, omegaX), offY = hmul(s, omegaY);
            const hf sampleOffsetLength = hsqrt(hdot2(offX, offY, offX, offY));
            const hf mipLevel = r16(clampf(hlog2(sampleOffsetLength) - k->DepthMIPSamplingOffset, 0.0f, 5.0f));
            offX = hmul(rintf(offX), pixelSizeX); offY = hmul(rintf(offY), pixelSizeY);

            const float u0 = nspx + offX, v0 = nspy + offY, u1 = nspx - offX, v1 = nspy - offY;
            const float SZ0 = sample_level(chain, W, H, u0, v0, mipLevel), SZ1 = sample_level(chain, W, H, u1, v1, mipLevel);
            const F3 p0 = view_position(u0, v0, SZ0, k), p1 = view_position(u1, v1, SZ1, k);
            const F3 d0 = { p0.x - pixCenterPos.x, p0.y - pixCenterPos.y, p0.z - pixCenterPos.z };
            const F3 d1 = { p1.x - pixCenterPos.x, p1.y - pixCenterPos.y, p1.z - pixCenterPos.z };
            const hf sampleDist0 = r16(sqrtf(dot3f(d0, d0))), sampleDist1 = r16(sqrtf(dot3f(d1, d1)));
            const H3 hv0 = { r16(d0.x / sampleDist0), r16(d0.y / sampleDist0), r16(d0.z / sampleDist0) };
            const H3 hv1 = { r16(d1.x / sampleDist1), r16(d1.y / sampleDist1), r16(d1.z / sampleDist1) };
            const hf weight0 = hsat(hadd(hmul(sampleDist0, falloffMul), falloffAdd)), weight1 = hsat(hadd(hmul(sampleDist1, falloffMul), falloffAdd));
            hf shc0 = hdot3(hv0, viewVec), shc1 = hdot3(hv1, viewVec);
            shc0 = hlerp(lowHorizonCos0, shc0, weight0);
            shc1 = hlerp(lowHorizonCos1, shc1, weight1);
            horizonCos0 = hmax(horizonCos0, shc0);
            horizonCos1 = hmax(horizonCos1, shc1);
        }
        projectedNormalVecLength = hlerp(projectedNormalVecLength, 1.0f, H_0_05);
        const hf h0 = -fast_acos(horizonCos1), h1 = fast_acos(horizonCos0);
        const hf sinN = hsin(n);
        const hf th0 = hmul(2.0f, h0), th1 = hmul(2.0f, h1);
        const hf iarc0 = hdiv(hsub(hadd(cosNorm, hmul(th0, sinN)), hcos(hsub(th0, n))), 4.0f);
        const hf iarc1 = hdiv(hsub(hadd(cosNorm, hmul(th1, sinN)), hcos(hsub(th1, n))), 4.0f);
        visibility = hadd(visibility, hmul(projectedNormalVecLength, hadd(iarc0, iarc1)));
    }
    visibility = hdiv(visibility, sliceCount);
    visibility = hpow(visibility, r16(k->FinalValuePower));
    visibility = hmax(H_0_03, visibility);
    visibility = hsat(hdiv(visibility, 1.5f));
    outAO[(uint64_t)py * W + px] = uint8_store(to_uint(hadd(hmul(visibility, 255.0f), 0.5f)));
}

void gt_main(const GtConsts* k, const GtMainPush* push, uint32_t W, uint32_t H, const uint16_t* chain, const uint32_t* gbufferA, uint8_t* outAO, uint8_t* outEdges)
{
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) main_pixel(k, push, W, H, chain, gbufferA, px, py, outAO, outEdges);
}

/* ---- pass 3: denoise ----------------------------------------------------------------------------------------------------- */
static H4 unpack_edges(hf packed)
{
    const uint32_t p = to_uint(hmul(packed, 255.5f));
    const H4 e = { hsat(hdiv((float)((p >> 6) & 3u), 3.0f)), hsat(hdiv((float)((p >> 4) & 3u), 3.0f)), hsat(hdiv((float)((p >> 2) & 3u), 3.0f)), hsat(hdiv((float)(p & 3u), 3.0f)) };
    return e;
}

static void denoise_pixel(const GtConsts* k, uint32_t finalApply, uint32_t W, uint32_t H, const uint8_t* ao, const uint8_t* edges, uint32_t px, uint32_t py, uint8_t* out)
{
    const hf blurAmount = finalApply ? r16(k->DenoiseBlurBeta) : hdiv(r16(k->DenoiseBlurBeta), 5.0f);
    const uint32_t xs[3] = { clampi((int32_t)px - 1, W), px, clampi((int32_t)px + 1, W) }, ys[3] = { clampi((int32_t)py - 1, H), py, clampi((int32_t)py + 1, H) };
#define EDGE(ix, iy) unpack_edges(unorm8_load(edges[(uint64_t)ys[iy] * W + xs[ix]]))
#define VIS(ix, iy) hdiv((float)ao[(uint64_t)ys[iy] * W + xs[ix]], 255.0f)
    const H4 eL = EDGE(0, 1), eT = EDGE(1, 0), eR = EDGE(2, 1), eB = EDGE(1, 2);
    H4 eC = EDGE(1, 1);
    eC.x = hmul(eC.x, eL.y); eC.y = hmul(eC.y, eR.x); eC.z = hmul(eC.z, eT.w); eC.w = hmul(eC.w, eB.z);
    const H4 ones = { 1.0f, 1.0f, 1.0f, 1.0f };
    const hf edginess = hmul(hdiv(hsat(hsub(hsub(4.0f, 2.5f), hdot4(eC, ones))), hsub(4.0f, 2.5f)), 0.5f);
    eC.x = hsat(hadd(eC.x, edginess)); eC.y = hsat(hadd(eC.y, edginess)); eC.z = hsat(hadd(eC.z, edginess)); eC.w = hsat(hadd(eC.w, edginess));
    const hf weightTL = hmul(H_DIAG, hadd(hmul(eC.x, eL.z), hmul(eC.z, eT.x)));
    const hf weightTR = hmul(H_DIAG, hadd(hmul(eC.z, eT.y), hmul(eC.y, eR.z)));
    const hf weightBL = hmul(H_DIAG, hadd(hmul(eC.w, eB.x), hmul(eC.x, eL.w)));
    const hf weightBR = hmul(H_DIAG, hadd(hmul(eC.y, eR.w), hmul(eC.w, eB.y)));
    hf sumWeight = blurAmount;
    hf sum = hmul(VIS(1, 1), sumWeight);
#define ADD_SAMPLE(v, w) do { const hf w_ = (w); sum = hadd(sum, hmul(w_, (v))); sumWeight = hadd(sumWeight, w_); } while (0)
    ADD_SAMPLE(VIS(0, 1), eC.x);
    ADD_SAMPLE(VIS(2, 1), eC.y);
    ADD_SAMPLE(VIS(1, 0), eC.z);
    ADD_SAMPLE(VIS(1, 2), eC.w);
    ADD_SAMPLE(VIS(0, 0), weightTL);
    ADD_SAMPLE(VIS(2, 0), weightTR);
    ADD_SAMPLE(VIS(0, 2), weightBL);
    ADD_SAMPLE(VIS(2, 2), weightBR);
    hf aoTerm = hdiv(sum, sumWeight);
    aoTerm = hmul(aoTerm, finalApply ? 1.5f : 1.0f);
    out[(uint64_t)py * W + px] = uint8_store(to_uint(hadd(hmul(aoTerm, 255.0f), 0.5f)));
#undef EDGE
#undef VIS
#undef ADD_SAMPLE
}

void gt_denoise(const GtConsts* k, uint32_t finalApply, uint32_t W, uint32_t H, const uint8_t* ao, const uint8_t* edges, uint8_t* out)
{
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) denoise_pixel(k, finalApply, W, H, ao, edges, px, py, out);
}

/* ---- array forms for the tests ------------------------------------------------------------------------------------------ */
void gt_r16_n(const float* x, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gt_r16(x[i]); }
void gt_half_bits_n(const float* x, uint64_t n, uint16_t* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gt_half_bits(x[i]); }
void gt_half_value_n(const uint16_t* w, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gt_half_value(w[i]); }
void gt_sin_n(const float* x, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gt_sin(x[i]); }
void gt_cos_n(const float* x, uint64_t n, float* out) { for (uint64_t i = 0; i < n; ++i) out[i] = gt_cos(x[i]); }
