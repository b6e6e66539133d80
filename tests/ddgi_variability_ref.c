/* ddgi_variability_ref.c -- the definition of probe variability: the value the radiance blend writes per interior texel with
 * DDGIVolumeDesc::flags bit 2 (csrc/k_giprobeblend.hip: blendKernel<radiance, variability>), and of the two reduction passes
 * "ReductionCS_DDGIReductionCS REDUCTION=1" / "ReductionCS_DDGIExtraReductionCS" (csrc/k_ddgireduction.hip) that average it over
 * the volume, which repeat the functions below word for word.  Compile with gcc -O2 -ffp-contract=off (tests/ddgi_variability_ref.py).
 *
 * The RTXGI SDK's shaders are not part of this project: this is the project's own statement of the published idea (a coefficient
 * of variation per texel, averaged over the active probes), and this file is what the tests pin.
 *
 * It includes tests/ddgi_update_ref.c for the blend: the left-alone decision and the ray directions (blend_setup), the texel
 * direction, dg_pow, the easing with its rule bits (ease_radiance), the 10-bit store and the border copy are that file's own
 * functions.  That file keeps the accumulation of `sum` and `sumW` inside blend_radiance, so the loop over the 256 records is
 * written out once more below, in its words; tests/test_ddgi_variability_ref.py holds dv_blend_radiance's irradiance equal to
 * du_blend_radiance's, word for word.
 *
 * CONVENTION.  binary32, no contraction, dot3 = fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)), / and sqrtf correctly rounded.
 *   value     of interior texel (ix, iy) of a probe that is not left alone: res this update's estimate after the soft pow, prev
 *             the decoded stored texel, out ease_radiance's result before saturate and the 10-bit store; per channel
 *             s2 = (res - prev) * (res - out); L = (0.2126f, 0.7152f, 0.0722f); lumS2 = dot3(s2, L); lumMean = dot3(out, L);
 *             value = (lumMean <= 1.0f / 1024.0f || !(lumS2 > 0.0f)) ? 0.0f : sqrtf(lumS2) / lumMean.  The floor of one 10-bit
 *             code and the > 0 guard are the project's own: a channel product can be negative, and no NaN is born here.
 *             A left-alone probe's 36 values keep what they held;
 *   buffer    float[counts.y][6 * counts.z][6 * counts.x]: probe (x, y, z)'s texel (ix, iy) at [y][6 * z + iy][6 * x + ix];
 *   reduction one group per output element (gx, gy, gz), 4 x 8 x 4 threads; thread (tx, ty, tz) covers x = 16 * gx + 4 * tx + i,
 *             y = 16 * gy + 2 * ty + j (i < 4, j < 2), plane z = 4 * gz + tz, summed row-major (j outer) from 0.0f; an input out of
 *             range contributes nothing.  First pass: w = 0.0f when the texel's probe (x / 6, z, y / 6) is inactive (flags bit 1 and
 *             data.w == 1.0f), else 1.0f; sumV = sumV + (w != 0.0f ? v : 0.0f); sumW = sumW + w.  Extra pass over (a, w) pairs:
 *             sumV = sumV + a * w; sumW = sumW + w.  The 128 pairs, t = tx + 4 * ty + 32 * tz, go through the tree
 *             p[t] = p[t] + p[t + stride] for t < stride, stride = 64, 32, ..., 1; the element is (sumW > 0 ? sumV / sumW : 0, sumW);
 *   average   the first pass over (6 * counts.x, 6 * counts.z, counts.y), then extra passes over ceil(extent / (16, 16, 4)) until the
 *             extent is (1, 1, 1) (GIRenderer.cpp:542-573); .x of element 0 of the last pass. */
#include "ddgi_update_ref.c"

/* bits 24.. of a texel's rule word, above ddgi_update_ref.c's DU_R_* bits (which ease_radiance sets in the same word) */
enum { DV_MEAN_FLOOR = 1u << 24,               /* lumMean <= 1 / 1024 */
       DV_S2_NEGATIVE = 1u << 25,              /* lumS2 < 0 */
       DV_S2_ZERO = 1u << 26,                  /* lumS2 == 0 */
       DV_S2_NAN = 1u << 27,
       DV_MEAN_AT_FLOOR = 1u << 28 };          /* lumMean == 1 / 1024 exactly with lumS2 > 0: where <= and < part */

float dv_texel(const float res[3], const float prev[3], const float out[3], uint32_t* rules)
{
    const float L[3] = { 0.2126f, 0.7152f, 0.0722f };
    const float s2[3] = { (res[0] - prev[0]) * (res[0] - out[0]), (res[1] - prev[1]) * (res[1] - out[1]), (res[2] - prev[2]) * (res[2] - out[2]) };
    const float lumS2 = dot3(s2, L), lumMean = dot3(out, L);
    if (rules) {
        if (lumMean <= 1.0f / 1024.0f) *rules |= DV_MEAN_FLOOR;
        if (lumS2 < 0.0f) *rules |= DV_S2_NEGATIVE;
        if (lumS2 == 0.0f) *rules |= DV_S2_ZERO;
        if (lumS2 != lumS2) *rules |= DV_S2_NAN;
        if (lumMean == 1.0f / 1024.0f && lumS2 > 0.0f) *rules |= DV_MEAN_AT_FLOOR;
    }
    return (lumMean <= 1.0f / 1024.0f || !(lumS2 > 0.0f)) ? 0.0f : sqrtf(lumS2) / lumMean;
}

/* The radiance blend with flags bit 2.  irradiance: uint32 [slices][cz * 8][cx * 8], read and written as blend_radiance does;
 * variability: float [slices][cz * 6][cx * 6], written for every probe that is not left alone; rules: uint32 [numProbes][6][6] or
 * NULL, DU_R_* and DV_* bits per interior texel. */
void dv_blend_radiance(const DuBlock* b, const uint16_t* data, const float* rays, uint32_t* irradiance, float* variability, uint32_t* rules)
{
    const DgDesc* D = &b->D;
    const uint32_t N = 8u, I = N - 2u, W = (uint32_t)D->probeCounts[0] * N, H = (uint32_t)D->probeCounts[2] * N;
    const uint32_t VW = (uint32_t)D->probeCounts[0] * I, VH = (uint32_t)D->probeCounts[2] * I;
    const uint32_t probes = (uint32_t)D->probeCounts[0] * (uint32_t)D->probeCounts[1] * (uint32_t)D->probeCounts[2];
    const float invGamma = 1.0f / D->probeIrradianceEncodingGamma;
    for (uint32_t p = 0; p < probes; ++p) {
        int32_t c[3];
        float dir[DU_RAYS][3];
        if (blend_setup(b, data, rays, p, c, dir)) { if (rules) for (uint32_t t = 0; t < 36u; ++t) rules[(uint64_t)p * 36u + t] = DU_R_LEFT_ALONE; continue; }
        uint32_t* tile = irradiance + (uint64_t)c[1] * W * H + (uint64_t)((uint32_t)c[2] * N) * W + (uint32_t)c[0] * N;
        for (uint32_t ty = 1; ty <= N - 2u; ++ty)
            for (uint32_t tx = 1; tx <= N - 2u; ++tx) {
                float texelDir[3], sum[3] = { 0.0f, 0.0f, 0.0f }, sumW = 0.0f, res[3], prev[3], out[3];
                du_texel_direction(tx - 1u, ty - 1u, N - 2u, texelDir);
                const uint32_t old = tile[ty * W + tx];
                for (uint32_t r = 0; r < DU_RAYS; ++r) {                      /* blend_radiance's loop, in its words */
                    const float* rec = rays + ((uint64_t)p * DU_RAYS + r) * 4u;
                    if (rec[3] < 0.0f) continue;
                    const float w = fmaxf(0.0f, dot3(texelDir, dir[r]));
                    sum[0] = sum[0] + rec[0] * w; sum[1] = sum[1] + rec[1] * w; sum[2] = sum[2] + rec[2] * w;
                    sumW = sumW + w;
                }
                const float den = 2.0f * fmaxf(sumW, 1e-9f * 256.0f);
                for (int ch = 0; ch < 3; ++ch) {
                    res[ch] = dg_pow(sum[ch] / den, invGamma);
                    prev[ch] = (float)((old >> (10 * ch)) & 1023u) / 1023.0f;
                }
                uint32_t* rule = rules ? rules + (uint64_t)p * 36u + (ty - 1u) * 6u + (tx - 1u) : NULL;
                if (rule) *rule = 0u;
                ease_radiance(&b->k, res, prev, 1, out, rule);
                tile[ty * W + tx] = du_unorm10(out[0]) | du_unorm10(out[1]) << 10 | du_unorm10(out[2]) << 20 | 3u << 30;
                variability[((uint64_t)c[1] * VH + ((uint32_t)c[2] * I + (ty - 1u))) * VW + ((uint32_t)c[0] * I + (tx - 1u))] = dv_texel(res, prev, out, rule);
            }
        for (uint32_t ty = 0; ty < N; ++ty)
            for (uint32_t tx = 0; tx < N; ++tx) {
                if (tx >= 1u && tx <= N - 2u && ty >= 1u && ty <= N - 2u) continue;
                uint32_t sx, sy;
                border_source(tx, ty, N, &sx, &sy);
                tile[ty * W + tx] = tile[sy * W + sx];
            }
    }
}

/* ---- the reductions ------------------------------------------------------------------------------------------------------------ */
#define DV_THREADS 128u

/* the group's tree over p[128], in place; the sum is p[0] */
void dv_tree(float* p)
{
    for (uint32_t stride = DV_THREADS / 2u; stride >= 1u; stride >>= 1)
        for (uint32_t t = 0; t < stride; ++t) p[t] = p[t] + p[t + stride];
}

static uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }

/* One pass.  first: in is float[Z][Y][X] and D, data say which probes are inactive; else in is float2[Z][Y][X].
 * out: float2 [ceil(Z / 4)][ceil(Y / 16)][ceil(X / 16)]. */
static void reduce(int first, const DgDesc* D, const uint16_t* data, const float* in, uint32_t X, uint32_t Y, uint32_t Z, float* out)
{
    const uint32_t GX = ceil_div(X, 16u), GY = ceil_div(Y, 16u), GZ = ceil_div(Z, 4u);
    for (uint32_t gz = 0; gz < GZ; ++gz)
        for (uint32_t gy = 0; gy < GY; ++gy)
            for (uint32_t gx = 0; gx < GX; ++gx) {
                float pV[DV_THREADS], pW[DV_THREADS];
                for (uint32_t tz = 0; tz < 4u; ++tz)
                    for (uint32_t ty = 0; ty < 8u; ++ty)
                        for (uint32_t tx = 0; tx < 4u; ++tx) {
                            float sumV = 0.0f, sumW = 0.0f;
                            const uint32_t z = 4u * gz + tz;
                            for (uint32_t j = 0; j < 2u && z < Z; ++j)
                                for (uint32_t i = 0; i < 4u; ++i) {
                                    const uint32_t x = 16u * gx + 4u * tx + i, y = 16u * gy + 2u * ty + j;
                                    if (x >= X || y >= Y) continue;
                                    const uint64_t at = ((uint64_t)z * Y + y) * X + x;
                                    if (first) {
                                        const uint32_t cx = (uint32_t)D->probeCounts[0], cz = (uint32_t)D->probeCounts[2];
                                        const float state = half_to_float(data[(((uint64_t)z * cz + y / 6u) * cx + x / 6u) * 4u + 3u]);
                                        const float w = ((D->flags & 2u) && state == 1.0f) ? 0.0f : 1.0f;
                                        const float v = in[at];
                                        sumV = sumV + (w != 0.0f ? v : 0.0f);
                                        sumW = sumW + w;
                                    } else {
                                        const float a = in[2u * at], w = in[2u * at + 1u];
                                        sumV = sumV + a * w;
                                        sumW = sumW + w;
                                    }
                                }
                            pV[tx + 4u * ty + 32u * tz] = sumV; pW[tx + 4u * ty + 32u * tz] = sumW;
                        }
                dv_tree(pV); dv_tree(pW);
                float* o = out + (((uint64_t)gz * GY + gy) * GX + gx) * 2u;
                o[0] = pW[0] > 0.0f ? pV[0] / pW[0] : 0.0f;
                o[1] = pW[0];
            }
}

void dv_reduce_first(const DgDesc* D, const uint16_t* data, const float* variability, float* out)
{
    reduce(1, D, data, variability, (uint32_t)D->probeCounts[0] * 6u, (uint32_t)D->probeCounts[2] * 6u, (uint32_t)D->probeCounts[1], out);
}

void dv_reduce_extra(const float* in, uint32_t X, uint32_t Y, uint32_t Z, float* out) { reduce(0, NULL, NULL, in, X, Y, Z, out); }

/* The whole average (GIRenderer.cpp:542-573): scratch holds two buffers of the first pass's output size, float2 each element;
 * returns .x of element 0 of the last pass and, in *weight, its .y; *passes (may be NULL) the number of passes. */
float dv_average(const DgDesc* D, const uint16_t* data, const float* variability, float* scratch, float* weight, uint32_t* passes)
{
    uint32_t X = (uint32_t)D->probeCounts[0] * 6u, Y = (uint32_t)D->probeCounts[2] * 6u, Z = (uint32_t)D->probeCounts[1], n = 0;
    const uint64_t elements = (uint64_t)ceil_div(X, 16u) * ceil_div(Y, 16u) * ceil_div(Z, 4u);
    float* buffers[2] = { scratch, scratch + 2u * elements };
    const float* last = NULL;
    while (n == 0 || X > 1u || Y > 1u || Z > 1u) {
        float* out = buffers[n & 1u];
        if (n == 0) dv_reduce_first(D, data, variability, out);
        else dv_reduce_extra(last, X, Y, Z, out);
        last = out;
        X = ceil_div(X, 16u); Y = ceil_div(Y, 16u); Z = ceil_div(Z, 4u);
        ++n;
    }
    if (weight) *weight = last[1];
    if (passes) *passes = n;
    return last[0];
}
