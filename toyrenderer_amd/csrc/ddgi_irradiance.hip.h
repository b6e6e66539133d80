// ddgi_irradiance.hip.h -- the DDGI irradiance query of "deferredlighting_PS_Main" / "_Debug" (k_deferredlighting.hip): what
// GetDDGIIrradiance(deferredlighting.hlsl:49-76, :133-153) returns for one surface point from a SUPPLIED probe volume.  The RTXGI
// SDK's Irradiance.hlsl is not part of this project; this is the project's own statement of the published query (Majercik et
// al., "Dynamic Diffuse Global Illumination with Ray-Traced Irradiance Fields", JCGT 2019) with the settings GIRenderer.cpp
// configures, and tests/ddgi_ref.c restates it word for word.  Parity with the SDK is unpinned, as for every pass here.
//
// INPUTS.  The DDGIVolumeDesc at t5 (ShaderInterop.h), read on the device; three 2D array textures, slice = probe y:
//   data        RGBA16_FLOAT, texel (x, z): xyz the relocation offset in units of the spacing, w the state (1 = inactive);
//   irradiance  R10G10B10A2_UNORM, probe (x, y, z)'s 8 x 8 tile at texel (x * 8, z * 8): 6 x 6 interior texels and a border;
//   distance    RG16_FLOAT, the 16 x 16 tile at (x * 16, z * 16): r the mean distance / 2, g the mean squared distance / 2.
//
// CONVENTION (the shared part is screen_pass.hip.h's: binary32, no contraction, fma only in dot3, / and sqrt correctly rounded).
//   ext       = (spacing * (float)(counts - 1)) * 0.5f per axis;  normalize(v) = v / sqrt(dot3(v, v)) (a zero vector gives NaN);
//   viewDir   = normalize(world - cameraOrigin);  delta = |world - origin| - ext;
//   blend     = 1 if delta.x < 0 && delta.y < 0 && delta.z < 0, else ((1 - saturate(delta.x / spacing.x)) * (1 - saturate(delta.y /
//               spacing.y))) * (1 - saturate(delta.z / spacing.z));  !(blend > 0): the result is (0, 0, 0);
//   P         = world + (N * normalBias - viewDir * viewBias), each product rounded, then the difference, then the sum;
//   base      = (int)fmin(fmax(((P - origin) + ext) / spacing, 0), (float)(counts - 1)) per axis: clamped as a float, then
//               truncated, which equals clamp(int(.), 0, counts - 1) and is defined for a NaN (0);
//   probePos(c) = ((spacing * (float)c) - ext) + origin, + data(c).xyz * spacing when flags bit 0 (relocation) is set;
//   alpha     = saturate((P - probePos(base)) / spacing);
//   neighbour i = 0..7: off = (i & 1, (i >> 1) & 1, (i >> 2) & 1); c = min(base + off, counts - 1); skipped when flags bit 1
//               (classification) is set and data(c).w == 1.0f; pp = probePos(c); dirW = normalize(pp - world); toB = pp - P;
//               dist = sqrt(dot3(toB, toB)); dirB = toB / dist; tri = fmax(0.001f, off ? alpha : 1 - alpha) per axis (the lerp with
//               a weight of 0 or 1 is a select); wrap = (dot3(dirW, N) + 1) * 0.5f; w = wrap * wrap + 0.2f;
//               d = 2 * bilinear(distance, probeUV(c, oct(-dirB), 14)).rg; var = |d.x * d.x - d.y|;
//               dist > d.x: v = dist - d.x, ch = var / (var + v * v), ch = fmax((ch * ch) * ch, 0); else ch = 1 (a NaN compares false);
//               w = w * fmax(0.05f, ch); w = fmax(0.000001f, w); w < 0.2f: w = w * ((w * w) * (1.0f / (0.2f * 0.2f)));
//               w = w * ((tri.x * tri.y) * tri.z); e = pow(bilinear(irradiance, probeUV(c, oct(N), 6)).rgb, gamma * 0.5f);
//               sum += w * e (product, then sum); wsum += w;
//   result    = wsum == 0 ? 0 : ((((sum / wsum) * (sum / wsum)) * RN(2 pi)) * 1.0989f) * blend per channel (1.0989: the 10-bit
//               format's energy loss);
//   oct(d)    : l = (|d.x| + |d.y|) + |d.z|; uv = (d.x / l, d.y / l); d.z < 0: uv = ((1 - |uv.y|) * s(uv.x), (1 - |uv.x|) * s(uv.y)),
//               s(x) = x >= 0 ? 1 : -1 (a NaN gives -1);
//   probeUV   : per axis ((float)(c * N) + (float)N * 0.5f + o * ((float)interior * 0.5f)) / (float)textureDim, N = interior + 2,
//               c the probe's x (for u) or z (for v), left to right; the slice is c.y;
//   bilinear  : k_bloom.hip's linear filter with WRAP addressing: t = uv * (float)dim - 0.5f; t0 = floor(t); f = t - t0;
//               i = (int)fmin(fmax(t0, -1), (float)dim) (a NaN gives -1); the texels (i + dim) % dim and (i + 1 + dim) % dim; the
//               same in y; per channel lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy);
//   texels    : UNORM10 (float)v / 1023.0f; binary16 loads are exact;
//   pow(x, e) : x > 0: exp2Signed(e * log2Soft(x)) (soft_math.hip.h); otherwise (0, negative, NaN) 0.
// A pixel that lies exactly on a probe divides 0 by 0 and follows binary32 rules from there.
//
// ADDRESSING.  The record function validated a host copy of the descriptor against the bound textures; the kernel reads the
// device's.  Where the two disagree every fetch still lands inside the textures: the bilinear wraps in the bound texture's own
// size, and the slice and the probe-data texel are clamped to it.  With a descriptor that matches, those clamps change nothing.
#pragma once

#include "cull_math.hip.h"
#include "screen_pass.hip.h"
#include "soft_math.hip.h"

namespace ddgi
{

struct Textures
{
    const interop::DDGIVolumeDesc* desc;       // t5
    const uint2* data;                         // t6 RGBA16_FLOAT array
    const uint32_t* irradiance;                // t7 R10G10B10A2_UNORM array
    const uint32_t* distance;                  // t8 RG16_FLOAT array
    uint32_t dataW, dataH, irrW, irrH, distW, distH, slices;
    uint32_t dataPitch, irrPitch, distPitch;   // texels per slice
};

struct I3 { int x, y, z; };

__device__ __forceinline__ cm::F3 sub(cm::F3 a, cm::F3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ cm::F3 normalize(cm::F3 v)
{
    const float len = cm::sqrt_(cm::dot3(v, v));
    return { cm::div_(v.x, len), cm::div_(v.y, len), cm::div_(v.z, len) };
}

__device__ __forceinline__ float powSoft(float x, float e) { return x > 0.0f ? softmath::exp2Signed(e * softmath::log2Soft(x)) : 0.0f; }

__device__ __forceinline__ void oct(cm::F3 d, float& u, float& v)
{
    const float l = (__builtin_fabsf(d.x) + __builtin_fabsf(d.y)) + __builtin_fabsf(d.z);
    u = cm::div_(d.x, l); v = cm::div_(d.y, l);
    if (d.z < 0.0f) {
        const float fu = (1.0f - __builtin_fabsf(v)) * (u >= 0.0f ? 1.0f : -1.0f), fv = (1.0f - __builtin_fabsf(u)) * (v >= 0.0f ? 1.0f : -1.0f);
        u = fu; v = fv;
    }
}

// one axis of the wrapped linear filter
struct Axis { uint32_t i0, i1; float f; };
__device__ __forceinline__ Axis axisOf(float uv, uint32_t dim)
{
    const float t = uv * (float)dim - 0.5f, t0 = __builtin_floorf(t);
    const int i = (int)cm::min_(cm::max_(t0, -1.0f), (float)dim);
    return { (uint32_t)(i + (int)dim) % dim, (uint32_t)(i + 1 + (int)dim) % dim, t - t0 };
}

__device__ __forceinline__ float probeCoord(int c, uint32_t interior, float o, uint32_t dim)
{
    const uint32_t n = interior + 2u;
    return cm::div_((float)(c * (int)n) + (float)n * 0.5f + o * ((float)interior * 0.5f), (float)dim);
}

__device__ __forceinline__ uint32_t sliceOf(int y, uint32_t slices) { return (uint32_t)(y < 0 ? 0 : y) < slices ? (uint32_t)(y < 0 ? 0 : y) : slices - 1u; }

// bilinear(irradiance, probeUV(c, (u, v), 6)): the four texels of probe c's irradiance tile around the direction whose oct() is (u, v),
// and channel(shift, halfGamma) = pow(their filtered channel, halfGamma).  The query's tap, and what the probe spheres are shaded
// with (k_giprobedraw.hip).
struct IrradianceTap
{
    uint32_t w00, w10, w01, w11;
    float fx, fy;
    __device__ __forceinline__ float channel(uint32_t shift, float halfGamma) const
    {
        const float t00 = cm::div_((float)((w00 >> shift) & 1023u), 1023.0f), t10 = cm::div_((float)((w10 >> shift) & 1023u), 1023.0f);
        const float t01 = cm::div_((float)((w01 >> shift) & 1023u), 1023.0f), t11 = cm::div_((float)((w11 >> shift) & 1023u), 1023.0f);
        return powSoft(sp::lerp_(sp::lerp_(t00, t10, fx), sp::lerp_(t01, t11, fx), fy), halfGamma);
    }
};

__device__ __forceinline__ IrradianceTap irradianceTap(const Textures& t, int cx, int cz, uint32_t slice, float u, float v)
{
    const Axis ax = axisOf(probeCoord(cx, interop::kDDGIIrradianceInteriorTexels, u, t.irrW), t.irrW);
    const Axis ay = axisOf(probeCoord(cz, interop::kDDGIIrradianceInteriorTexels, v, t.irrH), t.irrH);
    const uint32_t* s = t.irradiance + (uint64_t)slice * t.irrPitch;
    return { s[ay.i0 * t.irrW + ax.i0], s[ay.i0 * t.irrW + ax.i1], s[ay.i1 * t.irrW + ax.i0], s[ay.i1 * t.irrW + ax.i1], ax.f, ay.f };
}

__device__ __forceinline__ cm::F3 irradiance(const Textures& t, cm::F3 world, cm::F3 N, cm::F3 cameraOrigin)
{
    const interop::DDGIVolumeDesc& D = *t.desc;
    const cm::F3 origin = { D.origin[0], D.origin[1], D.origin[2] }, spacing = { D.probeSpacing[0], D.probeSpacing[1], D.probeSpacing[2] };
    const I3 last = { D.probeCounts[0] - 1, D.probeCounts[1] - 1, D.probeCounts[2] - 1 };
    const cm::F3 ext = { (spacing.x * (float)last.x) * 0.5f, (spacing.y * (float)last.y) * 0.5f, (spacing.z * (float)last.z) * 0.5f };
    const bool relocation = (D.flags & interop::kDDGIFlag_Relocation) != 0u, classification = (D.flags & interop::kDDGIFlag_Classification) != 0u;

    const cm::F3 viewDir = normalize(sub(world, cameraOrigin));
    const cm::F3 delta = { __builtin_fabsf(world.x - origin.x) - ext.x, __builtin_fabsf(world.y - origin.y) - ext.y, __builtin_fabsf(world.z - origin.z) - ext.z };
    float blend = 1.0f;
    if (!(delta.x < 0.0f && delta.y < 0.0f && delta.z < 0.0f))
        blend = ((1.0f - sp::saturate_(cm::div_(delta.x, spacing.x))) * (1.0f - sp::saturate_(cm::div_(delta.y, spacing.y)))) * (1.0f - sp::saturate_(cm::div_(delta.z, spacing.z)));
    if (!(blend > 0.0f)) return { 0.0f, 0.0f, 0.0f };

    const cm::F3 P = { world.x + (N.x * D.probeNormalBias - viewDir.x * D.probeViewBias), world.y + (N.y * D.probeNormalBias - viewDir.y * D.probeViewBias),
                       world.z + (N.z * D.probeNormalBias - viewDir.z * D.probeViewBias) };
    const I3 base = { (int)cm::min_(cm::max_(cm::div_((P.x - origin.x) + ext.x, spacing.x), 0.0f), (float)last.x),
                      (int)cm::min_(cm::max_(cm::div_((P.y - origin.y) + ext.y, spacing.y), 0.0f), (float)last.y),
                      (int)cm::min_(cm::max_(cm::div_((P.z - origin.z) + ext.z, spacing.z), 0.0f), (float)last.z) };

    auto dataAt = [&](I3 c) {
        const uint32_t x = (uint32_t)(c.x < 0 ? 0 : c.x), z = (uint32_t)(c.z < 0 ? 0 : c.z);
        return t.data[(uint64_t)sliceOf(c.y, t.slices) * t.dataPitch + (z < t.dataH ? z : t.dataH - 1u) * t.dataW + (x < t.dataW ? x : t.dataW - 1u)];
    };
    auto probePos = [&](I3 c, uint2 d) {
        cm::F3 p = { (spacing.x * (float)c.x - ext.x) + origin.x, (spacing.y * (float)c.y - ext.y) + origin.y, (spacing.z * (float)c.z - ext.z) + origin.z };
        if (relocation) {
            p.x = p.x + (float)sp::halfOf(d.x) * spacing.x;
            p.y = p.y + (float)sp::halfOf(d.x >> 16) * spacing.y;
            p.z = p.z + (float)sp::halfOf(d.y) * spacing.z;
        }
        return p;
    };

    const cm::F3 basePos = probePos(base, dataAt(base));
    const cm::F3 alpha = { sp::saturate_(cm::div_(P.x - basePos.x, spacing.x)), sp::saturate_(cm::div_(P.y - basePos.y, spacing.y)), sp::saturate_(cm::div_(P.z - basePos.z, spacing.z)) };
    float nu, nv;
    oct(N, nu, nv);
    const float halfGamma = D.probeIrradianceEncodingGamma * 0.5f;

    cm::F3 sum = { 0.0f, 0.0f, 0.0f };
    float wsum = 0.0f;
    for (int i = 0; i < 8; ++i) {
        const int ox = i & 1, oy = (i >> 1) & 1, oz = (i >> 2) & 1;
        const I3 c = { base.x + ox < last.x ? base.x + ox : last.x, base.y + oy < last.y ? base.y + oy : last.y, base.z + oz < last.z ? base.z + oz : last.z };
        const uint2 d = dataAt(c);
        if (classification && (float)sp::halfOf(d.y >> 16) == 1.0f) continue;
        const cm::F3 pp = probePos(c, d);
        const cm::F3 dirW = normalize(sub(pp, world)), toB = sub(pp, P);
        const float dist = cm::sqrt_(cm::dot3(toB, toB));
        const cm::F3 negDirB = { -cm::div_(toB.x, dist), -cm::div_(toB.y, dist), -cm::div_(toB.z, dist) };
        const float triX = cm::max_(0.001f, ox ? alpha.x : 1.0f - alpha.x), triY = cm::max_(0.001f, oy ? alpha.y : 1.0f - alpha.y), triZ = cm::max_(0.001f, oz ? alpha.z : 1.0f - alpha.z);
        const float wrap = (cm::dot3(dirW, N) + 1.0f) * 0.5f;
        float w = wrap * wrap + 0.2f;

        const uint32_t slice = sliceOf(c.y, t.slices);
        float du, dv;
        oct(negDirB, du, dv);
        {
            const Axis ax = axisOf(probeCoord(c.x, interop::kDDGIDistanceInteriorTexels, du, t.distW), t.distW);
            const Axis ay = axisOf(probeCoord(c.z, interop::kDDGIDistanceInteriorTexels, dv, t.distH), t.distH);
            const uint32_t* s = t.distance + (uint64_t)slice * t.distPitch;
            const uint32_t w00 = s[ay.i0 * t.distW + ax.i0], w10 = s[ay.i0 * t.distW + ax.i1], w01 = s[ay.i1 * t.distW + ax.i0], w11 = s[ay.i1 * t.distW + ax.i1];
            const float r = sp::lerp_(sp::lerp_((float)sp::halfOf(w00), (float)sp::halfOf(w10), ax.f), sp::lerp_((float)sp::halfOf(w01), (float)sp::halfOf(w11), ax.f), ay.f);
            const float g = sp::lerp_(sp::lerp_((float)sp::halfOf(w00 >> 16), (float)sp::halfOf(w10 >> 16), ax.f), sp::lerp_((float)sp::halfOf(w01 >> 16), (float)sp::halfOf(w11 >> 16), ax.f), ay.f);
            const float mean = 2.0f * r, mean2 = 2.0f * g;
            const float var = __builtin_fabsf(mean * mean - mean2);
            float ch = 1.0f;
            if (dist > mean) {
                const float v = dist - mean;
                ch = cm::div_(var, var + v * v);
                ch = cm::max_((ch * ch) * ch, 0.0f);
            }
            w = w * cm::max_(0.05f, ch);
        }
        w = cm::max_(0.000001f, w);
        if (w < 0.2f) w = w * ((w * w) * (1.0f / (0.2f * 0.2f)));
        w = w * ((triX * triY) * triZ);
        {
            const IrradianceTap tap = irradianceTap(t, c.x, c.z, slice, nu, nv);
            sum.x = sum.x + w * tap.channel(0u, halfGamma);
            sum.y = sum.y + w * tap.channel(10u, halfGamma);
            sum.z = sum.z + w * tap.channel(20u, halfGamma);
        }
        wsum = wsum + w;
    }
    if (wsum == 0.0f) return { 0.0f, 0.0f, 0.0f };
    auto finish = [&](float s) {
        const float r = cm::div_(s, wsum);
        return (((r * r) * 0x1.921fb6p+2f) * 1.0989f) * blend;
    };
    return { finish(sum.x), finish(sum.y), finish(sum.z) };
}

} // namespace ddgi
