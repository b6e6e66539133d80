// cull_arith_probe.hip -- test-only library (toyrenderer_amd/lib/libtrhip_probe.so, never linked into libtrhip.so).
//
// Runs the instruction sequences of cull_math.hip.h -- the real cm:: functions, included unchanged -- over large input
// domains on the GPU and compares them with the correctly rounded references of fp_ref.h.  Used by
// tests/test_gpu_primitives.py (GPU) and tests/test_probe_ref.py (the host copies of the references).
//
// Every launcher allocates, launches in bounded chunks, synchronises, copies the result out, frees, and returns the
// hipError_t.  Inputs come from the thread index or from a counter-based hash: nothing is read but what the probe
// generated, and the only writes are the counters of one ProbeResult.  Every call of a cm:: function runs in a full wave of
// 64 active lanes (sqrt2 and the stepQuotients masks assume EXEC is all ones): the tail of a sweep repeats an in-domain
// input and is masked out of the counts.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../toyrenderer_amd/csrc/cull_math.hip.h"
#include "fp_ref.h"

extern "C" {
struct ProbeResult
{
    unsigned long long tested;        // inputs (or lanes) compared
    unsigned long long mismatches;    // of them: outside the expectation
    unsigned long long hist[8];       // ulp distance to the reference: 0, 1, 2, 3, 4, 5, 6..15, >= 16 (or NaN vs number)
    unsigned long long aux[8];        // check-specific counters (see the launchers)
    unsigned int maxUlp;              // largest distance seen (saturated at 2^32 - 1)
    unsigned int nfail;               // failures recorded (all of them counted, the first 64 stored)
    unsigned int fail[64][4];         // first failing inputs: a, b, got, expected (or check-specific words)
};
}

namespace
{

constexpr uint32_t kBlock = 256;
constexpr uint32_t kGrid = 2048;
constexpr uint64_t kChunk = 1ull << 28;       // inputs per launch: a few ms of work each

__device__ __forceinline__ uint32_t laneId() { return __lane_id(); }

__device__ __forceinline__ uint32_t hash32(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return (uint32_t)x;
}
__device__ __forceinline__ float unit(uint32_t h) { return (float)(h >> 8) * 0x1p-24f; }              // [0, 1)

// per-lane counters, reduced once per wave at the end of a kernel
struct Acc
{
    unsigned long long tested = 0, bad = 0, hist[8] = {}, aux[8] = {};
    uint32_t maxUlp = 0;
    __device__ void add(bool valid, uint64_t dist, bool isBad)
    {
        if (!valid) return;
        ++tested;
        bad += isBad;
        const int b = dist < 6 ? (int)dist : dist < 16 ? 6 : 7;
#pragma unroll
        for (int j = 0; j < 8; ++j) hist[j] += b == j;               // (no dynamic index: the counters stay in registers)
        const uint32_t d = dist > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dist;
        maxUlp = d > maxUlp ? d : maxUlp;
    }
};

__device__ __forceinline__ unsigned long long waveSum(unsigned long long v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t waveMax(uint32_t v)
{
    for (int o = 32; o; o >>= 1) { const uint32_t w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}

__device__ void flush(const Acc& a, ProbeResult* R)
{
    unsigned long long s[18];
    s[0] = waveSum(a.tested); s[1] = waveSum(a.bad);
    for (int i = 0; i < 8; ++i) { s[2 + i] = waveSum(a.hist[i]); s[10 + i] = waveSum(a.aux[i]); }
    const uint32_t mx = waveMax(a.maxUlp);
    if (laneId() == 0) {
        if (s[0]) atomicAdd(&R->tested, s[0]);
        if (s[1]) atomicAdd(&R->mismatches, s[1]);
        for (int i = 0; i < 8; ++i) {
            if (s[2 + i]) atomicAdd(&R->hist[i], s[2 + i]);
            if (s[10 + i]) atomicAdd(&R->aux[i], s[10 + i]);
        }
        if (mx) atomicMax(&R->maxUlp, mx);
    }
}

// called by all 64 lanes; stores the first 64 failures of the whole launch sequence
__device__ void recordFail(ProbeResult* R, bool bad, uint32_t a, uint32_t b, uint32_t got, uint32_t ref)
{
    const unsigned long long m = __ballot(bad);
    if (m == 0ull) return;
    uint32_t base = 0;
    if (laneId() == 0) base = atomicAdd(&R->nfail, (unsigned)__popcll(m));
    base = __shfl(base, 0, 64);
    if (bad) {
        const uint32_t k = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (k < 64u) { R->fail[k][0] = a; R->fail[k][1] = b; R->fail[k][2] = got; R->fail[k][3] = ref; }
    }
}

// one compared value: counts it, records it when it is outside `tol` ulp (NaN only matches NaN)
__device__ __forceinline__ void compare(Acc& acc, ProbeResult* R, bool valid, uint32_t a, uint32_t b, uint32_t got, uint32_t ref, uint64_t tol)
{
    uint64_t dist;
    if (fr::isNaN(ref) || fr::isNaN(got)) dist = fr::isNaN(ref) && fr::isNaN(got) ? 0ull : ~0ull;
    else dist = fr::ulpDist(got, ref);
    const bool bad = valid && dist > tol;
    acc.add(valid, dist, bad);
    recordFail(R, bad, a, b, got, ref);
}

// Sweep driver: every thread runs the same number of iterations (full waves throughout); index i >= count is
// replaced by index 0 and marked invalid.
template <class F>
__global__ __launch_bounds__(kBlock) void sweepKernel(F f, uint64_t count, ProbeResult* R)
{
    Acc acc;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t iters = (count + stride - 1) / stride;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t it = 0; it < iters; ++it) {
        const uint64_t i = it * stride + t;
        const bool valid = i < count;
        f(valid ? i : 0ull, valid, acc, R);
    }
    flush(acc, R);
}

template <class F>
hipError_t runSweep(F f, uint64_t count, ProbeResult* out)
{
    ProbeResult* d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof(ProbeResult));
    if (e != hipSuccess) return e;
    e = hipMemset(d, 0, sizeof(ProbeResult));
    for (uint64_t at = 0; e == hipSuccess && at < count; at += kChunk) {
        F g = f;
        g.base += at;
        const uint64_t n = count - at < kChunk ? count - at : kChunk;
        hipLaunchKernelGGL(sweepKernel<F>, dim3(kGrid), dim3(kBlock), 0, 0, g, n, d);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d, sizeof(ProbeResult), hipMemcpyDeviceToHost);
    const hipError_t f2 = hipFree(d);
    return e != hipSuccess ? e : f2;
}

// ---- A, B, C: single-operand sequences over a range of bit patterns ------------------------------------------------
enum UnaryOp : int { kRsq = 0, kRcp = 1, kSqrtSeq1 = 2, kSqrtSeq2 = 3, kSqrt2 = 4, kSqrt2Lane0Out = 5 };

struct Unary
{
    uint64_t base;            // first pattern of this launch (the sweep index is added)
    uint64_t first, count;    // the whole range (sqrtSeq2's second lane walks it backwards)
    int op;
    uint32_t tol;
    __device__ void operator()(uint64_t i, bool valid, Acc& acc, ProbeResult* R) const
    {
        const uint32_t x = (uint32_t)(base + i);
        const float xf = fr::flt(x);
        switch (op) {
        case kRsq: compare(acc, R, valid, x, 0u, fr::bits(__builtin_amdgcn_rsqf(xf)), fr::rsqRN(x), tol); break;
        case kRcp: compare(acc, R, valid, x, 0u, fr::bits(__builtin_amdgcn_rcpf(xf)), fr::rcpRN(x), tol); break;
        case kSqrtSeq1: compare(acc, R, valid, x, 0u, fr::bits(cm::sqrtSeq1(xf)), fr::sqrtRN(x), tol); break;
        case kSqrtSeq2: {
            const uint32_t y = (uint32_t)(first + (first + count - 1 - (base + i)));   // the range backwards
            const cm::v2f s = cm::sqrtSeq2(cm::v2f{ xf, fr::flt(y) });
            compare(acc, R, valid, x, 0u, fr::bits(s.x), fr::sqrtRN(x), tol);
            compare(acc, R, valid, y, 1u, fr::bits(s.y), fr::sqrtRN(y), tol);
            break;
        }
        default: {   // sqrt2: (x, neighbour of x); kSqrt2Lane0Out: lane 0's second operand is -1 in every wave (fallback)
            const uint32_t y = op == kSqrt2Lane0Out && laneId() == 0 ? 0xBF800000u : x ^ 1u;
            const cm::v2f s = cm::sqrt2(cm::v2f{ xf, fr::flt(y) });
            compare(acc, R, valid, x, 0u, fr::bits(s.x), fr::sqrtRN(x), tol);
            compare(acc, R, valid, y, 1u, fr::bits(s.y), fr::sqrtRN(y), tol);
            break;
        }
        }
    }
};

// A pair whose quotient lies next to a midpoint m = M 2^-25 (M odd, 25 bits) of binary32: with D odd, M = delta D^-1 mod 2^25
// makes M D = N 2^s + delta (s = bitlen(M D) - 24, delta in {-3, -1, 1, 3}), so n / d = (N / D) 2^(en - ed) sits delta / (D 2^s)
// below the midpoint M / 2^s -- the hardest cases a division has (an exact tie needs a subnormal quotient).  When M comes
// out below 2^24 the pair is an ordinary random one.
__device__ __forceinline__ void nearMidpoint(uint32_t h0, uint32_t h1, int en, int ed, uint32_t& n, uint32_t& d)
{
    const uint32_t D = (h0 & 0xFFFFFFu) | 0x800001u;                    // 24 bits, odd
    const int32_t delta = (int32_t)((h1 & 3u) * 2u) - 3;              // -3, -1, 1, 3
    uint32_t inv = D;                                                   // D^-1 mod 2^32 (Newton: each step doubles the correct bits)
    for (int j = 0; j < 5; ++j) inv *= 2u - D * inv;
    const uint32_t M = ((uint32_t)delta * inv) & 0x1FFFFFFu;
    uint32_t N = (h1 >> 8) | 0x800000u;                                 // fallback: a random mantissa
    if (M >= 0x1000000u) {
        const uint64_t P = (uint64_t)M * D;
        const int s = 64 - __builtin_clzll(P) - 24;
        N = (uint32_t)((P - (uint64_t)(int64_t)delta) >> s);
    }
    n = ((uint32_t)(en + 127) << 23) | (N & 0x7FFFFFu) | (h1 & fr::kSign);
    d = ((uint32_t)(ed + 127) << 23) | (D & 0x7FFFFFu) | ((h0 >> 7) & fr::kSign);
}

// ---- D: div2 -------------------------------------------------------------------------------------------------------
enum DivMode : int { kDivSetNum = 0, kDivSetDen = 1, kDivHashed = 2, kDivExpPairs = 3, kDivMidpoints = 4 };

struct Div
{
    uint64_t base;
    int mode;
    uint32_t nset;
    uint32_t set[16];
    __device__ void check(Acc& acc, ProbeResult* R, bool valid, cm::v2f n, cm::v2f d) const
    {
        const cm::v2f q = cm::div2(n, d);
        compare(acc, R, valid, fr::bits(n.x), fr::bits(d.x), fr::bits(q.x), fr::divRN(fr::bits(n.x), fr::bits(d.x)), 0);
        compare(acc, R, valid, fr::bits(n.y), fr::bits(d.y), fr::bits(q.y), fr::divRN(fr::bits(n.y), fr::bits(d.y)), 0);
    }
    __device__ void operator()(uint64_t i, bool valid, Acc& acc, ProbeResult* R) const
    {
        const uint64_t k = base + i;
        if (mode == kDivSetNum || mode == kDivSetDen) {          // every pattern against each value of the set
            const float x = fr::flt((uint32_t)k);
            for (uint32_t j = 0; j < nset; j += 2) {
                const float a = fr::flt(set[j]), b = fr::flt(set[j + 1 < nset ? j + 1 : j]);
                if (mode == kDivSetNum) check(acc, R, valid, cm::v2f{ a, b }, cm::splat2(x));
                else check(acc, R, valid, cm::splat2(x), cm::v2f{ a, b });
            }
        } else if (mode == kDivHashed) {
            check(acc, R, valid, cm::v2f{ fr::flt(hash32(4 * k)), fr::flt(hash32(4 * k + 2)) },
                                 cm::v2f{ fr::flt(hash32(4 * k + 1)), fr::flt(hash32(4 * k + 3)) });
        } else if (mode == kDivMidpoints) {                     // near-midpoint quotients, exponents anywhere in the normal range
            const uint32_t h0 = hash32(4 * k), h1 = hash32(4 * k + 1), h2 = hash32(4 * k + 2), h3 = hash32(4 * k + 3);
            uint32_t n, d, n2, d2;
            nearMidpoint(h0, h1, -126 + (int)(h2 % 254u), -126 + (int)((h2 >> 8) % 254u), n, d);
            nearMidpoint(h2, h3, -126 + (int)(h0 % 254u), -126 + (int)((h1 >> 8) % 254u), n2, d2);
            check(acc, R, valid, cm::v2f{ fr::flt(n), fr::flt(n2) }, cm::v2f{ fr::flt(d), fr::flt(d2) });
        } else {                                                // k = (en << 19) | (ed << 11) | sample
            const uint32_t en = (uint32_t)(k >> 19) & 0xFFu, ed = (uint32_t)(k >> 11) & 0xFFu;
            const uint32_t h0 = hash32(2 * k + 0x9E37), h1 = hash32(2 * k + 0x79B9);
            const uint32_t n = (h0 & 0x807FFFFFu) | (en << 23), d = (h1 & 0x807FFFFFu) | (ed << 23);
            const uint32_t n2 = (h1 & 0x007FFFFFu) | (en << 23) | (h0 & fr::kSign), d2 = (h0 & 0x007FFFFFu) | (ed << 23) | (h1 & fr::kSign);
            check(acc, R, valid, cm::v2f{ fr::flt(n), fr::flt(n2) }, cm::v2f{ fr::flt(d), fr::flt(d2) });
        }
    }
};

// ---- E: rcpRefined + quotient (the fast path's division, and stepDeferred's depthSphere) -----------------------------
enum QuotMode : int { kQuotFullMant = 0, kQuotExpPairs = 1, kQuotMidpoints = 2, kQuotNearPlane = 3, kQuotOutside = 4 };

__device__ __forceinline__ uint32_t withExp(uint32_t h, int e /* unbiased */) { return (h & 0x807FFFFFu) | ((uint32_t)(e + 127) << 23); }
__device__ __forceinline__ int domExp(uint32_t h) { return -30 + (int)(h % 93u); }           // [2^-30, 2^63)

struct Quot
{
    uint64_t base;
    int mode;
    uint32_t ntrip;
    uint32_t trip[32][3];    // kQuotFullMant: (n exponent + 127, d exponent + 127, n pattern's sign | mantissa)
    __device__ void check(Acc& acc, ProbeResult* R, bool valid, uint32_t n, uint32_t d, uint32_t n2, uint32_t d2) const
    {
        const float nf = fr::flt(n), df = fr::flt(d);
        const uint32_t ref = fr::divRN(n, d), ref2 = fr::divRN(n2, d2);
        compare(acc, R, valid, n, d, fr::bits(cm::quotient1(nf, df, cm::rcpRefined1(df))), ref, 0);
        const cm::v2f nn = { nf, fr::flt(n2) }, dd = { df, fr::flt(d2) };
        const cm::v2f q = cm::quotient2(nn, dd, cm::rcpRefined2(dd));
        compare(acc, R, valid, n, d, fr::bits(q.x), ref, 0);
        compare(acc, R, valid, n2, d2, fr::bits(q.y), ref2, 0);
    }
    __device__ void operator()(uint64_t i, bool valid, Acc& acc, ProbeResult* R) const
    {
        const uint64_t k = base + i;
        const uint32_t h0 = hash32(3 * k + 11), h1 = hash32(3 * k + 12), h2 = hash32(3 * k + 13);
        uint32_t n, d, n2, d2;
        if (mode == kQuotFullMant) {                           // k = (triple << 23) | d mantissa
            const uint32_t* t = trip[(k >> 23) % ntrip];
            const uint32_t dm = (uint32_t)k & 0x7FFFFFu;
            n = t[2] | (t[0] << 23); d = dm | (t[1] << 23) | (h0 & fr::kSign);
            n2 = withExp(h1, domExp(h2)); d2 = withExp(h2, domExp(h1 >> 7));
        } else if (mode == kQuotExpPairs) {                    // k = (pair << 16) | sample, pair < 93 * 93
            const uint32_t p = (uint32_t)(k >> 16);
            n = withExp(h0, -30 + (int)(p / 93u)); d = withExp(h1, -30 + (int)(p % 93u));
            n2 = withExp(h2, -30 + (int)(p % 93u)); d2 = withExp(h0 ^ h1, -30 + (int)(p / 93u));
        } else if (mode == kQuotMidpoints) {                   // n / d within 2^-45 (relative) of a rounding midpoint
            const int en = domExp(h2), ed = domExp(h2 >> 8);
            nearMidpoint(h0, h1, en, ed, n, d);
            n2 = withExp(h2, domExp(h0)); d2 = withExp(h0, domExp(h1));
        } else if (mode == kQuotNearPlane) {                   // depthSphere: nearPlane in [2^-20, 2^20] over c.z - r
            n = withExp(h0 & 0x7FFFFFFFu, -20 + (int)(h2 % 40u)); d = withExp(h1, domExp(h2 >> 8));
            n2 = (h0 & 1u) ? 0x35800000u : 0x49800000u;        // the ends 2^-20, 2^20
            d2 = withExp(h2, domExp(h1 >> 9));
        } else {                                               // outside: d >= 2^126 (subnormal reciprocal / quotient)
            n = withExp(h0, domExp(h2)); d = withExp(h1, 126 + (int)(h2 & 1u));
            n2 = n; d2 = d;
        }
        check(acc, R, valid, n, d, n2, d2);
    }
};

// ---- H: bytes, hzbLevel, the frexp level choice -----------------------------------------------------------------------
enum LevelOp : int { kBytes = 0, kHzbLevel = 1, kFrexpLevel = 2 };

struct Levels
{
    uint64_t base;
    int op;
    uint32_t mips;
    __device__ void operator()(uint64_t i, bool valid, Acc& acc, ProbeResult* R) const
    {
        const uint32_t x = (uint32_t)(base + i);
        if (op == kBytes) {
            const uint32_t b = x & 0xFFu;
            const uint32_t q = fr::divRN(fr::bits((float)b), fr::bits(255.0f));
            compare(acc, R, valid, b, 0u, fr::bits(cm::u8Unorm(b)), q, 0);
            compare(acc, R, valid, b, 1u, fr::bits(cm::coneTableEntry(b)), q, 0);
            compare(acc, R, valid, b, 2u, fr::bits(cm::coneTableEntry(b | 0x100u)), q, 0);      // the index is masked to a byte
            const uint32_t by[4] = { b, (b + 85u) & 0xFFu, (b + 170u) & 0xFFu, (b + 43u) & 0xFFu };
            float cutoff = -1.0f;
            const cm::F3 a = cm::coneAxisCutoff(by[0] | (by[1] << 8) | (by[2] << 16) | (by[3] << 24), &cutoff);
            const float ax[3] = { a.x, a.y, a.z };
            for (int j = 0; j < 3; ++j) {                      // fma(q, 2, -1) = RN(2 q - 1): exact in binary64, rounded once
                const double qj = (double)fr::flt(fr::divRN(fr::bits((float)by[j]), fr::bits(255.0f)));
                compare(acc, R, valid, by[j], 3u + j, fr::bits(ax[j]), fr::bits((float)(2.0 * qj - 1.0)), 0);
            }
            compare(acc, R, valid, by[3], 6u, fr::bits(cutoff), fr::divRN(fr::bits((float)by[3]), fr::bits(255.0f)), 0);
        } else if (op == kHzbLevel) {
            // floor(log2(max(w, h))) clamped to [0, mips - 1]; below 1 and NaN -> 0 (Q6), +inf -> the last mip
            int ref;
            if (!(fr::flt(x) >= 1.0f)) ref = 0;
            else if (x == fr::kInf) ref = (int)mips - 1;
            else { ref = fr::floorLog2(x); ref = ref > (int)mips - 1 ? (int)mips - 1 : ref; }
            compare(acc, R, valid, x, 0u, (uint32_t)cm::hzbLevel(fr::flt(x), 0.5f, mips), (uint32_t)ref, 0);
            compare(acc, R, valid, x, 1u, (uint32_t)cm::hzbLevel(-2.0f, fr::flt(x), mips), (uint32_t)ref, 0);
        } else {
            // occTailQuad / occTailQuadFiltered: e = v_frexp_exp(m), clamped to [1, mips], for every finite m >= 1
            // (the clamps in front, w and h <= the HZB size and max(., 1), keep m finite and >= 1)
            const float m = fr::flt(x);
            int e = __builtin_amdgcn_frexp_expf(m);
            e = e < (int)mips ? e : (int)mips;
            e = e > 1 ? e : 1;
            int ref = fr::floorLog2(x) + 1;
            ref = ref < (int)mips ? ref : (int)mips;
            compare(acc, R, valid, x, 0u, (uint32_t)e, (uint32_t)ref, 0);
        }
    }
};

// ---- F, G: the cull step ----------------------------------------------------------------------------------------------
struct ProbeView
{
    float P00, P11, nearPlane;
    uint32_t hzbW, hzbH, mips;
    float view[9];               // rotation rows of the view matrix
    int spare;
};

__device__ cm::M33P packRows(const float* m)
{
    const cm::M43 v = { { m[0], m[1], m[2] }, { m[3], m[4], m[5] }, { m[6], m[7], m[8] }, { 0.f, 0.f, 0.f } };
    return cm::rot(cm::packM43(v));
}

// a random adjugate: entries in [-2, 2] times a power of two in [2^-4, 2^4]
__device__ cm::M33P randomAdj(uint64_t k)
{
    float m[9];
    const float s = __builtin_ldexpf(1.0f, (int)(hash32(k * 16 + 9) % 9u) - 4);
    for (int j = 0; j < 9; ++j) m[j] = (4.0f * unit(hash32(k * 16 + j)) - 2.0f) * s;
    return packRows(m);
}

// F: stepQuotients' FAST branch against its EXACT branch (forced with nearInRange = false)
template <bool OCC, bool CONE>
__global__ __launch_bounds__(kBlock) void stepKernel(uint64_t base, uint64_t count, ProbeView pv, int layout, ProbeResult* R)
{
    __shared__ float tab[cm::kConeTabEntries];
    for (uint32_t i = threadIdx.x; i < cm::kConeTabEntries; i += blockDim.x) tab[i] = cm::coneTableEntry(i);
    __syncthreads();
    Acc acc;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, iters = (count + stride - 1) / stride;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t it = 0; it < iters; ++it) {
        const uint64_t i = it * stride + t;
        const bool valid = i < count;
        const uint64_t k = base + (valid ? i : 0ull);
        // in-domain sphere: scale 2^-8 .. 2^12, r in (0, s], c.z >= r + nearPlane, |c.xy| up to 3 c.z
        const float s = __builtin_ldexpf(1.0f, (int)(hash32(k * 8 + 0) % 21u) - 8);
        float r = s * (0.001f + unit(hash32(k * 8 + 1)));
        cm::F3 c;
        c.z = r + pv.nearPlane + s * 8.0f * unit(hash32(k * 8 + 2));
        c.x = c.z * (6.0f * unit(hash32(k * 8 + 3)) - 3.0f);
        c.y = c.z * (6.0f * unit(hash32(k * 8 + 4)) - 3.0f);
        const uint32_t packed = hash32(k * 8 + 5);
        // layouts 1, 2: lane 5 of every wave is out of the SAFE range (|r| > 2^30); inactive (1) or active (2)
        cm::lmask active = ~0ull;
        if (layout != 0 && laneId() == 5) { r = 0x1p31f; c.z = 0x1p32f; }
        if (layout == 1) active &= ~(1ull << 5);
        const cm::M33P adj = randomAdj(k);
        cm::StepQuot qf, qe;
        cm::stepQuotients<OCC, CONE, true>(active, c, r, packed, adj, pv.nearPlane, true, qf, tab);
        cm::stepQuotients<OCC, CONE, true>(active, c, r, packed, adj, pv.nearPlane, false, qe, tab);
        const bool use = valid && ((active >> laneId()) & 1ull);
        if (OCC) {
            compare(acc, R, use, fr::bits(c.x), fr::bits(r), fr::bits(qf.mn.x), fr::bits(qe.mn.x), 0);
            compare(acc, R, use, fr::bits(c.y), fr::bits(r), fr::bits(qf.mn.y), fr::bits(qe.mn.y), 0);
            compare(acc, R, use, fr::bits(c.x), fr::bits(c.z), fr::bits(qf.mx.x), fr::bits(qe.mx.x), 0);
            compare(acc, R, use, fr::bits(c.y), fr::bits(c.z), fr::bits(qf.mx.y), fr::bits(qe.mx.y), 0);
            compare(acc, R, use, fr::bits(c.z), fr::bits(r), fr::bits(qf.depthSphere), fr::bits(qe.depthSphere), 0);
        }
        if (CONE) {
            compare(acc, R, use, packed, 0x70u, fr::bits(qf.tn.x), fr::bits(qe.tn.x), 5);
            compare(acc, R, use, packed, 0x71u, fr::bits(qf.tn.y), fr::bits(qe.tn.y), 5);
            compare(acc, R, use, packed, 0x72u, fr::bits(qf.tn.z), fr::bits(qe.tn.z), 5);
            compare(acc, R, use, fr::bits(c.x), 0x73u, fr::bits(qf.lenC), fr::bits(qe.lenC), 5);
            compare(acc, R, use, packed, 0x74u, fr::bits(qf.cutoff), fr::bits(qe.cutoff), 0);
        }
        // aux[0]: waves (counted at lane 0) whose first call took the FAST branch; aux[1]: exact-branch waves of the first call
        if (laneId() == 0 && valid) { acc.aux[0] += !qf.coneExact; acc.aux[1] += qf.coneExact; }
    }
    flush(acc, R);
}

// G: the deferred mode's sure lanes against the exact quotients
struct QuadGeom
{
    uint32_t offset[16], total;
};

__host__ QuadGeom quadGeom(uint32_t w, uint32_t h, uint32_t mips)
{
    QuadGeom g = {};
    uint32_t at = 0;
    for (uint32_t k = 0; k < mips; ++k) {
        const uint32_t mw = (w >> k) ? (w >> k) : 1u, mh = (h >> k) ? (h >> k) : 1u;
        g.offset[k] = at;
        at += ((mw >> 3) + 1u) * ((mh >> 3) + 1u) * 64u;
    }
    g.total = at;
    return g;
}

template <bool CONE>
__global__ __launch_bounds__(kBlock) void filteredKernel(uint64_t base, uint64_t count, ProbeView pv, QuadGeom qg, int noBand, ProbeResult* R)
{
    __shared__ float tab[cm::kConeTabEntries];
    __shared__ uint4 mipTab[17];
    __shared__ uint2 mipBand[17];
    cm::ProjBands bands = cm::projBands(pv.P00, pv.P11, pv.hzbW, pv.hzbH);
    if (noBand) { bands.K = cm::v2f{ 0.f, 0.f }; bands.mipDelta = 0u; bands.mFloor = 1.0f; }   // negative control
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < cm::kConeTabEntries; i += blockDim.x) tab[i] = cm::coneTableEntry(i);
    if (tid >= 1 && tid <= 16) {                                        // as k_basepass_as.hip builds them
        const uint32_t mip = tid - 1u < pv.mips ? tid - 1u : 0u;
        const uint32_t mw = (pv.hzbW >> mip) ? (pv.hzbW >> mip) : 1u, mh = (pv.hzbH >> mip) ? (pv.hzbH >> mip) : 1u;
        mipTab[tid] = make_uint4(qg.offset[mip], ((mw >> 3) + 1u) * 64u, __float_as_uint(0.5f * (float)mw), __float_as_uint(0.5f * (float)mh));
        const uint32_t d = noBand ? 0u : cm::projMipDelta(bands, tid);
        mipBand[tid] = make_uint2(d, 2u * d);
    }
    __syncthreads();
    cm::Hzb h = {};
    h.width = pv.hzbW; h.height = pv.hzbH; h.mips = pv.mips;           // occTailQuad* read no texel
    const cm::M33P viewRot = packRows(pv.view);
    cm::M43 V = { { pv.view[0], pv.view[1], pv.view[2] }, { pv.view[3], pv.view[4], pv.view[5] }, { pv.view[6], pv.view[7], pv.view[8] }, { 0.f, 0.f, 0.f } };
    const float kV = cm::coneSlackFactor(V);
    const float B[2] = { 1.125f / __builtin_fabsf(pv.P00) + 0.25f, 1.125f / __builtin_fabsf(pv.P11) + 0.25f };
    Acc acc;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, iters = (count + stride - 1) / stride;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + tid;
    for (uint64_t it = 0; it < iters; ++it) {
        const uint64_t i = it * stride + t;
        const bool valid = i < count;
        const uint64_t k = base + (valid ? i : 0ull);
        const uint32_t kind = hash32(k * 16 + 0) & 7u;
        const float s = __builtin_ldexpf(1.0f, (int)(hash32(k * 16 + 1) % 17u) - 4);   // depth scale 2^-4 .. 2^12
        cm::F3 c;
        c.z = pv.nearPlane + s * (0.05f + 4.0f * unit(hash32(k * 16 + 2)));
        float r = c.z * 0.125f * unit(hash32(k * 16 + 3));
        c.x = c.z * B[0] * (2.0f * unit(hash32(k * 16 + 4)) - 1.0f);
        c.y = c.z * B[1] * (2.0f * unit(hash32(k * 16 + 5)) - 1.0f);
        const float eps = (float)((int)(hash32(k * 16 + 6) % 2001u) - 1000) * 0x1p-23f;   // relative nudge, up to ~10^4 ulp
        if (kind == 1) r = c.z * 0.125f * (1.0f + eps);                                     // 8 |r| ~ c.z
        else if (kind == 2) c.x = c.z * B[0] * (1.0f + eps) * ((hash32(k * 16 + 7) & 1u) ? 1.0f : -1.0f);   // |c.x| ~ Bx c.z
        else if (kind == 3) c.y = c.z * B[1] * (1.0f + eps);
        else if (kind >= 4) {
            // footprints on texel edges / power-of-two widths: pick a level L and a footprint width w ~ 2^L (1 + eps) or
            // random in [2^L, 2^(L+1)), then put the centre's fractional coordinate on an edge of that level
            const uint32_t L = hash32(k * 16 + 8) % pv.mips;
            const float w = __builtin_ldexpf(kind == 4 ? 1.0f + eps : 1.0f + unit(hash32(k * 16 + 9)), (int)L);
            r = c.z * w / (__builtin_fabsf(pv.P00) * (float)pv.hzbW);
            const uint32_t mw = (pv.hzbW >> L) ? (pv.hzbW >> L) : 1u, mh = (pv.hzbH >> L) ? (pv.hzbH >> L) : 1u;
            const float ux = ((float)(hash32(k * 16 + 10) % (mw + 1u)) + (kind == 6 ? 0.5f : 0.0f)) / (float)mw * (1.0f + eps);
            const float uy = ((float)(hash32(k * 16 + 11) % (mh + 1u)) + (kind == 7 ? 0.5f : 0.0f)) / (float)mh * (1.0f - eps);
            c.x = c.z * (2.0f * ux - 1.0f) / pv.P00;
            c.y = -c.z * (2.0f * uy - 1.0f) / pv.P11;
            if (kind == 5) r = r * (1.0f + eps);
        }
        uint32_t packed = hash32(k * 16 + 12);
        const cm::M33P adj = randomAdj(k);
        if (CONE) {
            // half of the lanes: the cone test near its decision, r = D - cutoff |c| from the exact sequences, nudged by up
            // to ~10^4 ulp (evaluated by every lane: the sequences want full waves)
            cm::StepQuot q0;
            cm::stepQuotients<false, true, true>(~0ull, c, 0.0f, packed, adj, pv.nearPlane, false, q0, tab);
            cm::F3 axis = cm::mulVecP(q0.tn, viewRot);
            axis.z = -axis.z;
            const float D = cm::dot3(c, axis);
            const float rr = cm::fma_(-q0.cutoff, q0.lenC, D) * (1.0f + eps);
            if ((hash32(k * 16 + 13) & 1u) && __builtin_fabsf(rr) * 8.0f <= c.z) r = rr;
        }
        // the deferred mode
        cm::StepQuot qf;
        cm::lmask sureOcc, sureCone;
        cm::stepDeferred<CONE>(c, r, packed, adj, pv.nearPlane, bands, tab, qf, sureOcc, sureCone);
        const cm::OccQuad of = cm::occTailQuadFiltered(qf.mn, qf.mx, qf.depthSphere, c, r, pv.nearPlane, pv.P00, pv.P11, h, mipTab, mipBand, qg.total, bands, sureOcc);
        cm::lmask sureC = sureCone;
        const cm::lmask backF = CONE ? cm::coneBackSure(qf, c, r, viewRot, kV, sureC) : 0ull;
        // the exact sequences
        cm::StepQuot qe;
        cm::stepQuotients<true, CONE, true>(~0ull, c, r, packed, adj, pv.nearPlane, false, qe, tab);
        const cm::OccQuad oe = cm::occTailQuad(qe, c, r, pv.nearPlane, pv.P00, pv.P11, h, mipTab, qg.total);
        float unused;
        const cm::lmask backE = CONE ? __builtin_amdgcn_ballot_w64(cm::coneBackfacingP(packed, c, r, adj, viewRot, 1.0f, 1.0f, &unused)) : 0ull;
        const uint64_t bit = 1ull << laneId();
        const bool matters = valid && !(oe.accept & bit);                  // the lookup of an accepted lane is never used
        const bool sO = matters && (sureOcc & bit);
        // a sure lane: the same table entry (level, x0, y0) and no zero weight in the exact footprint; the same depthSphere
        const bool badO = sO && (of.iq != oe.iq || (oe.slow & bit) || fr::bits(qf.depthSphere) != fr::bits(qe.depthSphere));
        acc.add(sO, badO ? ~0ull : 0ull, badO);
        recordFail(R, badO, fr::bits(c.x), fr::bits(r), of.iq, oe.iq);
        const bool sC = CONE && valid && (sureC & bit);
        const bool badC = sC && (((backF ^ backE) & bit) != 0ull);
        acc.aux[4] += sC; acc.aux[5] += badC;
        recordFail(R, badC, fr::bits(c.z), fr::bits(r), 0xC0Eu, (uint32_t)((backE >> laneId()) & 1ull));
        acc.aux[0] += matters;                                              // lanes whose lookup matters
        acc.aux[3] += CONE && valid;
    }
    // cone mismatches count as mismatches too
    acc.bad += acc.aux[5];
    flush(acc, R);
}

hipError_t allocRun(ProbeResult** d)
{
    hipError_t e = hipMalloc(d, sizeof(ProbeResult));
    if (e == hipSuccess) e = hipMemset(*d, 0, sizeof(ProbeResult));
    return e;
}
hipError_t finishRun(hipError_t e, ProbeResult* d, ProbeResult* out)
{
    if (e == hipSuccess) e = hipMemcpy(out, d, sizeof(ProbeResult), hipMemcpyDeviceToHost);
    const hipError_t f = hipFree(d);
    return e != hipSuccess ? e : f;
}

} // namespace

extern "C" {

// A, B, C.  op: 0 v_rsq_f32, 1 v_rcp_f32, 2 sqrtSeq1, 3 sqrtSeq2 (second lane: the range backwards), 4 sqrt2 (second
// lane: the neighbouring pattern), 5 sqrt2 with lane 0's second operand -1 in every wave.  Patterns first .. first + count - 1.
int probe_unary(int op, uint64_t first, uint64_t count, uint32_t tol, ProbeResult* out)
{
    Unary u{ first, first, count, op, tol };
    return (int)runSweep(u, count, out);
}

// D.  mode 0: every pattern k in [first, first + count) as the denominator of each numerator of `set`; mode 1: as the
// numerator over each value of `set`; mode 2: hashed pairs k; mode 3: k = (en << 19) | (ed << 11) | sample, biased exponents;
// mode 4: quotients next to a rounding midpoint.
int probe_div2(int mode, uint64_t first, uint64_t count, const uint32_t* set, uint32_t nset, ProbeResult* out)
{
    Div dv{};
    dv.base = first; dv.mode = mode; dv.nset = nset > 16u ? 16u : nset;
    for (uint32_t j = 0; j < dv.nset; ++j) dv.set[j] = set[j];
    return (int)runSweep(dv, count, out);
}

// E.  mode 0: k = (triple << 23) | d mantissa with triples (n exponent + 127, d exponent + 127, n sign | mantissa);
// 1: every exponent pair of [2^-30, 2^63) (k >> 16 < 93 * 93); 2: quotients next to a rounding midpoint; 3: nearPlane in [2^-20, 2^20];
// 4: outside the domain (d >= 2^126), the negative control.
int probe_quotient(int mode, uint64_t first, uint64_t count, const uint32_t* triples, uint32_t ntrip, ProbeResult* out)
{
    Quot q{};
    q.base = first; q.mode = mode; q.ntrip = ntrip < 1u ? 1u : ntrip > 32u ? 32u : ntrip;
    for (uint32_t j = 0; j < q.ntrip * 3u && triples; ++j) q.trip[j / 3u][j % 3u] = triples[j];
    if (!triples) { q.trip[0][0] = 127u; q.trip[0][1] = 127u; q.trip[0][2] = 0u; }
    return (int)runSweep(q, count, out);
}

// H.  op 0: the 256 bytes (u8Unorm, coneTableEntry, coneAxisCutoff); 1: hzbLevel of every pattern; 2: the frexp level choice.
int probe_levels(int op, uint64_t first, uint64_t count, uint32_t mips, ProbeResult* out)
{
    Levels l{ first, op, mips };
    return (int)runSweep(l, count, out);
}

// F.  occ / cone: the template pair; layout 0: all lanes in the SAFE range; 1: lane 5 of every wave outside it and
// inactive; 2: lane 5 outside it and active.
int probe_step(int occ, int cone, int layout, uint64_t count, float nearPlane, ProbeResult* out)
{
    ProbeResult* d = nullptr;
    hipError_t e = allocRun(&d);
    ProbeView pv = {};
    pv.nearPlane = nearPlane;
    for (uint64_t at = 0; e == hipSuccess && at < count; at += kChunk) {
        const uint64_t n = count - at < kChunk ? count - at : kChunk;
        if (occ && cone) hipLaunchKernelGGL((stepKernel<true, true>), dim3(kGrid), dim3(kBlock), 0, 0, at, n, pv, layout, d);
        else if (occ) hipLaunchKernelGGL((stepKernel<true, false>), dim3(kGrid), dim3(kBlock), 0, 0, at, n, pv, layout, d);
        else hipLaunchKernelGGL((stepKernel<false, true>), dim3(kGrid), dim3(kBlock), 0, 0, at, n, pv, layout, d);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    return (int)finishRun(e, d, out);
}

// G.  view: P00, P11, nearPlane, HZB width, height, mips and the view rotation (row-major 3 x 3).  noBand: the bands
// zeroed (negative control).  aux[0]: lanes whose lookup matters; tested: of them the sure ones; aux[3]: cone lanes;
// aux[4]: of them the sure ones; aux[5]: cone mismatches (also counted in mismatches).
int probe_filtered(int cone, uint64_t count, float P00, float P11, float nearPlane, uint32_t hzbW, uint32_t hzbH, uint32_t mips,
                   const float* view, int noBand, ProbeResult* out)
{
    if (mips < 1u || mips > 16u) return (int)hipErrorInvalidValue;
    ProbeResult* d = nullptr;
    hipError_t e = allocRun(&d);
    ProbeView pv = {};
    pv.P00 = P00; pv.P11 = P11; pv.nearPlane = nearPlane; pv.hzbW = hzbW; pv.hzbH = hzbH; pv.mips = mips;
    for (int j = 0; j < 9; ++j) pv.view[j] = view[j];
    const QuadGeom qg = quadGeom(hzbW, hzbH, mips);
    for (uint64_t at = 0; e == hipSuccess && at < count; at += kChunk) {
        const uint64_t n = count - at < kChunk ? count - at : kChunk;
        if (cone) hipLaunchKernelGGL(filteredKernel<true>, dim3(kGrid), dim3(kBlock), 0, 0, at, n, pv, qg, noBand, d);
        else hipLaunchKernelGGL(filteredKernel<false>, dim3(kGrid), dim3(kBlock), 0, 0, at, n, pv, qg, noBand, d);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    return (int)finishRun(e, d, out);
}

// The references of fp_ref.h compiled for the host (tests/test_probe_ref.py checks them with exact rationals).
uint32_t probe_ref_sqrt(uint32_t x) { return fr::sqrtRN(x); }
uint32_t probe_ref_div(uint32_t n, uint32_t d) { return fr::divRN(n, d); }
uint32_t probe_ref_rcp(uint32_t x) { return fr::rcpRN(x); }
uint32_t probe_ref_rsq(uint32_t x) { return fr::rsqRN(x); }
uint64_t probe_ref_ulp_dist(uint32_t a, uint32_t b) { return fr::ulpDist(a, b); }
int probe_ref_floor_log2(uint32_t x) { return fr::floorLog2(x); }
uint32_t probe_result_size() { return (uint32_t)sizeof(ProbeResult); }

} // extern "C"
