// k_raster.hip -- "basepass_MS_Main_depth": depth of the visible meshlets of one pass slot, the compute stand-in for
// the mesh shader + fixed-function rasteriser + depth test of the reference's base pass
// (source/shaders/basepass.hlsl:124-188 MS_Main: vertex fetch through g_MeshletVertexIDsBuffer / g_MeshletIndexIDsBuffer,
// position * world * worldToClip; PSO BasePassRenderers.cpp:481-495, reverse-Z depth GREATER).  SURVEY.md 8(f) rank 1:
// it closes the two-phase loop with depth the path produced itself instead of a synthetic depth image.
//
// The geometry block, the chain from a visible-list entry to its meshlet, the vertex transform, the edge function and the
// visibility texel's format are those of mesh_stage.hip.h, which the resolve (visibility_resolve.hip.h) shares.
//
// The rasteriser has no source to restate: its rules are this build's CONVENTION (parity unpinned), stated once in
// oracle/tr_oracle.h (orc_raster_depth) and followed here operation for operation -- no near clipping (a triangle with a
// vertex at w <= near is dropped), pixel-centre samples, inclusive edge functions on both windings, depth interpolated
// with one fma chain and one division, atomic max on the float bits (depth > 0, so unsigned order = float order).  The
// result is a maximum, so it does not depend on the order the triangles are drawn in: bit-exact against the oracle.
//
// Two launches.  "main": one wave per visible meshlet -- lanes transform the (<= 64) vertices into the wave's LDS
// slice, then set up the triangles (lane t: triangle t); a triangle whose box exceeds kSmallBox pixels is appended to a
// queue (screen positions, depths, box; one counter update per wave), the others are drawn by the wave one after the
// other, 64 pixels of the bounding box per pass.  "tiles": one
// workgroup per 64x64-pixel screen tile collects the queued triangles that touch it and rasterises them into an LDS copy
// of the tile, 4096 pixels at a time, then merges the tile into the depth buffer; it looks for them in the list of its
// 256x256-pixel coarse bin, which "main" fills while it queues.  Without the second launch a dozen
// waves walked the 10^4-pixel boxes of a near wall while the chip idled (3.2 ms per pass at 3840x2160,
// tools/raster_time.py).  Every pixel value is computed by the same operations whichever launch produces it.
//
// "basepass_MS_Main_visibility": the same two launches and the same arithmetic, instantiated with a second sink.  Every
// covered sample of triangle t of visible-list entry v of pass slot s (push constant) also does one 64-bit atomic max of
// (depthBits << 32) | packVisibility(s, v, t) into u1, the RG32_UINT visibility buffer.  TIE RULE (a convention, parity
// unpinned: hardware resolves ties by draw order): on equal depth the larger payload wins, so the result does not depend
// on the draw order, as the depth does not.  The texel is 0 where nothing was drawn (depth > 0 on every written sample).
// Triangles with index >= 128 (out of contract: kMaxMeshletTriangles is 96) write depth but no visibility texel; a list
// capacity above 2^23 entries is refused at record time.  The tile launch keeps a 64x64 tile of u64 beside the depth tile
// in LDS; its far-depth early-out reads the visibility words and stays a strict "<", so a triangle that can tie the kept
// depth is still drawn (it can win the payload).  The early-out is taken only for a triangle whose largest vertex depth
// lies in [kSkipMinDepth, kSkipMaxDepth) = [2^-30, 1 - 2^-21): the range in which its samples are proven to stay below
// that depth times kSkipFactor (derivation at the constants; below it the products of weights and depths round in the
// subnormal range and samples exceed the bound, tests/test_raster_path_scenes.py).  The depth instantiation keeps its
// kernels, launches, op names and arithmetic; the compiler schedules and allocates its registers slightly differently
// (tiles: 58 VGPRs instead of 55).
// tools/raster_time.py at 3840x2160, per launch, before / after the template: main 142.4 / 146.7 us, tiles 179.4 / 176.5 us.
//
// "basepass_MS_Main_depth ALPHA_MASK_MODE=1" and "basepass_MS_Main_visibility ALPHA_MASK_MODE=1": the permutation the reference
// draws alpha-mask primitives with (BasePassRenderers.cpp:489, :690-691; its discard: basepass.hlsl:210-215), one more template
// argument of the same two launches.  BINDINGS: those of the plain shader, plus t3 = the MaterialData buffer (required) and t19 =
// the texture table (TRHIP_BIND_TEXTURE_TABLE, optional).  CONVENTION (parity unpinned, like the rest of the raster; restated in
// tests/alpha_test_ref.c).  A covered sample of a triangle passes these steps after `d > 0` and before either atomic:
//   1. q_i = e_i / w_i and s = (q0 + q1) + q2 from the sample's own edge values e_i and the vertices' clip w;
//   2. uv = fma(q2, a2, fma(q1, a1, q0 * a0)) / s of m_TexCoord (half -> float, exact);
//   3. ddx(uv), ddy(uv) from the same triangle's plane, re-evaluated at (cx + 1, cy) and at (cx, cy + 1), minus the centre value
//      (steps 1 to 3: mesh::uvFootprint, the formulas of the TEXTURED resolve);
//   4. alpha = m_ConstAlbedo.w, times mtex::sampleAlpha(...) with the albedo slot's m_IsWrapSampler if MaterialFlag_UseAlbedoTexture;
//   5. the sample is discarded iff alpha < m_AlphaCutoff; a NaN alpha is kept, as `discard` under a false comparison keeps it;
//   6. nothing of the triangle is drawn, like every broken chain here, when m_MaterialDataIdx is past the buffer, the albedo flag
//      is set with no table bound, the descriptor index is past the table, or the entry is empty or of another format.
// The surviving samples still feed a maximum, so the result stays independent of the draw order.  The material row and the table
// entry are resolved once per meshlet in "main" (one instance, one material) and once per queued triangle in "tiles", never per
// sample; a texture-free material is decided there for all its samples.  "main" keeps w and the packed m_TexCoord per vertex
// beside sx, sy and sd in the wave's LDS slice; a queued triangle carries three w, three uv words and the material index in a
// second scratch array beside queuePayload (AlphaTriangle, 32 bytes per entry), allocated by these instantiations only.
// The four plain kernels keep their names and arithmetic, and the compiler reports the same resources for them as before the
// template argument (VGPRs / SGPRs / LDS bytes / waves per SIMD, -Rpass-analysis=kernel-resource-usage): depth main 64 / 100 / 15360 /
// 8, visibility main 68 / 103 / 15360 / 7, depth tiles 58 / 82 / 20500 / 7, visibility tiles 55 / 83 / 53272 / 3, no scratch: no
// difference.  The new ones: depth main 141 / 106 / 25600 / 3, visibility main 144 / 106 / 25600 / 3, depth tiles 125 / 106 /
// 20500 / 4, visibility tiles 127 / 106 / 53272 / 3, no scratch (profiles/alpha_test/README.md).
// MEASURED (tools/alpha_test_cost.py, the generated city at 3840x2160 with 225 of 2251 instances alpha-masked and textured, the
// alpha-mask list alone so that both sides draw the same lists, sides alternated three times on one MI355X): visibility main 304.4
// us plain / 3433.3 us alpha-tested, tiles 268.4 / 2012.6 us.  Two thirds of it are the tap loop's bilinear fetches, run by the few lanes of a chunk that lie inside the triangle (attribution there).  Untuned: correctness came first.
#include "material_textures.hip.h"
#include "mesh_stage.hip.h"

using namespace mesh;

namespace
{

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWaves = kBlock / 64;
constexpr uint32_t kSmallBox = 1024;            // pixels: larger bounding boxes go to the tile pass
constexpr uint32_t kTile = 64;                  // pixels per side
constexpr uint32_t kQueueCapacity = 1u << 20;   // 48 MB; beyond it triangles are drawn in place (slow, still exact)
constexpr uint32_t kTileList = 1024;            // queued triangles a tile handles per round
constexpr uint32_t kBinShift = 8;               // coarse bins of 256x256 pixels (4x4 tiles): a tile scans its bin's list, not the whole queue
constexpr uint32_t kBinCapacity = 1u << 16;     // queue indices per bin; a fuller bin makes its tiles scan the whole queue

// The tile pass's far-depth early-out skips a queued triangle when M * kSkipFactor < tileFar, M = max(d0,d1,d2), and
// M lies in [kSkipMinDepth, kSkipMaxDepth).  Inside that range every sample d of the triangle is < tileFar.  With
// u = 2^-24, e_i >= 0 the weights of a covered centre, S = e0 + e1 + e2 exactly and den = fl(fl(e0 + e1) + e2):
//   * Screen coordinates come from fma(x, half, half) with half >= 0.5, so each is 0 or at least 2^-25 in magnitude: a
//     multiple of 2^-48.  Pixel centres are multiples of 2^-1.  The differences in edgeFn are then multiples of 2^-48,
//     its two products and its result multiples of 2^-96 (rounding only coarsens): a weight is 0 or >= 2^-96, and
//     den >= 2^-96 where den > 0.  The sums of the weights do not underflow: den >= S (1 - u)^2.
//   * The numerator fma(e2, d2, fma(e1, d1, e0 * d0)) rounds three times, each time by at most u relative where the
//     result is normal and by at most 2^-150 absolute where it is not.  Terms with d_i <= 0 only lower it, so it is at
//     most S M (1 + u)^3 + 3 * 2^-150, and it stays finite because den is finite and M < 1 - 8u.
//   * The division rounds once more: d <= M (1 + u)^4 / (1 - u)^2 + 3.01 * 2^-150 / den + 2^-150
//                                      <= M (1 + 7u) + 2^-52.
//     The last term is the one the normal range hides: it is at most 4u M exactly when M >= 2^-30.  Below that, or with
//     a smaller den, a product e_i * d_i rounds in the subnormal range and a sample can exceed M by any factor.
//   * So d <= M (1 + 11u) < M (1 + 16u)(1 - u) <= fl(M * kSkipFactor) < tileFar.  Strictly: the triangle cannot tie either.
// A triangle outside the range is drawn: depth = near / w, so M < 2^-30 needs w > 2^30 near and M >= 1 - 2^-21 a vertex
// within 2^-21 of the near plane.
constexpr float kSkipFactor = 0x1.00001p+0f;    // 1 + 16u
constexpr float kSkipMinDepth = 0x1p-30f;
constexpr float kSkipMaxDepth = 0x1.fffffp-1f;  // 1 - 8u

struct BigTriangle                              // 48 bytes
{
    float x0, y0, d0, x1, y1, d1, x2, y2, d2, sgn;
    uint32_t boxX, boxY;                        // x0 | x1 << 16, y0 | y1 << 16 (inclusive pixel bounds)
};

struct RasterArgs
{
    BasePassConstants k;
    Geometry geo;
    const MeshletAmplificationData* records; uint32_t recordCapacity;
    const uint32_t* visibleList; uint32_t listCapacity;
    const uint32_t* drawArgs;                                    // {numVisible, 1, 1}
    uint32_t* depth;                                             // R32F as bits
    uint32_t width, height;
    BigTriangle* queue;                                          // scratch: [kQueueCapacity]
    uint32_t* queueCount;                                        // scratch, zeroed before "main"
    uint32_t* binCount;                                          // scratch, zeroed: [binsX * binsY] entries appended (may exceed the capacity)
    uint32_t* binList;                                           // scratch: [binsX * binsY][kBinCapacity] queue indices
    uint32_t binsX, binsY;
};

// The visibility sink's extra state (nullptr / 0 in the depth instantiation, where it is never read).
struct VisArgs
{
    unsigned long long* vis;                                     // RG32_UINT as u64
    unsigned long long* queuePayload;                            // scratch: [kQueueCapacity], (1 << 32 | payload) or 0 = no texel
    uint32_t slotBits;                                           // visSlotBits(passSlot)
};

// The alpha test's extra state (nullptr / 0 in the plain instantiations, where it is never read).
struct AlphaTriangle                            // 32 bytes: what a queued triangle carries beside BigTriangle and queuePayload
{
    float w0, w1, w2;                           // clip w of the three vertices
    uint32_t tc0, tc1, tc2;                     // m_TexCoord, half2
    uint32_t material;                          // m_MaterialDataIdx of the triangle's instance
    uint32_t pad;
};

struct AlphaArgs
{
    const char* materials; uint32_t numMaterials;                // t3: MaterialData, 124-byte stride
    const mtex::TableEntry* table; uint32_t tableCount;          // t19, or nullptr / 0: no table bound
    AlphaTriangle* queueAlpha;                                   // scratch: [kQueueCapacity]
};

// What the test needs of one triangle's material, resolved once per meshlet ("main") or per queued triangle ("tiles"), never
// per sample.  draw == false: a broken chain, or a texture-free material whose constant alpha fails the test -- no sample of
// the triangle is drawn.
struct AlphaMaterial { bool draw; bool wrap; const mtex::TableEntry* tex; float alpha, cutoff; };

__device__ __forceinline__ AlphaMaterial alphaMaterial(const AlphaArgs& aa, uint32_t materialIdx)
{
    AlphaMaterial m = { false, false, nullptr, 0.0f, 0.0f };
    if (materialIdx >= aa.numMaterials) return m;
    const MaterialData& md = *reinterpret_cast<const MaterialData*>(aa.materials + (uint64_t)materialIdx * sizeof(MaterialData));
    m.alpha = md.m_ConstAlbedo.w; m.cutoff = md.m_AlphaCutoff;
    if (md.m_MaterialFlags & MaterialFlag_UseAlbedoTexture) {
        const uint32_t d = md.m_AlbedoTexture.m_DescriptorIndex;
        if (d >= aa.tableCount || !mtex::sampled(aa.table[d])) return m;                  // no table, past it, empty, another format
        m.tex = aa.table + d;
        m.wrap = md.m_AlbedoTexture.m_IsWrapSampler != 0u;
        m.draw = true;
    } else {
        m.draw = !(m.alpha < m.cutoff);                                                   // a NaN is kept
    }
    return m;
}

// coverBox, one triangle over the pixels of its box: mesh_stage.hip.h (the probe spheres' draw, k_giprobedraw.hip, shares it).

// ALPHA_MASK_MODE's discard at one covered sample of triangle (q, t) with material m (m.draw): see the header's CONVENTION.
__device__ __forceinline__ bool alphaKeeps(const BigTriangle& q, const AlphaTriangle& t, const AlphaMaterial& m, float cx, float cy, float e0, float e1, float e2)
{
    if (!m.tex) return true;                                                              // constant alpha: decided with the material
    const UvFootprint f = uvFootprint(q.x0, q.y0, q.x1, q.y1, q.x2, q.y2, q.sgn, t.w0, t.w1, t.w2, t.tc0, t.tc1, t.tc2, cx, cy, e0, e1, e2);
    const float alpha = m.alpha * mtex::sampleAlpha(*m.tex, m.wrap, f.u, f.v, f.dudx, f.dvdx, f.dudy, f.dvdy);
    return !(alpha < m.cutoff);                                                           // discard iff alpha < cutoff: a NaN is kept
}

template <bool Vis, bool Alpha>
__device__ __forceinline__ void rasterMain(const RasterArgs& a, const VisArgs& va, const AlphaArgs& aa)
{
    __shared__ float s_x[kWaves][64], s_y[kWaves][64], s_d[kWaves][64];
    __shared__ BigTriangle s_tri[kWaves][64];
    __shared__ float s_w[Alpha ? kWaves : 1][64];                                        // alpha test only: clip w and m_TexCoord per vertex,
    __shared__ uint32_t s_tc[Alpha ? kWaves : 1][64];
    __shared__ AlphaTriangle s_atri[Alpha ? kWaves : 1][64];                             // and per triangle drawn in place
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float* sx = s_x[wave]; float* sy = s_y[wave]; float* sd = s_d[wave];
    float* sw = s_w[Alpha ? wave : 0]; uint32_t* stc = s_tc[Alpha ? wave : 0];
    uint32_t V = a.drawArgs[0];
    V = V < a.listCapacity ? V : a.listCapacity;
    const uint32_t W = a.width, H = a.height;
    const float halfW = 0.5f * (float)W, halfH = 0.5f * (float)H;
    const cm::M43 clipXYZ = cm::loadM43(a.k.m_WorldToClip);
    for (uint32_t v = blockIdx.x * kWaves + wave; v < V; v += gridDim.x * kWaves) {
        withMeshlet(a.visibleList[v], a.records, a.recordCapacity, a.geo, [&](const Meshlet& ml) {   // the rest of the iteration, not indented
        const uint32_t nv = ml.nv, nt = ml.nt;
        AlphaMaterial am = {};
        if constexpr (Alpha) {
            am = alphaMaterial(aa, ml.inst->m_MaterialDataIdx);                           // the whole meshlet's: one instance, one material
            if (!am.draw) return;                                                        // wave-uniform, before the LDS slice is touched
        }
        const cm::M43 Wm = cm::loadM43(ml.inst->m_WorldMatrix);
        // ---- vertices (:149-158): lane l transforms vertex l ------------------------------------------------
        bool ok = false;
        if (lane < nv) {
            const uint32_t vid = a.geo.vertexIds[ml.vertexIdsAt + lane];
            if (vid < a.geo.numVertices) {
                const float* p = vertexAt(a.geo, vid).m_Position;
                const ScreenVertex s = toScreen({ p[0], p[1], p[2] }, Wm, clipXYZ, a.k.m_WorldToClip, halfW, halfH);
                ok = s.w > a.k.m_NearPlane;
                sx[lane] = s.sx; sy[lane] = s.sy; sd[lane] = s.depth;
                if constexpr (Alpha) { sw[lane] = s.w; stc[lane] = *reinterpret_cast<const uint32_t*>(vertexAt(a.geo, vid).m_TexCoord); }
            }
        }
        const unsigned long long okMask = __ballot(ok);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- triangles (:178-187).  Set-up in parallel: lane t prepares triangle t (64 at a time); the large ones are
        //      queued with ONE counter update per wave, the others are then drawn one after the other, 64 pixels of the
        //      bounding box per pass -----------------------------------------------------------------------------------
        BigTriangle* st = s_tri[wave];
        for (uint32_t tb = 0; tb < nt; tb += 64u) {
            const uint32_t t = tb + lane;
            bool live = false;
            BigTriangle q = {};
            AlphaTriangle qa = {};
            uint32_t bw = 0, bh = 0;
            if (t < nt) {
                const uint32_t packed = a.geo.triangles[ml.trianglesAt + t];
                const uint32_t ia = packed & 0xFFu, ib = (packed >> 8) & 0xFFu, ic = (packed >> 16) & 0xFFu;
                if (ia < nv && ib < nv && ic < nv && ((okMask >> ia) & (okMask >> ib) & (okMask >> ic) & 1ull)) {
                    q.x0 = sx[ia]; q.y0 = sy[ia]; q.x1 = sx[ib]; q.y1 = sy[ib]; q.x2 = sx[ic]; q.y2 = sy[ic];
                    q.d0 = sd[ia]; q.d1 = sd[ib]; q.d2 = sd[ic];
                    if constexpr (Alpha) qa = { sw[ia], sw[ib], sw[ic], stc[ia], stc[ib], stc[ic], ml.inst->m_MaterialDataIdx, 0u };
                    const float area = edgeFn(q.x0, q.y0, q.x1, q.y1, q.x2, q.y2);
                    const float fminx = cm::min_(cm::min_(q.x0, q.x1), q.x2), fmaxx = cm::max_(cm::max_(q.x0, q.x1), q.x2);
                    const float fminy = cm::min_(cm::min_(q.y0, q.y1), q.y2), fmaxy = cm::max_(cm::max_(q.y0, q.y1), q.y2);
                    if (area != 0.0f                                                          // not degenerate, not NaN
                        && fmaxx >= 0.0f && fmaxy >= 0.0f && fminx <= (float)W && fminy <= (float)H) {   // on screen, not NaN
                        q.sgn = area < 0.0f ? -1.0f : 1.0f;
                        const int bx0 = (int)cm::max_(__builtin_floorf(fminx), 0.0f), bx1 = (int)cm::min_(__builtin_ceilf(fmaxx), (float)(W - 1));
                        const int by0 = (int)cm::max_(__builtin_floorf(fminy), 0.0f), by1 = (int)cm::min_(__builtin_ceilf(fmaxy), (float)(H - 1));
                        if (bx1 >= bx0 && by1 >= by0) {
                            live = true;
                            bw = (uint32_t)(bx1 - bx0 + 1); bh = (uint32_t)(by1 - by0 + 1);
                            q.boxX = (uint32_t)bx0 | ((uint32_t)bx1 << 16); q.boxY = (uint32_t)by0 | ((uint32_t)by1 << 16);
                        }
                    }
                }
            }
            // large on screen: the tile pass draws them
            bool big = live && (uint64_t)bw * bh > kSmallBox && a.queue != nullptr;
            const unsigned long long bigMask = __ballot(big);
            if (bigMask) {
                uint32_t first = 0;
                if (lane == 0) first = atomicAdd(a.queueCount, (uint32_t)__popcll(bigMask));
                first = __shfl(first, 0);
                const uint32_t slot = first + (uint32_t)__popcll(bigMask & ((1ull << lane) - 1ull));
                if (big && slot < kQueueCapacity) {
                    a.queue[slot] = q;
                    if constexpr (Vis) va.queuePayload[slot] = t < kVisTriangles ? (1ull << 32) | packVisibility(va.slotBits, v, t) : 0ull;
                    if constexpr (Alpha) aa.queueAlpha[slot] = qa;
                    // its index goes to every coarse bin the box touches
                    const uint32_t cx0 = (q.boxX & 0xFFFFu) >> kBinShift, cx1 = (q.boxX >> 16) >> kBinShift;
                    const uint32_t cy0 = (q.boxY & 0xFFFFu) >> kBinShift, cy1 = (q.boxY >> 16) >> kBinShift;
                    for (uint32_t cy = cy0; cy <= cy1; ++cy)
                        for (uint32_t cx = cx0; cx <= cx1; ++cx) {
                            const uint32_t bin = cy * a.binsX + cx;
                            const uint32_t k = atomicAdd(&a.binCount[bin], 1u);
                            if (k < kBinCapacity) a.binList[(uint64_t)bin * kBinCapacity + k] = slot;
                        }
                } else {
                    big = false;                                                             // queue full: drawn in place
                }
            }
            // the others, in place
            const unsigned long long smallMask = __ballot(live && !big);
            if (smallMask) {
                st[lane] = q;
                if constexpr (Alpha) s_atri[wave][lane] = qa;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                uint32_t* depth = a.depth;
                for (unsigned long long mrem = smallMask; mrem; mrem &= mrem - 1ull) {
                    const BigTriangle c = st[__builtin_ctzll(mrem)];
                    AlphaTriangle ca = {};
                    if constexpr (Alpha) ca = s_atri[wave][__builtin_ctzll(mrem)];
                    const uint32_t bx0 = c.boxX & 0xFFFFu, by0 = c.boxY & 0xFFFFu;
                    const uint32_t tri = tb + (uint32_t)__builtin_ctzll(mrem);
                    const bool texel = tri < kVisTriangles;
                    const unsigned long long payload = packVisibility(va.slotBits, v, tri);
                    unsigned long long* vis = va.vis;
                    coverBox(c.x0, c.y0, c.d0, c.x1, c.y1, c.d1, c.x2, c.y2, c.d2, c.sgn, bx0, by0, (c.boxX >> 16) - bx0 + 1u, (c.boxY >> 16) - by0 + 1u, lane, 64u,
                             [&](float cx, float cy, float e0, float e1, float e2) { if constexpr (Alpha) return alphaKeeps(c, ca, am, cx, cy, e0, e1, e2); else return true; },
                             [=](uint32_t px, uint32_t py, uint32_t bits) {
                                 const uint64_t i = (uint64_t)py * W + px;
                                 atomicMax(&depth[i], bits);
                                 if constexpr (Vis) if (texel) atomicMax(&vis[i], (unsigned long long)bits << 32 | payload); });
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                       // st is rewritten by the next 64 triangles
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                           // the LDS slice is reused by the next meshlet
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        });                                                                              // withMeshlet: an entry out of bounds skips all of the above
    }
}

__global__ __launch_bounds__(kBlock) void rasterDepthKernel(RasterArgs a) { rasterMain<false, false>(a, VisArgs{}, AlphaArgs{}); }
__global__ __launch_bounds__(kBlock) void rasterVisibilityKernel(RasterArgs a, VisArgs va) { rasterMain<true, false>(a, va, AlphaArgs{}); }
__global__ __launch_bounds__(kBlock) void rasterDepthAlphaKernel(RasterArgs a, AlphaArgs aa) { rasterMain<false, true>(a, VisArgs{}, aa); }
__global__ __launch_bounds__(kBlock) void rasterVisibilityAlphaKernel(RasterArgs a, VisArgs va, AlphaArgs aa) { rasterMain<true, true>(a, va, aa); }


// The queued triangles, by screen tile.  Rounds of at most kTileList triangles: collect (all threads scan the queue,
// LDS append), rasterise into the LDS tile, next round; then merge.  A tile is owned by one workgroup and this launch
// follows "main" on the stream, so the merge needs no atomics.
template <bool Vis, bool Alpha>
__device__ __forceinline__ void rasterTiles(const RasterArgs& a, const VisArgs& va, const AlphaArgs& aa)
{
    __shared__ uint32_t s_depth[kTile * kTile];
    __shared__ uint32_t s_list[kTileList];
    __shared__ uint32_t s_count;
    __shared__ uint32_t s_waveMin[kWaves];
    __shared__ unsigned long long s_vis[Vis ? kTile * kTile : 1];                       // 32 KB beside the 16 KB depth tile (visibility only)
    const uint32_t tid = threadIdx.x;
    uint32_t n = *a.queueCount;
    n = n < kQueueCapacity ? n : kQueueCapacity;
    if (n == 0) return;
    const uint32_t tilesX = (a.width + kTile - 1) / kTile, tilesY = (a.height + kTile - 1) / kTile;
    for (uint32_t tile = blockIdx.x; tile < tilesX * tilesY; tile += gridDim.x) {
        const uint32_t tx0 = (tile % tilesX) * kTile, ty0 = (tile / tilesX) * kTile;
        const uint32_t tx1 = min(tx0 + kTile, a.width) - 1u, ty1 = min(ty0 + kTile, a.height) - 1u;
        for (uint32_t i = tid; i < kTile * kTile; i += kBlock) s_depth[i] = 0u;
        if constexpr (Vis)
            for (uint32_t i = tid; i < kTile * kTile; i += kBlock) s_vis[i] = 0ull;
        bool any = false;
        float tileFar = 0.0f;                                                            // farthest depth in the tile (0 = something still uncovered)
        // candidates: the list of the tile's coarse bin, or the whole queue when that list overflowed
        const uint32_t bin = (ty0 >> kBinShift) * a.binsX + (tx0 >> kBinShift);
        const uint32_t binned = a.binCount[bin];
        const bool wholeQueue = binned > kBinCapacity;
        const uint32_t* candidates = a.binList + (uint64_t)bin * kBinCapacity;
        const uint32_t nCand = wholeQueue ? n : binned;
        for (uint32_t base = 0; base < nCand;) {
            if (tid == 0) s_count = 0;
            __syncthreads();
            // collect: the scan stops early when the list is full; `base` advances to the first triangle not yet looked at
            uint32_t next = base;
            for (; next < nCand; next += kBlock) {
                const uint32_t c = next + tid;
                if (c < nCand) {
                    const uint32_t i = wholeQueue ? c : candidates[c];
                    const uint32_t bx = a.queue[i].boxX, by = a.queue[i].boxY;
                    if ((bx & 0xFFFFu) <= tx1 && (bx >> 16) >= tx0 && (by & 0xFFFFu) <= ty1 && (by >> 16) >= ty0) {
                        const uint32_t k = atomicAdd(&s_count, 1u);
                        s_list[k] = i;                                                     // room for it: checked below before the next chunk
                    }
                }
                __syncthreads();
                const bool full = s_count + kBlock > kTileList;                            // the next chunk might not fit
                __syncthreads();
                if (full) { next += kBlock; break; }
            }
            base = next;
            const uint32_t m = s_count;
            any |= m != 0;
            for (uint32_t k = 0; k < m; ++k) {
                // Every 32 triangles: the farthest depth the tile holds so far.  A triangle none of whose samples can be
                // nearer than that cannot change a maximum and is skipped: see kSkipMinDepth for the bound on its samples.
                // With the alpha test the bound holds as it is: a discard only removes samples from both sides of the
                // comparison's right hand (the skipped triangle's) and leaves holes at depth 0 on its left (tileFar = 0).
                if ((k & 31u) == 0u && (k != 0u || any)) {
                    uint32_t mn = 0xFFFFFFFFu;
                    const uint32_t w = tx1 - tx0 + 1u, h = ty1 - ty0 + 1u;
                    if constexpr (Vis) {
                        // the far depth of the TEXELS: a depth written by an out-of-contract triangle alone must not hide
                        // the triangles that can still win the texel below it
                        for (uint32_t i = tid; i < w * h; i += kBlock) { const uint32_t y = i / w, x = i - y * w; mn = min(mn, (uint32_t)(s_vis[y * kTile + x] >> 32)); }
                    } else {
                        for (uint32_t i = tid; i < w * h; i += kBlock) { const uint32_t y = i / w, x = i - y * w; mn = min(mn, s_depth[y * kTile + x]); }
                    }
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, d));
                    __syncthreads();                                                     // the previous value has been read by everyone
                    if ((tid & 63u) == 0u) s_waveMin[tid >> 6] = mn;
                    __syncthreads();
                    tileFar = __uint_as_float(min(min(s_waveMin[0], s_waveMin[1]), min(s_waveMin[2], s_waveMin[3])));   // depths are > 0: bit order = value order
                }
                const BigTriangle q = a.queue[s_list[k]];
                const float far = cm::max_(cm::max_(q.d0, q.d1), q.d2);
                if (far * kSkipFactor < tileFar && far >= kSkipMinDepth && far < kSkipMaxDepth) continue;   // NaN or inf: never skipped
                const uint32_t bx0 = max(q.boxX & 0xFFFFu, tx0), bx1 = min(q.boxX >> 16, tx1);
                const uint32_t by0 = max(q.boxY & 0xFFFFu, ty0), by1 = min(q.boxY >> 16, ty1);
                unsigned long long qp = 0ull;                                              // (1 << 32 | payload), or 0 = no texel
                if constexpr (Vis) qp = va.queuePayload[s_list[k]];
                const bool texel = (qp >> 32) != 0ull;
                const unsigned long long payload = qp & 0xFFFFFFFFull;
                AlphaTriangle qa = {};
                AlphaMaterial am = {};
                if constexpr (Alpha) {
                    qa = aa.queueAlpha[s_list[k]];
                    am = alphaMaterial(aa, qa.material);
                    if (!am.draw) continue;                                               // uniform over the workgroup; no barrier below in this iteration
                }
                coverBox(q.x0, q.y0, q.d0, q.x1, q.y1, q.d1, q.x2, q.y2, q.d2, q.sgn, bx0, by0, bx1 - bx0 + 1u, by1 - by0 + 1u, tid, kBlock,
                         [&](float cx, float cy, float e0, float e1, float e2) { if constexpr (Alpha) return alphaKeeps(q, qa, am, cx, cy, e0, e1, e2); else return true; },
                         [=](uint32_t px, uint32_t py, uint32_t bits) {
                             const uint32_t i = (py - ty0) * kTile + (px - tx0);
                             atomicMax(&s_depth[i], bits);
                             if constexpr (Vis) if (texel) atomicMax(&s_vis[i], (unsigned long long)bits << 32 | payload); });
            }
            __syncthreads();
        }
        if (any) {
            const uint32_t w = tx1 - tx0 + 1u, h = ty1 - ty0 + 1u;
            for (uint32_t i = tid; i < w * h; i += kBlock) {
                const uint32_t y = i / w, x = i - y * w;
                const uint32_t v = s_depth[y * kTile + x];
                if (v) { uint32_t* g = &a.depth[(uint64_t)(ty0 + y) * a.width + tx0 + x]; if (v > *g) *g = v; }
                if constexpr (Vis) {
                    const unsigned long long t = s_vis[y * kTile + x];
                    if (t) { unsigned long long* g = &va.vis[(uint64_t)(ty0 + y) * a.width + tx0 + x]; if (t > *g) *g = t; }
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void rasterTilesKernel(RasterArgs a) { rasterTiles<false, false>(a, VisArgs{}, AlphaArgs{}); }
__global__ __launch_bounds__(kBlock) void rasterVisibilityTilesKernel(RasterArgs a, VisArgs va) { rasterTiles<true, false>(a, va, AlphaArgs{}); }
__global__ __launch_bounds__(kBlock) void rasterTilesAlphaKernel(RasterArgs a, AlphaArgs aa) { rasterTiles<false, true>(a, VisArgs{}, aa); }
__global__ __launch_bounds__(kBlock) void rasterVisibilityTilesAlphaKernel(RasterArgs a, VisArgs va, AlphaArgs aa) { rasterTiles<true, true>(a, va, aa); }

template <bool Vis, bool Alpha>
int recordRaster(trhip::DispatchCtx& ctx)
{
    // Binding set of BasePassRenderers.cpp:463-479 (the geometry of mesh_stage.hip.h, t7 amplification records) + the
    // outputs of the cull half: t9 visible list, indirect args = its draw args; u0 = the depth buffer (R32_FLOAT).
    const BasePassConstants* k = (const BasePassConstants*)ctx.constants(0, sizeof(BasePassConstants));
    TRHIP_REQUIRE(k, "%s: constant buffer b0 (BasePassConstants, 256 bytes) missing", ctx.shaderName);
    RasterArgs a;
    memset(&a, 0, sizeof a);
    a.k = *k;
    if (const int rc = bindGeometry(ctx, a.geo)) return rc;
    trhip_buffer_t* records = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 7);
    trhip_buffer_t* list = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 9);
    uint32_t mip = 0;
    trhip_texture_t* depth = ctx.texture(TRHIP_BIND_TEXTURE_UAV, 0, &mip);
    TRHIP_REQUIRE(records && list, "%s: needs SRVs t7 (records), t9 (visible list)", ctx.shaderName);
    TRHIP_REQUIRE(depth && mip == 0 && depth->format == TRHIP_FORMAT_R32_FLOAT, "%s: needs Texture_UAV u0 = the R32_FLOAT depth buffer, mip 0", ctx.shaderName);
    TRHIP_REQUIRE(ctx.indirect && ctx.argsBuffer->byteSize - ctx.argsOffset >= 12, "%s: dispatched indirectly on the visible list's draw args", ctx.shaderName);
    TRHIP_REQUIRE(k->m_OutputResolution.x == depth->width && k->m_OutputResolution.y == depth->height,
                  "%s: m_OutputResolution %ux%u does not match the depth buffer %ux%u", ctx.shaderName, k->m_OutputResolution.x, k->m_OutputResolution.y, depth->width, depth->height);
    a.records = (const MeshletAmplificationData*)records->ptr; a.recordCapacity = elements32(records, sizeof(MeshletAmplificationData));
    a.visibleList = (const uint32_t*)list->ptr; a.listCapacity = elements32(list, 4);
    a.drawArgs = (const uint32_t*)((const char*)ctx.argsBuffer->ptr + ctx.argsOffset);
    a.depth = (uint32_t*)depth->ptr;
    a.width = depth->width; a.height = depth->height;
    TRHIP_REQUIRE(a.width <= 0xFFFFu && a.height <= 0xFFFFu, "%s: depth buffer %ux%u: at most 65535 pixels per side", ctx.shaderName, a.width, a.height);
    VisArgs va = {};
    if constexpr (Vis) {
        // + u1 = the visibility buffer (RG32_UINT, render resolution), push constants {uint32 passSlot}
        uint32_t visMip = 0;
        trhip_texture_t* vis = ctx.texture(TRHIP_BIND_TEXTURE_UAV, 1, &visMip);
        TRHIP_REQUIRE(vis && visMip == 0 && vis->format == TRHIP_FORMAT_RG32_UINT, "%s: needs Texture_UAV u1 = the RG32_UINT visibility buffer, mip 0", ctx.shaderName);
        TRHIP_REQUIRE(vis->width == depth->width && vis->height == depth->height,
                      "%s: visibility buffer %ux%u does not match m_OutputResolution and the depth buffer %ux%u", ctx.shaderName, vis->width, vis->height, depth->width, depth->height);
        bool pushBound = false;
        for (uint32_t i = 0; i < ctx.numBindings; ++i) pushBound |= ctx.bindings[i].type == TRHIP_BIND_PUSH_CONSTANTS;
        TRHIP_REQUIRE(pushBound && ctx.push && ctx.pushBytes >= 4, "%s: push constants {uint32 passSlot} (4 bytes) missing", ctx.shaderName);
        uint32_t slot;
        memcpy(&slot, ctx.push, 4);
        TRHIP_REQUIRE(slot <= 3u, "%s: pass slot %u: 0..3 (early opaque, late opaque, early alpha mask, late alpha mask)", ctx.shaderName, slot);
        TRHIP_REQUIRE(list->byteSize / 4 <= kVisListCapacity, "%s: visible list of %llu entries: the visibility payload holds list positions below 2^23",
                      ctx.shaderName, (unsigned long long)(list->byteSize / 4));
        va.vis = (unsigned long long*)vis->ptr;
        va.slotBits = visSlotBits(slot);
    }
    // queue of the triangles that are large on screen: scratch of this command; its counter is zeroed by the recording's
    // first clear launch
    a.queue = (BigTriangle*)ctx.scratch((size_t)kQueueCapacity * sizeof(BigTriangle));
    a.queueCount = (uint32_t*)ctx.scratch(16);
    TRHIP_REQUIRE(a.queue && a.queueCount, "%s: scratch allocation failed", ctx.shaderName);
    if constexpr (Vis) {
        va.queuePayload = (unsigned long long*)ctx.scratch((size_t)kQueueCapacity * 8);
        TRHIP_REQUIRE(va.queuePayload, "%s: scratch allocation failed", ctx.shaderName);
    }
    AlphaArgs aa = {};
    if constexpr (Alpha) {
        // + t3 = the MaterialData buffer (required), t19 = the texture table (optional: without it a material with
        // MaterialFlag_UseAlbedoTexture draws nothing)
        trhip_buffer_t* materials = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 3);
        TRHIP_REQUIRE(materials, "%s: needs SRV t3 = the MaterialData buffer (124-byte stride): the alpha test reads m_ConstAlbedo.w, m_AlphaCutoff and the albedo texture",
                      ctx.shaderName);
        aa.materials = (const char*)materials->ptr;
        aa.numMaterials = elements32(materials, sizeof(MaterialData));
        if (trhip_texture_table_t* table = ctx.textureTable(19)) {
            for (size_t d = 0; d < table->slots.size(); ++d)
                TRHIP_REQUIRE(!table->slots[d] || !table->slots[d]->isUAV, "%s: the texture table at t19 holds '%s' at index %zu, created with the UAV or render-target bit: a sampled texture is read only",
                              ctx.shaderName, table->slots[d]->name.c_str(), d);
            TRHIP_REQUIRE(table->entries.ptr, "%s: the texture table at t19 has no device data", ctx.shaderName);
            aa.table = (const mtex::TableEntry*)table->entries.ptr;
            aa.tableCount = (uint32_t)table->slots.size();
        }
        aa.queueAlpha = (AlphaTriangle*)ctx.scratch((size_t)kQueueCapacity * sizeof(AlphaTriangle));
        TRHIP_REQUIRE(aa.queueAlpha, "%s: scratch allocation failed", ctx.shaderName);
    }
    a.binsX = (a.width + (1u << kBinShift) - 1u) >> kBinShift;
    a.binsY = (a.height + (1u << kBinShift) - 1u) >> kBinShift;
    const uint32_t bins = a.binsX * a.binsY;
    a.binCount = (uint32_t*)ctx.scratch((size_t)bins * 4);
    a.binList = (uint32_t*)ctx.scratch((size_t)bins * kBinCapacity * 4);
    TRHIP_REQUIRE(a.binCount && a.binList, "%s: scratch allocation failed", ctx.shaderName);
    int rc = ctx.cl->recordClearWords(a.queueCount, 4, 0, true);
    if (rc == TRHIP_OK) rc = ctx.cl->recordClearWords(a.binCount, bins, 0, true);
    if (rc != TRHIP_OK) return rc;
    const uint32_t grid = ctx.computeUnits() * 4u;
    const uint32_t tiles = ((a.width + kTile - 1) / kTile) * ((a.height + kTile - 1) / kTile);
    const uint32_t tileGrid = tiles < ctx.computeUnits() * 8u ? tiles : ctx.computeUnits() * 8u;
    if constexpr (Vis && Alpha) {
        ctx.emit("main", [a, va, aa, grid](hipStream_t s) {
            TRHIP_LAUNCH(rasterVisibilityAlphaKernel, dim3(grid), dim3(kBlock), 0, s, a, va, aa);
            return trhip::launchStatus("rasterVisibilityAlphaKernel"); });
        ctx.emit("tiles", [a, va, aa, tileGrid](hipStream_t s) {
            TRHIP_LAUNCH(rasterVisibilityTilesAlphaKernel, dim3(tileGrid), dim3(kBlock), 0, s, a, va, aa);
            return trhip::launchStatus("rasterVisibilityTilesAlphaKernel"); });
    } else if constexpr (Alpha) {
        ctx.emit("main", [a, aa, grid](hipStream_t s) {
            TRHIP_LAUNCH(rasterDepthAlphaKernel, dim3(grid), dim3(kBlock), 0, s, a, aa);
            return trhip::launchStatus("rasterDepthAlphaKernel"); });
        ctx.emit("tiles", [a, aa, tileGrid](hipStream_t s) {
            TRHIP_LAUNCH(rasterTilesAlphaKernel, dim3(tileGrid), dim3(kBlock), 0, s, a, aa);
            return trhip::launchStatus("rasterTilesAlphaKernel"); });
    } else if constexpr (Vis) {
        ctx.emit("main", [a, va, grid](hipStream_t s) {
            TRHIP_LAUNCH(rasterVisibilityKernel, dim3(grid), dim3(kBlock), 0, s, a, va);
            return trhip::launchStatus("rasterVisibilityKernel"); });
        ctx.emit("tiles", [a, va, tileGrid](hipStream_t s) {
            TRHIP_LAUNCH(rasterVisibilityTilesKernel, dim3(tileGrid), dim3(kBlock), 0, s, a, va);
            return trhip::launchStatus("rasterVisibilityTilesKernel"); });
    } else {
        ctx.emit("main", [a, grid](hipStream_t s) {
            TRHIP_LAUNCH(rasterDepthKernel, dim3(grid), dim3(kBlock), 0, s, a);
            return trhip::launchStatus("rasterDepthKernel"); });
        ctx.emit("tiles", [a, tileGrid](hipStream_t s) {
            TRHIP_LAUNCH(rasterTilesKernel, dim3(tileGrid), dim3(kBlock), 0, s, a);
            return trhip::launchStatus("rasterTilesKernel"); });
    }
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("basepass_MS_Main_depth", recordRaster<false, false>, 0);
trhip::ShaderRegistrar r1("basepass_MS_Main_visibility", recordRaster<true, false>, 0);
trhip::ShaderRegistrar r2("basepass_MS_Main_depth ALPHA_MASK_MODE=1", recordRaster<false, true>, 0);
trhip::ShaderRegistrar r3("basepass_MS_Main_visibility ALPHA_MASK_MODE=1", recordRaster<true, true>, 0);

} // namespace
