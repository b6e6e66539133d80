// k_giprobedraw.hip -- the DDGI probe visualisation behind its cull (k_giprobe.hip): "giprobevisualization_CS_LoadGIProbes", the
// project's own pass that hands the cull the probes of the LIVE volume, and "giprobevisualization_PS_VisualizeGIProbes", the draw of
// GIDebugRenderer::RenderDDGIDebug (source/GIRenderer.cpp:737-808; source/shaders/giprobevisualization.hlsl:71-142): every probe the
// cull kept as a small sphere shaded with that probe's own irradiance, depth-tested against the scene, into the back buffer.  The
// vertex shader is part of the name, as "basepass_MS_Main_*" stands for mesh shader plus rasteriser.  tests/ddgi_probe_draw_ref.c is
// the definition of both and the functions below repeat it word for word.
//
// ---- giprobevisualization_CS_LoadGIProbes ---------------------------------------------------------------------------------------
// The reference does this inline in the cull through SDK functions (DDGILoadProbeState, DDGIGetProbeWorldPosition); here it is a
// pass in front of the cull, whose t10 / t11 take what it writes exactly as they take host-supplied buffers.
//   b0 the 64-byte DDGIVolumeDesc (the host copy the checks below rest on), t0 the same descriptor on the device, t1 the RGBA16_FLOAT
//   array of probe data, u0 positions (float3 per probe), u1 states (one float per probe); a direct dispatch of
//   ceil(numProbes / kNumThreadsPerWave) groups.  A probe count larger than either output is refused.
//   Probe p = y * cx * cz + x + cx * z (ddgiu::probeCoords); position = ddgiu::probePosition, the query's probePos; state = data.w when
//   flags bit 1 (classification) is set, else 0.0f (active): as the query honours the flag.  ddgi.Volume.probe_positions_and_states()
//   returns data.w whatever the flag says; it stays as it is, and the two differ exactly for a volume with classification off.
//
// ---- giprobevisualization_PS_VisualizeGIProbes ----------------------------------------------------------------------------------
// BINDINGS.  GIRenderer.cpp:754-765 where the reference has them: b0 GIProbeVisualizationConsts (96 bytes) and the descriptor's host
// copy behind it (160 bytes together); t0 the culled positions; t1 / t2 / t3 the probe data / irradiance / distance arrays (the distance
// is bound as the reference binds it and not read); t4 the descriptor; t5 instance -> probe index.  The project's own (include/trhip.h):
// t6 the DrawIndexedIndirectArguments, of which m_InstanceCount is read on the device and clamped to the capacities of t0 and t5 (and
// to 2^24) and m_IndexCount is not read; t7 the unit sphere's vertices (UncompressedRawVertexFormat, at most 128), t8 its indices
// (uint32, at most 256 triangles); Texture_UAV u0 the R32_FLOAT depth buffer, read and written; u1 the RGBA8_UNORM back buffer, of the
// depth buffer's size; optional u2 an RG32_UINT texture of that size that then holds the winner words (tests read them; without it
// they live in the command list's scratch).  Any direct dispatch; the launches size themselves.
//
// RULES (this build's convention, like the rest of the rasteriser; binary32, no contraction, fma only where written).
//   vertex    world = probePos + (radius * normal), product rounded, then the sum, probePos = t0[instance] (VS_VisualizeGIProbes; the
//             position attribute is unused, as in the reference); to the screen with mesh::worldToScreen, toScreen behind its world
//             transform: sx = fma(x / w, W / 2, W / 2), sy = fma(-(y / w), H / 2, H / 2), depth = z / w;
//   triangle  (v0, v1, v2) = three consecutive indices.  Dropped if any vertex has w <= near (no clipping, as in k_raster.hip) or an
//             index is past the vertices.  area = edgeFn(v0, v1, v2) on the screen; the OUTWARD faces of the reversed-winding sphere
//             have area < 0 under a projection that does not mirror, and those are the front faces: a triangle is drawn iff
//             area < 0 (CullBackFace); area == 0 and NaN draw nothing;
//   coverage  pixel-centre samples, e_i = -edgeFn(...) >= 0 on all three edges, den = (e0 + e1) + e2 > 0, depth d =
//             fma(e2, d2, fma(e1, d1, e0 * d0)) / den: mesh::coverBox, the rasters' arithmetic;
//   depth     GREATER_OR_EQUAL on reversed Z (DepthWriteStencilNone): a sample survives iff d > 0 and d >= the depth buffer's texel
//             (a NaN on either side fails).  Among the surviving samples of one texel the largest
//             (depthBits << 32) | instance << 8 | triangle wins: draw order under GREATER_OR_EQUAL (on equal depth the later
//             instance, then the later triangle), and a maximum, so independent of the order the atomics resolve in;
//   shade     (PS_VisualizeGIProbes) at the winning sample: q_i = e_i / w_i, s = (q0 + q1) + q2; world = fma(q2, world2, fma(q1, world1,
//             q0 * world0)) / s per component; probe = min(t5[instance], numProbes - 1) (DDGIGetScrollingProbeIndex is the identity:
//             scrolling is not built); probePosition = ddgiu::probePosition of that probe from the VOLUME, not t0; dir =
//             normalize(world - probePosition); e = ddgi::irradianceTap(probe, oct(dir)).channel(., gamma * 0.5f), the query's tap;
//             c = ((e * e) * 2.0f) * 1.0989f; the back buffer takes uint(saturate(c) * 255 + 0.5) per channel and alpha 255, as
//             k_postprocess.hip stores it; the depth buffer takes d.  Texels no sphere wins keep their colour and their depth.
//
// KERNELS.  Two launches over W * H 64-bit winner words, cleared in front of them: the visibility buffer and its resolve.
//   "main"    a workgroup of 256 per visible instance (grid-stride over the device's count): threads transform the vertices into
//             LDS, set the triangles up and compact the front-facing ones into LDS; each wave then takes every fourth of them and
//             strides its 64 lanes over the triangle's clipped screen box; a surviving sample does one 64-bit atomic max.  No size
//             switch: a sphere of one pixel and one that fills the screen take the same path, the second slowly.  UNTUNED.
//   "resolve" one thread per texel; a texel with a winner recomputes that triangle's three vertices with the functions "main" used
//             (bit for bit the same screen positions), shades and writes colour and depth.  "main" only reads the depth buffer and
//             "resolve" only writes its own texel: the launch order is the only synchronisation, and nothing spins.
// Code objects (-Rpass-analysis=kernel-resource-usage; VGPRs / SGPRs / LDS bytes / waves per SIMD): loadGIProbesKernel 12 / 30 / 0 / 8,
// probeDrawMainKernel 64 / 54 / 14340 / 8, probeDrawResolveKernel 36 / 54 / 0 / 8; no scratch and no spill in any.
#include "ddgi_update.hip.h"
#include "mesh_stage.hip.h"

namespace
{

using namespace interop;
using cm::F3;

constexpr uint32_t kWave = 64, kBlock = 256, kWaves = kBlock / kWave;
constexpr uint32_t kMaxVertices = 128, kMaxTriangles = 256;      // a triangle index has 8 bits of the winner word
constexpr uint32_t kTriangleBits = 8, kMaxInstances = 1u << 24;
constexpr float kFrontSign = -1.0f;                              // front faces: edgeFn(v0, v1, v2) < 0

// ---- LoadGIProbes -------------------------------------------------------------------------------------------------------------
struct LoadArgs
{
    DDGIVolumeDesc D;
    const uint2* data; uint32_t dataW, dataPitch;      // t1
    float* positions;                                  // u0
    float* states;                                     // u1
    uint32_t numProbes;
};

__global__ __launch_bounds__(kWave) void loadGIProbesKernel(LoadArgs a)
{
    const uint32_t probe = blockIdx.x * kWave + threadIdx.x;
    if (probe >= a.numProbes) return;
    const ddgiu::I3 c = ddgiu::probeCoords(probe, a.D);
    const uint2 data = a.data[(uint64_t)c.y * a.dataPitch + (uint32_t)c.z * a.dataW + (uint32_t)c.x];
    const F3 p = ddgiu::probePosition(a.D, c, data);
    a.positions[3u * probe] = p.x; a.positions[3u * probe + 1u] = p.y; a.positions[3u * probe + 2u] = p.z;
    a.states[probe] = (a.D.flags & kDDGIFlag_Classification) ? (float)sp::halfOf(data.y >> 16) : 0.0f;
}

// b0-resident host copy of the descriptor at byte `offset`, checked
int requireDescAt(const trhip::DispatchCtx& ctx, size_t offset, const char* what, DDGIVolumeDesc& D)
{
    const void* block = ctx.constants(0, offset + sizeof(DDGIVolumeDesc));
    TRHIP_REQUIRE(block, "%s: constant buffer b0 (%s) missing or short", ctx.shaderName, what);
    memcpy(&D, (const char*)block + offset, sizeof D);
    return ddgiu::requireDesc(ctx.shaderName, D);
}

int recordLoadGIProbes(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    LoadArgs a = sp::zeroed<LoadArgs>();
    if (const int rc = requireDescAt(ctx, 0, "the 64-byte DDGIVolumeDesc", a.D)) return rc;
    const uint32_t probes = a.numProbes = ddgiu::numProbes(a.D);
    if (const int rc = ddgiu::requireLinearDispatch(ctx, probes, kNumThreadsPerWave, "ceil(numProbes / 32)")) return rc;
    trhip_buffer_t* descBuffer = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 0);
    TRHIP_REQUIRE(descBuffer && descBuffer->byteSize >= sizeof(DDGIVolumeDesc), "%s: needs StructuredBuffer_SRV t0 = the 64-byte DDGIVolumeDesc", name);
    trhip_texture_t* data;
    if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_SRV, 1, TRHIP_FORMAT_RGBA16_FLOAT, 1, "Texture_SRV t1 = the RGBA16_FLOAT array of probe data", a.D, data)) return rc;
    trhip_buffer_t* positions = ctx.buffer(TRHIP_BIND_STRUCTURED_UAV, 0);
    trhip_buffer_t* states = ctx.buffer(TRHIP_BIND_STRUCTURED_UAV, 1);
    TRHIP_REQUIRE(positions && states, "%s: needs StructuredBuffer_UAV u0 = the probe positions (float3 per probe) and u1 = the probe states (one float per probe)", name);
    TRHIP_REQUIRE((uint64_t)probes * 12 <= positions->byteSize && (uint64_t)probes * 4 <= states->byteSize,
                  "%s: %u probes need %llu bytes at u0 and %llu at u1; they hold %llu and %llu", name, probes, (unsigned long long)probes * 12, (unsigned long long)probes * 4,
                  (unsigned long long)positions->byteSize, (unsigned long long)states->byteSize);
    a.data = (const uint2*)data->ptr; a.dataW = data->width; a.dataPitch = (uint32_t)(data->slicePitch / data->texelBytes);
    a.positions = (float*)positions->ptr; a.states = (float*)states->ptr;
    sp::launch(ctx, loadGIProbesKernel, "loadGIProbesKernel", dim3((probes + kWave - 1) / kWave), dim3(kWave), a);
    return TRHIP_OK;
}

// ---- the draw ---------------------------------------------------------------------------------------------------------------------
struct DrawArgs
{
    GIProbeVisualizationConsts k;
    DDGIVolumeDesc D;
    const float* positions; uint32_t positionCapacity;                   // t0
    const uint32_t* instanceToProbe; uint32_t indexCapacity;             // t5
    const uint32_t* drawArgs;                                            // t6
    const UncompressedRawVertexFormat* vertices; uint32_t numVertices;   // t7
    const uint32_t* indices; uint32_t numTriangles;                      // t8
    ddgi::Textures tex;                                                  // t1, t2 (the distance array is not read)
    float* depth;                                                        // u0
    uint32_t* color;                                                     // u1
    uint32_t width, height, numProbes;
    unsigned long long* winners;                                         // W * H words, zero in front of "main"
};

__device__ __forceinline__ uint32_t instanceCount(const DrawArgs& a)
{
    uint32_t n = a.drawArgs[1];                                          // m_InstanceCount
    n = n < a.positionCapacity ? n : a.positionCapacity;
    n = n < a.indexCapacity ? n : a.indexCapacity;
    return n < kMaxInstances ? n : kMaxInstances;
}

// VS_VisualizeGIProbes: vertex v (< numVertices) of instance inst (< instanceCount)
__device__ __forceinline__ F3 sphereVertex(const DrawArgs& a, uint32_t inst, uint32_t v)
{
    const float* p = a.positions + 3ull * inst;
    const float* n = a.vertices[v].m_Normal;
    const float r = a.k.m_ProbeRadius;
    return { p[0] + (r * n[0]), p[1] + (r * n[1]), p[2] + (r * n[2]) };
}

struct SphereTriangle                                                    // 48 bytes
{
    float x0, y0, d0, x1, y1, d1, x2, y2, d2;
    uint32_t boxX, boxY;                                                 // x0 | x1 << 16, y0 | y1 << 16 (inclusive pixel bounds)
    uint32_t triangle;
};

__global__ __launch_bounds__(kBlock) void probeDrawMainKernel(DrawArgs a)
{
    __shared__ float s_x[kMaxVertices], s_y[kMaxVertices], s_d[kMaxVertices];
    __shared__ uint32_t s_ok[kMaxVertices];
    __shared__ SphereTriangle s_tri[kMaxTriangles];
    __shared__ uint32_t s_live;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t count = instanceCount(a), W = a.width, H = a.height, nv = a.numVertices, nt = a.numTriangles;
    const float halfW = 0.5f * (float)W, halfH = 0.5f * (float)H;
    const cm::M43 clipXYZ = cm::loadM43(a.k.m_WorldToClip);
    for (uint32_t inst = blockIdx.x; inst < count; inst += gridDim.x) {  // uniform over the workgroup
        __syncthreads();                                                 // the last instance's triangles have been drawn
        if (tid == 0) s_live = 0u;
        if (tid < nv) {
            const mesh::ScreenVertex s = mesh::worldToScreen(sphereVertex(a, inst, tid), clipXYZ, a.k.m_WorldToClip, halfW, halfH);
            s_x[tid] = s.sx; s_y[tid] = s.sy; s_d[tid] = s.depth;
            s_ok[tid] = s.w > a.k.m_NearPlane ? 1u : 0u;
        }
        __syncthreads();
        if (tid < nt) {
            const uint32_t ia = a.indices[3u * tid], ib = a.indices[3u * tid + 1u], ic = a.indices[3u * tid + 2u];
            if (ia < nv && ib < nv && ic < nv && s_ok[ia] && s_ok[ib] && s_ok[ic]) {
                SphereTriangle q = { s_x[ia], s_y[ia], s_d[ia], s_x[ib], s_y[ib], s_d[ib], s_x[ic], s_y[ic], s_d[ic], 0u, 0u, tid };
                const float area = mesh::edgeFn(q.x0, q.y0, q.x1, q.y1, q.x2, q.y2);
                const float fminx = cm::min_(cm::min_(q.x0, q.x1), q.x2), fmaxx = cm::max_(cm::max_(q.x0, q.x1), q.x2);
                const float fminy = cm::min_(cm::min_(q.y0, q.y1), q.y2), fmaxy = cm::max_(cm::max_(q.y0, q.y1), q.y2);
                if (area < 0.0f                                                                  // CullBackFace; not degenerate, not NaN
                    && fmaxx >= 0.0f && fmaxy >= 0.0f && fminx <= (float)W && fminy <= (float)H) {   // on screen, not NaN
                    const int bx0 = (int)cm::max_(__builtin_floorf(fminx), 0.0f), bx1 = (int)cm::min_(__builtin_ceilf(fmaxx), (float)(W - 1));
                    const int by0 = (int)cm::max_(__builtin_floorf(fminy), 0.0f), by1 = (int)cm::min_(__builtin_ceilf(fmaxy), (float)(H - 1));
                    if (bx1 >= bx0 && by1 >= by0) {
                        q.boxX = (uint32_t)bx0 | ((uint32_t)bx1 << 16); q.boxY = (uint32_t)by0 | ((uint32_t)by1 << 16);
                        s_tri[atomicAdd(&s_live, 1u)] = q;
                    }
                }
            }
        }
        __syncthreads();
        const uint32_t live = s_live;
        for (uint32_t j = wave; j < live; j += kWaves) {
            const SphereTriangle c = s_tri[j];
            const uint32_t bx0 = c.boxX & 0xFFFFu, by0 = c.boxY & 0xFFFFu;
            const unsigned long long payload = (unsigned long long)(inst << kTriangleBits | c.triangle);
            const float* depth = a.depth;
            unsigned long long* winners = a.winners;
            mesh::coverBox(c.x0, c.y0, c.d0, c.x1, c.y1, c.d1, c.x2, c.y2, c.d2, kFrontSign, bx0, by0, (c.boxX >> 16) - bx0 + 1u, (c.boxY >> 16) - by0 + 1u, lane, kWave,
                           [](float, float, float, float, float) { return true; },
                           [=](uint32_t px, uint32_t py, uint32_t bits) {
                               const uint64_t i = (uint64_t)py * W + px;
                               if (__uint_as_float(bits) >= depth[i]) atomicMax(&winners[i], (unsigned long long)bits << 32 | payload); });   // GREATER_OR_EQUAL
        }
    }
}

__device__ __forceinline__ uint32_t unorm8(float c) { return (uint32_t)(sp::saturate_(c) * 255.0f + 0.5f); }   // k_postprocess.hip's store

__global__ __launch_bounds__(sp::kBlock) void probeDrawResolveKernel(DrawArgs a)
{
    const sp::Pixel at = sp::pixel();
    if (!at.inside(a.width, a.height)) return;
    const uint64_t i = at.index(a.width);
    const unsigned long long word = a.winners[i];
    if (word == 0ull) return;                                            // depth > 0 on every written sample
    const uint32_t payload = (uint32_t)word, inst = payload >> kTriangleBits, tri = payload & (kMaxTriangles - 1u);
    // the winner, with the functions "main" used: in range, or "main" would not have written it
    const uint32_t ia = a.indices[3u * tri], ib = a.indices[3u * tri + 1u], ic = a.indices[3u * tri + 2u];
    const float halfW = 0.5f * (float)a.width, halfH = 0.5f * (float)a.height;
    const cm::M43 clipXYZ = cm::loadM43(a.k.m_WorldToClip);
    const F3 w0 = sphereVertex(a, inst, ia), w1 = sphereVertex(a, inst, ib), w2 = sphereVertex(a, inst, ic);
    const mesh::ScreenVertex s0 = mesh::worldToScreen(w0, clipXYZ, a.k.m_WorldToClip, halfW, halfH), s1 = mesh::worldToScreen(w1, clipXYZ, a.k.m_WorldToClip, halfW, halfH),
                             s2 = mesh::worldToScreen(w2, clipXYZ, a.k.m_WorldToClip, halfW, halfH);
    const float cx = (float)at.x + 0.5f, cy = (float)at.y + 0.5f;
    const float e0 = kFrontSign * mesh::edgeFn(s1.sx, s1.sy, s2.sx, s2.sy, cx, cy), e1 = kFrontSign * mesh::edgeFn(s2.sx, s2.sy, s0.sx, s0.sy, cx, cy),
                e2 = kFrontSign * mesh::edgeFn(s0.sx, s0.sy, s1.sx, s1.sy, cx, cy);
    const float q0 = e0 / s0.w, q1 = e1 / s1.w, q2 = e2 / s2.w;
    const float s = (q0 + q1) + q2;
    const F3 world = { cm::fma_(q2, w2.x, cm::fma_(q1, w1.x, q0 * w0.x)) / s, cm::fma_(q2, w2.y, cm::fma_(q1, w1.y, q0 * w0.y)) / s,
                       cm::fma_(q2, w2.z, cm::fma_(q1, w1.z, q0 * w0.z)) / s };
    // PS_VisualizeGIProbes
    const DDGIVolumeDesc& D = a.D;
    const uint32_t last = a.numProbes - 1u, listed = a.instanceToProbe[inst];
    const ddgiu::I3 c = ddgiu::probeCoords(listed < last ? listed : last, D);
    const uint2 data = a.tex.data[(uint64_t)c.y * a.tex.dataPitch + (uint32_t)c.z * a.tex.dataW + (uint32_t)c.x];
    const F3 dir = ddgi::normalize(ddgi::sub(world, ddgiu::probePosition(D, c, data)));
    float u, v;
    ddgi::oct(dir, u, v);
    const ddgi::IrradianceTap tap = ddgi::irradianceTap(a.tex, c.x, c.z, ddgi::sliceOf(c.y, a.tex.slices), u, v);
    const float halfGamma = D.probeIrradianceEncodingGamma * 0.5f;
    const F3 e = { tap.channel(0u, halfGamma), tap.channel(10u, halfGamma), tap.channel(20u, halfGamma) };
    const F3 rgb = { ((e.x * e.x) * 2.0f) * 1.0989f, ((e.y * e.y) * 2.0f) * 1.0989f, ((e.z * e.z) * 2.0f) * 1.0989f };
    a.color[i] = unorm8(rgb.x) | unorm8(rgb.y) << 8 | unorm8(rgb.z) << 16 | 0xFF000000u;
    a.depth[i] = __uint_as_float((uint32_t)(word >> 32));
}

int recordProbeDraw(trhip::DispatchCtx& ctx)
{
    const char* name = ctx.shaderName;
    DrawArgs a = sp::zeroed<DrawArgs>();
    const void* block = ctx.constants(0, sizeof(GIProbeVisualizationConsts) + sizeof(DDGIVolumeDesc));
    TRHIP_REQUIRE(block, "%s: constant buffer b0 (the 96-byte GIProbeVisualizationConsts and the 64-byte DDGIVolumeDesc behind it, 160 bytes) missing or short", name);
    memcpy(&a.k, block, sizeof a.k);
    if (const int rc = requireDescAt(ctx, sizeof(GIProbeVisualizationConsts), "the 96-byte GIProbeVisualizationConsts and the 64-byte DDGIVolumeDesc behind it, 160 bytes", a.D)) return rc;
    const DDGIVolumeDesc& D = a.D;
    TRHIP_REQUIRE(!ctx.indirect, "%s: needs a direct dispatch (the launches size themselves)", name);
    trhip_buffer_t* positions = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 0);
    trhip_buffer_t* descBuffer = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 4);
    trhip_buffer_t* toProbe = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 5);
    trhip_buffer_t* drawArgs = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 6);
    trhip_buffer_t* vertices = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 7);
    trhip_buffer_t* indices = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, 8);
    TRHIP_REQUIRE(positions && toProbe, "%s: needs StructuredBuffer_SRV t0 = the culled probe positions (float3) and t5 = instance -> probe index", name);
    TRHIP_REQUIRE(descBuffer && descBuffer->byteSize >= sizeof(DDGIVolumeDesc), "%s: needs StructuredBuffer_SRV t4 = the 64-byte DDGIVolumeDesc", name);
    TRHIP_REQUIRE(drawArgs && drawArgs->byteSize >= sizeof(DrawIndexedIndirectArguments), "%s: needs StructuredBuffer_SRV t6 = the DrawIndexedIndirectArguments (20 bytes)", name);
    TRHIP_REQUIRE(vertices && indices, "%s: needs StructuredBuffer_SRV t7 = the unit sphere's vertices (UncompressedRawVertexFormat) and t8 = its indices (uint32)", name);
    const uint64_t nv = vertices->byteSize / sizeof(UncompressedRawVertexFormat), ni = indices->byteSize / 4;
    TRHIP_REQUIRE(nv >= 1 && nv <= kMaxVertices && vertices->byteSize % sizeof(UncompressedRawVertexFormat) == 0, "%s: t7 holds %llu bytes; the sphere has 1..%u vertices of 32 bytes", name,
                  (unsigned long long)vertices->byteSize, kMaxVertices);
    TRHIP_REQUIRE(ni >= 3 && ni % 3 == 0 && ni / 3 <= kMaxTriangles && indices->byteSize % 4 == 0, "%s: t8 holds %llu bytes; the sphere has 1..%u triangles of three uint32", name,
                  (unsigned long long)indices->byteSize, kMaxTriangles);
    trhip_texture_t *data, *irr, *dist;
    if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_SRV, 1, TRHIP_FORMAT_RGBA16_FLOAT, 1, "Texture_SRV t1 = the RGBA16_FLOAT array of probe data", D, data)) return rc;
    if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_SRV, 2, TRHIP_FORMAT_R10G10B10A2_UNORM, kDDGIIrradianceInteriorTexels + 2,
                                                  "Texture_SRV t2 = the R10G10B10A2_UNORM array of probe irradiance", D, irr)) return rc;
    if (const int rc = ddgiu::requireProbeTexture(ctx, TRHIP_BIND_TEXTURE_SRV, 3, TRHIP_FORMAT_RG16_FLOAT, kDDGIDistanceInteriorTexels + 2,
                                                  "Texture_SRV t3 = the RG16_FLOAT array of probe distances", D, dist)) return rc;
    const sp::Binding want[] = { { TRHIP_BIND_TEXTURE_UAV, 0, TRHIP_FORMAT_R32_FLOAT, "Texture_UAV u0 = the R32_FLOAT depth buffer, mip 0", true, sp::kOneMipOrAt0 },
                                 { TRHIP_BIND_TEXTURE_UAV, 1, TRHIP_FORMAT_RGBA8_UNORM, "Texture_UAV u1 = the RGBA8_UNORM back buffer", true, sp::kOneMip },
                                 { TRHIP_BIND_TEXTURE_UAV, 2, TRHIP_FORMAT_RG32_UINT, "Texture_UAV u2 = the RG32_UINT winner words", false, sp::kOneMip } };
    trhip_texture_t* target[3];
    if (const int rc = sp::bindTextures(ctx, want, target)) return rc;
    const uint32_t W = target[0]->width, H = target[0]->height;
    TRHIP_REQUIRE(target[1]->width == W && target[1]->height == H, "%s: the back buffer at u1 is %ux%u, the depth buffer at u0 is %ux%u", name, target[1]->width, target[1]->height, W, H);
    TRHIP_REQUIRE(!target[2] || (target[2]->width == W && target[2]->height == H), "%s: the winner words at u2 are %ux%u, the depth buffer at u0 is %ux%u", name,
                  target[2] ? target[2]->width : 0u, target[2] ? target[2]->height : 0u, W, H);
    TRHIP_REQUIRE(W >= 1 && H >= 1 && W <= 65535 && H <= 65535, "%s: the depth buffer is %ux%u; a screen box has 16 bits per bound", name, W, H);
    a.positions = (const float*)positions->ptr; a.positionCapacity = mesh::elements32(positions, 12);
    a.instanceToProbe = (const uint32_t*)toProbe->ptr; a.indexCapacity = mesh::elements32(toProbe, 4);
    a.drawArgs = (const uint32_t*)drawArgs->ptr;
    a.vertices = (const UncompressedRawVertexFormat*)vertices->ptr; a.numVertices = (uint32_t)nv;
    a.indices = (const uint32_t*)indices->ptr; a.numTriangles = (uint32_t)(ni / 3);
    a.tex.data = (const uint2*)data->ptr; a.tex.dataW = data->width; a.tex.dataH = data->height; a.tex.dataPitch = (uint32_t)(data->slicePitch / data->texelBytes);
    a.tex.irradiance = (const uint32_t*)irr->ptr; a.tex.irrW = irr->width; a.tex.irrH = irr->height; a.tex.irrPitch = (uint32_t)(irr->slicePitch / irr->texelBytes);
    a.tex.slices = irr->arraySize;
    a.depth = (float*)target[0]->ptr; a.color = (uint32_t*)target[1]->ptr; a.width = W; a.height = H; a.numProbes = ddgiu::numProbes(D);
    const uint64_t words = (uint64_t)W * H * 2;
    if (target[2]) {
        a.winners = (unsigned long long*)target[2]->ptr;
        if (const int rc = ctx.cl->recordClearWords(a.winners, words, 0)) return rc;
    } else {
        a.winners = (unsigned long long*)ctx.scratch(words * 4);
        TRHIP_REQUIRE(a.winners, "%s: scratch allocation failed", name);
        if (const int rc = ctx.cl->recordClearWords(a.winners, words, 0, true)) return rc;
    }
    const uint32_t capacity = std::min(std::min(a.positionCapacity, a.indexCapacity), kMaxInstances);
    if (capacity == 0) return TRHIP_OK;
    const uint32_t grid = std::min(capacity, ctx.computeUnits() * 8u);
    sp::launch(ctx, probeDrawMainKernel, "probeDrawMainKernel", dim3(grid), dim3(kBlock), a, "main");
    sp::launch(ctx, probeDrawResolveKernel, "probeDrawResolveKernel", sp::tiles(W, H), dim3(sp::kTileW, sp::kTileH), a, "resolve");
    return TRHIP_OK;
}

trhip::ShaderRegistrar r0("giprobevisualization_CS_LoadGIProbes", recordLoadGIProbes, 0);
trhip::ShaderRegistrar r1("giprobevisualization_PS_VisualizeGIProbes", recordProbeDraw, 0);

} // namespace
