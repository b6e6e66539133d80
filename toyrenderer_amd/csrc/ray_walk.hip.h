// ray_walk.hip.h -- the ONE statement on the device of how a ray goes through the project's acceleration structure (include/trhip.h,
// "acceleration structure"): the scene's pointers and their binding, the ray, the box test, the watertight triangle
// test, the bounds-checked triangle fetch and walk(), the stackless two-level skip-link walk.  The sun's any-hit rays
// (k_shadowmask.hip: occluded(), which needs the material textures) are one visitor of that walk, closestHit() below (the probe
// trace, its shadow ray and the placement's fixed rays: k_giprobetrace.hip, k_giprobeplacement.hip) is another, and the sun's
// penumbra rays (k_shadowmask.hip: closestCommit(), the smallest t among the candidates that pass the alpha test) are the third.
// tests/shadowmask_ref.c holds the same pieces once in C (sm_walk, tri_candidate, fetch_tri) and is the definition;
// k_shadowmask.hip states the arithmetic convention.
//
// walk.     The nodes are in depth-first preorder with skip links: `hit an inner box -> i + 1, else -> skip`.  No stack, no per-lane
//           array, no LDS; a link that does not move forward ends its level (a corrupt buffer cannot spin); every index is checked
//           before it is followed; a TLAS leaf whose instance has flags == 0 or a mesh past the buffer is not entered; the ray is
//           moved to object space once per instance (the refit's object-from-world rows; the direction without the translation and
//           NOT normalised, so t means the same in both spaces); a leaf holds (leaf >> 30) + 1 slots of triOrder from leaf &
//           0x3FFFFFFF on, and a slot past the mesh's num_tris or past triOrder ends the leaf.  Each remaining slot is a candidate:
//           visit(inst, flags, md, the MESH's triangle number, the object-space ray); a visitor that answers true stops the walk.
//           ONE WAY OUT of a leaf's loop: the visitor's answer goes into a flag that ends the loop, and walk() returns after it.
//           With `if (visit(...)) return true` beside the `break`, the compiler keeps the return's exit in the three loops even
//           for closestHit, whose visitor never stops, and the probe traces measured 7 to 8 % slower
//           (profiles/ray_walk/README.md).
// closestHit.  EVERY candidate commits: the reference traces its probe rays with RAY_FLAG_FORCE_OPAQUE, so no alpha test is applied
//           and a ForceNonOpaque instance is hit like an opaque one.
//   result    (instance, the MESH's triangle number -- not the triOrder slot --, t, b1, b2, front);
//   winner    the smallest t with tmin < t < tmax; on equal t the lower instance index, then the lower triangle number.  With
//             this rule the answer does not depend on the order in which the tree offers the candidates, so it equals brute
//             force over every triangle as long as boxHit never rejects a box whose triangle triTest accepts
//             (tests/test_ddgi_update_ref.py walks the same arrays on the CPU and allows no difference);
//   front     decided in OBJECT space, as DXR decides it (the instance's transform never flips it): front iff the watertight
//             test's det = (U + V) + W is > 0.  The ray is moved to object space by the refit's object-from-world rows, so a
//             mirrored instance mirrors the ray with the triangle and the sign is the one the mesh's own winding gives.  The
//             sign is chosen so that the Cornell fixture's walls, seen from inside the box, are front faces;
//   NO PRUNING against the best t so far: boxHit returns no entry distance, so the walk visits every box that the ray's line
//             touches, like an unoccluded sun ray.  Untuned: correctness came first.
#pragma once

#include "cull_math.hip.h"
#include "trhip_internal.h"

namespace rw
{

using cm::F3;

constexpr float kSlack = 0x1p-18f, kFloatMax = 3.402823466e38f;

// The scene and its acceleration structure as a tracing kernel's arguments hold them.
struct SceneArgs
{
    const interop::BasePassInstanceConstants* instances; uint32_t numInstances;
    const uint8_t* vertices; uint32_t numVertices;            // 20-byte stride
    const uint8_t* materials; uint32_t numMaterials;          // 124-byte stride
    const uint32_t* indices; uint32_t numIndices;
    const uint8_t* meshes; uint32_t numMeshes;                // 156-byte stride
    const trhip_accel_node* tlasNodes; uint32_t numTlasNodes;
    const trhip_tlas_instance* tlasInstances;
    const trhip_blas_header* headers;
    const trhip_accel_node* blasNodes; uint32_t numBlasNodes;
    const uint32_t* triOrder; uint32_t numTriOrder;
};

__device__ __forceinline__ float sel(F3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

struct M34 { float m[12]; };

__device__ __forceinline__ F3 mulPoint(F3 p, const M34& M, bool translate)
{
    const float* m = M.m;
    F3 r = { cm::fma_(p.z, m[6], cm::fma_(p.y, m[3], p.x * m[0])), cm::fma_(p.z, m[7], cm::fma_(p.y, m[4], p.x * m[1])), cm::fma_(p.z, m[8], cm::fma_(p.y, m[5], p.x * m[2])) };
    if (translate) { r.x = r.x + m[9]; r.y = r.y + m[10]; r.z = r.z + m[11]; }
    return r;
}

// ---- the ray and the two tests (tests/shadowmask_ref.c: make_ray, sm_box_hit, tri_candidate) ------------------------------------
struct Ray { F3 o, d, inv; int kx, ky, kz; float Sx, Sy, Sz; };

__device__ __forceinline__ Ray makeRay(F3 o, F3 d)
{
    Ray r;
    r.o = o; r.d = d;
    r.inv.x = cm::div_(1.0f, d.x); r.inv.y = cm::div_(1.0f, d.y); r.inv.z = cm::div_(1.0f, d.z);
    const float ax = __builtin_fabsf(d.x), ay = __builtin_fabsf(d.y), az = __builtin_fabsf(d.z);
    int kz = 0;
    float m = ax;
    if (ay > m) { kz = 1; m = ay; }
    if (az > m) { kz = 2; }
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dz = sel(d, kz);
    if (dz < 0.0f) { const int s = kx; kx = ky; ky = s; }
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.Sx = cm::div_(sel(d, kx), dz); r.Sy = cm::div_(sel(d, ky), dz); r.Sz = cm::div_(1.0f, dz);
    return r;
}

__device__ __forceinline__ bool boxHit(const trhip_accel_node& n, const Ray& r)
{
    float tenter = 0.0f, texit = __builtin_inff();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float o = sel(r.o, a), inv = sel(r.inv, a);
        if (!(__builtin_fabsf(inv) <= kFloatMax)) {
            if (!(o >= n.lo[a] && o <= n.hi[a])) return false;
        } else {
            const float t0 = (n.lo[a] - o) * inv, t1 = (n.hi[a] - o) * inv;
            float tn = cm::min_(t0, t1), tf = cm::max_(t0, t1);
            tn = tn - __builtin_fabsf(tn) * kSlack; tf = tf + __builtin_fabsf(tf) * kSlack;
            tenter = cm::max_(tenter, tn); texit = cm::min_(texit, tf);
        }
    }
    return tenter <= texit;
}

// The watertight test of Woop, Benthin and Wald (tests/shadowmask_ref.c: tri_candidate, which states it).  True iff the ray's line
// meets the triangle with det != 0 and tmin < t < tmax; b1, b2: the edge values of the second and third vertex over det,
// InterpolateVertex's barycentrics; front: det > 0.  A caller that ignores a member leaves its division dead.
struct TriHit { float t, b1, b2; bool front; };

__device__ __forceinline__ bool triTest(F3 v0, F3 v1, F3 v2, const Ray& r, float tmin, float tmax, TriHit& h)
{
    const F3 A = { v0.x - r.o.x, v0.y - r.o.y, v0.z - r.o.z }, B = { v1.x - r.o.x, v1.y - r.o.y, v1.z - r.o.z }, C = { v2.x - r.o.x, v2.y - r.o.y, v2.z - r.o.z };
    const float Akz = sel(A, r.kz), Bkz = sel(B, r.kz), Ckz = sel(C, r.kz);
    const float Ax = sel(A, r.kx) - r.Sx * Akz, Ay = sel(A, r.ky) - r.Sy * Akz;
    const float Bx = sel(B, r.kx) - r.Sx * Bkz, By = sel(B, r.ky) - r.Sy * Bkz;
    const float Cx = sel(C, r.kx) - r.Sx * Ckz, Cy = sel(C, r.ky) - r.Sy * Ckz;
    const float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return false;
    const float det = (U + V) + W;
    if (det == 0.0f) return false;
    const float Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
    const float T = (U * Az + V * Bz) + W * Cz;
    h.t = cm::div_(T, det);
    h.b1 = cm::div_(V, det); h.b2 = cm::div_(W, det);
    h.front = det > 0.0f;
    return h.t > tmin && h.t < tmax;
}

// Triangle `tri` of mesh `md`: its three vertex indices and positions; false when an index leaves its buffer.
struct Tri { uint64_t i[3]; F3 v[3]; };

template <typename Args>
__device__ __forceinline__ bool fetchTri(const Args& a, const interop::MeshData* md, uint32_t tri, Tri& out)
{
    const uint64_t base = (uint64_t)md->m_GlobalIndexBufferIdx + 3ull * tri;
    if (base + 3u > a.numIndices) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) out.i[k] = (uint64_t)md->m_GlobalVertexBufferIdx + a.indices[base + k];
    if (out.i[0] >= a.numVertices || out.i[1] >= a.numVertices || out.i[2] >= a.numVertices) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {                  // the three indices first, then the three vertices: each batch of loads is in flight together
        const float* p = reinterpret_cast<const float*>(a.vertices + out.i[k] * sizeof(interop::RawVertexFormat));
        out.v[k] = { p[0], p[1], p[2] };
    }
    return true;
}

// ---- the walk (the header states its rules) ---------------------------------------------------------------------------------------
template <typename Args, typename Visit>
__device__ __forceinline__ bool walk(const Args& a, F3 o, F3 d, Visit visit)
{
    const Ray wr = makeRay(o, d);
    uint32_t node = 0;
    while (node < a.numTlasNodes) {
        const trhip_accel_node n = a.tlasNodes[node];
        uint32_t next = n.skip > node ? n.skip : a.numTlasNodes;
        if (boxHit(n, wr)) {
            if (n.leaf == interop::kAccelInner) next = node + 1;
            else if (n.leaf < a.numInstances) {
                const uint32_t inst = n.leaf, flags = a.tlasInstances[inst].flags, mesh = a.instances[inst].m_MeshDataIdx;
                if (flags && mesh < a.numMeshes) {
                    const trhip_blas_header hd = a.headers[mesh];
                    const interop::MeshData* md = reinterpret_cast<const interop::MeshData*>(a.meshes + (uint64_t)mesh * sizeof(interop::MeshData));
                    M34 M;
#pragma unroll
                    for (int j = 0; j < 12; ++j) M.m[j] = a.tlasInstances[inst].object_from_world[j];
                    const Ray r = makeRay(mulPoint(o, M, true), mulPoint(d, M, false));
                    const uint32_t count = (uint64_t)hd.node_offset + hd.num_nodes <= a.numBlasNodes ? hd.num_nodes : 0u;
                    uint32_t b = 0;
                    while (b < count) {
                        const trhip_accel_node bn = a.blasNodes[hd.node_offset + b];
                        uint32_t bnext = bn.skip > b ? bn.skip : count;
                        if (boxHit(bn, r)) {
                            if (bn.leaf == interop::kAccelInner) bnext = b + 1;
                            else {
                                const uint32_t first = bn.leaf & 0x3FFFFFFFu, cnt = (bn.leaf >> 30) + 1u;
                                bool stop = false;     // not `if (visit(...)) return true` beside the break: see "one way out" in the header
                                for (uint32_t j = 0; j < cnt && !stop; ++j) {
                                    const uint64_t slot = (uint64_t)hd.tri_offset + first + j;
                                    if (first + j >= hd.num_tris || slot >= a.numTriOrder) break;
                                    stop = visit(inst, flags, md, a.triOrder[slot], r);
                                }
                                if (stop) return true;
                            }
                        }
                        b = bnext;
                    }
                }
            }
        }
        node = next;
    }
    return false;
}

// ---- the closest hit ---------------------------------------------------------------------------------------------------------------
struct Hit
{
    uint32_t inst, tri;                        // the instance and the mesh's triangle number; inst == 0xFFFFFFFF: a miss
    float t, b1, b2;
    uint32_t front;
};

// The closest-hit visitor of walk() (tests/ddgi_update_ref.c: closest_walk): fetch, test, tie rule; it never stops the walk.
template <typename Args>
__device__ Hit closestHit(const Args& a, F3 o, F3 d, float tmin, float tmax)
{
    Hit best = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0.0f, 0.0f, 0.0f, 0u };
    walk(a, o, d, [&](uint32_t inst, uint32_t, const interop::MeshData* md, uint32_t tri, const Ray& r) {
        Tri T;
        TriHit h;
        if (!fetchTri(a, md, tri, T) || !triTest(T.v[0], T.v[1], T.v[2], r, tmin, tmax, h)) return false;
        if (best.inst == 0xFFFFFFFFu || h.t < best.t || (h.t == best.t && (inst < best.inst || (inst == best.inst && tri < best.tri))))
            best = { inst, tri, h.t, h.b1, h.b2, h.front ? 1u : 0u };
        return false; });
    return best;
}

// ---- record side: the scene's ten buffers -------------------------------------------------------------------------------------------
// slots: the StructuredBuffer_SRV registers of the TLAS nodes, instances, vertices, materials, indices, mesh data, TLAS instances, BLAS
// headers, BLAS nodes and the triangle order, in this order.  The materials are asked for only with wantMaterials.
inline int bindScene(const trhip::DispatchCtx& ctx, const uint32_t (&slots)[10], bool wantMaterials, SceneArgs& s)
{
    struct WantBuf { uint32_t stride; const char* what; };
    const WantBuf wantBuf[10] = { { sizeof(trhip_accel_node), "the TLAS nodes" }, { sizeof(interop::BasePassInstanceConstants), "the instances" },
                                  { sizeof(interop::RawVertexFormat), "the vertices" }, { sizeof(interop::MaterialData), "the materials" }, { 4, "the indices" },
                                  { sizeof(interop::MeshData), "the mesh data" }, { sizeof(trhip_tlas_instance), "the TLAS instances" },
                                  { sizeof(trhip_blas_header), "the BLAS headers" }, { sizeof(trhip_accel_node), "the BLAS nodes" }, { 4, "the triangle order" } };
    const void* ptr[10] = {};
    uint32_t count[10] = {};
    for (int j = 0; j < 10; ++j) {
        if (j == 3 && !wantMaterials) continue;
        const trhip_buffer_t* buf = ctx.buffer(TRHIP_BIND_STRUCTURED_SRV, slots[j]);
        TRHIP_REQUIRE(buf, "%s: needs StructuredBuffer_SRV t%u = %s", ctx.shaderName, slots[j], wantBuf[j].what);
        const uint64_t n = buf->byteSize / wantBuf[j].stride;
        ptr[j] = buf->ptr;
        count[j] = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
    }
    s.tlasNodes = (const trhip_accel_node*)ptr[0]; s.numTlasNodes = count[0];
    s.instances = (const interop::BasePassInstanceConstants*)ptr[1]; s.numInstances = count[1] < count[6] ? count[1] : count[6];
    s.vertices = (const uint8_t*)ptr[2]; s.numVertices = count[2];
    s.materials = (const uint8_t*)ptr[3]; s.numMaterials = count[3];
    s.indices = (const uint32_t*)ptr[4]; s.numIndices = count[4];
    s.meshes = (const uint8_t*)ptr[5]; s.numMeshes = count[5] < count[7] ? count[5] : count[7];
    s.tlasInstances = (const trhip_tlas_instance*)ptr[6];
    s.headers = (const trhip_blas_header*)ptr[7];
    s.blasNodes = (const trhip_accel_node*)ptr[8]; s.numBlasNodes = count[8];
    s.triOrder = (const uint32_t*)ptr[9]; s.numTriOrder = count[9];
    return TRHIP_OK;
}

} // namespace rw
