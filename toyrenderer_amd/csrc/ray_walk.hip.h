// ray_walk.hip.h -- what the passes that trace rays through the project's acceleration structure (include/trhip.h, "acceleration
// structure") share: the scene's pointers, the ray, the box test and the watertight triangle test of the sun's
// any-hit walk (k_shadowmask.hip, which states their convention and keeps occluded()), and closestHit(), the walk of the probe
// trace (k_giprobetrace.hip).  tests/shadowmask_ref.c and tests/ddgi_update_ref.c restate the functions word for word.
//
// closestHit (tests/ddgi_update_ref.c: closest_walk).  The same stackless skip-link walk as occluded(): `hit an inner box -> i + 1,
// else -> skip`, a link that does not move forward ends the walk, every index is checked before it is followed, no per-lane
// array.  EVERY candidate commits: the reference traces its probe rays with RAY_FLAG_FORCE_OPAQUE, so no alpha test is applied and
// a ForceNonOpaque instance is hit like an opaque one; TLAS instances with flags == 0 are skipped, as in occluded().
//   result    (instance, the MESH's triangle number -- not the triOrder slot --, t, b1, b2, front);
//   winner    the smallest t with tmin < t < tmax; on equal t the lower instance index, then the lower triangle number.  With
//             this rule the answer does not depend on the order in which the tree offers the candidates, so it equals brute
//             force over every triangle as long as boxHit never rejects a box whose triangle triHit accepts
//             (tests/test_ddgi_update_ref.py walks the same arrays on the CPU and allows no difference);
//   front     decided in OBJECT space, as DXR decides it (the instance's transform never flips it): front iff the watertight
//             test's det = (U + V) + W is > 0.  The ray is moved to object space by the refit's object-from-world rows, so a
//             mirrored instance mirrors the ray with the triangle and the sign is the one the mesh's own winding gives.  The
//             sign is chosen so that the Cornell fixture's walls, seen from inside the box, are front faces;
//   NO PRUNING against the best t so far: boxHit is the any-hit walk's, unchanged, and returns no entry distance.  The walk
//             therefore visits every box that the ray's line touches, like an unoccluded sun ray.  Untuned: correctness came first.
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

// ---- the two tests (tests/shadowmask_ref.c: make_ray, sm_box_hit, sm_tri_hit) ---------------------------------------------------
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

// b1, b2 (TEXTURED only): the edge values of the second and third vertex over det, InterpolateVertex's barycentrics
__device__ __forceinline__ bool triHit(F3 v0, F3 v1, F3 v2, const Ray& r, float tmin, float tmax, float* b1 = nullptr, float* b2 = nullptr)
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
    const float t = cm::div_(T, det);
    if (b1) { *b1 = cm::div_(V, det); *b2 = cm::div_(W, det); }
    return t > tmin && t < tmax;
}

template <typename Args>
__device__ __forceinline__ F3 vertexOf(const Args& a, uint64_t i)
{
    const float* p = reinterpret_cast<const float*>(a.vertices + i * sizeof(interop::RawVertexFormat));
    return { p[0], p[1], p[2] };
}

// ---- the closest hit -------------------------------------------------------------------------------------------------------------
struct Hit
{
    uint32_t inst, tri;                        // the instance and the mesh's triangle number; inst == 0xFFFFFFFF: a miss
    float t, b1, b2;
    uint32_t front;
};

// triHit with what the closest hit keeps: the same operations in the same order, t and the sign of det handed out.
__device__ __forceinline__ bool triHitClosest(F3 v0, F3 v1, F3 v2, const Ray& r, float tmin, float tmax, float& t, float& b1, float& b2, uint32_t& front)
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
    t = cm::div_(T, det);
    b1 = cm::div_(V, det); b2 = cm::div_(W, det);
    front = det > 0.0f ? 1u : 0u;
    return t > tmin && t < tmax;
}

template <typename Args>
__device__ Hit closestHit(const Args& a, F3 o, F3 d, float tmin, float tmax)
{
    Hit best = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0.0f, 0.0f, 0.0f, 0u };
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
                                for (uint32_t j = 0; j < cnt; ++j) {
                                    const uint64_t slot = (uint64_t)hd.tri_offset + first + j;
                                    if (first + j >= hd.num_tris || slot >= a.numTriOrder) break;
                                    const uint32_t tri = a.triOrder[slot];
                                    const uint64_t base = (uint64_t)md->m_GlobalIndexBufferIdx + 3ull * tri;
                                    if (base + 3u > a.numIndices) continue;
                                    const uint64_t i0 = (uint64_t)md->m_GlobalVertexBufferIdx + a.indices[base], i1 = (uint64_t)md->m_GlobalVertexBufferIdx + a.indices[base + 1],
                                                   i2 = (uint64_t)md->m_GlobalVertexBufferIdx + a.indices[base + 2];
                                    if (i0 >= a.numVertices || i1 >= a.numVertices || i2 >= a.numVertices) continue;
                                    float t, b1, b2;
                                    uint32_t front;
                                    if (!triHitClosest(vertexOf(a, i0), vertexOf(a, i1), vertexOf(a, i2), r, tmin, tmax, t, b1, b2, front)) continue;
                                    const bool first_ = best.inst == 0xFFFFFFFFu;
                                    if (first_ || t < best.t || (t == best.t && (inst < best.inst || (inst == best.inst && tri < best.tri))))
                                        best = { inst, tri, t, b1, b2, front };
                                }
                            }
                        }
                        b = bnext;
                    }
                }
            }
        }
        node = next;
    }
    return best;
}

} // namespace rw
