/* shadowmask_ref.c -- the definition of "shadowmask_CS_ShadowMask" and "raytracing_CS_RefitTLAS" (csrc/k_shadowmask.hip) and of the
 * ray walk that every tracing pass shares (csrc/ray_walk.hip.h): the walk (sm_walk), the triangle test (tri_candidate) and the
 * triangle fetch (fetch_tri) are stated ONCE here, and tests/ddgi_update_ref.c, tests/alpha_test_ref.c and
 * tests/ddgi_placement_ref.c include this file for them.  Compile with gcc -O2 -ffp-contract=off (tests/shadowmask_ref.py).
 *
 * TWO EVALUATORS of one texel's occlusion:
 *   brute force (mode 0): every triangle of every instance's index list.  This is the definition of the mask.
 *   walk (mode 1):        the product's node arrays (include/trhip.h, "acceleration structure") with the kernel's box test.
 * Any-hit over all triangles does not depend on the order, so the two agree for any tree as long as sm_box_hit never rejects
 * a box whose triangle sm_tri_hit accepts; tests/test_shadowmask_ref.py demands zero differing texels.
 *
 * CONVENTION.  IEEE binary32, no contraction, fmaf only where written, / and sqrtf correctly rounded.
 *   worldPosition as tests/lighting_ref.c (csrc/k_deferredlighting.hip) states it; UnpackGBuffer's normal: tests/ref_formats.h unpack_oct;
 *   cross(a, b) = (fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x)));
 *   noise:    (float)byte / 255.0f of the texel's R and G bytes at (px % 128, py % 128), + m_NoisePhase, then fmod(x, 1) = x - truncf(x);
 *   MapToCone: offset = 2 * s - 1; both 0: n.  |ox| > |oy|: r = ox, theta = RN(pi / 4) * (oy / ox); else r = oy,
 *             theta = RN(pi / 2) * (1 - 0.5f * (ox / oy)); u = ((radius * r) * cosSoft(theta), (radius * r) * sinSoft(theta)) with the
 *             project's software sine and cosine (csrc/soft_math.hip.h; theta is in [-pi / 4, 3 pi / 4]); CreateTangentVectors as
 *             the HLSL; result (n + u.x * t0) + u.y * t1 per component; the ray direction is its normalize;
 *   ray:      origin = worldPosition + normal * m_RayStartOffset, TMin = m_RayStartOffset, TMax = 1e10f;
 *   instance: the object-from-world 3x4 is sm_object_from_world (cofactors / determinant, the order below); the ray is moved to
 *             object space ONCE per instance: origin by mulPoint (fma(o.z, r2, fma(o.y, r1, o.x * r0)) + r3), direction the same
 *             without r3 and NOT normalised, so t means the same in both spaces;
 *   triangle: sm_tri_hit, the watertight test of Woop, Benthin and Wald (JCGT 2013) in binary32 without its double fallback:
 *             the ray's largest axis becomes z, the vertices are sheared onto it, the three edge functions U, V, W are products
 *             of the SAME two numbers for the two triangles that share an edge (with opposite sign, exactly), so a ray cannot
 *             pass between them; hit iff not (some edge function < 0 and some > 0), det = (U + V) + W != 0 and
 *             TMin < t < TMax with t = ((U * Az + V * Bz) + W * Cz) / det.  Two-sided, no culling.  A triangle with a non-finite
 *             vertex is never hit (the builder leaves it out of the tree);
 *   alpha:    a candidate on a ForceNonOpaque instance counts iff m_ConstAlbedo.w >= m_AlphaCutoff of the CANDIDATE's instance's
 *             material (the reference reads Committed* there, shadowmask.hlsl:113-116, which is undefined before a commit);
 *   box:      sm_box_hit.  Per axis, a direction component whose reciprocal is not finite (0, -0, a subnormal) only asks
 *             lo <= origin <= hi -- no inf * 0; otherwise the slab interval, each end moved outward by 2^-18 of itself; the
 *             intervals are intersected with [0, inf).  Node boxes are already padded (include/trhip.h);
 *   output:   depth == 0.0f: u1 = 0x7BFF (65504), u0 kept.  Else u0 = occluded ? 0 : 255, u1 = binary16 round-to-nearest-even of
 *             length(worldPosition - m_CameraPosition) (overflow gives infinity, every NaN is stored as 0x7E00). */
#include "ref_formats.h"

typedef struct { float x, y, z; } F3;
typedef struct { float lo[3]; uint32_t skip; float hi[3]; uint32_t leaf; } SmNode;
typedef struct { uint32_t node_offset, num_nodes, tri_offset, num_tris; } SmHeader;
typedef struct { float m[12]; uint32_t flags, leaf_node, reserved[2]; } SmTlasInstance;
typedef struct { float world[16], prev[16]; uint32_t mesh, material; float pad[2]; } SmInstance;                 /* 144 bytes */
typedef struct { float sphere[4]; uint32_t lods[32]; uint32_t numLods, vertexBase, indexBase; } SmMesh;         /* 156 bytes */
typedef struct { float albedo[4], emissive[3], alphaCutoff; uint32_t rest[23]; } SmMaterial;                    /* 124 bytes */
typedef struct
{
    float clipToWorld[16], light[3], noisePhase, camera[3], tanSunAngularRadius;
    uint32_t W, H, doDenoising;
    float rayStartOffset;
} SmConsts;                                                                                                       /* 112 bytes */
typedef struct
{
    const SmInstance* instances; const uint32_t* flags; uint32_t numInstances;
    const uint8_t* vertices; uint32_t numVertices;                                                                /* 20-byte stride */
    const SmMaterial* materials; uint32_t numMaterials;
    const uint32_t* indices; uint32_t numIndices;
    const SmMesh* meshes; const uint32_t* meshIndexCounts; uint32_t numMeshes;
    const SmNode* tlasNodes; uint32_t numTlasNodes;
    const SmTlasInstance* tlasInstances;
    const SmHeader* headers;
    const SmNode* blasNodes; uint32_t numBlasNodes;
    const uint32_t* triOrder; uint32_t numTriOrder;
} SmScene;

#define SM_INNER 0xFFFFFFFFu
static const float kSlack = 0x1p-18f, kTlasPad = 0x1p-12f;

/* the by-value forms of ref_base.h's dot3, cross3 and normalize3: the same operations on an F3 */
static float dot3f(F3 a, F3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static F3 cross3f(F3 a, F3 b) { F3 r = { fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)) }; return r; }
static F3 normalize3f(F3 v) { const float len = sqrtf(dot3f(v, v)); F3 r = { v.x / len, v.y / len, v.z / len }; return r; }
static float sel(F3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

/* ---- sinSoft / cosSoft of csrc/soft_math.hip.h (derivation: tests/gtao_ref.c) ------------------------------------------------ */
static float sincos_soft(float x, int quarter)
{
    if (!(fabsf(x) <= 10.0f)) return float_of(0x7FC00000u);
    const float k = rintf(x * 0x1.45f306p-1f);
    float r = fmaf(-k, 0x1.921p+0f, x);
    r = fmaf(-k, 0x1.f6ap-13f, r);
    r = fmaf(-k, 0x1.110b46p-26f, r);
    const float z = r * r;
    const int q = ((int)k + quarter) & 3;
    float v;
    if (q & 1) {
        float p = 0x1.99bcaap-16f;
        p = fmaf(p, z, -0x1.6c0b94p-10f);
        p = fmaf(p, z, 0x1.55554ap-5f);
        v = fmaf(z * z, p, fmaf(-0.5f, z, 1.0f));
    } else {
        float p = -0x1.98896ep-13f;
        p = fmaf(p, z, 0x1.1104a6p-7f);
        p = fmaf(p, z, -0x1.55553cp-3f);
        v = fmaf(r * z, p, r);
    }
    return (q & 2) ? -v : v;
}

uint16_t sm_half_bits(float f) { return float_to_half(f); }

/* ---- the object-from-world 3x4 of one instance: rows r0 r1 r2 r3 of p_object = (p_world, 1) * M ------------------------------ */
void sm_object_from_world(const float* w, float* out)
{
    const F3 a = { w[0], w[1], w[2] }, b = { w[4], w[5], w[6] }, c = { w[8], w[9], w[10] }, t = { w[12], w[13], w[14] };
    const float c00 = b.y * c.z - b.z * c.y, c01 = b.z * c.x - b.x * c.z, c02 = b.x * c.y - b.y * c.x;
    const float det = (a.x * c00 + a.y * c01) + a.z * c02;
    float inv[3][3];
    inv[0][0] = c00 / det; inv[1][0] = c01 / det; inv[2][0] = c02 / det;
    inv[0][1] = (a.z * c.y - a.y * c.z) / det; inv[1][1] = (a.x * c.z - a.z * c.x) / det; inv[2][1] = (a.y * c.x - a.x * c.y) / det;
    inv[0][2] = (a.y * b.z - a.z * b.y) / det; inv[1][2] = (a.z * b.x - a.x * b.z) / det; inv[2][2] = (a.x * b.y - a.y * b.x) / det;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[3 * i + j] = inv[i][j];
    for (int j = 0; j < 3; ++j) out[9 + j] = -((t.x * inv[0][j] + t.y * inv[1][j]) + t.z * inv[2][j]);
}

static F3 mul_point(F3 p, const float* m, int translate)
{
    F3 r = { fmaf(p.z, m[6], fmaf(p.y, m[3], p.x * m[0])), fmaf(p.z, m[7], fmaf(p.y, m[4], p.x * m[1])), fmaf(p.z, m[8], fmaf(p.y, m[5], p.x * m[2])) };
    if (translate) { r.x = r.x + m[9]; r.y = r.y + m[10]; r.z = r.z + m[11]; }
    return r;
}

/* ---- "raytracing_CS_RefitTLAS": leaves, then the inner boxes height by height ----------------------------------------------- */
void sm_refit(const SmInstance* instances, uint32_t numInstances, const SmHeader* headers, uint32_t numMeshes, const SmNode* blasNodes, uint32_t numBlasNodes,
              const uint32_t* levelOffsets, const uint32_t* levelNodes, uint32_t numLevels, SmNode* nodes, uint32_t numNodes, SmTlasInstance* records)
{
    for (uint32_t i = 0; i < numInstances; ++i) {
        SmTlasInstance* rec = &records[i];
        if (!rec->flags || rec->leaf_node >= numNodes) continue;
        sm_object_from_world(instances[i].world, rec->m);
        SmNode* leaf = &nodes[rec->leaf_node];
        const uint32_t mesh = instances[i].mesh;
        float lo[3] = { 3.402823466e38f, 3.402823466e38f, 3.402823466e38f }, hi[3] = { -3.402823466e38f, -3.402823466e38f, -3.402823466e38f };
        if (mesh < numMeshes && headers[mesh].num_nodes && headers[mesh].node_offset < numBlasNodes) {
            const SmNode* root = &blasNodes[headers[mesh].node_offset];
            const float* w = instances[i].world;
            float largest = 0.0f;
            for (int c = 0; c < 8; ++c) {
                const F3 p = { c & 1 ? root->hi[0] : root->lo[0], c & 2 ? root->hi[1] : root->lo[1], c & 4 ? root->hi[2] : root->lo[2] };
                const float q[3] = { fmaf(p.z, w[8], fmaf(p.y, w[4], p.x * w[0])) + w[12], fmaf(p.z, w[9], fmaf(p.y, w[5], p.x * w[1])) + w[13],
                                     fmaf(p.z, w[10], fmaf(p.y, w[6], p.x * w[2])) + w[14] };
                for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], q[a]); hi[a] = fmaxf(hi[a], q[a]); largest = fmaxf(largest, fabsf(q[a])); }
            }
            const float pad = kTlasPad * largest;
            for (int a = 0; a < 3; ++a) { lo[a] = lo[a] - pad; hi[a] = hi[a] + pad; }
        }
        for (int a = 0; a < 3; ++a) { leaf->lo[a] = lo[a]; leaf->hi[a] = hi[a]; }
    }
    for (uint32_t l = 0; l < numLevels; ++l)
        for (uint32_t k = levelOffsets[l]; k < levelOffsets[l + 1]; ++k) {
            const uint32_t n = levelNodes[k];
            if (n >= numNodes || n + 1 >= numNodes) continue;
            const uint32_t right = nodes[n + 1].skip;
            if (right >= numNodes) continue;
            for (int a = 0; a < 3; ++a) {
                nodes[n].lo[a] = fminf(nodes[n + 1].lo[a], nodes[right].lo[a]);
                nodes[n].hi[a] = fmaxf(nodes[n + 1].hi[a], nodes[right].hi[a]);
            }
        }
}

/* ---- the two tests ------------------------------------------------------------------------------------------------------------ */
typedef struct { F3 o, d, inv; int kx, ky, kz; float Sx, Sy, Sz; } SmRay;

static SmRay make_ray(F3 o, F3 d)
{
    SmRay r;
    r.o = o; r.d = d;
    r.inv.x = 1.0f / d.x; r.inv.y = 1.0f / d.y; r.inv.z = 1.0f / d.z;
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    int kz = 0;
    float m = ax;
    if (ay > m) { kz = 1; m = ay; }
    if (az > m) { kz = 2; }
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dz = sel(d, kz);
    if (dz < 0.0f) { const int s = kx; kx = ky; ky = s; }
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.Sx = sel(d, kx) / dz; r.Sy = sel(d, ky) / dz; r.Sz = 1.0f / dz;
    return r;
}

int sm_box_hit(const float* lo, const float* hi, const SmRay* r)
{
    float tenter = 0.0f, texit = float_of(0x7F800000u);
    for (int a = 0; a < 3; ++a) {
        const float o = sel(r->o, a), inv = sel(r->inv, a);
        if (!(fabsf(inv) <= 3.402823466e38f)) {
            if (!(o >= lo[a] && o <= hi[a])) return 0;
        } else {
            const float t0 = (lo[a] - o) * inv, t1 = (hi[a] - o) * inv;
            float tn = fminf(t0, t1), tf = fmaxf(t0, t1);
            tn = tn - fabsf(tn) * kSlack; tf = tf + fabsf(tf) * kSlack;
            tenter = fmaxf(tenter, tn); texit = fminf(texit, tf);
        }
    }
    return tenter <= texit;
}

/* THE triangle test (csrc/ray_walk.hip.h: triTest): the edge test and det != 0; 1 with the candidate's t, which the caller holds against
 * the ray's interval, b1 = V / det and b2 = W / det (InterpolateVertex's barycentrics of the second and third vertex) and front = det > 0 */
typedef struct { float t, b1, b2; uint32_t front; } SmTriHit;

static int tri_candidate(F3 v0, F3 v1, F3 v2, const SmRay* r, SmTriHit* h)
{
    const F3 A = { v0.x - r->o.x, v0.y - r->o.y, v0.z - r->o.z }, B = { v1.x - r->o.x, v1.y - r->o.y, v1.z - r->o.z }, C = { v2.x - r->o.x, v2.y - r->o.y, v2.z - r->o.z };
    const float Akz = sel(A, r->kz), Bkz = sel(B, r->kz), Ckz = sel(C, r->kz);
    const float Ax = sel(A, r->kx) - r->Sx * Akz, Ay = sel(A, r->ky) - r->Sy * Akz;
    const float Bx = sel(B, r->kx) - r->Sx * Bkz, By = sel(B, r->ky) - r->Sy * Bkz;
    const float Cx = sel(C, r->kx) - r->Sx * Ckz, Cy = sel(C, r->ky) - r->Sy * Ckz;
    const float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return 0;
    const float det = (U + V) + W;
    if (det == 0.0f) return 0;
    const float Az = r->Sz * Akz, Bz = r->Sz * Bkz, Cz = r->Sz * Ckz;
    const float T = (U * Az + V * Bz) + W * Cz;
    h->t = T / det;
    h->b1 = V / det; h->b2 = W / det;
    h->front = det > 0.0f ? 1u : 0u;
    return 1;
}

int sm_tri_hit(F3 v0, F3 v1, F3 v2, const SmRay* r, float tmin, float tmax)
{
    SmTriHit h;
    return tri_candidate(v0, v1, v2, r, &h) && h.t > tmin && h.t < tmax;
}

/* ---- one texel's ray: 0 for a far texel, else origin and direction ------------------------------------------------------------- */
static float fmod1(float x) { return x - truncf(x); }

static F3 map_to_cone(float sx, float sy, F3 n, float radius)
{
    const float ox = 2.0f * sx - 1.0f, oy = 2.0f * sy - 1.0f;
    if (ox == 0.0f && oy == 0.0f) return n;
    float theta, r;
    if (fabsf(ox) > fabsf(oy)) { r = ox; theta = 0x1.921fb6p-1f * (oy / ox); }
    else { r = oy; theta = 0x1.921fb6p+0f * (1.0f - 0.5f * (ox / oy)); }
    const float ux = (radius * r) * sincos_soft(theta, 1), uy = (radius * r) * sincos_soft(theta, 0);
    const F3 up = { fabsf(n.z) < 0.99999f ? 0.0f : 1.0f, 0.0f, fabsf(n.z) < 0.99999f ? 1.0f : 0.0f };
    const F3 t0 = normalize3f(cross3f(up, n)), t1 = cross3f(n, t0);
    const F3 d = { (n.x + ux * t0.x) + uy * t1.x, (n.y + ux * t0.y) + uy * t1.y, (n.z + ux * t0.z) + uy * t1.z };
    return d;
}

int sm_texel_ray(const SmConsts* k, uint32_t px, uint32_t py, float depth, const uint32_t* g, const uint32_t* noise, float* origin, float* direction, float* world)
{
    if (depth == 0.0f) return 0;
    const float* m = k->clipToWorld;
    const float u = ((float)px + 0.5f) / (float)k->W, v = ((float)py + 0.5f) / (float)k->H;
    const float cx = u * 2.0f + -1.0f, cy = v * -2.0f + 1.0f;
    float h[4];
    for (int j = 0; j < 4; ++j) h[j] = fmaf(depth, m[8 + j], fmaf(cy, m[4 + j], cx * m[j])) + m[12 + j];
    const F3 wp = { h[0] / h[3], h[1] / h[3], h[2] / h[3] };
    float n[3];
    unpack_oct(g[1], n);
    const uint32_t texel = noise[(py % 128u) * 128u + (px % 128u)];
    const float sx = fmod1((float)(texel & 0xFFu) / 255.0f + k->noisePhase), sy = fmod1((float)((texel >> 8) & 0xFFu) / 255.0f + k->noisePhase);
    const F3 light = { k->light[0], k->light[1], k->light[2] };
    const F3 d = normalize3f(map_to_cone(sx, sy, light, k->tanSunAngularRadius));
    origin[0] = wp.x + n[0] * k->rayStartOffset; origin[1] = wp.y + n[1] * k->rayStartOffset; origin[2] = wp.z + n[2] * k->rayStartOffset;
    direction[0] = d.x; direction[1] = d.y; direction[2] = d.z;
    world[0] = wp.x; world[1] = wp.y; world[2] = wp.z;
    return 1;
}

/* ---- occlusion of one ray ----------------------------------------------------------------------------------------------------- */
static F3 vertex_of(const SmScene* s, uint64_t i) { F3 v; memcpy(&v, s->vertices + i * 20u, 12); return v; }
static int finite3(F3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

/* the candidate counts: ForceOpaque always, ForceNonOpaque by the alpha test of its instance's material */
static int commits(const SmScene* s, uint32_t inst, uint32_t flags)
{
    if (flags != 2u) return 1;
    const uint32_t mat = s->instances[inst].material;
    if (mat >= s->numMaterials) return 0;
    return s->materials[mat].albedo[3] >= s->materials[mat].alphaCutoff;
}

/* THE triangle fetch (csrc/ray_walk.hip.h: fetchTri): the three vertex indices and positions of triangle `tri` of mesh `mesh`; 0 when an
 * index leaves its buffer, and with requireFinite (the brute-force evaluators: the builder leaves such a triangle out of the tree)
 * when a vertex is not finite */
typedef struct { uint64_t i[3]; F3 v[3]; } SmTri;

static int fetch_tri(const SmScene* s, uint32_t mesh, uint32_t tri, int requireFinite, SmTri* out)
{
    const uint64_t base = (uint64_t)s->meshes[mesh].indexBase + 3ull * tri;
    if (base + 3u > s->numIndices) return 0;
    for (int k = 0; k < 3; ++k) {
        out->i[k] = (uint64_t)s->meshes[mesh].vertexBase + s->indices[base + k];
        if (out->i[k] >= s->numVertices) return 0;
        out->v[k] = vertex_of(s, out->i[k]);
        if (requireFinite && !finite3(out->v[k])) return 0;
    }
    return 1;
}

typedef struct { float tmin, tmax; } SmInterval;

/* triangle `tri` of mesh `mesh` against the object-space ray */
static int mesh_tri_hit(const SmScene* s, uint32_t mesh, uint32_t tri, int requireFinite, const SmRay* r, const SmInterval* in)
{
    SmTri T;
    return fetch_tri(s, mesh, tri, requireFinite, &T) && sm_tri_hit(T.v[0], T.v[1], T.v[2], r, in->tmin, in->tmax);
}

static int occluded_brute(const SmScene* s, F3 o, F3 d, const SmInterval* in)
{
    for (uint32_t i = 0; i < s->numInstances; ++i) {
        const uint32_t flags = s->flags[i] & 3u, mesh = s->instances[i].mesh;
        if (!flags || mesh >= s->numMeshes) continue;
        float m[12];
        sm_object_from_world(s->instances[i].world, m);
        const SmRay r = make_ray(mul_point(o, m, 1), mul_point(d, m, 0));
        for (uint32_t t = 0; t < s->meshIndexCounts[mesh] / 3u; ++t)
            if (mesh_tri_hit(s, mesh, t, 1, &r, in) && commits(s, i, flags)) return 1;
    }
    return 0;
}

/* THE walk (csrc/ray_walk.hip.h: walk, which states its rules): every candidate slot is handed to visit(ctx, s, instance, flags, mesh,
 * the mesh's triangle number, the object-space ray); a visit that answers 1 stops the walk, and the walk answers whether it was
 * stopped.  counters: NULL, or { box tests, candidate slots }, added to. */
typedef int (*SmVisit)(void* ctx, const SmScene* s, uint32_t inst, uint32_t flags, uint32_t mesh, uint32_t tri, const SmRay* r);

static int sm_walk(const SmScene* s, F3 o, F3 d, SmVisit visit, void* ctx, uint64_t* counters)
{
    uint64_t unread[2] = { 0, 0 };
    uint64_t *boxTests = counters ? &counters[0] : &unread[0], *triTests = counters ? &counters[1] : &unread[1];
    const SmRay wr = make_ray(o, d);
    uint32_t node = 0;
    while (node < s->numTlasNodes) {
        const SmNode* n = &s->tlasNodes[node];
        uint32_t next = n->skip > node ? n->skip : s->numTlasNodes;
        ++*boxTests;
        if (sm_box_hit(n->lo, n->hi, &wr)) {
            if (n->leaf == SM_INNER) next = node + 1;
            else if (n->leaf < s->numInstances) {
                const uint32_t inst = n->leaf, flags = s->tlasInstances[inst].flags, mesh = s->instances[inst].mesh;
                if (flags && mesh < s->numMeshes) {
                    const SmHeader hd = s->headers[mesh];
                    const float* m = s->tlasInstances[inst].m;
                    const SmRay r = make_ray(mul_point(o, m, 1), mul_point(d, m, 0));
                    const uint32_t count = (uint64_t)hd.node_offset + hd.num_nodes <= s->numBlasNodes ? hd.num_nodes : 0u;
                    uint32_t b = 0;
                    while (b < count) {
                        const SmNode* bn = &s->blasNodes[hd.node_offset + b];
                        uint32_t bnext = bn->skip > b ? bn->skip : count;
                        ++*boxTests;
                        if (sm_box_hit(bn->lo, bn->hi, &r)) {
                            if (bn->leaf == SM_INNER) bnext = b + 1;
                            else {
                                const uint32_t first = bn->leaf & 0x3FFFFFFFu, cnt = (bn->leaf >> 30) + 1u;
                                for (uint32_t j = 0; j < cnt; ++j) {
                                    const uint64_t slot = (uint64_t)hd.tri_offset + first + j;
                                    if (first + j >= hd.num_tris || slot >= s->numTriOrder) break;
                                    ++*triTests;
                                    if (visit(ctx, s, inst, flags, mesh, s->triOrder[slot], &r)) return 1;
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
    return 0;
}

/* the sun's any-hit visitor; ctx: the ray's SmInterval */
static int occluded_walk(void* ctx, const SmScene* s, uint32_t inst, uint32_t flags, uint32_t mesh, uint32_t tri, const SmRay* r)
{
    return mesh_tri_hit(s, mesh, tri, 0, r, (const SmInterval*)ctx) && commits(s, inst, flags);
}

/* The candidates of every texel's ray, for the tests' preconditions: brute force's loop over every triangle of every instance with
 * flags, WITHOUT the interval test and without the alpha test: each triangle that passes the edge test with det != 0, as (texel,
 * instance, t).  The direction is not normalised in object space, so t is the world's.  Returns how many there are; the first
 * `capacity` of them are stored. */
uint32_t sm_candidates(const SmConsts* k, const SmScene* s, const float* depth, const uint32_t* gbufferA, const uint32_t* noise, uint32_t capacity, uint32_t* texels,
                       uint32_t* insts, float* ts)
{
    uint32_t n = 0;
    for (uint32_t py = 0; py < k->H; ++py)
        for (uint32_t px = 0; px < k->W; ++px) {
            const uint64_t at = (uint64_t)py * k->W + px;
            float o[3], d[3], w[3];
            if (!sm_texel_ray(k, px, py, depth[at], gbufferA + 4 * at, noise, o, d, w)) continue;
            const F3 O = { o[0], o[1], o[2] }, D = { d[0], d[1], d[2] };
            for (uint32_t i = 0; i < s->numInstances; ++i) {
                const uint32_t mesh = s->instances[i].mesh;
                if (!(s->flags[i] & 3u) || mesh >= s->numMeshes) continue;
                float m[12];
                sm_object_from_world(s->instances[i].world, m);
                const SmRay r = make_ray(mul_point(O, m, 1), mul_point(D, m, 0));
                for (uint32_t t = 0; t < s->meshIndexCounts[mesh] / 3u; ++t) {
                    SmTri T;
                    SmTriHit h;
                    if (!fetch_tri(s, mesh, t, 1, &T) || !tri_candidate(T.v[0], T.v[1], T.v[2], &r, &h)) continue;
                    if (n < capacity) { texels[n] = (uint32_t)at; insts[n] = i; ts[n] = h.t; }
                    ++n;
                }
            }
        }
    return n;
}

/* The pass over a whole image.  mode 0: brute force, 1: the walk.  mask and lvd hold what the targets held before. */
void sm_trace(const SmConsts* k, const SmScene* s, const float* depth, const uint32_t* gbufferA, const uint32_t* noise, int mode, uint8_t* mask, uint16_t* lvd,
              uint64_t* counters)
{
    SmInterval in = { k->rayStartOffset, 1e10f };
    if (counters) counters[0] = counters[1] = 0;
    for (uint32_t py = 0; py < k->H; ++py)
        for (uint32_t px = 0; px < k->W; ++px) {
            const uint64_t i = (uint64_t)py * k->W + px;
            float o[3], d[3], w[3];
            if (!sm_texel_ray(k, px, py, depth[i], gbufferA + 4 * i, noise, o, d, w)) { lvd[i] = 0x7BFFu; continue; }
            const F3 O = { o[0], o[1], o[2] }, D = { d[0], d[1], d[2] };
            const int occ = mode ? sm_walk(s, O, D, occluded_walk, &in, counters) : occluded_brute(s, O, D, &in);
            mask[i] = occ ? 0u : 255u;
            const F3 v = { w[0] - k->camera[0], w[1] - k->camera[1], w[2] - k->camera[2] };
            lvd[i] = sm_half_bits(sqrtf(dot3f(v, v)));
        }
}
