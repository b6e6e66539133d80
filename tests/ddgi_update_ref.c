/* ddgi_update_ref.c -- the definition of "giprobetrace_CS_ProbeTrace" (csrc/k_giprobetrace.hip, csrc/ray_walk.hip.h: closestHit) and
 * of the two "ProbeBlendingCS_DDGIProbeBlendingCS" passes (csrc/k_giprobeblend.hip, csrc/ddgi_update.hip.h), which repeat the
 * functions below word for word.  Compile with gcc -O2 -ffp-contract=off (tests/ddgi_update_ref.py).
 *
 * The RTXGI SDK is not part of this project: the update is the project's own statement of the published algorithm (Majercik et
 * al., JCGT 2019) with the settings GIRenderer.cpp:74-121 configures, and this file is what the tests pin.
 *
 * It includes tests/shadowmask_ref.c for the ray, the box test, the watertight triangle test, the triangle fetch, the walk (sm_walk,
 * whose visitor closest_walk below is; closest_brute stays a loop of its own over every triangle) and the scene's arrays, and
 * tests/ddgi_ref.c (and through it tests/lighting_ref.c) for the irradiance query, the soft pow and the directional light's pieces.
 *
 * CONVENTION.  binary32 throughout, no contraction, fmaf only where written, / and sqrtf correctly rounded.
 *   probe     index p = (y * counts.z + z) * counts.x + x; data texel (x, z) of slice y; tiles at texel (x * N, z * N) of slice y;
 *             position: ddgi_ref.c's probe_pos; inactive: flags bit 1 and data.w == 1.0f;
 *   ray i     f = (float)i * 0.618034f; phi = RN(2 pi) * (f - floorf(f)); c = 1.0f - (float)(2 * i + 1) / 256.0f;
 *             s = sqrtf(saturate(1.0f - c * c)); d = (cos(phi) * s, sin(phi) * s, c) with the soft sine and cosine;
 *             rotated = (dot3(row0, d), dot3(row1, d), dot3(row2, d)); direction = rotated / sqrtf(dot3(rotated, rotated));
 *   octDecode v = (o.x, o.y, (1 - |o.x|) - |o.y|); v.z < 0: v.xy = ((1 - |o.y|) * s(o.x), (1 - |o.x|) * s(o.y)), s(x) = x >= 0 ? 1 : -1;
 *             normalize.  Interior texel i of n has o = (float)(2 * i + 1) / (float)n - 1;
 *   closest hit: TWO EVALUATORS, brute force over every triangle of every instance (mode 0, the definition) and the walk of the
 *             product's node arrays (mode 1).  Every candidate commits (RAY_FLAG_FORCE_OPAQUE), instances with flags == 0 are
 *             skipped.  The winner has the smallest t in (tmin, tmax); on equal t the lower instance index, then the lower
 *             triangle number of the mesh.  front iff det = (U + V) + W of the object-space watertight test is > 0;
 *   trace     miss (1, 1, 1, 1e27f); back face (0, 0, 0, -0.2f * t); front face: b0 = (1.0f - b1) - b2; position and normal
 *             ((0 + v0 * b0) + v1 * b1) + v2 * b2; normal components (float)q / 1023.0f * 2 - 1, kept in OBJECT space, not normalised
 *             (the reference's quirk); world through the instance's world matrix in fmaf; albedo m_ConstAlbedo.rgb, emissive
 *             m_ConstEmissive, roughness 1, metallic 0; the shadow ray starts at the PROBE (the reference's quirk), direction the
 *             light vector, TMin 0, TMax 1e10f, occluded iff the closest hit finds anything; rgb = lit(surface, viewer = probe,
 *             shadow = occluded ? 0 : 1) (lr_lit's words, emissive included) + (fminf(albedo, 0.9f) * kInvPi) * dg_irradiance(world,
 *             normal, cameraOrigin = probe); record (saturate(rgb), t).  An inactive probe's records keep what they held;
 *   blends    stated in csrc/k_giprobeblend.hip ("CONVENTION") in the words of the functions below. */
#include "shadowmask_ref.c"
#include "ddgi_ref.c"

typedef struct
{
    float light[3], strength;
    float rotation[3][4];
    float maxRayDistance, hysteresis, distanceExponent, irradianceThreshold, brightnessThreshold;
    uint32_t pad[3];
} DuConsts;                                                                                                      /* 96 bytes */
typedef struct { DuConsts k; DgDesc D; } DuBlock;                                                               /* 160 bytes: b0 */
typedef struct { uint32_t inst, tri; float t, b1, b2; uint32_t front; } DuHit;                                  /* inst 0xFFFFFFFF: a miss */

#define DU_RAYS 256u
#define DU_BACKFACE_LIMIT 25u

/* ---- probes, rays, texels ---------------------------------------------------------------------------------------------------- */
/* position and state of one probe (tests/ddgi_ref.c probe_at); returns 1 when it is inactive */
static int probe_of(const DgDesc* D, const uint16_t* data, uint32_t probe, int32_t c[3], float pos[3])
{
    float state;
    probe_at(D, data, probe, c, pos, &state);
    return (D->flags & 2u) && state == 1.0f;
}

void du_ray_direction(const DuConsts* k, uint32_t i, float out[3])
{
    const float f = (float)i * 0.618034f, phi = 0x1.921fb6p+2f * (f - floorf(f));
    const float c = 1.0f - (float)(2u * i + 1u) / (float)DU_RAYS, s = sqrtf(saturate(1.0f - c * c));
    const float d[3] = { sincos_soft(phi, 1) * s, sincos_soft(phi, 0) * s, c };
    const float r[3] = { dot3(k->rotation[0], d), dot3(k->rotation[1], d), dot3(k->rotation[2], d) };
    normalize3(r, out);
}

void du_oct_decode(float ox, float oy, float out[3])
{
    float v[3] = { ox, oy, (1.0f - fabsf(ox)) - fabsf(oy) };
    if (v[2] < 0.0f) oct_fold(ox, oy, v);
    normalize3(v, out);
}

void du_texel_direction(uint32_t ix, uint32_t iy, uint32_t n, float out[3])
{
    du_oct_decode((float)(2u * ix + 1u) / (float)n - 1.0f, (float)(2u * iy + 1u) / (float)n - 1.0f, out);
}

/* ---- the closest hit ------------------------------------------------------------------------------------------------------------ */
typedef struct { SmInterval in; DuHit best; } DuClosest;

/* triangle `tri` of mesh `mesh` against the object-space ray, offered to c->best under the tie rule; with requireFinite a
 * triangle with a non-finite vertex is left out (the builder leaves it out of the tree).  Returns 1 on equal t with another
 * candidate (a tie that the rule decided). */
static int offer(const SmScene* s, uint32_t inst, uint32_t mesh, uint32_t tri, const SmRay* r, int requireFinite, DuClosest* c)
{
    SmTri T;
    SmTriHit h;
    if (!fetch_tri(s, mesh, tri, requireFinite, &T) || !tri_candidate(T.v[0], T.v[1], T.v[2], r, &h) || !(h.t > c->in.tmin && h.t < c->in.tmax)) return 0;
    DuHit* best = &c->best;
    const int first = best->inst == 0xFFFFFFFFu, tie = !first && h.t == best->t;
    if (first || h.t < best->t || (tie && (inst < best->inst || (inst == best->inst && tri < best->tri)))) {
        const DuHit won = { inst, tri, h.t, h.b1, h.b2, h.front };
        *best = won;
    }
    return tie;
}

static void closest_brute(const SmScene* s, F3 o, F3 d, DuClosest* c, uint64_t* ties)
{
    for (uint32_t i = 0; i < s->numInstances; ++i) {
        const uint32_t flags = s->flags[i] & 3u, mesh = s->instances[i].mesh;
        if (!flags || mesh >= s->numMeshes) continue;
        float m[12];
        sm_object_from_world(s->instances[i].world, m);
        const SmRay r = make_ray(mul_point(o, m, 1), mul_point(d, m, 0));
        for (uint32_t t = 0; t < s->meshIndexCounts[mesh] / 3u; ++t) *ties += (uint64_t)offer(s, i, mesh, t, &r, 1, c);
    }
}

/* the closest hit's visitor of sm_walk (tests/shadowmask_ref.c); ctx: the ray's DuClosest.  Never stops the walk. */
static int closest_walk(void* ctx, const SmScene* s, uint32_t inst, uint32_t flags, uint32_t mesh, uint32_t tri, const SmRay* r)
{
    (void)flags;
    offer(s, inst, mesh, tri, r, 0, (DuClosest*)ctx);
    return 0;
}

/* mode 0: brute force, 1: the walk.  ties: the equal-t decisions brute force met (added to). */
static DuHit closest(const SmScene* s, F3 o, F3 d, float tmin, float tmax, int mode, uint64_t* ties)
{
    DuClosest c = { { tmin, tmax }, { 0xFFFFFFFFu, 0xFFFFFFFFu, 0.0f, 0.0f, 0.0f, 0u } };
    if (mode) sm_walk(s, o, d, closest_walk, &c, NULL);
    else closest_brute(s, o, d, &c, ties);
    return c.best;
}

/* n rays; mode 0: brute force, 1: the walk.  ties: uint64[1] or NULL, the equal-t decisions brute force met (added to). */
void du_closest_n(const SmScene* s, const float* o, const float* d, uint64_t n, float tmin, float tmax, int mode, DuHit* out, uint64_t* ties)
{
    uint64_t local = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const F3 O = { o[3 * i], o[3 * i + 1], o[3 * i + 2] }, Dir = { d[3 * i], d[3 * i + 1], d[3 * i + 2] };
        out[i] = closest(s, O, Dir, tmin, tmax, mode, &local);
    }
    if (ties) *ties += local;
}

/* ---- the trace ------------------------------------------------------------------------------------------------------------------ */
static float bary(float v0, float v1, float v2, float b0, float b1, float b2) { return ((0.0f + v0 * b0) + v1 * b1) + v2 * b2; }

/* lr_lit's words (tests/lighting_ref.c) for a surface given outright, seen from `viewer` */
static void lit_surface(const LrGBuffer* p, const float viewer[3], const float world[3], const float L[3], float strength, float shadow, float rgb[3])
{
    float toEye[3], V[3], VL[3], H[3], diffuse[3], f0[3], env[3];
    const float oneMinusMetal = 1.0f - p->metallic, dielectric = 0.08f * 0.5f;
    for (int c = 0; c < 3; ++c) {
        diffuse[c] = p->albedo[c] * oneMinusMetal;
        f0[c] = dielectric + p->metallic * (p->albedo[c] - dielectric);
        toEye[c] = viewer[c] - world[c];
    }
    normalize3(toEye, V);
    for (int c = 0; c < 3; ++c) VL[c] = V[c] + L[c];
    normalize3(VL, H);
    const float NdotV = saturate(fabsf(dot3(p->normal, V)) + 1e-5f), NdotL = saturate(dot3(p->normal, L));
    const float NdotH = saturate(dot3(p->normal, H)), VdotH = saturate(dot3(V, H));
    const float a = p->roughness * p->roughness, a2 = fminf(fmaxf(a * a, 0.0001f), 1.0f);
    const float d = (NdotH * a2 - NdotH) * NdotH + 1.0f;
    const float D = a2 / ((kPi * d) * d);
    const float smithV = NdotL * (NdotV * (1.0f - a2) + a2), smithL = NdotV * (NdotL * (1.0f - a2) + a2);
    const float Vis = 0.5f * (1.0f / (smithV + smithL));
    const float x = 1.0f - VdotH, xx = x * x, Fc = (xx * xx) * x;
    const float DVis = D * Vis;
    env_brdf_approx(f0, p->roughness, NdotV, env);
    for (int c = 0; c < 3; ++c) {
        const float F = Fc + (1.0f - Fc) * f0[c];
        const float spec = DVis * F + env[c];
        rgb[c] = (((diffuse[c] * kInvPi + spec) * NdotL) * strength) * shadow + p->emissive[c];
    }
}

/* One record.  kind (may be NULL): 0 miss, 1 back face, 2 front face lit, 3 front face in shadow. */
static void trace_ray(const DuBlock* b, const SmScene* s, const uint16_t* data, const uint32_t* irradiance, const uint16_t* distance, const float origin[3], uint32_t ray,
                      int mode, float rec[4], uint32_t* kind)
{
    uint64_t ties = 0;
    float dir[3];
    du_ray_direction(&b->k, ray, dir);
    const F3 O = { origin[0], origin[1], origin[2] }, Dir = { dir[0], dir[1], dir[2] }, L = { b->k.light[0], b->k.light[1], b->k.light[2] };
    const DuHit hit = closest(s, O, Dir, 0.0f, b->k.maxRayDistance, mode, &ties);
    if (hit.inst == 0xFFFFFFFFu) { rec[0] = rec[1] = rec[2] = 1.0f; rec[3] = 1e27f; if (kind) *kind = 0; return; }
    if (!hit.front) { rec[0] = rec[1] = rec[2] = 0.0f; rec[3] = -0.2f * hit.t; if (kind) *kind = 1; return; }
    const SmInstance* inst = &s->instances[hit.inst];
    SmTri T;
    if (!fetch_tri(s, inst->mesh, hit.tri, 0, &T)) return;                   /* cannot fail: the closest hit fetched this triangle */
    const F3* v = T.v;
    float n[3][3];
    for (int j = 0; j < 3; ++j) {
        uint32_t packed;
        memcpy(&packed, s->vertices + T.i[j] * 20u + 12u, 4);
        unpack_normal10(packed, n[j]);
    }
    const float b1 = hit.b1, b2 = hit.b2, b0 = (1.0f - b1) - b2;
    const float p[3] = { bary(v[0].x, v[1].x, v[2].x, b0, b1, b2), bary(v[0].y, v[1].y, v[2].y, b0, b1, b2), bary(v[0].z, v[1].z, v[2].z, b0, b1, b2) };
    LrGBuffer g;
    memset(&g, 0, sizeof g);
    for (int c = 0; c < 3; ++c) g.normal[c] = bary(n[0][c], n[1][c], n[2][c], b0, b1, b2);
    const float* w = inst->world;
    const float world[3] = { fmaf(p[2], w[8], fmaf(p[1], w[4], p[0] * w[0])) + w[12], fmaf(p[2], w[9], fmaf(p[1], w[5], p[0] * w[1])) + w[13],
                             fmaf(p[2], w[10], fmaf(p[1], w[6], p[0] * w[2])) + w[14] };
    if (inst->material < s->numMaterials) {
        memcpy(g.albedo, s->materials[inst->material].albedo, sizeof g.albedo);
        memcpy(g.emissive, s->materials[inst->material].emissive, sizeof g.emissive);
    }
    g.roughness = 1.0f; g.metallic = 0.0f;
    const int occluded = closest(s, O, L, 0.0f, 1e10f, mode, &ties).inst != 0xFFFFFFFFu;
    float lit[3], irr[3];
    lit_surface(&g, origin, world, b->k.light, b->k.strength, occluded ? 0.0f : 1.0f, lit);
    dg_irradiance(&b->D, data, irradiance, distance, world, g.normal, origin, irr, NULL);
    for (int c = 0; c < 3; ++c) rec[c] = saturate(lit[c] + (fminf(g.albedo[c], 0.9f) * kInvPi) * irr[c]);
    rec[3] = hit.t;
    if (kind) *kind = occluded ? 3u : 2u;
}

/* The pass: rays float[numProbes * 256 * 4] holds what the buffer held before.  kinds: uint32[numProbes * 256] or NULL (an
 * inactive probe's stay untouched). */
void du_trace(const DuBlock* b, const SmScene* s, const uint16_t* data, const uint32_t* irradiance, const uint16_t* distance, int mode, float* rays, uint32_t* kinds)
{
    const uint32_t probes = (uint32_t)b->D.probeCounts[0] * (uint32_t)b->D.probeCounts[1] * (uint32_t)b->D.probeCounts[2];
    for (uint32_t p = 0; p < probes; ++p) {
        int32_t c[3];
        float pos[3];
        if (probe_of(&b->D, data, p, c, pos)) continue;
        for (uint32_t r = 0; r < DU_RAYS; ++r)
            trace_ray(b, s, data, irradiance, distance, pos, r, mode, rays + ((uint64_t)p * DU_RAYS + r) * 4u, kinds ? kinds + (uint64_t)p * DU_RAYS + r : NULL);
    }
}

void du_probe_positions(const DgDesc* D, const uint16_t* data, float* pos, uint32_t* inactive)
{
    const uint32_t probes = (uint32_t)D->probeCounts[0] * (uint32_t)D->probeCounts[1] * (uint32_t)D->probeCounts[2];
    for (uint32_t p = 0; p < probes; ++p) {
        int32_t c[3];
        inactive[p] = (uint32_t)probe_of(D, data, p, c, pos + 3 * p);
    }
}

/* ---- the blends ----------------------------------------------------------------------------------------------------------------- */
static float sign1(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
static float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

/* One word of rule bits per interior texel, written by du_blend_radiance_rules / du_blend_distance_rules: the decisions the
 * functions below took, in their own binary32.  A NULL `rules` changes nothing: the arithmetic is stated once. */
enum { DU_R_LEFT_ALONE = 1u << 0, DU_R_PREV_ZERO = 1u << 1, DU_R_IRRADIANCE = 1u << 2, DU_R_BRIGHTNESS = 1u << 3, DU_R_DARKER = 1u << 4,
       DU_R_FLOOR = 1u << 5, DU_R_CAP = 1u << 8, DU_R_SIGN_ZERO = 1u << 11,           /* << channel: the floor gives the step, |delta| gives it, sign(step) == 0 */
       DU_R_CLAMP_ONE = 1u << 14, DU_R_CLAMP_ZERO = 1u << 17,                         /* << channel: saturate clamped the store */
       DU_R_NAN = 1u << 20,                                                           /* a NaN in sum, res or the store */
       DU_R_MAX_SHIFT = 21,                                                           /* two bits: 1 + the channel whose |delta| is the fmax of the three (0: not eased) */
       DU_R_SUM_NAN = 1u << 23 };
enum { DU_D_LEFT_ALONE = 1u << 0, DU_D_PREV_ZERO = 1u << 1, DU_D_SUMW_FLOOR = 1u << 2, DU_D_STORE_INF = 1u << 3, DU_D_STORE_NAN = 1u << 4, DU_D_STORE_SUBNORMAL = 1u << 5,
       DU_D_PREV_INF = 1u << 6, DU_D_PREV_NAN = 1u << 7, DU_D_CLIPPED_SHIFT = 16 };   /* bits 16..24: rays with !(|w| <= maxDistance) */

/* floorRule 0 leaves the 1/1024 rule out: only for the test that shows what it is for */
static void ease_radiance(const DuConsts* k, const float res[3], const float prev[3], int floorRule, float out[3], uint32_t* rules)
{
    if (prev[0] == 0.0f && prev[1] == 0.0f && prev[2] == 0.0f) { memcpy(out, res, 12); if (rules) *rules |= DU_R_PREV_ZERO; return; }
    float h = k->hysteresis;
    float delta[3] = { res[0] - prev[0], res[1] - prev[1], res[2] - prev[2] };
    if (rules) {
        const float m = max3(fabsf(delta[0]), fabsf(delta[1]), fabsf(delta[2]));
        *rules |= (fabsf(delta[0]) == m ? 1u : fabsf(delta[1]) == m ? 2u : fabsf(delta[2]) == m ? 3u : 0u) << DU_R_MAX_SHIFT;
    }
    if (max3(fabsf(delta[0]), fabsf(delta[1]), fabsf(delta[2])) > k->irradianceThreshold) { h = fmaxf(0.0f, h - 0.75f); if (rules) *rules |= DU_R_IRRADIANCE; }
    if (sqrtf(dot3(delta, delta)) > k->brightnessThreshold) { delta[0] = delta[0] * 0.25f; delta[1] = delta[1] * 0.25f; delta[2] = delta[2] * 0.25f; if (rules) *rules |= DU_R_BRIGHTNESS; }
    float step[3] = { (1.0f - h) * delta[0], (1.0f - h) * delta[1], (1.0f - h) * delta[2] };
    if (floorRule && max3(prev[0] + delta[0], prev[1] + delta[1], prev[2] + delta[2]) < max3(prev[0], prev[1], prev[2])) {
        const float t = 1.0f / 1024.0f;
        if (rules) {
            *rules |= DU_R_DARKER;
            for (int c = 0; c < 3; ++c) {
                const float floored = fmaxf(t, fabsf(step[c]));
                if (fminf(floored, fabsf(delta[c])) != floored) *rules |= DU_R_CAP << c;
                else if (floored != fabsf(step[c])) *rules |= DU_R_FLOOR << c;
                if (sign1(step[c]) == 0.0f) *rules |= DU_R_SIGN_ZERO << c;
            }
        }
        for (int c = 0; c < 3; ++c) step[c] = fminf(fmaxf(t, fabsf(step[c])), fabsf(delta[c])) * sign1(step[c]);
    }
    for (int c = 0; c < 3; ++c) out[c] = prev[c] + step[c];
}

void du_ease_radiance(const DuConsts* k, const float res[3], const float prev[3], int floorRule, float out[3]) { ease_radiance(k, res, prev, floorRule, out, NULL); }

uint32_t du_unorm10(float v) { return (uint32_t)rintf(saturate(v) * 1023.0f); }

/* source texel of border texel (tx, ty) of an N-square tile */
static void border_source(uint32_t tx, uint32_t ty, uint32_t N, uint32_t* sx, uint32_t* sy)
{
    const int edgeX = tx == 0u || tx == N - 1u, edgeY = ty == 0u || ty == N - 1u;
    if (edgeX && edgeY) { *sx = tx == 0u ? N - 2u : 1u; *sy = ty == 0u ? N - 2u : 1u; }
    else if (edgeY) { *sx = N - 1u - tx; *sy = ty == 0u ? 1u : N - 2u; }
    else { *sx = tx == 0u ? 1u : N - 2u; *sy = N - 1u - ty; }
}

/* 1 when the probe's tiles are left alone; else its ray directions */
static int blend_setup(const DuBlock* b, const uint16_t* data, const float* rays, uint32_t probe, int32_t c[3], float (*dir)[3])
{
    float pos[3];
    if (probe_of(&b->D, data, probe, c, pos)) return 1;
    uint32_t back = 0;
    for (uint32_t r = 0; r < DU_RAYS; ++r) {
        back += rays[((uint64_t)probe * DU_RAYS + r) * 4u + 3u] < 0.0f ? 1u : 0u;
        du_ray_direction(&b->k, r, dir[r]);
    }
    return back >= DU_BACKFACE_LIMIT;
}

/* irradiance: uint32 [slices][cz * 8][cx * 8], read and written */
static void blend_radiance(const DuBlock* b, const uint16_t* data, const float* rays, uint32_t* irradiance, uint32_t* rules)
{
    const DgDesc* D = &b->D;
    const uint32_t N = 8u, W = (uint32_t)D->probeCounts[0] * N, H = (uint32_t)D->probeCounts[2] * N;
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
                for (uint32_t r = 0; r < DU_RAYS; ++r) {
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
                if (rule)
                    for (int ch = 0; ch < 3; ++ch) {
                        if (out[ch] > 1.0f) *rule |= DU_R_CLAMP_ONE << ch;
                        if (out[ch] < 0.0f) *rule |= DU_R_CLAMP_ZERO << ch;
                        if (sum[ch] != sum[ch]) *rule |= DU_R_SUM_NAN | DU_R_NAN;
                        if (res[ch] != res[ch] || out[ch] != out[ch]) *rule |= DU_R_NAN;
                    }
                tile[ty * W + tx] = du_unorm10(out[0]) | du_unorm10(out[1]) << 10 | du_unorm10(out[2]) << 20 | 3u << 30;
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

void du_blend_radiance(const DuBlock* b, const uint16_t* data, const float* rays, uint32_t* irradiance) { blend_radiance(b, data, rays, irradiance, NULL); }
/* the same, and rules: uint32 [numProbes][6][6], one word of DU_R_* bits per interior texel */
void du_blend_radiance_rules(const DuBlock* b, const uint16_t* data, const float* rays, uint32_t* irradiance, uint32_t* rules) { blend_radiance(b, data, rays, irradiance, rules); }

/* distance: uint16 [slices][cz * 16][cx * 16][2], read and written */
static void blend_distance(const DuBlock* b, const uint16_t* data, const float* rays, uint16_t* distance, uint32_t* rules)
{
    const DgDesc* D = &b->D;
    const uint32_t N = 16u, W = (uint32_t)D->probeCounts[0] * N, H = (uint32_t)D->probeCounts[2] * N;
    const uint32_t probes = (uint32_t)D->probeCounts[0] * (uint32_t)D->probeCounts[1] * (uint32_t)D->probeCounts[2];
    const float maxDistance = 1.5f * sqrtf(dot3(D->probeSpacing, D->probeSpacing));
    for (uint32_t p = 0; p < probes; ++p) {
        int32_t c[3];
        float dir[DU_RAYS][3];
        if (blend_setup(b, data, rays, p, c, dir)) { if (rules) for (uint32_t t = 0; t < 196u; ++t) rules[(uint64_t)p * 196u + t] = DU_D_LEFT_ALONE; continue; }
        uint16_t* tile = distance + ((uint64_t)c[1] * W * H + (uint64_t)((uint32_t)c[2] * N) * W + (uint32_t)c[0] * N) * 2u;
        for (uint32_t ty = 1; ty <= N - 2u; ++ty)
            for (uint32_t tx = 1; tx <= N - 2u; ++tx) {
                float texelDir[3], sx = 0.0f, sy = 0.0f, sumW = 0.0f;
                du_texel_direction(tx - 1u, ty - 1u, N - 2u, texelDir);
                for (uint32_t r = 0; r < DU_RAYS; ++r) {
                    const float w = dg_pow(fmaxf(0.0f, dot3(texelDir, dir[r])), b->k.distanceExponent);
                    const float d = fminf(fabsf(rays[((uint64_t)p * DU_RAYS + r) * 4u + 3u]), maxDistance);
                    sx = sx + d * w; sy = sy + (d * d) * w;
                    sumW = sumW + w;
                }
                const float den = 2.0f * fmaxf(sumW, 1e-9f * 256.0f);
                const float rx = sx / den, ry = sy / den;
                uint16_t* t = tile + ((uint64_t)ty * W + tx) * 2u;
                const float px = half_to_float(t[0]), py = half_to_float(t[1]);
                const float h = (px == 0.0f && py == 0.0f) ? 0.0f : b->k.hysteresis;
                if (rules) {
                    uint32_t word = 0u, clipped = 0u;
                    for (uint32_t r = 0; r < DU_RAYS; ++r) clipped += !(fabsf(rays[((uint64_t)p * DU_RAYS + r) * 4u + 3u]) <= maxDistance) ? 1u : 0u;
                    if (px == 0.0f && py == 0.0f) word |= DU_D_PREV_ZERO;
                    if (!(sumW >= 1e-9f * 256.0f)) word |= DU_D_SUMW_FLOOR;
                    for (int ch = 0; ch < 2; ++ch) {
                        const uint32_t before = t[ch] & 0x7FFFu, after = sm_half_bits(lerp(ch ? ry : rx, ch ? py : px, h)) & 0x7FFFu;
                        if (before == 0x7C00u) word |= DU_D_PREV_INF;
                        if (before > 0x7C00u) word |= DU_D_PREV_NAN;
                        if (after == 0x7C00u) word |= DU_D_STORE_INF;
                        if (after > 0x7C00u) word |= DU_D_STORE_NAN;
                        if (after != 0u && after < 0x0400u) word |= DU_D_STORE_SUBNORMAL;
                    }
                    rules[(uint64_t)p * 196u + (ty - 1u) * 14u + (tx - 1u)] = word | clipped << DU_D_CLIPPED_SHIFT;
                }
                t[0] = sm_half_bits(lerp(rx, px, h)); t[1] = sm_half_bits(lerp(ry, py, h));
            }
        for (uint32_t ty = 0; ty < N; ++ty)
            for (uint32_t tx = 0; tx < N; ++tx) {
                if (tx >= 1u && tx <= N - 2u && ty >= 1u && ty <= N - 2u) continue;
                uint32_t sx, sy;
                border_source(tx, ty, N, &sx, &sy);
                memcpy(tile + ((uint64_t)ty * W + tx) * 2u, tile + ((uint64_t)sy * W + sx) * 2u, 4);
            }
    }
}

void du_blend_distance(const DuBlock* b, const uint16_t* data, const float* rays, uint16_t* distance) { blend_distance(b, data, rays, distance, NULL); }
/* the same, and rules: uint32 [numProbes][14][14], one word of DU_D_* bits per interior texel */
void du_blend_distance_rules(const DuBlock* b, const uint16_t* data, const float* rays, uint16_t* distance, uint32_t* rules) { blend_distance(b, data, rays, distance, rules); }
