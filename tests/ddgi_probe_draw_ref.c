/* ddgi_probe_draw_ref.c -- the definition of "giprobevisualization_CS_LoadGIProbes" and "giprobevisualization_PS_VisualizeGIProbes"
 * (csrc/k_giprobedraw.hip): the probes of the live DDGI volume as positions and states, and the culled probes drawn as small
 * spheres shaded with their own irradiance, depth-tested against the scene.  The rasteriser has no source to restate: its rules
 * are this build's convention, stated here independently of the kernel and followed by it operation for operation.
 * IEEE binary32, no contraction (the library is compiled with -ffp-contract=off), fmaf only where written.
 *
 * LOAD.   probe p of cx * cy * cz: x = p % cx, z = (p / cx) % cz, y = p / (cx * cz); position = ((spacing * (float)c) - ext) + origin
 *         with ext = (spacing * (float)(counts - 1)) * 0.5f, + data.xyz * spacing when flags bit 0 is set (ddgi_ref.c's probe_pos);
 *         state = data.w when flags bit 1 is set, else 0.0f.
 * SPHERE. CommonResources.cpp:40-102 with tessellation 6: 7 rings of 13 vertices, 156 triangles, winding reversed.  Every angle is a
 *         multiple of pi / 6, so the sines are EXACTLY S = { 0, 1/2, RN(sqrt(3) / 2), 1, ... } with the quadrant's sign, no libm:
 *         ring i has dy = S[(i + 9) % 12], dxz = S[i]; column j has dx = S[j % 12], dz = S[(j + 3) % 12]; normal = (dx * dxz, dy,
 *         dz * dxz), binary32 products; position = normal * 0.5f; texcoord = (1 - (float)j / 12.0f, 1 - (float)i / 6.0f).  Cell (i, j),
 *         n = (j + 1) % 13: triangles (i*13 + n, (i+1)*13 + j, i*13 + j) and ((i+1)*13 + n, (i+1)*13 + j, i*13 + n).  The poles and the
 *         seam column (j = 12, n = 0: columns 12 and 0 coincide) are exactly degenerate; 120 triangles have area.
 * VERTEX. world = probePos + (radius * normal) (product rounded, then the sum); clip_j = fmaf(z, M[2][j], fmaf(y, M[1][j], x * M[0][j]))
 *         + M[3][j]; sx = fmaf(clip.x / w, W / 2, W / 2), sy = fmaf(-(clip.y / w), H / 2, H / 2), depth = clip.z / w.
 * TRIANGLE. dropped if any vertex has w <= near (no clipping).  edge(a, b, p) = fmaf(b.x - a.x, p.y - a.y, -((b.y - a.y) * (p.x - a.x)));
 *         area = edge(v0, v1, v2).  THE SIGN: with y pointing down the screen and a projection that does not mirror, the outward
 *         faces of the sphere above have area < 0.  They are the front faces: a triangle is drawn iff area < 0.
 * COVERAGE. at the pixel centre (px + 0.5, py + 0.5): e0 = -edge(v1, v2, p), e1 = -edge(v2, v0, p), e2 = -edge(v0, v1, p); covered iff
 *         all three >= 0 and den = (e0 + e1) + e2 > 0; d = fmaf(e2, d2, fmaf(e1, d1, e0 * d0)) / den.
 * DEPTH.  a sample survives iff d > 0 and d >= depth[texel] (GREATER_OR_EQUAL, reversed Z).  Per texel the largest
 *         (bits(d) << 32) | instance << 8 | triangle wins; 0 = no winner.
 * SHADE.  q_i = e_i / w_i, s = (q0 + q1) + q2, world = fmaf(q2, world2, fmaf(q1, world1, q0 * world0)) / s; probe = min(instanceToProbe
 *         [instance], numProbes - 1); pp = its position from the volume (as LOAD); dir = (world - pp) / sqrtf(dot3(.)); o = dg_oct(dir);
 *         e = dg_pow(dg_fetch_irradiance(probe, o), gamma * 0.5f); c = ((e * e) * 2.0f) * 1.0989f; colour = uint(saturate(c) * 255.0f +
 *         0.5f) per channel, R in the low byte, alpha 255; depth[texel] = d.  A texel without a winner keeps both.
 */
#include <stdlib.h>

#include "ddgi_ref.c"

typedef struct
{
    float worldToClip[4][4];
    float cameraDirection[3];
    float probeRadius;
    float nearPlane;
    uint32_t pad[3];
} PdConsts;

enum { PD_WON, PD_LOST_TO_SCENE, PD_MULTI_INSTANCE, PD_TIE, PD_NEAR_DROPPED, PD_BACK_CULLED, PD_NO_AREA, PD_CLIP_LEFT, PD_CLIP_RIGHT, PD_CLIP_TOP, PD_CLIP_BOTTOM,
       PD_NO_CENTRE, PD_COUNTERS };

#define PD_RING 13u
#define PD_VERTICES 91u
#define PD_INDICES 468u

/* vertices: 91 x (position 3, normal 3, texcoord 2) floats; indices: 468 */
void pd_unit_sphere(float* vertices, uint32_t* indices)
{
    const float R = 0x1.bb67aep-1f;                                    /* RN(sqrt(3) / 2) */
    const float S[12] = { 0.0f, 0.5f, R, 1.0f, R, 0.5f, 0.0f, -0.5f, -R, -1.0f, -R, -0.5f };
    for (uint32_t i = 0; i <= 6u; ++i) {
        const float dy = S[(i + 9u) % 12u], dxz = S[i];
        for (uint32_t j = 0; j <= 12u; ++j) {
            float* v = vertices + (i * PD_RING + j) * 8u;
            const float n[3] = { S[j % 12u] * dxz, dy, S[(j + 3u) % 12u] * dxz };
            for (int a = 0; a < 3; ++a) { v[a] = n[a] * 0.5f; v[3 + a] = n[a]; }
            v[6] = 1.0f - (float)j / 12.0f;
            v[7] = 1.0f - (float)i / 6.0f;
        }
    }
    uint32_t* t = indices;
    for (uint32_t i = 0; i < 6u; ++i)
        for (uint32_t j = 0; j <= 12u; ++j) {
            const uint32_t n = (j + 1u) % PD_RING;
            *t++ = i * PD_RING + n; *t++ = (i + 1u) * PD_RING + j; *t++ = i * PD_RING + j;
            *t++ = (i + 1u) * PD_RING + n; *t++ = (i + 1u) * PD_RING + j; *t++ = i * PD_RING + n;
        }
}

/* LOAD of probe p (tests/ddgi_ref.c probe_at) */
static void pd_probe(const DgDesc* D, const uint16_t* data, uint32_t p, int32_t c[3], float pos[3], float* state)
{
    float w;
    probe_at(D, data, p, c, pos, &w);
    *state = (D->flags & 2u) ? w : 0.0f;
}

void pd_load_probes(const DgDesc* D, const uint16_t* data, float* positions, float* states)
{
    const uint32_t n = (uint32_t)D->probeCounts[0] * (uint32_t)D->probeCounts[1] * (uint32_t)D->probeCounts[2];
    for (uint32_t p = 0; p < n; ++p) {
        int32_t c[3];
        pd_probe(D, data, p, c, positions + 3u * p, states + p);
    }
}

typedef struct { float world[3], sx, sy, d, w; } PdVertex;

static PdVertex pd_vertex(const PdConsts* k, const float pos[3], const float normal[3], uint32_t W, uint32_t H)
{
    PdVertex v;
    float clip[4];
    for (int a = 0; a < 3; ++a) v.world[a] = pos[a] + (k->probeRadius * normal[a]);
    for (int j = 0; j < 4; ++j)
        clip[j] = fmaf(v.world[2], k->worldToClip[2][j], fmaf(v.world[1], k->worldToClip[1][j], v.world[0] * k->worldToClip[0][j])) + k->worldToClip[3][j];
    const float halfW = 0.5f * (float)W, halfH = 0.5f * (float)H;
    v.w = clip[3];
    v.sx = fmaf(clip[0] / v.w, halfW, halfW);
    v.sy = fmaf(-(clip[1] / v.w), halfH, halfH);
    v.d = clip[2] / v.w;
    return v;
}

static uint32_t pd_unorm8(float c) { return (uint32_t)(saturate(c) * 255.0f + 0.5f); }

static uint32_t pd_shade(const PdConsts* k, const DgDesc* D, const uint16_t* data, const uint32_t* irradiance, uint32_t probe, const PdVertex* v0, const PdVertex* v1,
                         const PdVertex* v2, float e0, float e1, float e2)
{
    (void)k;
    const float q0 = e0 / v0->w, q1 = e1 / v1->w, q2 = e2 / v2->w;
    const float s = (q0 + q1) + q2;
    float world[3], pp[3], dir[3], state, o[2], rgb[3];
    int32_t c[3];
    for (int a = 0; a < 3; ++a) world[a] = fmaf(q2, v2->world[a], fmaf(q1, v1->world[a], q0 * v0->world[a])) / s;
    const uint32_t n = (uint32_t)D->probeCounts[0] * (uint32_t)D->probeCounts[1] * (uint32_t)D->probeCounts[2];
    pd_probe(D, data, probe < n - 1u ? probe : n - 1u, c, pp, &state);
    for (int a = 0; a < 3; ++a) dir[a] = world[a] - pp[a];
    const float len = sqrtf(dot3(dir, dir));
    for (int a = 0; a < 3; ++a) dir[a] = dir[a] / len;
    dg_oct(dir, o);
    dg_fetch_irradiance(D, irradiance, c, o, rgb);
    uint32_t word = 0xFF000000u;
    for (int ch = 0; ch < 3; ++ch) {
        const float e = dg_pow(rgb[ch], D->probeIrradianceEncodingGamma * 0.5f);
        word |= pd_unorm8(((e * e) * 2.0f) * 1.0989f) << (8 * ch);
    }
    return word;
}

/* depth and color: W * H, read and written; winners: W * H, written (0 = none); counters: PD_COUNTERS, added to (NULL: none).
 * positions / instanceToProbe: instanceCount entries (the caller clamps m_InstanceCount as the pass does). */
void pd_draw(const PdConsts* k, const DgDesc* D, const uint16_t* data, const uint32_t* irradiance, const float* positions, const uint32_t* instanceToProbe,
             uint32_t instanceCount, const float* vertices, uint32_t numVertices, const uint32_t* indices, uint32_t numTriangles, uint32_t W, uint32_t H, float* depth,
             uint32_t* color, uint64_t* winners, uint64_t* counters)
{
    uint64_t none[PD_COUNTERS];
    uint64_t* n = counters ? counters : none;
    const uint64_t texels = (uint64_t)W * H;
    /* per texel, for the counters: bit 0 a sample lost to the scene, bit 1 two instances survived, bit 2 a tie with the winner */
    uint8_t* seen = (uint8_t*)calloc(texels, 1);
    uint32_t* firstInstance = (uint32_t*)malloc(texels * 4u);
    memset(winners, 0, texels * 8u);
    memset(firstInstance, 0xFF, texels * 4u);
    for (int pass = 0; pass < 2; ++pass)                                  /* 0: the winners; 1: which texels the tie rule decided */
        for (uint32_t inst = 0; inst < instanceCount; ++inst) {
            uint64_t samples = 0, drawn = 0;
            int left = 0, right = 0, top = 0, bottom = 0;
            for (uint32_t t = 0; t < numTriangles; ++t) {
                const uint32_t ia = indices[3u * t], ib = indices[3u * t + 1u], ic = indices[3u * t + 2u];
                if (ia >= numVertices || ib >= numVertices || ic >= numVertices) continue;
                const PdVertex v0 = pd_vertex(k, positions + 3u * inst, vertices + 8u * ia + 3u, W, H), v1 = pd_vertex(k, positions + 3u * inst, vertices + 8u * ib + 3u, W, H),
                               v2 = pd_vertex(k, positions + 3u * inst, vertices + 8u * ic + 3u, W, H);
                if (!(v0.w > k->nearPlane && v1.w > k->nearPlane && v2.w > k->nearPlane)) { n[PD_NEAR_DROPPED] += pass == 0; continue; }
                const float area = edge(v0.sx, v0.sy, v1.sx, v1.sy, v2.sx, v2.sy);
                if (!(area < 0.0f)) { n[area > 0.0f ? PD_BACK_CULLED : PD_NO_AREA] += pass == 0; continue; }
                const float minx = fminf(fminf(v0.sx, v1.sx), v2.sx), maxx = fmaxf(fmaxf(v0.sx, v1.sx), v2.sx);
                const float miny = fminf(fminf(v0.sy, v1.sy), v2.sy), maxy = fmaxf(fmaxf(v0.sy, v1.sy), v2.sy);
                /* a generous box around the triangle: every pixel centre outside it fails an edge */
                const float lox = fmaxf(floorf(minx) - 1.0f, 0.0f), hix = fminf(ceilf(maxx) + 1.0f, (float)(W - 1u));
                const float loy = fmaxf(floorf(miny) - 1.0f, 0.0f), hiy = fminf(ceilf(maxy) + 1.0f, (float)(H - 1u));
                if (!(hix >= lox && hiy >= loy)) continue;                 /* off screen, or a NaN */
                ++drawn;
                left |= minx < 0.0f; right |= maxx > (float)W; top |= miny < 0.0f; bottom |= maxy > (float)H;
                for (uint32_t py = (uint32_t)loy; py <= (uint32_t)hiy; ++py)
                    for (uint32_t px = (uint32_t)lox; px <= (uint32_t)hix; ++px) {
                        const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
                        const float e0 = -edge(v1.sx, v1.sy, v2.sx, v2.sy, cx, cy), e1 = -edge(v2.sx, v2.sy, v0.sx, v0.sy, cx, cy),
                                    e2 = -edge(v0.sx, v0.sy, v1.sx, v1.sy, cx, cy);
                        if (!(e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f)) continue;
                        const float den = (e0 + e1) + e2;
                        if (!(den > 0.0f)) continue;
                        const float d = fmaf(e2, v2.d, fmaf(e1, v1.d, e0 * v0.d)) / den;
                        if (!(d > 0.0f)) continue;
                        ++samples;
                        const uint64_t i = (uint64_t)py * W + px;
                        if (!(d >= depth[i])) { seen[i] |= 1u; continue; }
                        const uint64_t word = (uint64_t)bits_of(d) << 32 | (uint64_t)(inst << 8 | t);
                        if (pass == 0) {
                            if (firstInstance[i] == 0xFFFFFFFFu) firstInstance[i] = inst;
                            else if (firstInstance[i] != inst) seen[i] |= 2u;
                            if (word > winners[i]) winners[i] = word;
                        } else if (word != winners[i] && (word >> 32) == (winners[i] >> 32)) {
                            seen[i] |= 4u;
                        }
                    }
            }
            if (pass == 0) {
                n[PD_CLIP_LEFT] += left; n[PD_CLIP_RIGHT] += right; n[PD_CLIP_TOP] += top; n[PD_CLIP_BOTTOM] += bottom;
                n[PD_NO_CENTRE] += drawn != 0 && samples == 0;
            }
        }
    /* the resolve: depth is read by the test above and written only here */
    for (uint64_t i = 0; i < texels; ++i) {
        n[PD_LOST_TO_SCENE] += (seen[i] & 1u) != 0; n[PD_MULTI_INSTANCE] += (seen[i] & 2u) != 0; n[PD_TIE] += (seen[i] & 4u) != 0;
        if (!winners[i]) continue;
        ++n[PD_WON];
        const uint32_t payload = (uint32_t)winners[i], inst = payload >> 8, t = payload & 255u;
        const uint32_t px = (uint32_t)(i % W), py = (uint32_t)(i / W);
        const uint32_t ia = indices[3u * t], ib = indices[3u * t + 1u], ic = indices[3u * t + 2u];
        const PdVertex v0 = pd_vertex(k, positions + 3u * inst, vertices + 8u * ia + 3u, W, H), v1 = pd_vertex(k, positions + 3u * inst, vertices + 8u * ib + 3u, W, H),
                       v2 = pd_vertex(k, positions + 3u * inst, vertices + 8u * ic + 3u, W, H);
        const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
        const float e0 = -edge(v1.sx, v1.sy, v2.sx, v2.sy, cx, cy), e1 = -edge(v2.sx, v2.sy, v0.sx, v0.sy, cx, cy), e2 = -edge(v0.sx, v0.sy, v1.sx, v1.sy, cx, cy);
        color[i] = pd_shade(k, D, data, irradiance, instanceToProbe[inst], &v0, &v1, &v2, e0, e1, e2);
        depth[i] = float_of((uint32_t)(winners[i] >> 32));
    }
    free(seen); free(firstInstance);
}
