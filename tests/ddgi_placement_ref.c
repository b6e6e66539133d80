/* ddgi_placement_ref.c -- the definition of "giprobetrace_CS_ProbeTraceFixedRays", "ProbeRelocationCS_DDGIProbeRelocationCS" and
 * "ProbeClassificationCS_DDGIProbeClassificationCS" (csrc/k_giprobeplacement.hip, csrc/ddgi_update.hip.h: fixedRayDirection), which
 * repeat the functions below word for word.  Compile with gcc -O2 -ffp-contract=off (tests/ddgi_placement_ref.py).
 *
 * The RTXGI SDK is not part of this project: the three passes are the project's own statement of the published probe relocation
 * and classification, and this file is what the tests pin.  It includes tests/ddgi_update_ref.c for the closest hit (closest():
 * brute force, or the one walk of tests/shadowmask_ref.c), a probe's position and the constant block.
 *
 * CONVENTION.  binary32 throughout, no contraction, fmaf only in dot3, / and sqrtf correctly rounded; S the spacing.
 *   fixed ray i   of 32: f = (float)i * 0.618034f; phi = RN(2 pi) * (f - floorf(f)); c = 1.0f - (float)(2 * i + 1) / 32.0f; s =
 *                 sqrtf(saturate(1.0f - c * c)); d = (cos(phi) * s, sin(phi) * s, c) with the soft sine and cosine; direction = d /
 *                 sqrtf(dot3(d, d)): du_ray_direction's words with 32 for 256 and no rotation;
 *   fixed trace   every probe, whatever its state: origin probe_pos, TMin 0, TMax maxRayDistance; a miss stores 1e27f, a front face t,
 *                 a back face -0.2f * t;
 *   relocation    relocate_probe below; classification: classify_probe below.  csrc/k_giprobeplacement.hip ("CONVENTION") states both
 *                 in prose.
 * DuConsts (tests/ddgi_update_ref.c) still calls the block's last three words pad: pad[0] holds probeMinFrontfaceDistance and pad[1]
 * probeFixedRayBackfaceThreshold, both binary32. */
#include "ddgi_update_ref.c"

#define DP_FIXED_RAYS 32u

static float min_frontface_distance(const DuConsts* k) { float f; memcpy(&f, &k->pad[0], 4); return f; }
static float fixed_ray_backface_threshold(const DuConsts* k) { float f; memcpy(&f, &k->pad[1], 4); return f; }

/* which branch relocation took for a probe */
enum { DP_A_TAKEN, DP_A_REFUSED, DP_B_TAKEN, DP_B_REFUSED, DP_B_NO_FAR, DP_C_TAKEN, DP_C_REFUSED, DP_C_ZERO_OFFSET, DP_NO_MOVE, DP_BRANCHES };
/* why classification chose a probe's state */
enum { DP_ACTIVE, DP_OFF_BACKFACES, DP_OFF_NOTHING_NEAR, DP_REASONS };

void dp_fixed_direction(uint32_t i, float out[3])
{
    const float f = (float)i * 0.618034f, phi = 0x1.921fb6p+2f * (f - floorf(f));
    const float c = 1.0f - (float)(2u * i + 1u) / (float)DP_FIXED_RAYS, s = sqrtf(saturate(1.0f - c * c));
    const float d[3] = { sincos_soft(phi, 1) * s, sincos_soft(phi, 0) * s, c };
    normalize3(d, out);
}

/* distances float[numProbes * 32]; mode 0: brute force, 1: the walk */
void dp_trace_fixed(const DuBlock* b, const SmScene* s, const uint16_t* data, int mode, float* distances)
{
    const uint32_t probes = (uint32_t)b->D.probeCounts[0] * (uint32_t)b->D.probeCounts[1] * (uint32_t)b->D.probeCounts[2];
    for (uint32_t p = 0; p < probes; ++p) {
        int32_t c[3];
        float pos[3];
        probe_of(&b->D, data, p, c, pos);                                /* the state is not looked at */
        const F3 O = { pos[0], pos[1], pos[2] };
        for (uint32_t r = 0; r < DP_FIXED_RAYS; ++r) {
            uint64_t ties = 0;
            float dir[3];
            dp_fixed_direction(r, dir);
            const F3 Dir = { dir[0], dir[1], dir[2] };
            const DuHit hit = closest(s, O, Dir, 0.0f, b->k.maxRayDistance, mode, &ties);
            distances[(uint64_t)p * DP_FIXED_RAYS + r] = hit.inst == 0xFFFFFFFFu ? 1e27f : (hit.front ? hit.t : -0.2f * hit.t);
        }
    }
}

/* One probe: d its 32 distances, dir the 32 fixed directions, h its data.xyz as binary16 words (read and written).  Returns the
 * branch taken. */
static int relocate_probe(const DuConsts* k, const float S[3], const float* d, float (*dir)[3], uint16_t h[3])
{
    const float minFront = min_frontface_distance(k);
    float o[3] = { half_to_float(h[0]) * S[0], half_to_float(h[1]) * S[1], half_to_float(h[2]) * S[2] };
    float closestBack = 1e27f, closestFront = 1e27f, farthestFront = 0.0f;
    int iBack = -1, iFront = -1, iFar = -1, branch = DP_NO_MOVE, move = 0;
    uint32_t back = 0;
    for (int i = 0; i < (int)DP_FIXED_RAYS; ++i) {
        const float di = d[i];
        if (di < 0.0f) {
            ++back;
            const float undone = di * -5.0f;
            if (undone < closestBack) { closestBack = undone; iBack = i; }
        }
        else if (di < closestFront) { closestFront = di; iFront = i; }
        else if (di > farthestFront) { farthestFront = di; iFar = i; }
    }
    float full[3] = { o[0], o[1], o[2] };
    if (iBack != -1 && (float)back / (float)DP_FIXED_RAYS > fixed_ray_backface_threshold(k)) {
        const float s = closestBack + minFront * 0.5f;
        for (int a = 0; a < 3; ++a) full[a] = o[a] + dir[iBack][a] * s;
        move = 1; branch = DP_A_TAKEN;
    } else if (closestFront < minFront) {
        if (iFront != -1 && iFar != -1 && dot3(dir[iFront], dir[iFar]) <= 0.5f) {
            const float s = fminf(farthestFront, 1.0f);
            for (int a = 0; a < 3; ++a) full[a] = o[a] + dir[iFar][a] * s;
            move = 1; branch = DP_B_TAKEN;
        } else branch = DP_B_NO_FAR;
    } else if (closestFront > minFront) {
        const float len = sqrtf(dot3(o, o));
        if (len > 0.0f) {
            const float inv = -1.0f / len, s = fminf(closestFront - minFront, len);
            for (int a = 0; a < 3; ++a) full[a] = o[a] + (o[a] * inv) * s;
            move = 1; branch = DP_C_TAKEN;
        } else branch = DP_C_ZERO_OFFSET;
    }
    if (move) {
        const float n[3] = { full[0] / S[0], full[1] / S[1], full[2] / S[2] };
        if (dot3(n, n) < 0.2025f) { o[0] = full[0]; o[1] = full[1]; o[2] = full[2]; }
        else branch += 1;                                                /* X_TAKEN -> X_REFUSED */
    }
    for (int a = 0; a < 3; ++a) h[a] = sm_half_bits(o[a] / S[a]);
    return branch;
}

/* One probe's state, 0 (active) or 1; reason: one of DP_ACTIVE, DP_OFF_BACKFACES, DP_OFF_NOTHING_NEAR. */
static float classify_probe(const DuConsts* k, const float S[3], const float* d, float (*dir)[3], int* reason)
{
    uint32_t back = 0;
    for (int i = 0; i < (int)DP_FIXED_RAYS; ++i) back += d[i] < 0.0f ? 1u : 0u;
    if ((float)back / (float)DP_FIXED_RAYS > fixed_ray_backface_threshold(k)) { *reason = DP_OFF_BACKFACES; return 1.0f; }
    for (int i = 0; i < (int)DP_FIXED_RAYS; ++i) {
        if (d[i] < 0.0f) continue;
        float plane = 1e27f;
        for (int a = 0; a < 3; ++a) {
            const float m = fabsf(dir[i][a]);
            plane = fminf(plane, m == 0.0f ? 1e27f : S[a] / fmaxf(m, 1e-6f));
        }
        if (d[i] <= plane) { *reason = DP_ACTIVE; return 0.0f; }
    }
    *reason = DP_OFF_NOTHING_NEAR;
    return 1.0f;
}

static void fixed_directions(float (*dir)[3])
{
    for (uint32_t r = 0; r < DP_FIXED_RAYS; ++r) dp_fixed_direction(r, dir[r]);
}

/* data: uint16 [slices][cz][cx][4], read and written; branches: uint32[numProbes] or NULL */
void dp_relocate(const DuBlock* b, const float* distances, uint16_t* data, uint32_t* branches)
{
    const uint32_t probes = (uint32_t)b->D.probeCounts[0] * (uint32_t)b->D.probeCounts[1] * (uint32_t)b->D.probeCounts[2];
    float dir[DP_FIXED_RAYS][3];
    fixed_directions(dir);
    for (uint32_t p = 0; p < probes; ++p) {
        int32_t c[3];
        probe_coords(&b->D, p, c);
        uint16_t* t = data + (((uint64_t)c[1] * (uint32_t)b->D.probeCounts[2] + (uint32_t)c[2]) * (uint32_t)b->D.probeCounts[0] + (uint32_t)c[0]) * 4u;
        const int branch = relocate_probe(&b->k, b->D.probeSpacing, distances + (uint64_t)p * DP_FIXED_RAYS, dir, t);
        if (branches) branches[p] = (uint32_t)branch;
    }
}

void dp_classify(const DuBlock* b, const float* distances, uint16_t* data, uint32_t* reasons)
{
    const uint32_t probes = (uint32_t)b->D.probeCounts[0] * (uint32_t)b->D.probeCounts[1] * (uint32_t)b->D.probeCounts[2];
    float dir[DP_FIXED_RAYS][3];
    fixed_directions(dir);
    for (uint32_t p = 0; p < probes; ++p) {
        int32_t c[3];
        int reason;
        probe_coords(&b->D, p, c);
        uint16_t* t = data + (((uint64_t)c[1] * (uint32_t)b->D.probeCounts[2] + (uint32_t)c[2]) * (uint32_t)b->D.probeCounts[0] + (uint32_t)c[0]) * 4u;
        t[3] = sm_half_bits(classify_probe(&b->k, b->D.probeSpacing, distances + (uint64_t)p * DP_FIXED_RAYS, dir, &reason));
        if (reasons) reasons[p] = (uint32_t)reason;
    }
}

/* binary16(half_to_float(h) * s / s): what relocation stores for a probe that does not move */
uint16_t dp_round_trip(uint16_t h, float s) { return sm_half_bits((half_to_float(h) * s) / s); }
