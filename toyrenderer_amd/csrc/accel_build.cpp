// accel_build.cpp -- the host-side builder of the project's own ray tracing acceleration structure (include/trhip.h,
// "acceleration structure"): trhip_blas_build (one mesh's triangles, object space) and trhip_tlas_build (the
// topology over a scene's instances).  Plain C++: no device code, no device needed.  Both hosts (toyrenderer_amd/frame.py through
// ctypes, csrc/host/Scene.cpp) call these two functions; there is no second builder.
//
// ONE BUILDER over a list of boxes (struct Bvh below), a binary tree written in DEPTH-FIRST PREORDER:
//   node i's first child is node i + 1, its second child is nodes[i + 1].skip, and nodes[i].skip is the first node behind i's
//   subtree (numNodes for the last).  A walk needs no stack: box hit on an inner node -> i + 1, anything else -> skip.
//   Split: the longest axis of the box of the centroids (0.5 * lo + 0.5 * hi; ties take the lower axis), at its middle; primitives
//   with centroid < middle go left, in their order (std::stable_partition).  The heuristic DEGENERATES when a side receives less
//   than 1/8 of the primitives (or none), and it is not trusted below level kHeuristicLevels: then the slice is sorted by
//   (centroid on the axis, the next axis, the third, primitive id) -- a total order, so the result does not depend on the sort --
//   and cut in halves (MEDIAN split).
//   DEPTH BOUND: at most kHeuristicLevels = 24 heuristic levels, then every level halves the count, and a count below 2^32 is
//   at most leafCapacity after 32 halvings: depth <= kAccelMaxDepth = 56 for every input.  The builder checks it as it goes.
//   DETERMINISM: no hashing, no threads, no uninitialised bytes (every word of every node is written), sorts on total orders.
//   BOXES: a node's box is the union of its primitives' boxes, moved outward by `pad` on every side (see the callers).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "trhip_internal.h"

namespace
{

constexpr uint32_t kHeuristicLevels = 24, kAccelMaxDepth = 56, kBlasLeafCapacity = 4;
constexpr uint32_t kInner = 0xFFFFFFFFu;
constexpr float kBlasPad = 0x1p-16f;                            // relative to the mesh's largest |coordinate|; the TLAS leaves are padded by the refit (k_shadowmask.hip)

struct Box { float lo[3], hi[3]; };

struct Bvh
{
    const Box* boxes;
    uint32_t leafCapacity;
    float pad;
    std::vector<uint32_t> order;               // primitive ids, permuted in place
    trhip_accel_node* nodes;
    uint32_t capacity, numNodes = 0, depth = 0;
    bool overflow = false;

    float centroid(uint32_t prim, int axis) const { return 0.5f * boxes[prim].lo[axis] + 0.5f * boxes[prim].hi[axis]; }

    void build(uint32_t first, uint32_t count, uint32_t level)
    {
        if (numNodes >= capacity || level > kAccelMaxDepth) { overflow = true; return; }
        const uint32_t idx = numNodes++;
        depth = std::max(depth, level);
        Box b = boxes[order[first]], c;
        for (int a = 0; a < 3; ++a) c.lo[a] = c.hi[a] = centroid(order[first], a);
        for (uint32_t i = first + 1; i < first + count; ++i) {
            const Box& p = boxes[order[i]];
            for (int a = 0; a < 3; ++a) {
                b.lo[a] = std::min(b.lo[a], p.lo[a]); b.hi[a] = std::max(b.hi[a], p.hi[a]);
                const float m = centroid(order[i], a);
                c.lo[a] = std::min(c.lo[a], m); c.hi[a] = std::max(c.hi[a], m);
            }
        }
        trhip_accel_node& n = nodes[idx];
        for (int a = 0; a < 3; ++a) { n.lo[a] = b.lo[a] - pad; n.hi[a] = b.hi[a] + pad; }
        if (count <= leafCapacity) {
            n.leaf = leafCapacity == 1 ? order[first] : (first | (count - 1) << 30);
            n.skip = numNodes;
            return;
        }
        n.leaf = kInner;
        int axis = 0;
        for (int a = 1; a < 3; ++a) if (c.hi[a] - c.lo[a] > c.hi[axis] - c.lo[axis]) axis = a;
        uint32_t nl = 0;
        if (level < kHeuristicLevels) {
            const float mid = 0.5f * c.lo[axis] + 0.5f * c.hi[axis];
            auto it = std::stable_partition(order.begin() + first, order.begin() + first + count, [&](uint32_t p) { return centroid(p, axis) < mid; });
            nl = (uint32_t)(it - (order.begin() + first));
        }
        const uint32_t least = count / 8;
        if (nl == 0 || nl == count || nl < least || count - nl < least) {                           // degenerate, or below the heuristic levels: median
            const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
            std::sort(order.begin() + first, order.begin() + first + count, [&](uint32_t p, uint32_t q) {
                const float pk[3] = { centroid(p, axis), centroid(p, a1), centroid(p, a2) }, qk[3] = { centroid(q, axis), centroid(q, a1), centroid(q, a2) };
                for (int k = 0; k < 3; ++k) if (pk[k] != qk[k]) return pk[k] < qk[k];
                return p < q; });
            nl = count / 2;
        }
        build(first, nl, level + 1);
        build(first + nl, count - nl, level + 1);
        nodes[idx].skip = numNodes;
    }
};

bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

} // namespace

extern "C" {

uint32_t trhip_accel_max_depth(void) { return kAccelMaxDepth; }
uint32_t trhip_blas_leaf_capacity(void) { return kBlasLeafCapacity; }
uint32_t trhip_accel_max_nodes(uint32_t num_primitives) { return num_primitives ? 2u * num_primitives - 1u : 0u; }

int trhip_blas_build(const void* vertices, uint32_t vertex_stride, uint32_t num_vertices, const uint32_t* indices, uint32_t num_indices,
                     trhip_accel_node* nodes, uint32_t node_capacity, uint32_t* tri_order, uint32_t* num_nodes, uint32_t* num_tris, uint32_t* depth)
{
    TRHIP_REQUIRE(num_nodes && num_tris, "trhip_blas_build: num_nodes and num_tris are required");
    TRHIP_REQUIRE(num_indices % 3 == 0, "trhip_blas_build: %u indices are not whole triangles", num_indices);
    TRHIP_REQUIRE(vertex_stride >= 12 && vertex_stride % 4 == 0, "trhip_blas_build: vertex stride %u (needs a multiple of 4, at least 12)", vertex_stride);
    const uint32_t triangles = num_indices / 3;
    TRHIP_REQUIRE(triangles < (1u << 30) - 4u, "trhip_blas_build: %u triangles (the leaf word holds 30 bits)", triangles);
    TRHIP_REQUIRE(!triangles || (vertices && indices && nodes && tri_order), "trhip_blas_build: null array");
    std::vector<Box> boxes(triangles);
    Bvh b;
    b.order.reserve(triangles);
    float largest = 0.0f;
    for (uint32_t t = 0; t < triangles; ++t) {
        const float* v[3];
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            const uint32_t i = indices[3 * t + k];
            TRHIP_REQUIRE(i < num_vertices, "trhip_blas_build: index %u of triangle %u is outside the %u vertices", i, t, num_vertices);
            v[k] = (const float*)((const char*)vertices + (size_t)i * vertex_stride);
            ok = ok && finite3(v[k]);
        }
        if (!ok) continue;                                                                          // never hit (tests/shadowmask_ref.c): not in the tree
        for (int a = 0; a < 3; ++a) {
            boxes[t].lo[a] = std::min(v[0][a], std::min(v[1][a], v[2][a]));
            boxes[t].hi[a] = std::max(v[0][a], std::max(v[1][a], v[2][a]));
            largest = std::max(largest, std::max(std::fabs(boxes[t].lo[a]), std::fabs(boxes[t].hi[a])));
        }
        b.order.push_back(t);
    }
    const uint32_t n = (uint32_t)b.order.size();
    *num_tris = n;
    *num_nodes = 0;
    if (depth) *depth = 0;
    if (!n) return TRHIP_OK;
    TRHIP_REQUIRE(node_capacity >= trhip_accel_max_nodes(n), "trhip_blas_build: room for %u nodes, %u triangles need %u", node_capacity, n, trhip_accel_max_nodes(n));
    b.boxes = boxes.data(); b.leafCapacity = kBlasLeafCapacity; b.pad = kBlasPad * largest; b.nodes = nodes; b.capacity = node_capacity;
    b.build(0, n, 0);
    TRHIP_REQUIRE(!b.overflow, "trhip_blas_build: the tree left its depth or node bound (a bug of the builder)");
    memcpy(tri_order, b.order.data(), (size_t)n * 4);
    *num_nodes = b.numNodes;
    if (depth) *depth = b.depth;
    return TRHIP_OK;
}

int trhip_tlas_build(const void* instances, uint32_t num_instances, const uint32_t* flags, const trhip_blas_header* headers, uint32_t num_meshes,
                     const trhip_accel_node* blas_nodes, uint32_t num_blas_nodes, trhip_accel_node* nodes, uint32_t node_capacity, trhip_tlas_instance* records,
                     uint32_t* level_nodes, uint32_t* level_offsets, uint32_t* num_nodes, uint32_t* num_levels)
{
    TRHIP_REQUIRE(num_nodes && num_levels && level_offsets, "trhip_tlas_build: num_nodes, num_levels and level_offsets are required");
    TRHIP_REQUIRE(!num_instances || (instances && flags && records), "trhip_tlas_build: null array");
    const interop::BasePassInstanceConstants* inst = (const interop::BasePassInstanceConstants*)instances;
    std::vector<Box> boxes(num_instances);
    Bvh b;
    for (uint32_t i = 0; i < num_instances; ++i) {
        memset(&records[i], 0, sizeof records[i]);
        records[i].flags = flags[i] & 3u;
        records[i].leaf_node = kInner;
        const uint32_t mesh = inst[i].m_MeshDataIdx;
        if (!records[i].flags || mesh >= num_meshes || !headers[mesh].num_nodes || headers[mesh].node_offset >= num_blas_nodes) continue;
        const trhip_accel_node& root = blas_nodes[headers[mesh].node_offset];
        Box w;
        bool ok = true;
        for (int c = 0; c < 8; ++c) {                                                               // the rest box: topology only, so plain float arithmetic
            const float p[3] = { c & 1 ? root.hi[0] : root.lo[0], c & 2 ? root.hi[1] : root.lo[1], c & 4 ? root.hi[2] : root.lo[2] };
            for (int a = 0; a < 3; ++a) {
                const float x = p[0] * inst[i].m_WorldMatrix.m[0][a] + p[1] * inst[i].m_WorldMatrix.m[1][a] + p[2] * inst[i].m_WorldMatrix.m[2][a] + inst[i].m_WorldMatrix.m[3][a];
                ok = ok && std::isfinite(x);
                w.lo[a] = c ? std::min(w.lo[a], x) : x; w.hi[a] = c ? std::max(w.hi[a], x) : x;
            }
        }
        if (!ok)                                                                                    // still a leaf (the refit decides its box); placed at the origin
            for (int a = 0; a < 3; ++a) w.lo[a] = w.hi[a] = 0.0f;
        boxes[i] = w;
        b.order.push_back(i);
    }
    const uint32_t n = (uint32_t)b.order.size();
    *num_nodes = 0; *num_levels = 0; level_offsets[0] = 0;
    if (!n) return TRHIP_OK;
    TRHIP_REQUIRE(nodes && level_nodes, "trhip_tlas_build: null array");
    TRHIP_REQUIRE(node_capacity >= trhip_accel_max_nodes(n), "trhip_tlas_build: room for %u nodes, %u instances need %u", node_capacity, n, trhip_accel_max_nodes(n));
    b.boxes = boxes.data(); b.leafCapacity = 1; b.pad = 0.0f; b.nodes = nodes; b.capacity = node_capacity;
    b.build(0, n, 0);
    TRHIP_REQUIRE(!b.overflow, "trhip_tlas_build: the tree left its depth or node bound (a bug of the builder)");
    // heights, children before parents (a child's index is larger than its parent's); inner nodes grouped by height for the refit
    std::vector<uint32_t> height(b.numNodes, 0);
    uint32_t top = 0;
    for (uint32_t i = b.numNodes; i-- > 0;) {
        if (nodes[i].leaf != kInner) { records[nodes[i].leaf].leaf_node = i; continue; }
        height[i] = 1 + std::max(height[i + 1], height[nodes[i + 1].skip]);
        top = std::max(top, height[i]);
    }
    std::vector<uint32_t> count(top + 2, 0);
    for (uint32_t i = 0; i < b.numNodes; ++i) if (height[i]) ++count[height[i]];
    for (uint32_t h = 1; h <= top; ++h) level_offsets[h] = level_offsets[h - 1] + count[h];
    std::vector<uint32_t> at(level_offsets, level_offsets + top + 1);
    for (uint32_t i = 0; i < b.numNodes; ++i) if (height[i]) level_nodes[at[height[i] - 1]++] = i;
    *num_nodes = b.numNodes;
    *num_levels = top;
    return TRHIP_OK;
}

} // extern "C"
