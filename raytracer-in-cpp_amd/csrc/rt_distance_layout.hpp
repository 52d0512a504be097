// rt_distance_layout.hpp -- the arithmetic of the closest-point query (rt_closest_points_device; DESIGN.md §5, Closest points) that the host
// and k_nearest share: the one definition of the point-triangle routine (rt_closest_point_triangle calls it, the kernel calls it), the lower
// bound of a point's distance to a box, the pruning rule with its slack, the records of the query's own bounds (a vertex box per node, a
// vertex record per leaf reference), how a candidate replaces the best so far, the bottom-up pass over the node boxes, a one-point walk of
// the tree from these parts (tools/distance_check.cpp holds it against brute force) and the argument rule of the calls.  Header-only and
// free of HIP.  Every float operation stands on its own (the library and the check are built with -ffp-contract=off).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "rt_query_chunks.hpp"

namespace rtamd {

// ---- the records -------------------------------------------------------------------------------------------------------------------------
// One per leaf reference, in the order of leaf_tris: the world-space vertices of the face as uploaded (rt_scene.tri_verts) and its id.
// 48 B = three 16-byte loads.
struct alignas(16) NearTri {
    float a[3], b[3], c[3];
    uint32_t face;
    uint32_t pad[2];
};
static_assert(sizeof(NearTri) == 48, "NearTri must be 48 bytes");
// One per node, in the order of the node array: the exact box of the vertices of every face referenced below the node (a min / max of
// floats: no rounding, no inflation; lo > hi: nothing is referenced below) and the node's own first / count_flags (rt_node).  32 B.
struct alignas(32) NearNode {
    float lo[3];
    uint32_t first;
    float hi[3];
    uint32_t count_flags;
};
static_assert(sizeof(NearNode) == 32, "NearNode must be 32 bytes");
// One more NearNode per 64-record chunk of a leaf, numbered as the upload numbers a leaf's chunks (leaf_chunk0[node] + c): the box of the
// chunk's vertices, first = its first record, count_flags = its records.  A leaf's records are in the Morton order of leaf_tris, so a chunk
// is a compact part of a leaf whose own box is wide (the reference's builder misfiles triangles: they stick out of their cells).
constexpr uint32_t kNearChunk = 64u;
RT_QUERY_HD uint32_t near_chunks(const uint32_t records) { return (records + kNearChunk - 1u) / kNearChunk; }
RT_QUERY_HD uint32_t near_min_u32(const uint32_t a, const uint32_t b) { return b < a ? b : a; }
constexpr uint32_t kNearLeaf = 0x80000000u;          // RT_NODE_LEAF
constexpr float kNearInf = __builtin_huge_valf();
constexpr uint32_t kNearNoFace = 0xffffffffu;

RT_QUERY_HD bool near_is_leaf(const NearNode &n) { return (n.count_flags & kNearLeaf) != 0u; }
RT_QUERY_HD uint32_t near_leaf_count(const NearNode &n) { return n.count_flags & 0x7fffffffu; }
RT_QUERY_HD uint32_t near_child_count(const NearNode &n) { return n.count_flags & 0xfu; }           // 0: a lost node
RT_QUERY_HD bool near_empty(const NearNode &n) { return !(n.lo[0] <= n.hi[0]); }
RT_QUERY_HD float near_min(const float a, const float b) { return b < a ? b : a; }
RT_QUERY_HD float near_max(const float a, const float b) { return a < b ? b : a; }
RT_QUERY_HD void near_box_clear(NearNode &n) {
    for (int q = 0; q < 3; ++q) { n.lo[q] = kNearInf; n.hi[q] = -kNearInf; }
}
RT_QUERY_HD void near_box_add(NearNode &n, const float x, const float y, const float z) {
    n.lo[0] = near_min(n.lo[0], x); n.lo[1] = near_min(n.lo[1], y); n.lo[2] = near_min(n.lo[2], z);
    n.hi[0] = near_max(n.hi[0], x); n.hi[1] = near_max(n.hi[1], y); n.hi[2] = near_max(n.hi[2], z);
}
RT_QUERY_HD void near_box_add(NearNode &n, const NearTri &t) {
    near_box_add(n, t.a[0], t.a[1], t.a[2]); near_box_add(n, t.b[0], t.b[1], t.b[2]); near_box_add(n, t.c[0], t.c[1], t.c[2]);
}
// element offsets in 64 bits (i * 3 leaves 32 bits above 715 M points)
RT_QUERY_HD size_t near_out3(const uint64_t i) { return static_cast<size_t>(i) * 3u; }

// ---- point to triangle (rt_closest_point_triangle; the header writes the same sequence out line by line) -----------------------------------
RT_QUERY_HD float near_dot(const float ax, const float ay, const float az, const float bx, const float by, const float bz) {
    return (ax * bx + ay * by) + az * bz;
}
// Region of P in the Voronoi walk of Ericson 5.1.5, tested in this order: 0 A, 1 B, 2 AB, 3 C, 4 AC, 5 BC, 6 face.
// Every quantity is a pure function of (P, A, B, C), so all of them are formed first and the tests then pick a region: the values, and so
// the answer, are those of the sequential walk, and a wave of points in different regions runs ONE division.
struct NearClosest {
    float qx, qy, qz, d2;
    int32_t region;
};
RT_QUERY_HD NearClosest near_point_triangle(const float px, const float py, const float pz, const float ax, const float ay, const float az,
                                            const float bx, const float by, const float bz, const float cx, const float cy, const float cz) {
    const float abx = bx - ax, aby = by - ay, abz = bz - az;
    const float acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float apx = px - ax, apy = py - ay, apz = pz - az;
    const float d1 = near_dot(abx, aby, abz, apx, apy, apz), d2 = near_dot(acx, acy, acz, apx, apy, apz);
    const float bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const float d3 = near_dot(abx, aby, abz, bpx, bpy, bpz), d4 = near_dot(acx, acy, acz, bpx, bpy, bpz);
    const float cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const float d5 = near_dot(abx, aby, abz, cpx, cpy, cpz), d6 = near_dot(acx, acy, acz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    const int32_t region = (d1 <= 0.0f && d2 <= 0.0f)                 ? 0
                           : (d3 >= 0.0f && d4 <= d3)                 ? 1
                           : (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) ? 2
                           : (d6 >= 0.0f && d5 <= d6)                 ? 3
                           : (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) ? 4
                           : (va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f) ? 5
                                                                        : 6;
    // the one division: AB d1 / (d1 - d3), AC d2 / (d2 - d6), BC (d4 - d3) / ((d4 - d3) + (d5 - d6)), face 1 / ((va + vb) + vc)
    const float num = region == 2 ? d1 : (region == 4 ? d2 : (region == 5 ? d43 : 1.0f));
    const float den = region == 2 ? d1 - d3 : (region == 4 ? d2 - d6 : (region == 5 ? d43 + d56 : (va + vb) + vc));
    const float s = num / den;
    NearClosest r;
    r.region = region;
    if (region == 0) { r.qx = ax; r.qy = ay; r.qz = az; }
    else if (region == 1) { r.qx = bx; r.qy = by; r.qz = bz; }
    else if (region == 3) { r.qx = cx; r.qy = cy; r.qz = cz; }
    else if (region == 6) {
        const float v = vb * s, w = vc * s;
        r.qx = (ax + abx * v) + acx * w; r.qy = (ay + aby * v) + acy * w; r.qz = (az + abz * v) + acz * w;
    } else {
        // an edge: base + e * s with (base, e) = (A, ab), (A, ac), (B, C - B)
        const float ox = region == 5 ? bx : ax, oy = region == 5 ? by : ay, oz = region == 5 ? bz : az;
        const float ex = region == 2 ? abx : (region == 4 ? acx : cx - bx), ey = region == 2 ? aby : (region == 4 ? acy : cy - by),
                    ez = region == 2 ? abz : (region == 4 ? acz : cz - bz);
        r.qx = ox + ex * s; r.qy = oy + ey * s; r.qz = oz + ez * s;
    }
    const float dx = px - r.qx, dy = py - r.qy, dz = pz - r.qz;
    r.d2 = near_dot(dx, dy, dz, dx, dy, dz);
    return r;
}
RT_QUERY_HD NearClosest near_point_triangle(const float px, const float py, const float pz, const NearTri &t) {
    return near_point_triangle(px, py, pz, t.a[0], t.a[1], t.a[2], t.b[0], t.b[1], t.b[2], t.c[0], t.c[1], t.c[2]);
}

// ---- the best so far -----------------------------------------------------------------------------------------------------------------------
// The answer is the candidate (d2 <= r2; a NaN d2 is none) with the smallest d2, ties to the lowest face id: a minimum over a set under a
// total order, so the order in which the faces are met cannot change it.
struct NearBest {
    float d2;            // +inf: none yet
    uint32_t face;       // kNearNoFace: none yet
    float q[3];
};
RT_QUERY_HD NearBest near_none(const float px, const float py, const float pz) { return NearBest{kNearInf, kNearNoFace, {px, py, pz}}; }
RT_QUERY_HD bool near_better(const NearBest &b, const float d2, const uint32_t face, const float r2) {
    return d2 <= r2 && (d2 < b.d2 || (d2 == b.d2 && face < b.face));
}
RT_QUERY_HD void near_take(NearBest &b, const NearClosest &c, const uint32_t face, const float r2) {
    if (near_better(b, c.d2, face, r2)) { b.d2 = c.d2; b.face = face; b.q[0] = c.qx; b.q[1] = c.qy; b.q[2] = c.qz; }
}
// what a face must not exceed to matter: the best so far, the radius before there is one
RT_QUERY_HD float near_limit(const NearBest &b, const float r2) { return b.d2 < r2 ? b.d2 : r2; }

// ---- the box bound and the pruning rule (Closest points, has the error argument) ---------------------------------------------
// sigma: the absolute slack per axis, 2^-20 * (extent + |P|_1); extent = max |coordinate| of the scene (DScene::extent)
RT_QUERY_HD float near_abs(const float x) { return x < 0.0f ? -x : x; }
RT_QUERY_HD float near_sigma(const float extent, const float px, const float py, const float pz) {
    return 9.5367431640625e-07f * (extent + ((near_abs(px) + near_abs(py)) + near_abs(pz)));
}
// max(x, 0) that sends NaN to 0: a gap that cannot be formed bounds nothing
RT_QUERY_HD float near_pos(const float x) { return x > 0.0f ? x : 0.0f; }
RT_QUERY_HD float near_gap(const float lo, const float hi, const float p, const float sigma) {
    const float g = near_pos(near_max(lo - p, p - hi));
    return near_pos(g - sigma);
}
// the squared lower bound of the COMPUTED d2 of every face whose vertices lie in [lo, hi]
RT_QUERY_HD float near_box_bound2(const float lo[3], const float hi[3], const float px, const float py, const float pz, const float sigma) {
    const float gx = near_gap(lo[0], hi[0], px, sigma), gy = near_gap(lo[1], hi[1], py, sigma), gz = near_gap(lo[2], hi[2], pz, sigma);
    return (gx * gx + gy * gy) + gz * gz;
}
// no face in the box can be a candidate, improve the best or tie with it (a NaN or an overflow on either side: not pruned)
RT_QUERY_HD bool near_pruned(const float bound2, const float limit) { return bound2 > limit * 1.00000095367431640625f; }

// ---- the bounds on the host ----------------------------------------------------------------------------------------------------------------
// The bottom-up pass: nodes[] holds the leaves' boxes (inner nodes: cleared) and every node's first / count_flags; children follow their
// parents in the breadth-first array, so one sweep from the last node to the first completes every box.  false: a child index that does
// not lie behind its parent inside the array.
inline bool near_sweep_nodes(NearNode *nodes, const uint32_t n_nodes) {
    for (uint32_t j = n_nodes; j-- > 0u;) {
        NearNode &n = nodes[j];
        if (near_is_leaf(n)) continue;
        const uint32_t kids = near_child_count(n);
        if (kids == 0u) continue;
        if (n.first <= j || n.first >= n_nodes || n_nodes - n.first < kids) return false;
        for (uint32_t k = 0; k < kids; ++k) {
            const NearNode &c = nodes[n.first + k];
            if (near_empty(c)) continue;
            near_box_add(n, c.lo[0], c.lo[1], c.lo[2]);
            near_box_add(n, c.hi[0], c.hi[1], c.hi[2]);
        }
    }
    return true;
}

// ---- the walk, one point (the kernel runs the same steps for 64 points with a wave-uniform stack and order) -------------------------------
// Depth-first from the root, nearest child first; an entry is tested against the best of the moment when it is popped.
constexpr int32_t kNearStack = 128;          // RT_STACK: 7 pushed per level + 8, depth <= 15 (checked on upload)
struct NearWalkStats {
    uint64_t nodes, tris;
    bool overflow;          // kept children were dropped for want of stack: the answer may be wrong (never, within the upload's depth bound)
};
// chunks / chunk0: the boxes of the leaves' 64-record chunks, those of leaf j from chunks[chunk0[j]] on (a leaf of one chunk: not read)
inline NearBest near_walk(const NearNode *nodes, const NearTri *tris, const NearNode *chunks, const uint32_t *chunk0, const float extent, const float px,
                          const float py, const float pz, const float r2, NearWalkStats *stats = nullptr) {
    NearBest best = near_none(px, py, pz);
    const float sigma = near_sigma(extent, px, py, pz);
    uint32_t stack[kNearStack];
    int32_t sp = 0;
    stack[sp++] = 0u;
    while (sp > 0) {
        const uint32_t ni = stack[--sp];
        const NearNode &n = nodes[ni];
        if (near_empty(n) || near_pruned(near_box_bound2(n.lo, n.hi, px, py, pz, sigma), near_limit(best, r2))) continue;
        if (stats) ++stats->nodes;
        if (near_is_leaf(n)) {
            const uint32_t cnt = near_leaf_count(n);
            for (uint32_t c = 0; c < near_chunks(cnt); ++c) {
                if (cnt > kNearChunk) {
                    const NearNode &cb = chunks[chunk0[ni] + c];
                    if (near_pruned(near_box_bound2(cb.lo, cb.hi, px, py, pz, sigma), near_limit(best, r2))) continue;
                }
                const uint32_t end = near_min_u32(cnt, (c + 1u) * kNearChunk);
                for (uint32_t k = c * kNearChunk; k < end; ++k) {
                    const NearTri &t = tris[n.first + k];
                    near_take(best, near_point_triangle(px, py, pz, t), t.face, r2);
                }
                if (stats) stats->tris += end - c * kNearChunk;
            }
            continue;
        }
        // the kept children, pushed farthest first
        const uint32_t kids = near_child_count(n);
        float key[8];
        uint32_t idx[8];
        uint32_t kept = 0;
        for (uint32_t k = 0; k < kids && k < 8u; ++k) {
            const NearNode &c = nodes[n.first + k];
            if (near_empty(c)) continue;
            const float b2 = near_box_bound2(c.lo, c.hi, px, py, pz, sigma);
            if (near_pruned(b2, near_limit(best, r2))) continue;
            uint32_t at = kept++;
            for (; at > 0u && key[at - 1u] < b2; --at) { key[at] = key[at - 1u]; idx[at] = idx[at - 1u]; }
            key[at] = b2; idx[at] = n.first + k;
        }
        // (7 pushed per level + 8 at depth <= 15 fit: the upload refuses deeper trees.  A tree that did overflow would lose children
        // silently, so the check program asserts on the flag.)
        if (stats && sp + static_cast<int32_t>(kept) > kNearStack) stats->overflow = true;
        for (uint32_t k = 0; k < kept && sp < kNearStack; ++k) stack[sp++] = idx[k];
    }
    return best;
}

// ---- the argument rule.  0: valid; else the rule that failed, as a text for rt_last_error --------------------------------------------------
inline const char *near_args(const int32_t n, const void *point_in, const float max_dist, const void *face, const void *dist2, const void *point) {
    if (n < 0) return "n is negative";
    if (!(max_dist >= 0.0f)) return "max_dist must be >= 0 (+inf: unbounded)";
    if (n == 0) return nullptr;
    if (!point_in) return "the points are null";
    if (!face && !dist2 && !point) return "face, dist2 and point are all null";
    const size_t v1 = static_cast<size_t>(n) * 4, v3 = v1 * 3;
    if (query_any_overlap({{face, v1}, {dist2, v1}, {point, v3}}, {{point_in, v3}})) return "an output overlaps the input";
    if (query_any_overlap({{face, v1}}, {{dist2, v1}, {point, v3}}) || query_any_overlap({{dist2, v1}}, {{point, v3}})) return "two outputs overlap";
    return nullptr;
}

}  // namespace rtamd
