// rt_hits_layout.hpp -- what the ordered multi-hit ray query (rt_ray_hits_device; DESIGN.md §5, Ordered ray hits) shares between k_ray_hits
// and the host: the sorted list a ray keeps, its insertion, the rule that turns the list into the k output slots and the count, the
// instantiation a k runs on, and the argument rule of the two calls.  Header-only and free of HIP (RT_QUERY_HD is `inline` in a host
// program), so that tools/hits_layout_check.cpp can run it under a sanitizer.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rt_query_chunks.hpp"

// full unrolling keeps every list index a constant (a run-time index would send the list to scratch); a host compiler needs no hint
#if defined(__clang__)
#define RT_HITS_UNROLL _Pragma("unroll")
#else
#define RT_HITS_UNROLL
#endif

namespace rtamd {

constexpr int32_t kMaxRayHits = 8;               // RT_MAX_RAY_HITS of the header
constexpr int32_t kHitNoFace = INT32_MAX;        // the face of an empty entry: above every face id of a scene

// the part of the hit rule that follows rayTriangleIntersection's acceptance: x > 0.00001f and x <= t_max (a NaN fails both)
RT_QUERY_HD bool hit_in_range(const float x, const float t_max) { return x > 0.00001f && x <= t_max; }

// The list of one ray: N entries ascending by (t, face), distinct faces.  An empty entry is (t_max, kHitNoFace): a hit has t <= t_max and a
// face below kHitNoFace, so every hit sorts before every empty entry, and the t of the LAST entry is what the conservative tests of the walk
// may bound by -- t_max until the list is full, the N-th smallest hit from then on.  The kernel keeps N = K + 1 entries for K output slots.
template <int N>
struct HitList {
    float t[N];
    int32_t f[N];
};
template <int N>
RT_QUERY_HD void hits_clear(HitList<N> &L, const float t_max) {
RT_HITS_UNROLL
    for (int j = 0; j < N; ++j) { L.t[j] = t_max; L.f[j] = kHitNoFace; }
}
// Insert the hit (t, f) if `ok`; a fixed chain of N compare-exchanges at constant indices (no run-time index: the list stays in
// registers).  The candidate moves up the list; where it sorts before an entry the two are swapped and the displaced entry moves on (it is
// below everything behind it, so it ripples to the end and the last entry falls off).  A candidate whose face an entry already holds
// (the same face seen in another leaf: the same t) is dropped there -- it meets that entry before any larger one.
template <int N>
RT_QUERY_HD void hits_insert(HitList<N> &L, const bool ok, const float t, const int32_t f) {
    const float inf = __builtin_inff();
    float ct = ok ? t : inf;
    int32_t cf = ok ? f : kHitNoFace;
RT_HITS_UNROLL
    for (int j = 0; j < N; ++j) {
        const float et = L.t[j];
        const int32_t ef = L.f[j];
        const bool same = cf == ef;
        const bool before = !same && (ct < et || (ct == et && cf < ef));
        L.t[j] = before ? ct : et;
        L.f[j] = before ? cf : ef;
        ct = same ? inf : (before ? et : ct);
        cf = same ? kHitNoFace : (before ? ef : cf);
    }
}
// hits held (the empty entries are at the end)
template <int N>
RT_QUERY_HD int32_t hits_held(const HitList<N> &L) {
    int32_t h = 0;
RT_HITS_UNROLL
    for (int j = 0; j < N; ++j) h += L.f[j] != kHitNoFace ? 1 : 0;
    return h;
}
// The output rule for a call with k slots on a list of N > k entries: count = min(H, k + 1), slot j < min(H, k) the j-th hit, the other
// slots -1 / -1.0f.  (The list holds min(H, N) hits and N >= k + 1, so min(held, k + 1) = min(H, k + 1).)
template <int N>
RT_QUERY_HD int32_t hits_count(const HitList<N> &L, const int32_t k) {
    const int32_t h = hits_held(L);
    return h < k + 1 ? h : k + 1;
}
template <int N>
RT_QUERY_HD void hits_store(const HitList<N> &L, const int32_t k, int32_t *face, float *t, int32_t *count) {
RT_HITS_UNROLL
    for (int j = 0; j < N - 1; ++j) {
        if (j < k) {
            const bool held = L.f[j] != kHitNoFace;
            if (face) face[j] = held ? L.f[j] : -1;
            if (t) t[j] = held ? L.t[j] : -1.0f;
        }
    }
    if (count) *count = hits_count(L, k);
}

// the instantiation K of k_ray_hits<K> that a call with k slots runs on: the next of 1, 2, 4, 8 (0: k is out of range)
RT_QUERY_HD int32_t hits_variant(const int32_t k) {
    return k < 1 || k > kMaxRayHits ? 0 : (k == 1 ? 1 : (k == 2 ? 2 : (k <= 4 ? 4 : 8)));
}

// The argument rule.  0: valid; else the rule that failed, as a text for rt_last_error.
inline const char *hits_args(const int32_t n, const void *origin, const void *dir, const int32_t k, const float t_max, const void *face,
                             const void *t, const void *count) {
    if (n < 0) return "n is negative";
    if (k < 1 || k > kMaxRayHits) return "k must be in 1 .. 8";
    if (!(t_max > 0.0f)) return "t_max must be > 0 (+inf: unbounded)";
    if (n == 0) return nullptr;
    if (!origin || !dir) return "origin or dir is null";
    if (!face && !t && !count) return "face, t and count are all null";
    const size_t v1 = static_cast<size_t>(n) * 4, vk = v1 * static_cast<size_t>(k), v3 = v1 * 3;
    if (query_any_overlap({{face, vk}, {t, vk}, {count, v1}}, {{origin, v3}, {dir, v3}})) return "an output overlaps an input";
    if (query_any_overlap({{face, vk}}, {{t, vk}, {count, v1}}) || query_any_overlap({{t, vk}}, {{count, v1}})) return "two outputs overlap";
    return nullptr;
}

}  // namespace rtamd
