// rt_ao_layout.hpp -- the arithmetic of the ambient-occlusion query (rt_ambient_occlusion_device; DESIGN.md §5, Ambient occlusion) that the
// host and k_occlusion share: how many points a wave owns, in how many rounds it walks their directions, which (point, direction) a lane
// holds, the 64-bit element indices, where the table of a grid size starts, the per-point hash, and the argument rules of the calls.
// The function macro RT_QUERY_HD, the grid rule (capped_grid) and the overlap rule (query_any_overlap) are those of rt_query_chunks.hpp.
// Header-only and free of HIP, so that tools/ao_layout_check.cpp can run it under a sanitizer.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rt_query_chunks.hpp"

namespace rtamd {

constexpr int32_t kAoMaxGrid = 16, kAoRotations = 64;       // RT_AO_MAX_GRID, RT_AO_ROTATIONS
RT_QUERY_HD bool ao_grid_ok(const int32_t m) { return m >= 1 && m <= kAoMaxGrid; }

// The device tables, one float array: the directions of m = 1 .. 16 back to back (m * m entries of xyz each), then the 64 (c, s) pairs.
RT_QUERY_HD uint32_t ao_dir_offset(const int32_t m) {            // entries in front of the grid of m: 1 + 4 + .. + (m - 1)^2
    const uint32_t j = static_cast<uint32_t>(m - 1);
    return j * (j + 1u) * (2u * j + 1u) / 6u;
}
constexpr uint32_t kAoDirEntries = 1496u;                     // ao_dir_offset(17)
constexpr uint32_t kAoTableFloats = kAoDirEntries * 3u + static_cast<uint32_t>(kAoRotations) * 2u;

// A wave owns whole points, and every lane of every round holds a segment.  With g = gcd(K, 64) a wave unit is `group` = 64 / g points walked
// in `rounds` = K / g rounds of 64 segments: group * K = rounds * 64, so the unit's segments, numbered e = p * K + k (p: the point's place in
// the unit, k: the direction), fill the rounds exactly: lane l of round r holds e = r * 64 + l.  K = 1, 4, 16, 64: 64, 16, 4, 1 points in
// one round; K = 256: one point in four rounds; K = 36: 16 points in 9 rounds, where a point's segments may lie in two rounds.
struct AoLayout {
    int32_t K, group, rounds;
    int32_t q64, r64;        // 64 / K and 64 % K: what a lane's (p, k) moves by from one round to the next (ao_next)
};
RT_QUERY_HD AoLayout ao_layout(const int32_t m) {
    const int32_t K = m * m;
    int32_t g = 64;
    while (K % g != 0) g >>= 1;                            // gcd(K, 64)
    return AoLayout{K, 64 / g, K / g, 64 / K, 64 % K};
}
// wave units of a call on n points: unit u holds the points [u * group, min(n, (u + 1) * group))
RT_QUERY_HD uint64_t ao_units(const int32_t n, const AoLayout &L) {
    return n <= 0 ? 0u : (static_cast<uint64_t>(n) + static_cast<uint64_t>(L.group) - 1u) / static_cast<uint64_t>(L.group);
}
// what lane `lane` of unit `unit` holds in round `round`: point index and direction; live = the point exists (point < n)
struct AoSlot {
    uint64_t point;
    int32_t p, k;            // the point's place in the unit, the direction
    bool live;
};
RT_QUERY_HD AoSlot ao_slot(const int32_t n, const AoLayout &L, const uint64_t unit, const int32_t round, const int32_t lane) {
    const int32_t e = round * 64 + lane, p = e / L.K, k = e - p * L.K;
    const uint64_t point = unit * static_cast<uint64_t>(L.group) + static_cast<uint64_t>(p);
    return AoSlot{point, p, k, point < static_cast<uint64_t>(n)};
}
// (p, k) of a lane in the next round, without a division: e grows by 64
RT_QUERY_HD void ao_next(const AoLayout &L, int32_t &p, int32_t &k) {
    p += L.q64; k += L.r64;
    if (k >= L.K) { k -= L.K; ++p; }
}
// Lane p < group keeps the count of point p of the unit.  Its segments in round `round` are the lanes [p * K - round * 64, (p + 1) * K -
// round * 64) cut to [0, 64): the bits this returns (0: none of them lies in that round).
RT_QUERY_HD unsigned long long ao_point_lanes(const AoLayout &L, const int32_t p, const int32_t round) {
    const int32_t lo = p * L.K - round * 64, hi = lo + L.K;
    const int32_t a = lo < 0 ? 0 : lo, b = hi > 64 ? 64 : hi;
    if (b <= a) return 0ull;
    const unsigned long long below_b = b >= 64 ? ~0ull : ((1ull << b) - 1ull), below_a = (1ull << a) - 1ull;
    return below_b & ~below_a;
}
// first float of point i in a float[n * 3] array (n * 3 leaves 32 bits above 715 M points)
RT_QUERY_HD size_t ao_xyz(const uint64_t i) { return static_cast<size_t>(i) * 3u; }
// segments of a call, for the figures a caller reports (n * K leaves 32 bits)
RT_QUERY_HD uint64_t ao_segments(const int32_t n, const int32_t m) { return n <= 0 ? 0u : static_cast<uint64_t>(n) * static_cast<uint64_t>(m * m); }
// grid of k_occlusion: RT_WAVES = 4 units per block and, for units of one round, at most 8 blocks per CU with the rest by grid stride -- the
// rule of the other query kernels (capped_grid).  A unit of several rounds is that many times the work, and a wave that strides over two of them while
// its neighbour has one is a long tail, so the cap grows with the rounds, up to 4 times: more and shorter blocks, which the dispatcher
// hands out as slots free up (DESIGN.md 6 has the figures under both caps, and those of a rule that did worse: consecutive units per wave).
RT_QUERY_HD int32_t ao_grid(const uint64_t units, const int32_t cus, const int32_t rounds) {
    return capped_grid(units, 4u, cus, rounds < 4 ? rounds : 4);
}

// the per-point hash of rt_ao_rotation: rotation r = ao_hash(seed, i) >> 26
RT_QUERY_HD uint32_t ao_hash(const uint32_t seed, const uint32_t i) {
    uint32_t h = (i * 0x9E3779B1u) ^ (seed * 0x85EBCA6Bu);
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return h;
}

// The argument rules.  0: valid; else the rule that failed, as a text for rt_last_error.  (The radius is tested as !(radius > 0) || radius
// > FLT_MAX so that NaN fails without <cmath>.)
inline const char *ao_args(const int32_t n, const void *point, const void *normal, const int32_t m, const float radius, const void *open, const void *ao) {
    if (n < 0) return "n is negative";
    if (!ao_grid_ok(m)) return "the grid size m must be in 1 .. 16";
    if (!(radius > 0.0f) || radius > 3.402823466e+38f) return "the radius must be finite and > 0";
    if (n == 0) return nullptr;
    if (!point || !normal) return "point or normal is null";
    if (!open && !ao) return "open and ao are both null";
    const size_t in = static_cast<size_t>(n) * 3 * sizeof(float);
    if (query_any_overlap({{open, static_cast<size_t>(n) * 2}, {ao, static_cast<size_t>(n) * 4}}, {{point, in}, {normal, in}})) return "an output overlaps an input";
    return nullptr;
}
inline const char *ao_hit_points_args(const int32_t n, const void *origin, const void *dir, const void *face, const void *t, const void *point, const void *normal) {
    if (n < 0) return "n is negative";
    if (n == 0) return nullptr;
    if (!origin || !dir || !face || !t || !point || !normal) return "a pointer is null";
    const size_t v3 = static_cast<size_t>(n) * 3 * sizeof(float), v1 = static_cast<size_t>(n) * 4;
    if (query_any_overlap({{point, v3}, {normal, v3}}, {{origin, v3}, {dir, v3}, {face, v1}, {t, v1}})) return "an output overlaps an input";
    return nullptr;
}

}  // namespace rtamd
