// rt_gather_layout.hpp -- what the one-bounce diffuse gather (rt_indirect_diffuse_device; DESIGN.md §5, Indirect diffuse) adds to the
// arithmetic of rt_ao_layout.hpp, which it shares whole with k_occlusion (AoLayout, ao_units, ao_next, ao_point_lanes, ao_xyz, ao_grid, the
// tables and the hash): the lanes whose radiances the owner lane of a point adds in a round, in the order it adds them, and the argument
// rule of the two calls.  Header-only and free of HIP, so that tools/gather_layout_check.cpp can run it under a sanitizer.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rt_ao_layout.hpp"

namespace rtamd {

// Lane p < group adds the radiances of point p of the unit.  In round `round` they sit in the lanes [first, first + count) -- the bits of
// ao_point_lanes, which are consecutive -- and lane first + i holds direction k0 + i of the point: ascending lanes are ascending k, and the
// rounds continue each other, so adding lane by lane, round after round, is the definition's sum over k = 0 .. K - 1.
struct GatherRange {
    int32_t first, count, k0;
};
RT_QUERY_HD GatherRange gather_range(const AoLayout &L, const int32_t p, const int32_t round) {
    const int32_t lo = p * L.K - round * 64, hi = lo + L.K;
    const int32_t a = lo < 0 ? 0 : lo, b = hi > 64 ? 64 : hi;
    if (b <= a) return GatherRange{0, 0, 0};
    return GatherRange{a, b - a, a - lo};
}

// The argument rule.  0: valid; else the rule that failed, as a text for rt_last_error.
inline const char *gather_args(const int32_t n, const void *point, const void *normal, const int32_t m, const void *rgb) {
    if (n < 0) return "n is negative";
    if (!ao_grid_ok(m)) return "the grid size m must be in 1 .. 16";
    if (n == 0) return nullptr;
    if (!point || !normal || !rgb) return "a pointer is null";
    const size_t v3 = static_cast<size_t>(n) * 3 * sizeof(float);
    if (query_any_overlap({{rgb, v3}}, {{point, v3}, {normal, v3}})) return "the output overlaps an input";
    return nullptr;
}

}  // namespace rtamd
