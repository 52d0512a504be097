// rt_query_chunks.hpp -- the base of the query headers (rt_ao_layout.hpp, rt_gbuffer_layout.hpp and rt_denoise_layout.hpp include it) and the
// host arithmetic of the device ray queries (rt_capi.cpp; DESIGN.md §5, Device ray queries).  What every query shares is defined here once:
// the host/device function macro RT_QUERY_HD, the grid rule capped_grid, the overlap predicate query_ranges_overlap and query_any_overlap over
// lists of ranges.  Of the ray queries themselves: query_grid, the range of rt_set_query_chunk, how a batch of n rays splits into chunks, the
// 64-bit element offsets a chunk applies to the caller's pointers, and the argument rules of the calls.  Header-only and free of HIP
// (RT_QUERY_HD is `inline` in a host program), so that a host program can run it under a sanitizer (tools/query_chunks_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#if defined(__HIPCC__)
#define RT_QUERY_HD __host__ __device__ __forceinline__
#else
#define RT_QUERY_HD inline
#endif

namespace rtamd {

// The grid rule of the query kernels: a block per `per_block` items of work, at most 8 * cap_mult blocks per CU, the rest by grid stride.
RT_QUERY_HD int32_t capped_grid(const uint64_t work, const uint32_t per_block, const int32_t cus, const int32_t cap_mult = 1) {
    const uint64_t blocks = work / per_block + (work % per_block != 0u), cap = static_cast<uint64_t>(cus) * 8u * static_cast<uint64_t>(cap_mult);
    return static_cast<int32_t>(blocks < cap ? blocks : cap);
}
// grid of the lane = ray kernels k_segments and k_closest: a block of 256 threads per 256 rays
RT_QUERY_HD int32_t query_grid(const int32_t n, const int32_t cus) { return capped_grid(n > 0 ? static_cast<uint64_t>(n) : 0u, 256u, cus); }

constexpr int64_t kQueryChunkMin = 64, kQueryChunkMax = int64_t{1} << 24, kQueryChunkDefault = int64_t{1} << 22;
inline bool query_chunk_ok(const int64_t rays) { return rays >= kQueryChunkMin && rays <= kQueryChunkMax; }

// chunk k of a batch of n rays traced `chunk` at a time: rays [first, first + count); first counts rays, so a float[3] array moves by
// first * 3 elements and a per-ray array by first
struct QueryChunk {
    size_t first;
    int32_t count;
};
inline size_t query_chunk_count(const int32_t n, const int32_t chunk) {
    return n <= 0 ? 0 : (static_cast<size_t>(n) + static_cast<size_t>(chunk) - 1) / static_cast<size_t>(chunk);
}
inline QueryChunk query_chunk_at(const int32_t n, const int32_t chunk, const size_t k) {
    const size_t first = k * static_cast<size_t>(chunk), left = static_cast<size_t>(n) - first;
    return QueryChunk{first, static_cast<int32_t>(left < static_cast<size_t>(chunk) ? left : static_cast<size_t>(chunk))};
}

// [a, a + a_bytes) and [b, b + b_bytes) share a byte (a null pointer or an empty range shares none)
inline bool query_ranges_overlap(const void *a, const size_t a_bytes, const void *b, const size_t b_bytes) {
    if (!a || !b || a_bytes == 0 || b_bytes == 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 ? b0 - a0 < a_bytes : a0 - b0 < b_bytes;
}
// some range of `outs` shares a byte with some range of `ins`
struct QueryRange {
    const void *p;
    size_t bytes;
};
inline bool query_any_overlap(const std::initializer_list<QueryRange> outs, const std::initializer_list<QueryRange> ins) {
    for (const QueryRange &o : outs)
        for (const QueryRange &i : ins)
            if (query_ranges_overlap(o.p, o.bytes, i.p, i.bytes)) return true;
    return false;
}

// The argument rules.  0: valid; else the rule that failed, as a text for rt_last_error.
inline const char *query_closest_args(const int32_t n, const void *origin, const void *dir, const void *face, const void *t) {
    if (n < 0) return "n is negative";
    if (n == 0) return nullptr;
    if (!origin || !dir) return "origin or dir is null";
    if (!face && !t) return "face and t are both null";
    const size_t in = static_cast<size_t>(n) * 3 * sizeof(float), out = static_cast<size_t>(n) * 4;
    if (query_any_overlap({{face, out}, {t, out}}, {{origin, in}, {dir, in}})) return "an output overlaps an input";
    return nullptr;
}
// (the count rule of the segments on its own: rt_light_strikes tests it before it stages, and has no overlap rule -- its device arrays are its own)
inline const char *query_strikes_count(const int32_t n) {
    return n > INT32_MAX / 3 ? "n above 715,827,882 (the segment kernel indexes its floats in 32 bits)" : nullptr;
}
inline const char *query_strikes_args(const int32_t n, const void *hit, const void *light, const void *vis) {
    if (n < 0) return "n is negative";
    if (n == 0) return nullptr;
    if (!hit || !light || !vis) return "hit, light or vis is null";
    if (const char *bad = query_strikes_count(n)) return bad;
    const size_t in = static_cast<size_t>(n) * 3 * sizeof(float);
    if (query_any_overlap({{vis, static_cast<size_t>(n)}}, {{hit, in}, {light, in}})) return "vis overlaps an input";
    return nullptr;
}
inline const char *query_trace_args(const int32_t n, const void *origin, const void *dir, const void *rgb, const void *face, const void *t) {
    if (n < 0) return "n is negative";
    if (n == 0) return nullptr;
    if (!origin || !dir || !rgb) return "origin, dir or out_rgb is null";
    const size_t in = static_cast<size_t>(n) * 3 * sizeof(float), out = static_cast<size_t>(n) * 4;
    if (query_any_overlap({{rgb, in}, {face, out}, {t, out}}, {{origin, in}, {dir, in}})) return "an output overlaps an input";
    return nullptr;
}

}  // namespace rtamd
