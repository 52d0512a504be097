// rt_query_chunks.hpp -- the host arithmetic of the device ray queries (rt_capi.cpp; DESIGN.md §5, Device ray queries): the range of
// rt_set_query_chunk, how a batch of n rays splits into chunks, the 64-bit element offsets a chunk applies to the caller's pointers, and the
// argument rules of the four query calls.  Header-only and free of HIP, so that a host program can run it under a sanitizer
// (tools/query_chunks_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace rtamd {

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

// The argument rules.  0: valid; else the rule that failed, as a text for rt_last_error.
inline const char *query_closest_args(const int32_t n, const void *origin, const void *dir, const void *face, const void *t) {
    if (n < 0) return "n is negative";
    if (n == 0) return nullptr;
    if (!origin || !dir) return "origin or dir is null";
    if (!face && !t) return "face and t are both null";
    const size_t in = static_cast<size_t>(n) * 3 * sizeof(float), out = static_cast<size_t>(n) * 4;
    for (const void *o : {face, t})
        if (query_ranges_overlap(o, out, origin, in) || query_ranges_overlap(o, out, dir, in)) return "an output overlaps an input";
    return nullptr;
}
inline const char *query_strikes_args(const int32_t n, const void *hit, const void *light, const void *vis) {
    if (n < 0) return "n is negative";
    if (n == 0) return nullptr;
    if (!hit || !light || !vis) return "hit, light or vis is null";
    if (n > INT32_MAX / 3) return "n above 715,827,882 (the segment kernel indexes its floats in 32 bits)";
    const size_t in = static_cast<size_t>(n) * 3 * sizeof(float);
    if (query_ranges_overlap(vis, static_cast<size_t>(n), hit, in) || query_ranges_overlap(vis, static_cast<size_t>(n), light, in)) return "vis overlaps an input";
    return nullptr;
}
inline const char *query_trace_args(const int32_t n, const void *origin, const void *dir, const void *rgb, const void *face, const void *t) {
    if (n < 0) return "n is negative";
    if (n == 0) return nullptr;
    if (!origin || !dir || !rgb) return "origin, dir or out_rgb is null";
    const size_t in = static_cast<size_t>(n) * 3 * sizeof(float);
    const struct { const void *p; size_t bytes; } outs[] = {{rgb, in}, {face, static_cast<size_t>(n) * 4}, {t, static_cast<size_t>(n) * 4}};
    for (const auto &o : outs)
        if (query_ranges_overlap(o.p, o.bytes, origin, in) || query_ranges_overlap(o.p, o.bytes, dir, in)) return "an output overlaps an input";
    return nullptr;
}

}  // namespace rtamd
