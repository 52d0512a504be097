// rt_gbuffer_layout.hpp -- the arithmetic of the geometry-buffer query (rt_gbuffer_device; DESIGN.md §5, Geometry buffers as a query) that the
// host and k_gbuffer share: the tiles of the output frame, which output pixel a lane of a tile holds, the 64-bit output indices, where the
// offsets of a pass start in the pass table, the grid, and the argument rules of the calls.  The function macro RT_QUERY_HD and the grid
// rule (capped_grid) are those of rt_query_chunks.hpp.  Header-only and free of HIP, so that tools/gbuffer_layout_check.cpp can run it
// under a sanitizer.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rt_query_chunks.hpp"

namespace rtamd {

constexpr int32_t kGbChannels = 8;                              // RT_GBUFFER_CHANNELS
constexpr int32_t kGbMaxSupersampling = 4, kGbMaxPasses = 256;  // RT_MAX_SUPERSAMPLING, RT_MAX_PASSES

// The pass table, one float array: for n = 1 .. 4, for p = 0 .. 255, eight floats -- ox[0..3] then oy[0..3] of rt_pass_offsets(n, p), the
// entries s >= n zero.  32 KB.
constexpr uint32_t kGbPassTabFloats = static_cast<uint32_t>(kGbMaxSupersampling) * static_cast<uint32_t>(kGbMaxPasses) * 8u;
RT_QUERY_HD bool gb_pass_ok(const int32_t n, const int32_t p) { return n >= 1 && n <= kGbMaxSupersampling && p >= 0 && p < kGbMaxPasses; }
RT_QUERY_HD uint32_t gb_pass_entry(const int32_t n, const int32_t p) {          // first float of (n, p); gb_pass_ok(n, p)
    return (static_cast<uint32_t>(n - 1) * static_cast<uint32_t>(kGbMaxPasses) + static_cast<uint32_t>(p)) * 8u;
}

// The size rule (the one of a frame, make_frame in rt_capi.cpp): the frame of sub-samples of the call's rows has at most UINT32_MAX / 3
// sub-samples and n * W, n * H fit an int32.  So output pixel numbers (rows * W <= 1,431,655,765) and tile numbers fit 32 bits with room
// for a partial tile past the edge, an internal column or row (n * (W + 7)) fits 32 unsigned bits, and only the float index of a pixel
// (pixel * 8) needs 64.
RT_QUERY_HD bool gb_size_ok(const int32_t n, const int32_t width, const int32_t height, const int32_t rows) {
    if (n < 1 || n > kGbMaxSupersampling || width <= 0 || height <= 0 || rows < 0 || rows > height) return false;
    const int64_t n64 = n;
    return n64 * width <= INT32_MAX && n64 * height <= INT32_MAX && n64 * n64 * rows * width <= static_cast<int64_t>(UINT32_MAX / 3u);
}

// A wave owns an 8 x 8 tile of OUTPUT pixels of the call's local rows: tile t is tile column t % tiles_x of tile row t / tiles_x, lane l
// holds column tx * 8 + (l & 7) of local row ty * 8 + (l >> 3); live = that pixel exists.
struct GbTiles {
    uint32_t tiles_x, tiles_y, tiles;
};
RT_QUERY_HD GbTiles gb_tiles(const int32_t width, const int32_t rows) {           // gb_size_ok
    const uint32_t tx = (static_cast<uint32_t>(width) + 7u) / 8u, ty = (static_cast<uint32_t>(rows) + 7u) / 8u;
    return GbTiles{tx, ty, tx * ty};
}
struct GbLane {
    int32_t i, lr;           // output column, local row
    bool live;
};
RT_QUERY_HD GbLane gb_lane(const GbTiles &T, const int32_t width, const int32_t rows, const uint32_t tile, const int32_t lane) {
    const uint32_t tx = tile % T.tiles_x, ty = tile / T.tiles_x;
    const int32_t i = static_cast<int32_t>(tx * 8u) + (lane & 7), lr = static_cast<int32_t>(ty * 8u) + (lane >> 3);
    return GbLane{i, lr, i < width && lr < rows};
}
// first of the two float4 of output pixel (lr, i): pixel q = lr * W + i is at float q * 8
RT_QUERY_HD uint64_t gb_out_vec4(const int32_t width, const int32_t lr, const int32_t i) {
    return (static_cast<uint64_t>(lr) * static_cast<uint64_t>(width) + static_cast<uint64_t>(i)) * 2u;
}
RT_QUERY_HD uint64_t gb_out_floats(const int32_t width, const int32_t rows) {
    return static_cast<uint64_t>(rows) * static_cast<uint64_t>(width) * static_cast<uint64_t>(kGbChannels);
}
// grid of k_gbuffer: RT_WAVES = 4 tiles per block, at most 8 blocks per CU, the rest by grid stride -- the rule of the other query kernels (capped_grid)
RT_QUERY_HD int32_t gb_grid(const uint32_t tiles, const int32_t cus) {
    return capped_grid(tiles, 4u, cus);
}

// The argument rules that need neither a context nor a device.  0: valid; else the rule that failed, as a text for rt_last_error.  (The
// checks of rt_params are the frame's own, make_frame.)  `out` takes two float4 stores per pixel: it is 16-byte aligned.
inline const char *gb_args(const void *cam, const void *params, const void *out) {
    if (!cam) return "the camera is null";
    if (!params) return "the params are null";
    if (!out) return "the output is null";
    if ((reinterpret_cast<uintptr_t>(out) & 15u) != 0u) return "the output must be 16-byte aligned";
    return nullptr;
}

}  // namespace rtamd
