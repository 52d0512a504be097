// rt_denoise_layout.hpp -- the arithmetic of the edge-avoiding denoiser (rt_denoise_device; DESIGN.md §5, Denoising) that the host and the
// kernels of rt_denoise.hip share: the scratch layout (two guide planes, two working images), the tiles of the image, which pixel a lane of
// a tile holds, the 64-bit indices, the grid, the per-iteration scales and the argument rules of the calls.  The function macro RT_QUERY_HD, the
// grid rule (capped_grid) and the overlap predicate (query_ranges_overlap) are those of rt_query_chunks.hpp.  Header-only and free of HIP, so
// that tools/denoise_layout_check.cpp can run it under a sanitizer.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "rt_query_chunks.hpp"

namespace rtamd {

constexpr int32_t kDnMaxIterations = 8;                  // RT_DENOISE_MAX_ITERATIONS
constexpr int32_t kDnGbChannels = 8;                     // RT_GBUFFER_CHANNELS
constexpr int32_t kDnTileW = 64, kDnTileH = 4;           // a wave owns a 64 x 1 run of a row, a workgroup of 4 waves the 64 x 4 tile

// The size rule: channels is 1 or 3, width >= 1, rows >= 0 and width * rows <= INT32_MAX.  So pixel numbers and tile numbers fit 32 bits
// (a tile past the edge included), and only float and byte offsets need 64.
RT_QUERY_HD bool dn_channels_ok(const int32_t channels) { return channels == 1 || channels == 3; }
RT_QUERY_HD bool dn_shape_ok(const int32_t width, const int32_t rows) { return width >= 1 && rows >= 0; }
RT_QUERY_HD bool dn_size_ok(const int32_t width, const int32_t rows) {          // dn_shape_ok
    return static_cast<int64_t>(width) * static_cast<int64_t>(rows) <= static_cast<int64_t>(INT32_MAX);
}
RT_QUERY_HD uint64_t dn_pixels(const int32_t width, const int32_t rows) { return static_cast<uint64_t>(width) * static_cast<uint64_t>(rows); }
RT_QUERY_HD uint64_t dn_image_bytes(const int32_t width, const int32_t rows, const int32_t channels) {     // the caller's packed image
    return dn_pixels(width, rows) * static_cast<uint64_t>(channels) * 4u;
}
RT_QUERY_HD uint64_t dn_gbuffer_bytes(const int32_t width, const int32_t rows) { return dn_pixels(width, rows) * static_cast<uint64_t>(kDnGbChannels) * 4u; }

// Scratch: guide plane 0 (float4 {Nx, Ny, Nz, z} per pixel), guide plane 1 (float4 {Ar, Ag, Ab, covered}), working image 0, working image
// 1.  A working image holds 16 bytes per pixel for three channels (RGBx) and 4 for one; every part starts 16-byte aligned.
struct DnLayout {
    uint64_t guide0, guide1, work0, work1, bytes;        // byte offsets from d_scratch, and the total
    uint32_t work_pixel_bytes;
};
RT_QUERY_HD uint64_t dn_align16(const uint64_t b) { return (b + 15u) & ~static_cast<uint64_t>(15u); }
RT_QUERY_HD DnLayout dn_layout(const int32_t width, const int32_t rows, const int32_t channels) {          // valid arguments
    const uint64_t px = dn_pixels(width, rows);
    DnLayout L;
    L.work_pixel_bytes = channels == 3 ? 16u : 4u;
    const uint64_t work = dn_align16(px * L.work_pixel_bytes);
    L.guide0 = 0;
    L.guide1 = px * 16u;
    L.work0 = px * 32u;
    L.work1 = L.work0 + work;
    L.bytes = L.work1 + work;
    return L;
}
// rt_denoise_scratch_bytes: 0 for invalid arguments (and for rows == 0, which needs none)
inline size_t dn_scratch_bytes(const int32_t width, const int32_t rows, const int32_t channels) {
    if (!dn_channels_ok(channels) || !dn_shape_ok(width, rows) || !dn_size_ok(width, rows)) return 0;
    return static_cast<size_t>(dn_layout(width, rows, channels).bytes);
}

// Tile t is tile column t % tiles_x of tile row t / tiles_x; wave v of the workgroup holds row ty * 4 + v, lane l column tx * 64 + l.
struct DnTiles {
    uint32_t tiles_x, tiles_y, tiles;
};
RT_QUERY_HD DnTiles dn_tiles(const int32_t width, const int32_t rows) {
    const uint32_t tx = (static_cast<uint32_t>(width) + static_cast<uint32_t>(kDnTileW) - 1u) / static_cast<uint32_t>(kDnTileW);
    const uint32_t ty = (static_cast<uint32_t>(rows) + static_cast<uint32_t>(kDnTileH) - 1u) / static_cast<uint32_t>(kDnTileH);
    return DnTiles{tx, ty, tx * ty};
}
struct DnLane {
    int32_t x, y;
    bool live;               // the pixel exists
};
RT_QUERY_HD DnLane dn_lane(const DnTiles &T, const int32_t width, const int32_t rows, const uint32_t tile, const int32_t wave, const int32_t lane) {
    const uint32_t tx = tile % T.tiles_x, ty = tile / T.tiles_x;
    // (as unsigned: the last tile column of a width near INT32_MAX reaches past it; such a lane is not live)
    const uint32_t x = tx * static_cast<uint32_t>(kDnTileW) + static_cast<uint32_t>(lane), y = ty * static_cast<uint32_t>(kDnTileH) + static_cast<uint32_t>(wave);
    const bool live = x < static_cast<uint32_t>(width) && y < static_cast<uint32_t>(rows);
    return DnLane{static_cast<int32_t>(live ? x : 0u), static_cast<int32_t>(live ? y : 0u), live};
}
RT_QUERY_HD uint64_t dn_pixel(const int32_t width, const int32_t x, const int32_t y) {
    return static_cast<uint64_t>(y) * static_cast<uint64_t>(width) + static_cast<uint64_t>(x);
}
// the pixel a tap of live pixel (x, y) reads, `off` = step * dx or step * dy with step <= 128: inside the image?
RT_QUERY_HD bool dn_tap_inside(const int32_t v, const int32_t off, const int32_t extent) {
    const int64_t t = static_cast<int64_t>(v) + off;
    return t >= 0 && t < extent;
}
// ... and its coordinate, the pixel's own where the tap is outside (so that an address formed from it is always inside the image)
RT_QUERY_HD int32_t dn_tap_coord(const int32_t v, const int32_t off, const int32_t extent) {
    const int64_t t = static_cast<int64_t>(v) + off;
    return t >= 0 && t < extent ? static_cast<int32_t>(t) : v;
}
// grid: one workgroup per tile, at most 8 per CU, the rest by grid stride (capped_grid)
RT_QUERY_HD int32_t dn_grid(const uint32_t tiles, const int32_t cus) { return capped_grid(tiles, 1u, cus); }

// grid of k_denoise_guide: one thread per pixel in blocks of 256, at most 8 blocks per CU, the rest by grid stride
RT_QUERY_HD int32_t dn_guide_grid(const uint64_t pixels, const int32_t cus) { return capped_grid(pixels, 256u, cus); }

// The scales of iteration k, squared once each, in float32 on the host: sc = sigma_color * 2^-k, sn = sigma_normal,
// sz = sigma_depth * (float)step, sa = sigma_albedo.
struct DnScales {
    float sc2, sn2, sz2, sa2;
};
inline DnScales dn_scales(const float sigma_color, const float sigma_normal, const float sigma_depth, const float sigma_albedo, const int32_t k) {
    const float sc = sigma_color * std::ldexp(1.0f, -k), sz = sigma_depth * static_cast<float>(1 << k);
    return DnScales{sc * sc, sigma_normal * sigma_normal, sz * sz, sigma_albedo * sigma_albedo};
}

inline bool dn_sigma_ok(const float s) { return s > 0.0f; }         // false for NaN; +inf is allowed

// The argument rules, none of which needs a context or a device.  0: valid; else the rule that failed, as a text for rt_last_error, and
// *unsupported says whether the failure is RT_ERR_UNSUPPORTED (else RT_ERR_INVALID).  `device`: the rules of rt_denoise_device -- scratch
// is required, scratch and out are 16-byte aligned and share no byte with each other or with an input; the host form has no scratch and
// copies, so it has no such rule.
inline const char *dn_args(const void *in, const int32_t channels, const void *gbuffer, const int32_t width, const int32_t rows, const int32_t *iterations,
                           const float *sigmas4, const void *scratch, const void *out, const bool device, bool *unsupported) {
    *unsupported = false;
    if (!in || !gbuffer || !out || !iterations || !sigmas4 || (device && !scratch)) return "a pointer is null";
    if (!dn_channels_ok(channels)) return "channels must be 1 or 3";
    if (width < 1) return "width must be at least 1";
    if (rows < 0) return "rows is negative";
    if (*iterations < 1 || *iterations > kDnMaxIterations) return "iterations outside 1 .. RT_DENOISE_MAX_ITERATIONS";
    for (int k = 0; k < 4; ++k)
        if (!dn_sigma_ok(sigmas4[k])) return "a sigma is not > 0";
    if (!dn_size_ok(width, rows)) { *unsupported = true; return "width * rows above INT32_MAX"; }
    if (!device) return nullptr;
    if ((reinterpret_cast<uintptr_t>(out) & 15u) != 0u) return "the output must be 16-byte aligned";
    if ((reinterpret_cast<uintptr_t>(scratch) & 15u) != 0u) return "the scratch must be 16-byte aligned";
    const uint64_t img = dn_image_bytes(width, rows, channels), gb = dn_gbuffer_bytes(width, rows), sb = dn_layout(width, rows, channels).bytes;
    if (query_ranges_overlap(out, img, scratch, sb)) return "the output overlaps the scratch";
    if (query_ranges_overlap(out, img, in, img)) return "the output overlaps the input image";
    if (query_ranges_overlap(out, img, gbuffer, gb)) return "the output overlaps the geometry buffers";
    if (query_ranges_overlap(scratch, sb, in, img)) return "the scratch overlaps the input image";
    if (query_ranges_overlap(scratch, sb, gbuffer, gb)) return "the scratch overlaps the geometry buffers";
    return nullptr;
}

}  // namespace rtamd
