// rt_upsample_layout.hpp -- the arithmetic of the guided upsample (rt_upsample_device; include/rt_mi355x.h, "upsampling"; DESIGN.md §5,
// Upsampling) that the host and the kernel of rt_upsample.hip share: the size of the low image, the two low pixels a high coordinate lies
// between and its offset from the first, the nearest low pixel, the scales and the argument rules of the calls.  The tiles, the lane's
// pixel, the 64-bit indices and the grid are the denoiser's (rt_denoise_layout.hpp).  Header-only and free of HIP, so that
// tools/upsample_layout_check.cpp can run it under a sanitizer.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rt_denoise_layout.hpp"

namespace rtamd {

constexpr int32_t kUpMaxFactor = 8;                      // RT_UPSAMPLE_MAX_FACTOR

RT_QUERY_HD bool up_factor_ok(const int32_t s) { return s >= 2 && s <= kUpMaxFactor; }

// the extent of the low image along an axis of `n` high pixels: ceil(n / s); n >= 0, s >= 1
RT_QUERY_HD int32_t up_low_extent(const int32_t n, const int32_t s) {
    return static_cast<int32_t>((static_cast<int64_t>(n) + static_cast<int64_t>(s) - 1) / static_cast<int64_t>(s));
}
// rt_upsample_low_size: false for arguments no call would take (width < 1, rows < 0, a factor out of range)
inline bool up_low_size(const int32_t width, const int32_t rows, const int32_t s, int32_t *w, int32_t *r) {
    if (!dn_shape_ok(width, rows) || !up_factor_ok(s)) return false;
    *w = up_low_extent(width, s);
    *r = up_low_extent(rows, s);
    return true;
}

// High coordinate v lies on or behind low coordinate i0 = v / s, f = v - i0 * s high pixels behind it (0 <= f < s); the other tap is
// i0 + 1.  i0 is inside the low image for every v inside the high one; i0 + 1 may be its extent.
struct UpTap {
    int32_t i0, f;
};
RT_QUERY_HD UpTap up_tap(const int32_t v, const int32_t s) {
    const int32_t i0 = v / s;
    return UpTap{i0, v - i0 * s};
}
// tap e (0 or 1) of that pair: inside the low image?
RT_QUERY_HD bool up_tap_inside(const int32_t i0, const int32_t e, const int32_t extent) { return static_cast<int64_t>(i0) + e < extent; }
// ... and its coordinate, i0 itself where the tap is outside (so that an address formed from it is always inside the low image)
RT_QUERY_HD int32_t up_tap_coord(const int32_t i0, const int32_t e, const int32_t extent) { return up_tap_inside(i0, e, extent) ? i0 + e : i0; }
// the nearest low coordinate: min((2v + s) / (2s), extent - 1), the low pixel whose high position is closest to v (a tie goes up)
RT_QUERY_HD int32_t up_nearest(const int32_t v, const int32_t s, const int32_t extent) {
    const int64_t n = (2 * static_cast<int64_t>(v) + s) / (2 * static_cast<int64_t>(s));
    return static_cast<int32_t>(n < extent - 1 ? n : extent - 1);
}

RT_QUERY_HD uint64_t up_miss_bytes(const int32_t width, const int32_t rows) { return dn_pixels(width, rows); }

// The squared scales, in float32 on the host: sn = sigma_normal, sz = sigma_depth * (float)s, sa = sigma_albedo.
struct UpScales {
    float sn2, sz2, sa2;
};
inline UpScales up_scales(const float sigma_normal, const float sigma_depth, const float sigma_albedo, const int32_t s) {
    const float sz = sigma_depth * static_cast<float>(s);
    return UpScales{sigma_normal * sigma_normal, sz * sz, sigma_albedo * sigma_albedo};
}

// The argument rules, none of which needs a context or a device.  0: valid; else the rule that failed, as a text for rt_last_error, and
// *unsupported says whether the failure is RT_ERR_UNSUPPORTED (else RT_ERR_INVALID).  `device`: the rules of rt_upsample_device -- out and
// both geometry buffers are 16-byte aligned, out and miss share no byte with each other or with an input; the host form copies, so it has
// no such rule.  miss may be null in both forms.
inline const char *up_args(const void *low, const int32_t channels, const void *gb_low, const void *gb_high, const int32_t width, const int32_t rows,
                           const int32_t *factor, const float *sigmas3, const void *out, const void *miss, const bool device, bool *unsupported) {
    *unsupported = false;
    if (!low || !gb_low || !gb_high || !out || !factor || !sigmas3) return "a pointer is null";
    if (!dn_channels_ok(channels)) return "channels must be 1 or 3";
    if (width < 1) return "width must be at least 1";
    if (rows < 0) return "rows is negative";
    if (!up_factor_ok(*factor)) return "factor outside 2 .. RT_UPSAMPLE_MAX_FACTOR";
    for (int k = 0; k < 3; ++k)
        if (!dn_sigma_ok(sigmas3[k])) return "a sigma is not > 0";
    if (!dn_size_ok(width, rows)) { *unsupported = true; return "width * rows above INT32_MAX"; }
    if (!device) return nullptr;
    if ((reinterpret_cast<uintptr_t>(out) & 15u) != 0u) return "the output must be 16-byte aligned";
    if ((reinterpret_cast<uintptr_t>(gb_low) & 15u) != 0u) return "the low geometry buffers must be 16-byte aligned";
    if ((reinterpret_cast<uintptr_t>(gb_high) & 15u) != 0u) return "the high geometry buffers must be 16-byte aligned";
    const int32_t w = up_low_extent(width, *factor), r = up_low_extent(rows, *factor);
    const uint64_t img = dn_image_bytes(width, rows, channels), mb = up_miss_bytes(width, rows);
    const uint64_t lb = dn_image_bytes(w, r, channels), gl = dn_gbuffer_bytes(w, r), gh = dn_gbuffer_bytes(width, rows);
    if (query_ranges_overlap(out, img, miss, mb)) return "the output overlaps the miss mask";
    if (query_ranges_overlap(out, img, low, lb)) return "the output overlaps the low image";
    if (query_ranges_overlap(out, img, gb_low, gl)) return "the output overlaps the low geometry buffers";
    if (query_ranges_overlap(out, img, gb_high, gh)) return "the output overlaps the high geometry buffers";
    if (query_ranges_overlap(miss, mb, low, lb)) return "the miss mask overlaps the low image";
    if (query_ranges_overlap(miss, mb, gb_low, gl)) return "the miss mask overlaps the low geometry buffers";
    if (query_ranges_overlap(miss, mb, gb_high, gh)) return "the miss mask overlaps the high geometry buffers";
    return nullptr;
}

}  // namespace rtamd
