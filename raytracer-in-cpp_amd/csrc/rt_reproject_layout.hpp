// rt_reproject_layout.hpp -- the arithmetic of the temporal reprojection (rt_reproject_device; include/rt_mi355x.h, "temporal reprojection";
// DESIGN.md §5, Temporal reprojection) that the host and the kernel of rt_reproject.hip share: where a pixel of the current frame lay in the
// previous one, the two history pixels a coordinate lies between, the scales, the argument rules of the calls and -- host only -- the map
// of rt_reproject_map.  The tiles, the lane's pixel, the 64-bit indices and the grid are the denoiser's (rt_denoise_layout.hpp).
// Header-only and free of HIP, so that tools/reproject_layout_check.cpp can run it under a sanitizer.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "rt_denoise_layout.hpp"

namespace rtamd {

constexpr int32_t kRpMaxHistory = 255;                   // RT_REPROJECT_MAX_HISTORY: a length is one byte

RT_QUERY_HD bool rp_history_ok(const int32_t n) { return n >= 1 && n <= kRpMaxHistory; }
RT_QUERY_HD uint64_t rp_len_bytes(const int32_t width, const int32_t rows) { return dn_pixels(width, rows); }

// the map as a kernel argument: m[r * 4 + k], rows r = x, y, depth, columns k = E, U, V, W
struct RpMap {
    float m[12];
};

// Where current pixel (xf, yf) with ray parameter z lay in the previous frame: num_r = m[r][E] * rho + ((xf * m[r][U] + yf * m[r][V]) +
// m[r][W]) with rho = 1.0f / z; den = num_depth; x' = num_x / den, y' = num_y / den, zr = z * den.  ok: den > 0.0f.
struct RpPos {
    float x, y, zr;
    bool ok;
};
RT_QUERY_HD float rp_num(const float *row, const float rho, const float xf, const float yf) {
    return row[0] * rho + ((xf * row[1] + yf * row[2]) + row[3]);
}
RT_QUERY_HD RpPos rp_project(const RpMap &M, const float xf, const float yf, const float z) {
    const float rho = 1.0f / z;
    const float nx = rp_num(M.m, rho, xf, yf), ny = rp_num(M.m + 4, rho, xf, yf), den = rp_num(M.m + 8, rho, xf, yf);
    return RpPos{nx / den, ny / den, z * den, den > 0.0f};
}
// v > -1.0f && v < (float)extent: a float test, made before any conversion to an integer (a NaN fails it)
RT_QUERY_HD bool rp_inside(const float v, const int32_t extent) { return v > -1.0f && v < static_cast<float>(extent); }
// A coordinate v that passed rp_inside lies on or behind history pixel i0 = (int)floorf(v), f = v - (float)i0 behind it; -1 <= i0 and, as
// (float)extent <= 2^31 and v is below it, i0 <= 2147483520: the conversion is defined.  The other tap is i0 + 1.
struct RpTap {
    int32_t i0;
    float f;
};
RT_QUERY_HD RpTap rp_tap(const float v) {
    const int32_t i0 = static_cast<int32_t>(floorf(v));
    return RpTap{i0, v - static_cast<float>(i0)};
}
// tap e (0 or 1) of that pair: inside the image?
RT_QUERY_HD bool rp_tap_inside(const int32_t i0, const int32_t e, const int32_t extent) {
    const int64_t t = static_cast<int64_t>(i0) + e;
    return t >= 0 && t < extent;
}
// ... and its coordinate, clamped into the image where the tap is outside (so that an address formed from it is always inside); extent >= 1
RT_QUERY_HD int32_t rp_tap_coord(const int32_t i0, const int32_t e, const int32_t extent) {
    const int64_t t = static_cast<int64_t>(i0) + e;
    return static_cast<int32_t>(t < 0 ? 0 : (t < extent ? t : static_cast<int64_t>(extent) - 1));
}

// The squared scales, in float32 on the host
struct RpScales {
    float sn2, sz2, sa2;
};
inline RpScales rp_scales(const float sigma_normal, const float sigma_depth, const float sigma_albedo) {
    return RpScales{sigma_normal * sigma_normal, sigma_depth * sigma_depth, sigma_albedo * sigma_albedo};
}

// The argument rules, none of which needs a context or a device.  0: valid; else the rule that failed, as a text for rt_last_error, and
// *unsupported says whether the failure is RT_ERR_UNSUPPORTED (else RT_ERR_INVALID).  `device`: the rules of rt_reproject_device -- out and
// both geometry buffers are 16-byte aligned, out and len_out share no byte with each other or with an input; the host form copies, so it
// has no such rule.
inline const char *rp_args(const void *cur, const int32_t channels, const void *gb_cur, const void *hist, const void *gb_hist, const void *len_hist,
                           const int32_t width, const int32_t rows, const float *m12, const int32_t *max_history, const float *sigmas3, const void *out,
                           const void *len_out, const bool device, bool *unsupported) {
    *unsupported = false;
    if (!cur || !gb_cur || !hist || !gb_hist || !len_hist || !m12 || !max_history || !sigmas3 || !out || !len_out) return "a pointer is null";
    if (!dn_channels_ok(channels)) return "channels must be 1 or 3";
    if (width < 1) return "width must be at least 1";
    if (rows < 0) return "rows is negative";
    if (!rp_history_ok(*max_history)) return "max_history outside 1 .. RT_REPROJECT_MAX_HISTORY";
    for (int k = 0; k < 3; ++k)
        if (!dn_sigma_ok(sigmas3[k])) return "a sigma is not > 0";
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(m12[k])) return "an entry of the map is not finite";
    if (!dn_size_ok(width, rows)) { *unsupported = true; return "width * rows above INT32_MAX"; }
    if (!device) return nullptr;
    if ((reinterpret_cast<uintptr_t>(out) & 15u) != 0u) return "the output must be 16-byte aligned";
    if ((reinterpret_cast<uintptr_t>(gb_cur) & 15u) != 0u) return "the current geometry buffers must be 16-byte aligned";
    if ((reinterpret_cast<uintptr_t>(gb_hist) & 15u) != 0u) return "the history's geometry buffers must be 16-byte aligned";
    const uint64_t img = dn_image_bytes(width, rows, channels), lb = rp_len_bytes(width, rows), gb = dn_gbuffer_bytes(width, rows);
    if (query_ranges_overlap(out, img, len_out, lb)) return "the output overlaps the output lengths";
    const struct { const void *p; uint64_t bytes; const char *out_text, *len_text; } ins[5] = {
        {cur, img, "the output overlaps the current image", "the output lengths overlap the current image"},
        {gb_cur, gb, "the output overlaps the current geometry buffers", "the output lengths overlap the current geometry buffers"},
        {hist, img, "the output overlaps the history image", "the output lengths overlap the history image"},
        {gb_hist, gb, "the output overlaps the history's geometry buffers", "the output lengths overlap the history's geometry buffers"},
        {len_hist, lb, "the output overlaps the history lengths", "the output lengths overlap the history lengths"}};
    for (const auto &i : ins) {
        if (query_ranges_overlap(out, img, i.p, i.bytes)) return i.out_text;
        if (query_ranges_overlap(len_out, lb, i.p, i.bytes)) return i.len_text;
    }
    return nullptr;
}

// ---- rt_reproject_map (host only) ----------------------------------------------------------------------------------------------------------
// a camera by its fields (the layout of rt_camera, without the public header)
struct RpCam {
    const float *center, *inv_view;      // [3], [12] 3x4 row-major
    float fovy, aspect;
    const float *viewport;               // [4]
};
inline bool rp_cam_finite(const RpCam &c) {
    for (int k = 0; k < 3; ++k) if (!std::isfinite(c.center[k])) return false;
    for (int k = 0; k < 12; ++k) if (!std::isfinite(c.inv_view[k])) return false;
    for (int k = 0; k < 4; ++k) if (!std::isfinite(c.viewport[k])) return false;
    return std::isfinite(c.fovy) && std::isfinite(c.aspect);
}
inline bool rp_cam_equal(const RpCam &a, const RpCam &b) {                  // in every bit
    return std::memcmp(a.center, b.center, 12) == 0 && std::memcmp(a.inv_view, b.inv_view, 48) == 0 && std::memcmp(&a.fovy, &b.fovy, 4) == 0 &&
           std::memcmp(&a.aspect, &b.aspect, 4) == 0 && std::memcmp(a.viewport, b.viewport, 16) == 0;
}
// B[r * 3 + k] in double: D(x, y) = screenToWorld(x, y) - center = B (x, y, 1)^T.  scale and aspect * scale are the floats of screen_to_world.
inline void rp_ray_matrix(const RpCam &c, double B[9]) {
    const float persp = static_cast<float>(static_cast<double>(1.0f) / std::tan(static_cast<double>(c.fovy / 2.0f) * (M_PI / static_cast<double>(180.0f))));
    const float scale = static_cast<float>(1.0 / static_cast<double>(persp));
    const double sc = static_cast<double>(scale), as = static_cast<double>(c.aspect * scale);
    const double v0 = c.viewport[0], v1 = c.viewport[1], v2 = c.viewport[2], v3 = c.viewport[3];
    const double ax = (2.0 / v2) * as, bx = ((-2.0 * v0) / v2 - 1.0) * as;
    const double ay = (-2.0 / v3) * sc, by = (1.0 + (2.0 * v1) / v3) * sc;
    for (int r = 0; r < 3; ++r) {
        const double m0 = c.inv_view[r * 4], m1 = c.inv_view[r * 4 + 1], m2 = c.inv_view[r * 4 + 2], t = c.inv_view[r * 4 + 3];
        B[r * 3] = m0 * ax;
        B[r * 3 + 1] = m1 * ay;
        B[r * 3 + 2] = (((m0 * bx + m1 * by) - m2) + t) - static_cast<double>(c.center[r]);
    }
}
inline double rp_cofactor3(const double m[9], const int i, const int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
}
// false: the matrix is singular (det is 0 or not finite)
inline bool rp_mat3_inverse(const double m[9], double inv[9]) {
    const double c0 = rp_cofactor3(m, 0, 0), c1 = rp_cofactor3(m, 1, 0), c2 = rp_cofactor3(m, 2, 0);
    const double det = c0 * m[0] + (c1 * m[3] + c2 * m[6]);
    if (det == 0.0 || !std::isfinite(det)) return false;
    const double invdet = 1.0 / det;
    inv[0] = c0 * invdet; inv[1] = c1 * invdet; inv[2] = c2 * invdet;
    inv[3] = rp_cofactor3(m, 0, 1) * invdet; inv[4] = rp_cofactor3(m, 1, 1) * invdet; inv[5] = rp_cofactor3(m, 2, 1) * invdet;
    inv[6] = rp_cofactor3(m, 0, 2) * invdet; inv[7] = rp_cofactor3(m, 1, 2) * invdet; inv[8] = rp_cofactor3(m, 2, 2) * invdet;
    return true;
}
// 0: m is written; else the rule that failed (nothing is written)
inline const char *rp_map(const RpCam &cur, const RpCam &prev, float m[12]) {
    if (!rp_cam_finite(cur) || !rp_cam_finite(prev)) return "a camera field is not finite";
    if (cur.viewport[2] == 0.0f || cur.viewport[3] == 0.0f || prev.viewport[2] == 0.0f || prev.viewport[3] == 0.0f) return "a viewport size is zero";
    double L[9], Linv[9];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) L[r * 3 + k] = prev.inv_view[r * 4 + k];
    if (!rp_mat3_inverse(L, Linv)) return "the previous inv_view is singular";
    double Bc[9], Bp[9], Bi[9];
    rp_ray_matrix(cur, Bc);
    rp_ray_matrix(prev, Bp);
    if (!rp_mat3_inverse(Bp, Bi)) return "the previous camera's rays do not span space";
    float o[12];
    if (rp_cam_equal(cur, prev)) {                                          // the identity, by rule
        for (int k = 0; k < 12; ++k) o[k] = 0.0f;
        o[1] = o[6] = o[11] = 1.0f;
    } else {
        const double d0 = static_cast<double>(cur.center[0]) - static_cast<double>(prev.center[0]);
        const double d1 = static_cast<double>(cur.center[1]) - static_cast<double>(prev.center[1]);
        const double d2 = static_cast<double>(cur.center[2]) - static_cast<double>(prev.center[2]);
        for (int r = 0; r < 3; ++r) {
            const double i0 = Bi[r * 3], i1 = Bi[r * 3 + 1], i2 = Bi[r * 3 + 2];
            o[r * 4] = static_cast<float>(i0 * d0 + (i1 * d1 + i2 * d2));
            for (int k = 0; k < 3; ++k) o[r * 4 + 1 + k] = static_cast<float>(i0 * Bc[k] + (i1 * Bc[3 + k] + i2 * Bc[6 + k]));
        }
    }
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(o[k])) return "the map is not finite";
    std::memcpy(m, o, sizeof o);
    return nullptr;
}

}  // namespace rtamd
